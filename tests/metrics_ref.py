"""Float64 numpy restatement of mixgan_tts_amd/metrics.py (csrc/dtw.hip): the cepstra, the DTW with its recurrence and
tie rule, the cost of a given path and the two F0 figures; and the seeded inputs the metric tests share."""
import numpy as np

MCD_SCALE = 10.0 / np.log(10.0) * np.sqrt(2.0)


# ------------------------------------------------------------------ cepstra
def dct_rows(M, n_coef):
    """[n_coef, M] float64: rows k = 1 .. n_coef of the orthonormal DCT-II over M bins."""
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / M) * np.cos(np.pi / M * (m + 0.5) * k)


def cepstra(mel, lengths=None, n_coef=13):
    """mel [B, T, M] -> float64 [B, T, n_coef], zero at and past lengths[b]."""
    mel = np.asarray(mel, np.float64)
    B, T, M = mel.shape
    live = np.ones((B, T), bool) if lengths is None else np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    out = np.where(live[..., None], mel, 0.0) @ dct_rows(M, n_coef).T
    return np.where(live[..., None], out, 0.0)


# ------------------------------------------------------------------ DTW
def local_cost(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for i0 in range(0, a.shape[0], 128):
        out[i0:i0 + 128] = np.sqrt(((a[i0:i0 + 128, None, :] - b[None, :, :]) ** 2).sum(-1))
    return out


def _backtrace(code, n, m):
    i, j, path = n - 1, m - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        c = code[i, j]
        i, j = i - (c != 2), j - (c != 1)
    return np.array(path[::-1], np.int64)


def dtw(a, b):
    """a [n, D], b [m, D] -> (total, Dacc [n, m], path [len, 2]).  Dacc(0, 0) = c(0, 0); Dacc(i, j) = c(i, j) + the
    least of Dacc(i-1, j-1), Dacc(i-1, j), Dacc(i, j-1) over those that exist, ties to the diagonal, then (i-1, j),
    then (i, j-1).  Vectorised over each anti-diagonal."""
    cost = local_cost(a, b)
    n, m = cost.shape
    Dacc = np.full((n, m), np.inf)
    code = np.zeros((n, m), np.int8)
    for d in range(n + m - 1):
        i = np.arange(max(0, d - m + 1), min(d, n - 1) + 1)
        j = d - i
        diag = np.where((i > 0) & (j > 0), Dacc[np.maximum(i - 1, 0), np.maximum(j - 1, 0)], np.inf)
        up = np.where(i > 0, Dacc[np.maximum(i - 1, 0), j], np.inf)
        left = np.where(j > 0, Dacc[i, np.maximum(j - 1, 0)], np.inf)
        best, c = diag.copy(), np.zeros(len(i), np.int8)
        sel = up < best
        best[sel], c[sel] = up[sel], 1
        sel = left < best
        best[sel], c[sel] = left[sel], 2
        if d == 0:
            best[:] = 0.0
        Dacc[i, j] = cost[i, j] + best
        code[i, j] = c
    return Dacc[n - 1, m - 1], Dacc, _backtrace(code, n, m)


def dtw_loops(a, b):
    """The same recurrence cell by cell: (total, path)."""
    cost = local_cost(a, b)
    n, m = cost.shape
    Dacc = np.zeros((n, m))
    code = np.zeros((n, m), np.int8)
    for i in range(n):
        for j in range(m):
            best, c = 0.0, 0
            if i > 0 or j > 0:
                best = np.inf
                if i > 0 and j > 0:
                    best, c = Dacc[i - 1, j - 1], 0
                if i > 0 and Dacc[i - 1, j] < best:
                    best, c = Dacc[i - 1, j], 1
                if j > 0 and Dacc[i, j - 1] < best:
                    best, c = Dacc[i, j - 1], 2
            Dacc[i, j] = cost[i, j] + best
            code[i, j] = c
    return Dacc[n - 1, m - 1], _backtrace(code, n, m)


def path_cost(a, b, path):
    """The float64 cost of a given path [len, 2]."""
    a, b, path = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(path)
    return float(np.sqrt(((a[path[:, 0]] - b[path[:, 1]]) ** 2).sum(-1)).sum())


def check_path(path, n, m):
    """A monotone path from (0, 0) to (n - 1, m - 1) whose every step is one of the three moves."""
    path = np.asarray(path)
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n - 1, m - 1), (path[0], path[-1], n, m)
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    assert steps <= {(1, 1), (1, 0), (0, 1)}, steps


def total_bar(n, m, ref):
    """|total - ref| allowed: float32 accumulation over a path of at most n + m - 1 terms, with headroom for the local
    cost's rounding."""
    return 8.0 * (n + m) * 2.0 ** -24 * ref


def mcd(total, path_len):
    return MCD_SCALE * total / path_len


def mcd_framewise(c_ref, c_syn, n):
    """align="none": the mean over the first n frames of the frame-wise distance, in dB."""
    c_ref, c_syn = np.asarray(c_ref, np.float64)[:n], np.asarray(c_syn, np.float64)[:n]
    return MCD_SCALE * np.sqrt(((c_ref - c_syn) ** 2).sum(-1)).mean()


# ------------------------------------------------------------------ F0
def f0_figures(f0_ref, f0_syn, path):
    """(f0_rmse_cents, vuv_error) of one utterance along path [len, 2]; indices past a track are clipped to its last
    frame; 0 is unvoiced; NaN RMSE when no cell is voiced on both sides."""
    f0_ref, f0_syn, path = np.asarray(f0_ref, np.float64), np.asarray(f0_syn, np.float64), np.asarray(path)
    fr = f0_ref[np.minimum(path[:, 0], len(f0_ref) - 1)]
    fs = f0_syn[np.minimum(path[:, 1], len(f0_syn) - 1)]
    both = (fr > 0) & (fs > 0)
    rmse = np.sqrt(np.mean((1200.0 * np.log2(fs[both] / fr[both])) ** 2)) if both.any() else np.nan
    return rmse, float(((fr > 0) != (fs > 0)).mean())


# ------------------------------------------------------------------ seeded inputs
DTW_SHAPES = [(1, 1), (1, 5), (5, 1), (63, 65), (64, 64), (37, 130), (300, 270), (513, 17)]
DTW_FEATURES = [1, 13, 64]
# Ta above the 1024 threads of a workgroup: a thread owns the rows tid, tid + 1024, tid + 2048, so two and three of
# its rows are live, with the other side short; the long side as b, where every thread still owns one row; and a
# pair long on both sides, whose path warps across the boundary between a thread's first and second row
DTW_LONG_SHAPES = [(1100, 40), (40, 1100), (2100, 17), (1100, 900)]


def random_walk_mel(rng, T, M=80):
    """A smooth log-mel: a spectral tilt from about -3 to -9, plus a random walk in time smoothed over the bins."""
    steps = rng.normal(0.0, 0.25, (T, M))
    kernel = np.hanning(9) / np.hanning(9).sum()
    steps = np.stack([np.convolve(s, kernel, mode="same") for s in steps])
    walk = np.cumsum(steps, 0) + rng.normal(0.0, 1.0, (1, M))
    return (np.linspace(-3.0, -9.0, M)[None, :] + walk).astype(np.float32)


def warp_index(rng, Ta, Tb):
    """Tb monotone indices into Ta frames, first 0 and last Ta - 1: seeded runs that repeat frames (speed 0), keep
    them (1) or drop every other one (2), scaled to end on the last frame."""
    speed = np.empty(0)
    while len(speed) < Tb:
        speed = np.concatenate([speed, np.full(rng.integers(3, 12), float(rng.integers(0, 3)))])
    pos = np.concatenate([[0.0], np.cumsum(speed[:Tb - 1] + 0.05)])
    if pos[-1] > 0:
        pos *= (Ta - 1) / pos[-1]
    return np.rint(pos).astype(np.int64)


def warped_pair(seed, Ta, Tb, D=13, noise=0.02):
    """(a [Ta, D], b [Tb, D]) float32: a is the cepstra of a random-walk log-mel, b a piecewise time-warped copy of it
    plus small Gaussian noise, so that the optimal path warps for real."""
    rng = np.random.default_rng(seed)
    a = cepstra(random_walk_mel(rng, Ta)[None], None, D)[0].astype(np.float32)
    b = a[warp_index(rng, Ta, Tb)] + rng.normal(0.0, noise, (Tb, D))
    return a, b.astype(np.float32)


def pair_seed(Ta, Tb, D):
    return 1000 * Ta + 7 * Tb + D


def repeated_copy(seed, T, D=13):
    """(a [T, D], b [sum r, D]) float32: b repeats frame i of a r_i times, seeded r_i in 1 .. 3."""
    rng = np.random.default_rng(seed)
    a = cepstra(random_walk_mel(rng, T)[None], None, D)[0].astype(np.float32)
    return a, np.repeat(a, rng.integers(1, 4, T), axis=0)
