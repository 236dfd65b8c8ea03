"""The resampler's oracle, restated for the tests in float64 numpy: the filter, the direct-form sum of the definition

    y[n] = up sum_k h[n down - k up + half] x[k],   0 <= k < len(x),  0 <= n down - k up + half <= 2 half,

and the float32 error bound of tests/test_gpu_resample.py.  Nothing here imports the package."""
import numpy as np

RATIOS = {(44100, 22050): (1, 2), (48000, 22050): (147, 320), (24000, 22050): (147, 160), (16000, 22050): (441, 320),
          (22050, 16000): (320, 441)}
U24 = 2.0 ** -24


def ref_filter(up, down, num_zeros=64, beta=14.769656459379492, rolloff=0.9475937167399596):
    m = max(up, down)
    n = np.arange(-num_zeros * m, num_zeros * m + 1, dtype=np.float64)
    h = rolloff / m * np.sinc(rolloff / m * n) * np.kaiser(len(n), beta)
    return h / h.sum()


def out_len(n, up, down):
    return -(-int(n) * up // down)


def direct(x, up, down, h, outputs=None):
    """(y, sabs, K) in float64 for the output indices `outputs` (default: all ceil(len up / down)): the sum above, the
    sum of |up h x| over the same terms, and the number of terms."""
    x = np.asarray(x, dtype=np.float64)
    half = (len(h) - 1) // 2
    n = np.arange(out_len(len(x), up, down), dtype=np.int64) if outputs is None else np.asarray(outputs, np.int64)
    nd = n * down
    k_lo = -((half - nd) // up)                 # ceil((nd - half) / up)
    kmax = 2 * half // up + 1
    k = k_lo[:, None] + np.arange(kmax, dtype=np.int64)[None, :]
    hi = nd[:, None] - k * up + half
    ok = (k >= 0) & (k < len(x)) & (hi >= 0) & (hi <= 2 * half)
    terms = np.where(ok, up * h[np.clip(hi, 0, 2 * half)] * x[np.clip(k, 0, max(len(x) - 1, 0))], 0.0) \
        if len(x) else np.zeros(k.shape)
    return terms.sum(1), np.abs(terms).sum(1), ok.sum(1)


def bound(sabs, K):
    """|y32 - y64| <= (K + 3) 2^-24 sum |up h x|: a float32 dot product of K terms in any order (gamma_K), plus one
    rounding each of the tap, the input and the result."""
    return (K + 3) * U24 * sabs
