"""Shared helpers for the parity tests (oracle side)."""
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import weights as WR  # noqa: E402
from oracle import refmath  # noqa: E402


def golden(name):
    return {k: v for k, v in np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def seeded(manifest, name, seed, prefix="", requires_grad=False):
    """Draw the weights of fixture module `name` exactly as tests/golden/make_golden.py did."""
    w = WR.draw(manifest[name]["seeded"], seed)
    out = {}
    for k, a in w.items():
        t = torch.from_numpy(a)
        if requires_grad and not (k.endswith("running_mean") or k.endswith("running_var")):
            t.requires_grad_()
        out[prefix + k] = t
    return out, WR.checksum(w)


def oracle_grads(W, x, t, cond, spk, go, dtype, chunk=4):
    """out and every gradient of sum(out * go) by torch.autograd through the oracle, in `dtype`, `chunk` utterances at a
    time (parameter gradients accumulate over the chunks; bounds the graph's memory at B = 16, L = 1000)."""
    for w in W.values():
        w.grad = None
    res = {"out": [], "d_x": [], "d_cond": [], "d_spk": []}
    for b0 in range(0, x.shape[0], chunk):
        s = slice(b0, b0 + chunk)
        xs, cs = x[s].to(dtype).requires_grad_(), cond[s].to(dtype).requires_grad_()
        ss = None if spk is None else spk[s].to(dtype).requires_grad_()
        out = refmath.denoiser_forward(W, "", xs, t[s], cs, ss)
        (out * go[s].to(dtype)).sum().backward()
        res["out"].append(out.detach())
        res["d_x"].append(xs.grad)
        res["d_cond"].append(cs.grad)
        if ss is not None:
            res["d_spk"].append(ss.grad)
    ref = {k: torch.cat(v) for k, v in res.items() if v}
    for k, w in W.items():
        ref["param/" + k] = w.grad
        w.grad = None
    return ref


def condition_relu_kinks(W64, x, t, cond, spk, go, band, gen, chunk=4):
    """The denoiser's gradient is discontinuous where the input of one of its two ReLUs is zero, and a forward that is
    right to `band` (relative to the largest such input) may put any element within that band on either side: there the
    gradient has two legitimate values that differ by O(1) -- at B*L = 16 000 frames about 300 of the 8 M ReLU inputs
    lie within 2e-5.  Makes the float64 reference single-valued without touching the product, in place:
      input ReLU (a function of one frame of x): frames with an input inside the band are drawn again;
      skip ReLU: at frames with an input inside the band, go loses its component along the output-projection columns
      of those channels, so that the gradient arriving at them is zero and their mask bit multiplies nothing.
    Returns (frames of x redrawn, frames of go projected)."""
    Wd = {k: v.detach() for k, v in W64.items()}
    w_in, b_in = Wd["input_projection.0.conv.weight"][:, :, 0], Wd["input_projection.0.conv.bias"]
    redrawn = 0
    while True:
        pre = torch.einsum("cm,bml->bcl", w_in, x[:, 0].double()) + b_in[None, :, None]
        bad = (pre.abs() <= band * pre.abs().max()).any(1)                # [B, L]
        if not bool(bad.any()):
            break
        idx = bad.nonzero()
        redrawn += len(idx)
        x[idx[:, 0], 0, :, idx[:, 1]] = torch.randn(len(idx), x.shape[2], generator=gen)
    pres = []
    with torch.no_grad():
        for b0 in range(0, x.shape[0], chunk):
            s = slice(b0, b0 + chunk)
            taps = {}
            refmath.denoiser_forward(Wd, "", x[s].double(), t[s], cond[s].double(), None if spk is None else spk[s].double(),
                                     taps=taps)
            pres.append(taps["skip_pre"])
    pre = torch.cat(pres)
    bad = pre.abs() <= band * pre.abs().max()                             # [B, C, L]
    w_out = Wd["output_projection.conv.weight"][:, :, 0]                  # [M, C]: d y_c = sum_m w_out[m, c] go[m]
    frames = bad.any(1).nonzero()
    for b, l in frames.tolist():
        A = w_out[:, bad[b, :, l]]                                        # [M, k]
        g = go[b, 0, :, l].double()
        go[b, 0, :, l] = (g - A @ torch.linalg.lstsq(A, g[:, None]).solution[:, 0]).float()
    return redrawn, len(frames)


# Model sizes off the hand-tuned point (C = H = 256, M <= 96), DESIGN.md section 7.6: name -> (residual_layers NL,
# residual_channels C, encoder_hidden H, n_mel_channels M, multi_speaker).  test_gpu_denoiser_dims.py runs them,
# test_denoiser_plan_cpu.py pins the path each takes.
DEN_SIZES = {
    "A": (3, 128, 192, 80, 0),    # C below 256; H a multiple of 32, not of 64
    "B": (3, 64, 32, 20, 1),      # every minimum at once: 64-row packs, M below one 32-row block, K = H = 32 speaker projection
    "C": (2, 384, 256, 100, 0),   # C above 256, 2C = 768: the x / skip split falls inside a 128-row tile; NL < 3
    "D": (4, 256, 256, 100, 0),   # fused layers, generic head, fused tail
    "E": (3, 256, 256, 136, 1),   # fused layers, generic head and tail
    "F": (3, 256, 384, 80, 0),    # only H differs
    "G": (3, 256, 256, 80, 0),    # the control: single launch by default, generic under MG_DENOISER_GENERIC
}
DEN_SMALL_SHAPES = [(1, 1), (2, 63), (3, 129), (2, 260)]   # one frame; a partial 64-frame tile; one past two; float4, 128-frame tiles
DEN_LARGE_SHAPE = ("C", 16, 700)                           # the conv kernel's large forms (test_conv_forms_reached)


def den_size_configs(name, sizes=None):
    """(preprocess_config, model_config) of hot_path_configs with the sizes of DEN_SIZES[name] (or `sizes`)."""
    NL, C, H, M, ms = sizes or DEN_SIZES[name]
    _, pre, mc, _ = hot_path_configs(multi_speaker=bool(ms), stats_dir=None)
    pre["preprocessing"]["mel"]["n_mel_channels"] = M
    mc["transformer"]["encoder_hidden"] = H
    mc["denoiser"]["residual_channels"], mc["denoiser"]["residual_layers"], mc["denoiser"]["keep_bins"] = C, NL, M
    return pre, mc


def live_output_projection(den, seed=3):
    """Denoiser.__init__ zeroes output_projection's weight: with it the output would be the bias broadcast over the
    frames whatever the layers compute.  Seeded weight and bias instead."""
    gen = torch.Generator().manual_seed(seed)
    conv = den.output_projection.conv
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.05)
        conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)


def den_size_model(mg, name, sizes=None):
    """(product Denoiser of DEN_SIZES[name] (or `sizes`) on the CPU, its weights as float64 leaves, as float32 tensors).  No fixture
    recipe exists for these sizes: the module's own initialisation under a fixed seed, the same in every process."""
    torch.manual_seed(4100 + ord(name))
    den = mg.Denoiser(*den_size_configs(name, sizes))
    live_output_projection(den, 4200 + ord(name))
    W32 = {k: v.detach().clone() for k, v in den.state_dict().items()}
    W64 = {k: v.double().requires_grad_() for k, v in W32.items()}
    return den, W64, W32


# The denoiser tests' bars (max-abs error / max-abs reference, per tensor) against float64: forward, data gradients,
# parameter gradients -- and the one fallback for a tensor that misses its bar (den_judge).
DEN_FT, DEN_GT, DEN_PT = 2e-5, 5e-5, 1e-4


def den_kind(key):
    return re.sub(r"residual_layers\.\d+\.", "residual_layers.*.", key)


def den_bar(key):
    return DEN_FT if key == "out" else DEN_PT if key.startswith("param/") else DEN_GT


def den_err(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


def den_f32_cpu_errors(W32, x, t, cond, spk, go, ref):
    """The yardstick for a missed bar: the float32 CPU oracle's autograd error against the float64 one (`ref`) on the
    same inputs, worst tensor per kind."""
    W = {k: v.clone().requires_grad_() for k, v in W32.items()}
    got = oracle_grads(W, x, t, cond, spk, go, torch.float32)
    worst = {}
    for k, v in got.items():
        worst[den_kind(k)] = max(worst.get(den_kind(k), 0.0), den_err(v, ref[k]))
    return worst


def den_run(case):
    """One product forward in grad mode + backward of a case (den, x, t, cond, spk, go, ms, B, L); every result on the GPU,
    and how far the backward workspace's `launches` advanced."""
    den = case.den
    den.zero_grad(set_to_none=True)
    before = den.backward_status(case.B, case.L)
    x, cond = case.x.cuda().requires_grad_(), case.cond.cuda().requires_grad_()
    spk = case.spk.cuda().requires_grad_() if case.ms else None
    out = den(x, case.t.cuda(), cond, spk)
    (out * case.go.cuda()).sum().backward()
    after = den.backward_status(case.B, case.L)
    den.check()
    got = {"out": out.detach(), "d_x": x.grad, "d_cond": cond.grad}
    if case.ms:
        got["d_spk"] = spk.grad
    for k, p in den.named_parameters():
        assert p.grad is not None, k
        got["param/" + k] = p.grad
    den.zero_grad(set_to_none=True)
    assert after["error"] == 0 and before["error"] == 0, (before, after)
    return got, after["launches"] - before["launches"]


def den_judge(case, label, got, fails, keys=None, ref_of=None, tag="BWDERR"):
    """Every tensor against float64 (case.ref_gpu(key), or ref_of(key)) at its bar; a tensor that misses it passes only
    within 8 x the float32 CPU oracle's error at the same case (case.f32_cpu_error(kind)), and only where that exceeds
    the bar.  Prints and returns the worst error per tensor kind."""
    worst = {}
    for k in (keys or got):
        e = den_err(got[k], ref_of(k) if ref_of else case.ref_gpu(k))
        kind, bar = den_kind(k), den_bar(k)
        worst[kind] = max(worst.get(kind, 0.0), e)
        if not e <= bar:
            f32 = case.f32_cpu_error(kind)
            if 8 * f32 > bar and e <= 8 * f32:
                print("%s-WIDENED %s %s: %.3e > %.1e, within 8 x the float32 CPU oracle's %.3e" % (tag, label, k, e, bar, f32))
            else:
                fails.append("%s %s: %.3e > %.1e (float32 CPU oracle: %.3e)" % (label, k, e, bar, f32))
    for kind in sorted(worst):
        print("%s %-28s %-52s %.3e" % (tag, label, kind, worst[kind]))
    return worst


def jcu_oracle_grads(W, x_ts, x_t_prevs, s, t, cot, dtype, masks=None):
    """The ten maps of refmath.jcu_forward in `dtype` and every gradient of sum_i <cond_i, cot[0][i]> + <uncond_i, cot[1][i]>
    by torch.autograd (the three shared maps appear in both lists and get both cotangents).  `W`: leaves of `dtype` that
    require grad; `masks`: see jcu_forward.  Keys: "cond%d" / "uncond%d", "pre/..." (the pre-activations), "d_x_ts",
    "d_x_t_prevs", "d_s" (multi-speaker), "param/<state_dict key>"."""
    for w in W.values():
        w.grad = None
    leaf = lambda v: v.detach().to(dtype, copy=True).requires_grad_()     # never the caller's tensor
    a, b = leaf(x_ts), leaf(x_t_prevs)
    ss = None if s is None else leaf(s)
    taps = {}
    c, u = refmath.jcu_forward(W, a, b, ss, t, masks=masks, taps=taps)
    loss = sum((m * g.to(dtype)).sum() for m, g in zip(c, cot[0])) + sum((m * g.to(dtype)).sum() for m, g in zip(u, cot[1]))
    loss.backward()
    ref = {"d_x_ts": a.grad, "d_x_t_prevs": b.grad}
    if ss is not None:
        ref["d_s"] = ss.grad
    for i in range(len(c)):
        ref["cond%d" % i], ref["uncond%d" % i] = c[i].detach(), u[i].detach()
    for k, v in taps.items():
        ref["pre/" + k] = v
    for k, w in W.items():
        ref["param/" + k] = w.grad
        w.grad = None
    return ref


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def assert_close(a, b, tol, what=""):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(b, torch.Tensor):
        b = b.detach().cpu().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    e = rel_err(a, b)
    assert e <= tol, "%s: max-abs err / max-abs ref = %.3e > %.1e" % (what, e, tol)


def bar_for(ref32, ref64, bar):
    """The project's fallback rule: `bar`, or 8 x the float32 CPU restatement's own error where that exceeds bar / 8."""
    e = rel_err(ref32.detach().double().numpy(), ref64.detach().numpy())
    return bar if e <= bar / 8 else 8 * e


def check(got, ref32, ref64, bar, what):
    b = bar_for(ref32, ref64, bar)
    e = rel_err(got.detach().cpu().double().numpy(), ref64.detach().numpy())
    print("%-40s err %.3e  bar %.1e" % (what, e, b))
    assert_close(got.detach().cpu().double(), ref64, b, what)


def digest(g):
    g = g.detach().double().cpu()
    corner = g[tuple(slice(0, min(4, s)) for s in g.shape)].float().numpy()
    return np.array([g.sum().item(), g.abs().sum().item()]), corner


def assert_digest(g, gold, key, tol):
    """Compare a gradient against the (sum, abs-sum, corner) digest stored in the fixture."""
    d, corner = digest(g)
    ref = gold["dw_sum/" + key]
    scale = abs(ref[1]) + 1e-30
    assert abs(d[0] - ref[0]) / scale <= tol, (key, d, ref)
    assert abs(d[1] - ref[1]) / scale <= tol, (key, d, ref)
    if ("dw_corner/" + key) in gold:
        c = gold["dw_corner/" + key]
        # corner tolerance is relative to the tensor's mean magnitude
        mean_mag = ref[1] / max(1, g.numel())
        assert np.abs(corner - c).max() <= tol * max(np.abs(c).max(), mean_mag) * 4, (key,)


# ----------------------------------------------------------------------------------------------
# Hot-path configuration keys (SURVEY.md section 5 "Config / flags"), LJSpeech values.
def hot_path_configs(model="naive", T=4, mode="vpsde", multi_speaker=False, stats_dir=None, max_seq_len=1000):
    import types
    pre = {"preprocessing": {"mel": {"n_mel_channels": 80}, "speaker_embedder": "none"},
           "path": {"preprocessed_path": stats_dir}}
    mc = {
        "transformer": {"encoder_hidden": 256, "decoder_layer": 6, "decoder_head": 2, "decoder_hidden": 256,
                        "conv_filter_size": 1024, "conv_kernel_size": 9, "decoder_dropout": 0.2},
        "denoiser": {"denoiser_hidden": 512, "denoiser_dropout": 0.2, "residual_layers": 20, "residual_channels": 256,
                     "noise_schedule_naive": mode, "timesteps": T, "shallow_timesteps": T, "min_beta": 0.1,
                     "max_beta": 40, "s": 0.008, "keep_bins": 80},
        "discriminator": {"n_layer": 3, "n_uncond_layer": 2, "n_cond_layer": 2, "n_channels": [64, 128, 512, 128, 1],
                          "kernel_sizes": [3, 5, 5, 5, 3], "strides": [1, 2, 2, 1, 1]},
        "multi_speaker": multi_speaker, "max_seq_len": max_seq_len,
    }
    tr = {"loss": {"noise_loss": "l1", "adv_loss_mode": "lsgan", "lambda_fm": 10.0, "lambda_fm_shallow": 0.001},
          "optimizer": {"batch_size": 8, "betas": [0.5, 0.9], "gamma": 0.999, "grad_clip_thresh": 1, "grad_acc_step": 1,
                        "init_lr_G": 0.0001, "init_lr_D": 0.0002}}
    return types.SimpleNamespace(model=model), pre, mc, tr


def write_stats(tmpdir, spec_min, spec_max, n_speakers=0):
    import json
    with open(os.path.join(str(tmpdir), "stats.json"), "w") as f:
        json.dump({"pitch": [-2.0, 8.0, 0.0, 1.0], "energy": [-1.5, 7.0, 0.0, 1.0],
                   "spec_min": [float(v) for v in spec_min], "spec_max": [float(v) for v in spec_max]}, f)
    if n_speakers:
        with open(os.path.join(str(tmpdir), "speakers.json"), "w") as f:
            json.dump({"spk%d" % i: i for i in range(n_speakers)}, f)
    return str(tmpdir)


def load_seeded(module, manifest, name, seed, prefix=""):
    """Seed a product module with the fixture recipe through load_state_dict (checks key parity)."""
    w = WR.draw(manifest[name]["seeded"], seed)
    sd = module.state_dict()
    for k, a in w.items():
        assert prefix + k in sd, "missing state_dict key " + prefix + k
        assert tuple(sd[prefix + k].shape) == a.shape, (k, tuple(sd[prefix + k].shape), a.shape)
        sd[prefix + k] = torch.from_numpy(a)
    module.load_state_dict(sd)
    return WR.checksum(w)


class Tape:
    """noise_fn / t_fn stand-in replaying fixture tensors in call order."""

    def __init__(self, items):
        self.items = [torch.from_numpy(np.ascontiguousarray(a)) for a in items]
        self.i = 0

    def __call__(self, shape):
        x = self.items[self.i]
        self.i += 1
        assert tuple(x.shape) == tuple(shape), (tuple(x.shape), tuple(shape))
        return x


# ----------------------------------------------------------------------------------------------
# (a16) MixGANTTS.forward fixtures (tests/golden/mixgantts_*.npz): the recorded outputs of the reference's
# LinguisticEncoder, the 16 slots + p_targets + coarse_mels with their None-ness / requires_grad flags.
MIXGANTTS_CASES = [("naive", 0, True), ("naive", 1, True), ("naive", 0, False), ("shallow", 0, True),
                   ("shallow", 0, False), ("aux", 0, True)]


def mixgantts_case_name(model, ms, train):
    return "mixgantts_%s_ms%d_%s" % (model, ms, "train" if train else "infer")


def mixgantts_encoder_outputs(g, train, device=None):
    """The nine outputs of model/linguistic_encoder.py:373-383 as recorded; in training the float ones require grad,
    as they do coming out of the reference's encoder."""
    def one(key):
        t = T(g[key])
        if device is not None:
            t = t.to(device)
        if train and t.is_floating_point():
            t.requires_grad_()
        return t
    out = []
    for i in range(9):
        if ("enc/%d" % i) in g:
            out.append(one("enc/%d" % i))
        else:
            n = len([k for k in g if k.startswith("enc/%d/" % i)])
            out.append([one("enc/%d/%d" % (i, j)) for j in range(n)])
    return tuple(out)


def mixgantts_leaves(out, p_targets, coarse):
    """name -> tensor|None for every leaf of MixGANTTS.forward's return value (names as in the fixture)."""
    d = {}
    for i, o in enumerate(out):
        if isinstance(o, (list, tuple)):
            for j, oo in enumerate(o):
                d["slot%02d/%d" % (i, j)] = oo
        else:
            d["slot%02d" % i] = o
    d["p_targets"], d["coarse_mels"] = p_targets, coarse
    return d


def assert_mixgantts_slots(leaves, g, tol, check_flags):
    """Values, None-ness and (in training) requires_grad of every leaf against the fixture."""
    flags = dict(zip([str(k) for k in g["flag_names"]], [int(v) for v in g["flags"]]))
    assert sorted(leaves) == sorted(flags), (sorted(leaves), sorted(flags))
    for k, v in leaves.items():
        if flags[k] < 0:
            assert v is None, k + " should be None"
            continue
        assert v is not None, k + " is None"
        ref = g[k]
        a = v.detach().cpu().numpy()
        assert a.shape == ref.shape and str(a.dtype) == str(ref.dtype), (k, a.shape, a.dtype, ref.shape, ref.dtype)
        if a.dtype.kind == "f":
            fin = np.isfinite(ref)                 # encoder pass-throughs hold log(0) = -inf for padded words
            assert np.array_equal(a[~fin], ref[~fin], equal_nan=True), k
            assert_close(np.where(fin, a, 0), np.where(fin, ref, 0), tol, k)
        else:
            assert (a == ref).all(), k
        if check_flags:
            assert int(v.requires_grad) == flags[k], "%s.requires_grad = %s, reference %d" % (k, v.requires_grad, flags[k])


def mixgantts_tapes(g):
    """(rng draws in call order, dropout keep-masks in call order) of the fixture."""
    n = len([k for k in g if k.startswith("rng")])
    m = len([k for k in g if k.startswith("mask")])
    return [g["rng%d" % i] for i in range(n)], [g["mask%d" % i] for i in range(m)]


def pin_width(monkeypatch, nt):
    """MG_PERSIST_NT pins a tile width; 16: teams of workgroups per tile where they fit (denoiser_team16.h: 4 members,
    else 2), 216: teams of 2 only, 116: 16-frame tiles with one workgroup per tile (denoiser_persist16.h) everywhere;
    328: 32-frame tiles, 8 waves; 64: 64-frame tiles as four waves (one per SIMD), 864: as eight waves of 32 channels."""
    monkeypatch.setenv("MG_PERSIST_NT", str(16 if nt in (116, 216) else 32 if nt == 232 else nt))
    if nt == 232:      # 32-frame tiles, the two-workgroups-per-CU build also where one tile per CU would get the other one
        monkeypatch.setenv("MG_PERSIST_SOLO", "0")
    else:
        monkeypatch.delenv("MG_PERSIST_SOLO", raising=False)
    if nt == 116:
        monkeypatch.setenv("MG_PERSIST_TEAM", "0")
    elif nt == 216:
        monkeypatch.setenv("MG_PERSIST_TEAM", "2")
    else:
        monkeypatch.delenv("MG_PERSIST_TEAM", raising=False)
