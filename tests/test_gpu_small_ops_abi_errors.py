"""Argument checks of the small entry points (csrc/elementwise.hip, misc_api.hip, losses.hip, lingops.hip) on real device
buffers of a valid size: a null operand gives MG_ERR_ARG, so does an unknown mode or activation, a size that is not
positive or that is past a documented limit gives MG_ERR_SHAPE, and in every such case nothing is launched -- the outputs
keep their sentinel.  The unchanged call then returns MG_OK and writes them."""
import pytest
import torch

from mixgan_tts_amd import _lib
from mixgan_tts_amd._lib import MG_ERR_ARG, MG_ERR_SHAPE, MG_OK, stream_ptr

pytestmark = pytest.mark.gpu
B, L, M, T, C, D0, D1, D2, N, K, TW, TP, H, W = 2, 8, 4, 4, 3, 4, 6, 5, 5, 7, 4, 9, 3, 4


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def f(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).cuda()


def i64(*shape, v=1):
    return torch.full(shape, v, dtype=torch.int64).cuda()


def u8(*shape):
    return torch.ones(*shape, dtype=torch.uint8).cuda()


class P:
    """A required input pointer."""
    def __init__(self, t):
        self.t = t


class O(P):
    """A required output pointer, filled with a sentinel."""
    def __init__(self, *shape, dtype=torch.float32):
        self.t = torch.full(shape, 7, dtype=dtype).cuda()


class Opt(P):
    """A pointer that may be null."""


class Size:
    """A size that has to be positive."""
    def __init__(self, v):
        self.v = v


def ptr(t):
    return None if t is None else t.data_ptr()


def run(L_, name, spec, extra=()):
    """spec: the arguments of one valid call (P / O / Opt / Size / plain values; the stream is appended).  extra:
    ({index: value}, expected code) pairs for what the generic sweep does not reach."""
    fn = getattr(L_, name)
    base = [ptr(a.t) if isinstance(a, P) else a.v if isinstance(a, Size) else a for a in spec]

    def call(changes):
        args = list(base)
        for k, v in changes.items():
            args[k] = v
        return fn(*args, stream_ptr())

    for k, a in enumerate(spec):
        if isinstance(a, P) and not isinstance(a, Opt):
            assert call({k: None}) == MG_ERR_ARG, "%s: argument %d null" % (name, k)
        if isinstance(a, Size):
            for bad in (0, -1):
                assert call({k: bad}) == MG_ERR_SHAPE, "%s: argument %d = %d" % (name, k, bad)
    for changes, code in extra:
        assert call(changes) == code, "%s: %s" % (name, changes)
    torch.cuda.synchronize()
    outs = [a.t for a in spec if isinstance(a, O)]
    for o in outs:
        assert bool((o == 7).all()), name + ": an output was written by a refused call"
    assert call({}) == MG_OK, name
    torch.cuda.synchronize()
    assert not outs or any(not bool((o == 7).all()) for o in outs), name + ": the valid call wrote nothing"


def test_diffusion_entry_points(mg):
    Lb = mg.lib()
    smin, smax, tab = f(M) - 5, f(M) + 5, torch.rand(T).cuda()
    t = i64(B)
    for name, more in (("mg_transpose_bml", []), ("mg_transpose_bml_strided", [M * L])):
        spec = [P(f(B, L, M)), O(B, M, L), P(smin), P(smax), Opt(u8(B, L)), 0, 1, Size(B), Size(L), Size(M)] + more
        run(Lb, name, spec, [({6: 3}, MG_ERR_ARG), ({6: -1}, MG_ERR_ARG)])
        run(Lb, name, [P(f(B, M, L)), O(B, L, M), Opt(None), Opt(None), Opt(None), 1, 0, Size(B), Size(L), Size(M)] + more,
            [({6: 2}, MG_ERR_ARG), ({6: 1}, MG_ERR_ARG)])             # modes 1 and 2 need the statistics
    run(Lb, "mg_diffuse_fwd", [P(f(B, L, M)), P(t), P(f(B, M, L)), Opt(u8(B, L)), P(smin), P(smax), P(tab), P(tab), O(B, M, L),
                               Size(B), Size(L), Size(M), Size(T)])
    run(Lb, "mg_posterior_sample_fwd", [P(f(B, M, L)), P(f(B, M, L)), P(t), P(f(B, M, L)), Opt(u8(B, L)), P(tab), P(tab), P(tab),
                                        O(B, M, L), Opt(None), 1, Size(B), Size(L), Size(M), Size(T)])
    run(Lb, "mg_posterior_sample_bwd", [P(f(B, M, L)), P(t), Opt(u8(B, L)), P(tab), Opt(f(B, M, L)), Opt(f(B, M, L)), O(B, M, L),
                                        1, Size(B), Size(L), Size(M), Size(T)], [({4: None, 5: None}, MG_ERR_ARG)])
    run(Lb, "mg_spec_affine", [P(f(B * L, M)), O(B * L, M), P(smin), P(smax), 1, B * L * M, Size(M)],
        [({4: 0}, MG_ERR_ARG), ({4: 5}, MG_ERR_ARG)])
    run(Lb, "mg_diffuse_trace_bwd", [P(f(T + 1, B, L, M)), P(f(B, L, M)), P(smin), P(smax), Opt(u8(B, L)), P(tab), O(B, L, M), T,
                                     Size(B), Size(L), Size(M)], [({7: -1}, MG_ERR_SHAPE)])


def test_misc_entry_points(mg):
    Lb = mg.lib()
    n = B * C * L
    run(Lb, "mg_act_bwd", [P(f(n)), P(f(n)), O(n), _lib.MG_ACT_RELU, n], [({3: -1}, MG_ERR_ARG), ({3: _lib.MG_ACT_LRELU}, MG_ERR_ARG)])
    run(Lb, "mg_gate_bwd", [P(f(B, C, L)), P(torch.rand(B, C, L).cuda()), P(f(B, C, L).tanh()), O(B, 2 * C, L), Size(B), Size(C), Size(L)])
    run(Lb, "mg_mish_fwd", [P(f(n)), O(n), n])
    run(Lb, "mg_mish_bwd", [P(f(n)), P(f(n)), O(n), n])
    run(Lb, "mg_upsample_zero_act", [P(f(C, L)), O(C, 3 * L), Size(C), Size(L), Size(3), Size(3 * L), 0.1])
    run(Lb, "mg_upsample_zero", [P(f(C, L)), O(C, 3 * L), Size(C), Size(L), Size(3), Size(3 * L)])
    t, freq = i64(B, v=3), torch.rand(D0 // 2).cuda()
    run(Lb, "mg_step_embed", [P(t), P(freq), O(B, D0), Size(B), Size(D0)], [({4: 3}, MG_ERR_SHAPE)])
    run(Lb, "mg_step_mlp_fwd", [P(t), P(freq), P(f(D1, D0)), P(f(D2, D1)), O(B, D0), O(B, D1), O(B, D1), O(B, D2), Size(B), Size(D0),
                                Size(D1), Size(D2)], [({9: 3}, MG_ERR_SHAPE)])
    run(Lb, "mg_step_mlp_bwd", [P(f(B, D2)), P(f(B, D0)), P(f(B, D1)), P(f(B, D1)), P(f(D2, D1)), O(D1, D0), O(D2, D1), O(2 * B * D1),
                                Size(B), Size(D0), Size(D1), Size(D2)])
    run(Lb, "mg_linear_small_fwd", [P(f(B, K)), P(f(N, K)), O(B, N), Size(B), Size(N), Size(K)])
    dx, dW = O(B, K), O(N, K)
    run(Lb, "mg_linear_small_bwd", [P(f(B, N)), P(f(B, K)), P(f(N, K)), Opt(dx.t), Opt(dW.t), Size(B), Size(N), Size(K)],
        [({3: None, 4: None}, MG_ERR_ARG)])
    assert not bool((dx.t == 7).all()) and not bool((dW.t == 7).all())


def test_small_linear_alignment_is_checked(mg):
    """K % 256 == 0 runs on 16-byte loads: a weight or an input 4 bytes into its storage is MG_ERR_ARG for both entry points;
    any other K takes it."""
    Lb = mg.lib()
    Kv = 256
    store = torch.zeros(N * Kv + B * Kv + 8).cuda()
    Wm, xm = store[1:1 + N * Kv], store[1 + N * Kv + 4:1 + N * Kv + 4 + B * Kv]
    Wa, xa, out = f(N, Kv), f(B, Kv), O(B, N)
    assert Wm.data_ptr() % 16 == 4 and xm.data_ptr() % 16 == 4 and Wa.data_ptr() % 16 == 0
    for x_, W_ in ((xm, Wa), (xa, Wm), (xm, Wm)):
        assert Lb.mg_linear_small_fwd(ptr(x_), ptr(W_), ptr(out.t), B, N, Kv, stream_ptr()) == MG_ERR_ARG
    t, freq = i64(B, v=3), torch.rand(Kv // 2).cuda()
    emb, pre, h, o2 = O(B, Kv), O(B, Kv), O(B, Kv), O(B, D2)
    big, W2a = torch.zeros(Kv * Kv + 1).cuda(), f(D2, Kv)
    W0m = big[1:]

    def mlp(W0, W2, e=emb.t, hh=h.t):
        return Lb.mg_step_mlp_fwd(ptr(t), ptr(freq), ptr(W0), ptr(W2), ptr(e), ptr(pre.t), ptr(hh), ptr(o2.t), B, Kv, Kv, D2,
                                  stream_ptr())

    W0a = f(Kv, Kv)
    big2 = torch.zeros(D2 * Kv + 1).cuda()
    assert mlp(W0m, W2a) == MG_ERR_ARG and mlp(W0a, big2[1:]) == MG_ERR_ARG
    spare = torch.zeros(B * Kv + 1).cuda()
    assert mlp(W0a, W2a, e=spare[1:]) == MG_ERR_ARG and mlp(W0a, W2a, hh=spare[1:]) == MG_ERR_ARG
    torch.cuda.synchronize()
    for o in (out, emb, pre, h, o2):
        assert bool((o.t == 7).all())
    assert Lb.mg_linear_small_fwd(ptr(xa), ptr(Wa), ptr(out.t), B, N, Kv, stream_ptr()) == MG_OK and mlp(W0a, W2a) == MG_OK
    # K = 255: the scalar form, no requirement
    assert Lb.mg_linear_small_fwd(ptr(xm), ptr(Wm), ptr(out.t), B, N, 255, stream_ptr()) == MG_OK
    torch.cuda.synchronize()
    assert not bool((o2.t == 7).all())


def test_loss_entry_points(mg):
    Lb = mg.lib()
    n, g = 100, torch.ones(1).cuda()
    run(Lb, "mg_loss_sum", [P(f(n)), P(f(n)), 0.0, 1, n, O(1)], [({3: 2}, MG_ERR_ARG), ({3: -1}, MG_ERR_ARG)])
    run(Lb, "mg_loss_sum", [P(f(n)), Opt(None), 0.5, 0, n, O(1)], [({3: 1}, MG_ERR_ARG)])     # L1 needs b
    run(Lb, "mg_loss_grad", [P(f(n)), P(f(n)), 0.0, 1, P(g), 0.01, n, O(n)], [({3: 2}, MG_ERR_ARG), ({3: -1}, MG_ERR_ARG)])
    rows = B * L
    run(Lb, "mg_mel_l1_fwd", [P(f(rows, M)), P(f(rows, M)), Opt(u8(rows)), Size(rows), Size(M), O(2)])
    run(Lb, "mg_mel_l1_bwd", [P(f(rows, M)), P(f(rows, M)), Opt(u8(rows)), Size(rows), Size(M), P(g), P(g), O(rows, M)])
    run(Lb, "mg_mel_count_rows", [P(f(rows, M)), Opt(u8(rows)), Size(rows), Size(M), O(1, dtype=torch.int64)])


def test_lingops_entry_points(mg):
    Lb = mg.lib()
    wb, swl, dur = i64(B, TW, v=2), i64(B, v=TW), i64(B, TW, v=2)
    run(Lb, "mg_length_regulate_fwd", [P(f(B, TW, H)), P(dur), O(B, L, H), O(B, dtype=torch.int64), Size(B), Size(TW), Size(H), Size(L)])
    run(Lb, "mg_length_regulate_bwd", [P(f(B, L, H)), P(dur), O(B, TW, H), Size(B), Size(TW), Size(H), Size(L)])
    run(Lb, "mg_word_pool_fwd", [P(f(B, TP, H)), P(wb), P(swl), O(B, W, H), Size(B), Size(TP), Size(TW), Size(H), Size(W), 0])
    run(Lb, "mg_word_pool_bwd", [P(f(B, W, H)), P(wb), P(swl), O(B, TP, H), Size(B), Size(TP), Size(TW), Size(H), Size(W), 1])
    run(Lb, "mg_mapping_mask", [P(dur), P(wb), P(swl), O(B, L, TP, dtype=torch.uint8), Size(B), Size(TW), Size(L), Size(TP)])
    run(Lb, "mg_rel_coef", [P(dur), P(swl), P(u8(B, L)), O(B, L), Size(B), Size(TW), Size(L)])
    # one word past what the prefix sums hold in LDS, on buffers that really are that long
    for tw, names in ((4097, ("regulate", "pool", "rel")), (2049, ("mask",))):
        big, one = i64(1, tw), i64(1, v=tw)
        x, out, mk = f(1, tw, 1), O(1, tw, 1), u8(1, tw)
        s = stream_ptr()
        if "regulate" in names:
            assert Lb.mg_length_regulate_fwd(ptr(x), ptr(big), ptr(out.t), ptr(one), 1, tw, 1, tw, s) == MG_ERR_SHAPE
            assert Lb.mg_length_regulate_bwd(ptr(x), ptr(big), ptr(out.t), 1, tw, 1, tw, s) == MG_ERR_SHAPE
            assert Lb.mg_word_pool_fwd(ptr(x), ptr(big), ptr(one), ptr(out.t), 1, tw, tw, 1, tw, 0, s) == MG_ERR_SHAPE
            assert Lb.mg_word_pool_bwd(ptr(x), ptr(big), ptr(one), ptr(out.t), 1, tw, tw, 1, tw, 0, s) == MG_ERR_SHAPE
            assert Lb.mg_rel_coef(ptr(big), ptr(one), ptr(mk), ptr(out.t), 1, tw, tw, s) == MG_ERR_SHAPE
        else:
            m = O(1, 4, 4, dtype=torch.uint8)
            assert Lb.mg_mapping_mask(ptr(big), ptr(big), ptr(one), ptr(m.t), 1, tw, 4, 4, s) == MG_ERR_SHAPE
            assert bool((m.t == 7).all())
        torch.cuda.synchronize()
        assert bool((out.t == 7).all())
