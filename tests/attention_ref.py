"""Plain torch restatement of the decoder's multi-head attention (transformer/SubLayers.py:29-57, Modules.py:16-23) on
the channel-major layout of mg_attention_fwd, its fp16-operand variants, and the input sets of
tests/test_gpu_attention_forms.py.  attention() follows the dtype it is given: float64 is the reference, float32 feeds
the fallback rule (helpers.bar_for).  Nothing here touches a GPU."""
import functools
import math

import numpy as np
import torch

D_HEAD = 128
LOG2E = 1.44269504088896341


def split_heads(qkv, n_head):
    """qkv [B, 3*H*d, L] -> q, k, v [B, H, d, L] (rows = [Q heads | K heads | V heads], head-major)."""
    B, C3, L = qkv.shape
    HD = C3 // 3
    return [t.reshape(B, n_head, HD // n_head, L) for t in qkv.split(HD, 1)]


def attention(qkv, key_pad, n_head):
    """softmax(q.k / sqrt(d), masked keys at -inf) . v -> [B, H*d, L]; key_pad [B, L] (non-zero = masked) or None."""
    q, k, v = split_heads(qkv, n_head)
    s = torch.einsum("bhdq,bhdk->bhqk", q, k) / math.sqrt(q.shape[2])
    if key_pad is not None:
        s = s.masked_fill(key_pad.bool()[:, None, None, :], -math.inf)
    out = torch.einsum("bhqk,bhdk->bhdq", torch.softmax(s, -1), v)
    return out.reshape(qkv.shape[0], -1, qkv.shape[2])


def f16_operands(qkv, n_head, fused=False):
    """q, k, v as attention_fwd_f16_kernel's source rounds them: q times the float32 product scale * log2(e) in float32,
    then to fp16 (scores come out in log2 units); k and v to fp16.
    fused: the exact product q * c rounded ONCE, to fp16.  The compiled kernel does that for a quarter of its q
    elements (where the compiler folds the multiply and the conversion into v_fma_mixlo_f16) and the two roundings for
    the rest; the two differ in about 1e-4 of the elements, each by one fp16 unit of q: a shift of every score of that
    query by up to 2^-10 |k|.  Printed beside each case of the GPU test, asserted nowhere."""
    q, k, v = split_heads(qkv.float(), n_head)
    c = np.float32(np.float32(float(q.shape[2]) ** -0.5) * np.float32(LOG2E))
    if fused:       # float64 holds the 48-bit product exactly; numpy rounds float64 to float16 directly
        return torch.from_numpy((q.double().numpy() * float(c)).astype(np.float16)), k.half(), v.half()
    return (q * float(c)).half(), k.half(), v.half()


def attention_f16_ref(qkv, key_pad, n_head, fused=False):
    """float64 attention on the rounded operands: what the fp16 kernel would give with exact arithmetic after them."""
    q, k, v = [t.double() for t in f16_operands(qkv, n_head, fused)]
    s = torch.einsum("bhdq,bhdk->bhqk", q, k)
    if key_pad is not None:
        s = s.masked_fill(key_pad.bool()[:, None, None, :], -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    out = torch.einsum("bhqk,bhdk->bhdq", p / p.sum(-1, keepdim=True), v)
    return out.reshape(qkv.shape[0], -1, qkv.shape[2])


def attention_f16_emulation(qkv, key_pad, n_head, running_max=False, block=32):
    """The fp16 kernel's arithmetic on the CPU: fp16 operands, float32 scores, probabilities exp2(s - max) rounded to
    fp16 in the numerator and summed in float32 in the denominator, float32 accumulation.  Its distance from
    attention_f16_ref is the size of error that arithmetic has; 8 x that is the kernel's bar.
    running_max: as the kernel, walk the keys in blocks of 32, round each block's probabilities relative to the maximum
    so far and rescale what was accumulated; off: relative to the row's final maximum."""
    q, k, v = [t.float() for t in f16_operands(qkv, n_head)]
    B, H, d, L = q.shape
    s = torch.einsum("bhdq,bhdk->bhqk", q, k)
    masked = torch.zeros(B, 1, 1, L, dtype=torch.bool) if key_pad is None else key_pad.bool()[:, None, None, :]
    s = s.masked_fill(masked, -1.0e30)
    if not running_max:
        p = torch.where(masked, torch.zeros(()), torch.exp2(s - s.amax(-1, keepdim=True)))
        num = torch.einsum("bhqk,bhdk->bhdq", p.half().float(), v)
        return (num / p.sum(-1)[:, :, None, :]).reshape(B, H * d, L)
    m = torch.full((B, H, L), -1.0e30)
    l = torch.zeros(B, H, L)
    O = torch.zeros(B, H, d, L)
    for k0 in range(0, L, block):
        sb, mb = s[..., k0:k0 + block], masked[..., k0:k0 + block]
        m_new = torch.maximum(m, sb.amax(-1))
        corr = torch.exp2(m - m_new)
        p = torch.where(mb, torch.zeros(()), torch.exp2(sb - m_new[..., None]))
        l = l * corr + p.sum(-1)
        O = O * corr[:, :, None, :] + torch.einsum("bhqk,bhdk->bhdq", p.half().float(), v[..., k0:k0 + block])
        m = m_new
    return (O / l[:, :, None, :]).reshape(B, H * d, L)


# ------------------------------------------------------------------------------------------------ input sets
B, N_HEAD = 2, 3
COMMON_L = (1, 3, 4, 33, 63, 64, 65, 700)
INPUTS = ("unit", "peaked", "late_max")
MASKS = ("none", "suffix", "scattered")


def key_mask(L, kind):
    """uint8 [B, L], 1 = masked key, or None.  suffix: lengths [L, 1].  scattered: about a third of the keys at random
    places, every item keeps at least one key (L // 2), and from L = 128 on keys 0..31 and 96..127 -- two whole aligned
    32-key blocks, the first one among them -- are masked in every item."""
    if kind == "none":
        return None
    m = torch.zeros(B, L, dtype=torch.uint8)
    if kind == "suffix":
        m[1, 1:] = 1
        return m
    g = torch.Generator().manual_seed(7000 + L)
    m = (torch.rand(B, L, generator=g) < 0.35).to(torch.uint8)
    if L >= 128:
        m[:, 0:32] = 1
        m[:, 96:128] = 1
    m[:, L // 2 if L < 128 else 40] = 0
    assert int((m == 0).sum(1).min()) >= 1
    return m


@functools.lru_cache(maxsize=None)
def case(L, inputs, mask):
    """(qkv float32 [B, 3*H*128, L], key_pad or None).
    unit: unit-variance q, k, v.  peaked: three times that, a near one-hot softmax.  late_max: unit variance, then the K
    column of each item's last valid key times 6 (for about half the queries the row maximum arrives with the last key
    block); with a mask, the K column of each item's first masked key times 50 and V of every masked key at 1e4, so that
    a leak through the mask is an error of order 1e4."""
    g = torch.Generator().manual_seed(100 * L + 10 * INPUTS.index(inputs) + MASKS.index(mask))
    HD = N_HEAD * D_HEAD
    qkv = torch.randn(B, 3 * HD, L, generator=g)
    pad = key_mask(L, mask)
    if inputs == "peaked":
        qkv *= 3
    if inputs == "late_max":
        for b in range(B):
            valid = torch.ones(L, dtype=torch.bool) if pad is None else pad[b] == 0
            qkv[b, HD:2 * HD, int(valid.nonzero().max())] *= 6
            if not bool(valid.all()):
                qkv[b, HD:2 * HD, int((~valid).nonzero().min())] *= 50
                qkv[b, 2 * HD:, ~valid] = 1.0e4
    return qkv, pad


@functools.lru_cache(maxsize=None)
def refs(L, inputs, mask):
    """(float32 restatement, float64 reference) of case(L, inputs, mask): computed once, shared by every form."""
    qkv, pad = case(L, inputs, mask)
    return attention(qkv, pad, N_HEAD), attention(qkv.double(), pad, N_HEAD)


@functools.lru_cache(maxsize=None)
def refs_f16(L, inputs, mask):
    """(rounded-operand float64 reference, plain emulation, running-maximum emulation, the reference with q rounded
    once) of the same case."""
    qkv, pad = case(L, inputs, mask)
    return (attention_f16_ref(qkv, pad, N_HEAD), attention_f16_emulation(qkv, pad, N_HEAD),
            attention_f16_emulation(qkv, pad, N_HEAD, running_max=True), attention_f16_ref(qkv, pad, N_HEAD, fused=True))
