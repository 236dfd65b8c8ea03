// Backward passes of the LinguisticEncoder's own kernels (lingenc.hip), for training the native encoder:
//   mg_rel_attention_bwd   RelativeSelfAttention.attention (model/blocks.py:1016-1061) with dropout on p_attn
//   mg_w2p_attention_bwd   ScaledDotProductAttention of WordToPhonemeAttention (model/blocks.py:741-768)
//   mg_embed_cm_bwd        nn.Embedding gradient from a channel-major output (src_emb, pitch / energy embeddings)
//   mg_variance_head_bwd   VariancePredictor.linear_layer (+ mask, control)
//   mg_duration_head_bwd   log(word sum of exp(log_d_p))
//   mg_posenc_add_bwd      d table[l, c] = sum_b coef[b, l] dOut[b, c, l]
//   mg_dropout_apply       out = keep ? x * scale : 0 (its own backward)
// The dense contractions of both attentions are mg_bgemm (as attention_train_bwd); the kernels here do the
// row-local parts (relative band, dropout, softmax backward, masks).  Every reduction has a fixed order: partial sums
// land in per-slot buffers that one more kernel adds up in slot order, so two runs give bit-identical gradients.
#include "common.h"

#define LT_D 128     // head width (LE_D of lingenc.hip)
#define LT_WMAX 8    // largest window (LE_WMAX)
#define LT_NREL (2 * LT_WMAX + 1)
#define LT_SLOTS 32  // partial-sum slots of the d emb_rel_k / d emb_rel_v reduction

// ------------------------------------------------------------------------------------ relative self-attention
// One wave per score row (b, h, i), four rows per workgroup.  dPd (the bgemm's dO.V^T) arrives in dS and leaves as
// the score gradient dS (unscaled by 1/sqrt(d)):
//   dPd[j] += dO_i . E_v[j - i + w] inside the band;  dP = dPd * keep * scale;  dS = P o (dP - sum_j P dP);
//   dS = 0 where the reference's masked_fill(-1e4) replaced the score (query or key padded).
// Also writes Pd = dropout(P) for the dV product, the band values of Pd and dS per row for the table gradients, and
// the band part of dq, sum_band dS[i,j] E_k[j-i+w] / sqrt(d), into dq (the dQ bgemm accumulates onto it).
__global__ __launch_bounds__(256) void lt_rel_rows_kernel(const float *__restrict__ P, const uint8_t *__restrict__ keep,
                                                          float keep_scale, const uint8_t *__restrict__ valid,
                                                          const float *__restrict__ dO, const float *__restrict__ emb_k,
                                                          const float *__restrict__ emb_v, float *__restrict__ dS,
                                                          float *__restrict__ Pd, float *__restrict__ bandS,
                                                          float *__restrict__ bandP, float *__restrict__ dq, int B, int H,
                                                          int L, int w)
{
    __shared__ float bt[4][LT_NREL], bs[4][LT_NREL], bp[4][LT_NREL];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t R = (size_t)B * H * L;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    const bool live = row < R;
    const int nrel = 2 * w + 1;
    const int i = live ? (int)(row % L) : 0;
    const int h = live ? (int)((row / L) % H) : 0;
    const int b = live ? (int)(row / ((size_t)L * H)) : 0;
    const long HD = (long)H * LT_D;
    const float rs = 1.f / sqrtf((float)LT_D);
    if (lane < LT_NREL) {
        bs[wave][lane] = 0.f;
        bp[wave][lane] = 0.f;
    }
    // band term dO_i . E_v[m]: lanes own channels lane and lane + 64
    float do0 = 0.f, do1 = 0.f;
    if (live) {
        const float *dob = dO + ((size_t)b * HD + (size_t)h * LT_D) * L + i;
        do0 = dob[(size_t)lane * L];
        do1 = dob[(size_t)(lane + 64) * L];
    }
    for (int m = 0; m < nrel; ++m) {
        const float s = mg_wave_sum(do0 * emb_v[m * LT_D + lane] + do1 * emb_v[m * LT_D + lane + 64]);
        if (lane == 0) bt[wave][m] = s;
    }
    __syncthreads();
    if (live) {
        const size_t off = row * L;
        const bool qv = valid[(size_t)b * L + i] != 0;
        float dot = 0.f;
        for (int j = lane; j < L; j += 64) {
            const int m = j - i + w;
            const bool band = m >= 0 && m < nrel;
            const float ks = keep ? (keep[off + j] ? keep_scale : 0.f) : 1.f;
            const float p = P[off + j];
            const float pd = p * ks;
            const float dp = (dS[off + j] + (band ? bt[wave][m] : 0.f)) * ks;
            dS[off + j] = dp;
            Pd[off + j] = pd;
            if (band) bp[wave][m] = pd;
            dot = fmaf(p, dp, dot);
        }
        dot = mg_wave_sum(dot);
        for (int j = lane; j < L; j += 64) {
            const int m = j - i + w;
            const bool ok = qv && valid[(size_t)b * L + j] != 0;
            const float s = ok ? P[off + j] * (dS[off + j] - dot) : 0.f;
            dS[off + j] = s;
            if (m >= 0 && m < nrel) bs[wave][m] = s;
        }
    }
    __syncthreads();
    if (live) {
        if (lane < nrel) {
            bandS[row * nrel + lane] = bs[wave][lane];
            bandP[row * nrel + lane] = bp[wave][lane];
        }
        float a0 = 0.f, a1 = 0.f;
        for (int m = 0; m < nrel; ++m) {
            a0 = fmaf(bs[wave][m], emb_k[m * LT_D + lane], a0);
            a1 = fmaf(bs[wave][m], emb_k[m * LT_D + lane + 64], a1);
        }
        float *dqb = dq + ((size_t)b * 3 * HD + (size_t)h * LT_D) * L + i;
        dqb[(size_t)lane * L] = a0 * rs;
        dqb[(size_t)(lane + 64) * L] = a1 * rs;
    }
}

// part[which][slot][m][d]: slot s sums rows s, s + 32, ...; which 0: bandS . q (d emb_rel_k before 1/sqrt(d)),
// which 1: bandP . dO (d emb_rel_v).  Grid (nrel, 2, LT_SLOTS / 2), two slots per workgroup.
__global__ __launch_bounds__(256) void lt_rel_table_part_kernel(const float *__restrict__ qkv,
                                                                const float *__restrict__ dO,
                                                                const float *__restrict__ bandS,
                                                                const float *__restrict__ bandP,
                                                                float *__restrict__ part, int B, int H, int L, int nrel)
{
    const int m = blockIdx.x, which = blockIdx.y, d = threadIdx.x & (LT_D - 1);
    const int slot = blockIdx.z * 2 + (threadIdx.x >> 7);
    const size_t R = (size_t)B * H * L;
    const long HD = (long)H * LT_D;
    const float *band = which ? bandP : bandS;
    float acc = 0.f;
    for (size_t r = slot; r < R; r += LT_SLOTS) {
        const int i = (int)(r % L), h = (int)((r / L) % H), b = (int)(r / ((size_t)L * H));
        const float x = which ? dO[((size_t)b * HD + (size_t)h * LT_D + d) * L + i]
                              : qkv[((size_t)b * 3 * HD + (size_t)h * LT_D + d) * L + i];
        acc = fmaf(band[r * nrel + m], x, acc);
    }
    part[(((size_t)which * LT_SLOTS + slot) * nrel + m) * LT_D + d] = acc;
}

__global__ __launch_bounds__(256) void lt_rel_table_sum_kernel(const float *__restrict__ part, float *__restrict__ d_ek,
                                                               float *__restrict__ d_ev, int nrel)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * nrel * LT_D) return;
    const int which = e / (nrel * LT_D), md = e % (nrel * LT_D);
    float s = 0.f;
    for (int slot = 0; slot < LT_SLOTS; ++slot) s += part[((size_t)which * LT_SLOTS + slot) * nrel * LT_D + md];
    if (which) d_ev[md] = s;
    else d_ek[md] = s * (1.f / sqrtf((float)LT_D));
}

extern "C" size_t mg_rel_attention_bwd_ws_floats(int B, int L, int n_head, int window)
{
    if (B <= 0 || L <= 0 || n_head <= 0 || window < 0 || window > LT_WMAX) return 0;
    const size_t R = (size_t)B * n_head * L, nrel = 2 * (size_t)window + 1;
    return 2 * R * L + 2 * R * nrel + 2 * (size_t)LT_SLOTS * nrel * LT_D;
}

extern "C" int mg_rel_attention_bwd(const float *qkv, const uint8_t *valid, const float *P, const uint8_t *keep,
                                    float keep_scale, const float *dOut, const float *emb_k, const float *emb_v,
                                    float *dqkv, float *d_emb_k, float *d_emb_v, float *ws, size_t ws_floats, int B,
                                    int L, int n_head, int d_head, int window, void *stream)
{
    if (!qkv || !valid || !P || !dOut || !emb_k || !emb_v || !dqkv || !d_emb_k || !d_emb_v || !ws) return MG_ERR_ARG;
    if (B <= 0 || L <= 0 || n_head <= 0 || d_head != LT_D || window < 0 || window > LT_WMAX) return MG_ERR_SHAPE;
    if (ws_floats < mg_rel_attention_bwd_ws_floats(B, L, n_head, window)) return MG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int H = n_head, d = LT_D, nrel = 2 * window + 1;
    const long HD = (long)H * d, bs = 3 * HD * L, hs = (long)d * L, pbs = (long)H * L * L, phs = (long)L * L;
    const size_t R = (size_t)B * H * L;
    float *dS = ws, *Pd = dS + R * L, *bandS = Pd + R * L, *bandP = bandS + R * nrel, *part = bandP + R * nrel;
    const float *q = qkv, *k = qkv + HD * L, *v = qkv + 2 * HD * L;
    float *dq = dqkv, *dk = dqkv + HD * L, *dv = dqkv + 2 * HD * L;
    const float rs = 1.f / sqrtf((float)d);
    // dPd[q,k] = sum_d dO[d,q] V[d,k]
    MG_TRY(mg_bgemm(dOut, v, dS, L, L, d, B, H, 1, L, HD * L, hs, L, 1, bs, hs, L, pbs, phs, 1.f, 0, stream));
    hipLaunchKernelGGL(lt_rel_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, P, keep, keep_scale, valid,
                       dOut, emb_k, emb_v, dS, Pd, bandS, bandP, dq, B, H, L, window);
    MG_LAUNCH_CHECK();
    // dV[d,k] = sum_q dO[d,q] Pd[q,k]
    MG_TRY(mg_bgemm(dOut, Pd, dv, d, L, L, B, H, L, 1, HD * L, hs, L, 1, pbs, phs, L, bs, hs, 1.f, 0, stream));
    // dQ[d,q] += sum_k K[d,k] dS[q,k] / sqrt(d);  dK[d,k] = sum_q Q[d,q] dS[q,k] / sqrt(d)
    MG_TRY(mg_bgemm(k, dS, dq, d, L, L, B, H, L, 1, bs, hs, 1, L, pbs, phs, L, bs, hs, rs, 1, stream));
    MG_TRY(mg_bgemm(q, dS, dk, d, L, L, B, H, L, 1, bs, hs, L, 1, pbs, phs, L, bs, hs, rs, 0, stream));
    hipLaunchKernelGGL(lt_rel_table_part_kernel, dim3(nrel, 2, LT_SLOTS / 2), dim3(256), 0, st, qkv, dOut, bandS, bandP,
                       part, B, H, L, nrel);
    MG_LAUNCH_CHECK();
    hipLaunchKernelGGL(lt_rel_table_sum_kernel, dim3(mg_cdiv(2 * nrel * d, 256)), dim3(256), 0, st, part, d_emb_k,
                       d_emb_v, nrel);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// ------------------------------------------------------------------------------------ word-to-phoneme attention
// One wave per row (h, b, i) of the head-major [H, B, Lq, Lk] tensors; G holds dA = dO.V^T (bgemm) and leaves as the
// score gradient (unscaled by 1/sqrt(d)):
//   dP = (dA + d_attn) * mapping + d_raw;  dP' = qmask * dP   (raw = softmax(s') * qmask, s' the logprob scores)
//   ds' = raw o (dP' - sum raw dP') + d_logprob
//   prior: ds = ds' - softmax(s) * sum ds', softmax(s) = exp(logprob - log(prior + 1e-8));  else ds = ds'
//   ds = 0 at padded keys (the masked_fill(-inf) passes nothing; it also keeps 0 * inf out of the sums).
__global__ __launch_bounds__(256) void lt_w2p_rows_kernel(float *__restrict__ G, const float *__restrict__ d_attn,
                                                          const float *__restrict__ d_raw,
                                                          const float *__restrict__ d_logp,
                                                          const float *__restrict__ raw,
                                                          const float *__restrict__ logprob,
                                                          const float *__restrict__ prior,
                                                          const uint8_t *__restrict__ mapping,
                                                          const uint8_t *__restrict__ qvalid,
                                                          const uint8_t *__restrict__ kvalid, int B, int H, int Lq,
                                                          int Lk)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t R = (size_t)H * B * Lq;
    const size_t row = (size_t)blockIdx.x * 4 + wave;
    if (row >= R) return;
    const int i = (int)(row % Lq), b = (int)((row / Lq) % B);
    const size_t off = row * Lk;
    const uint8_t *mp = mapping + ((size_t)b * Lq + i) * Lk;
    const uint8_t *kv = kvalid + (size_t)b * Lk;
    const float qm = qvalid[(size_t)b * Lq + i] ? 1.f : 0.f;
    float dot = 0.f;
    for (int j = lane; j < Lk; j += 64) {
        const float da = G[off + j] + (d_attn ? d_attn[off + j] : 0.f);
        const float dp = qm * ((mp[j] ? da : 0.f) + (d_raw ? d_raw[off + j] : 0.f));
        G[off + j] = dp;
        dot = fmaf(raw[off + j], dp, dot);
    }
    dot = mg_wave_sum(dot);
    float tot = 0.f;
    for (int j = lane; j < Lk; j += 64) {
        float s = raw[off + j] * (G[off + j] - dot) + (d_logp ? d_logp[off + j] : 0.f);
        if (!prior && !kv[j]) s = 0.f;
        G[off + j] = s;
        tot += s;
    }
    if (!prior) return;
    tot = mg_wave_sum(tot);
    const float *pb = prior + (size_t)b * Lk * Lq + i;
    for (int j = lane; j < Lk; j += 64) {
        float s = 0.f;
        if (kv[j]) s = G[off + j] - expf(logprob[off + j] - logf(pb[(size_t)j * Lq] + 1e-8f)) * tot;
        G[off + j] = s;
    }
}

extern "C" size_t mg_w2p_attention_bwd_ws_floats(int B, int Lq, int Lk, int n_head)
{
    if (B <= 0 || Lq <= 0 || Lk <= 0 || n_head <= 0) return 0;
    return (size_t)n_head * B * Lq * Lk;
}

extern "C" int mg_w2p_attention_bwd(const float *q, const float *kv, const uint8_t *key_valid,
                                    const uint8_t *query_valid, const uint8_t *mapping, const float *prior,
                                    const float *attn, const float *attn_raw, const float *logprob, const float *dOut,
                                    const float *d_attn, const float *d_raw, const float *d_logprob, float *dq,
                                    float *dkv, float *ws, size_t ws_floats, int B, int Lq, int Lk, int n_head,
                                    int d_head, void *stream)
{
    if (!q || !kv || !key_valid || !query_valid || !mapping || !attn || !attn_raw || !logprob || !dOut || !dq || !dkv ||
        !ws)
        return MG_ERR_ARG;
    if (B <= 0 || Lq <= 0 || Lk <= 0 || n_head <= 0 || d_head != LT_D) return MG_ERR_SHAPE;
    if (ws_floats < mg_w2p_attention_bwd_ws_floats(B, Lq, Lk, n_head)) return MG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int H = n_head, d = LT_D;
    const long HD = (long)H * d, qbs = HD * Lq, qhs = (long)d * Lq, kbs = 2 * HD * Lk, khs = (long)d * Lk;
    const long pbs = (long)Lq * Lk, phs = (long)B * Lq * Lk;
    const float *k = kv, *v = kv + HD * Lk;
    float *dk = dkv, *dv = dkv + HD * Lk, *G = ws;
    const float rs = 1.f / sqrtf((float)d);
    // dA[i,j] = sum_d dO[d,i] V[d,j]
    MG_TRY(mg_bgemm(dOut, v, G, Lq, Lk, d, B, H, 1, Lq, qbs, qhs, Lk, 1, kbs, khs, Lk, pbs, phs, 1.f, 0, stream));
    const size_t R = (size_t)H * B * Lq;
    hipLaunchKernelGGL(lt_w2p_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, G, d_attn, d_raw, d_logprob,
                       attn_raw, logprob, prior, mapping, query_valid, key_valid, B, H, Lq, Lk);
    MG_LAUNCH_CHECK();
    // dV[d,j] = sum_i dO[d,i] attn[i,j];  dQ[d,i] = sum_j K[d,j] ds[i,j] / sqrt(d);  dK[d,j] = sum_i Q[d,i] ds[i,j] / sqrt(d)
    MG_TRY(mg_bgemm(dOut, attn, dv, d, Lk, Lq, B, H, Lq, 1, qbs, qhs, Lk, 1, pbs, phs, Lk, kbs, khs, 1.f, 0, stream));
    MG_TRY(mg_bgemm(k, G, dq, d, Lq, Lk, B, H, Lk, 1, kbs, khs, 1, Lk, pbs, phs, Lq, qbs, qhs, rs, 0, stream));
    MG_TRY(mg_bgemm(q, G, dk, d, Lk, Lq, B, H, Lq, 1, qbs, qhs, Lk, 1, pbs, phs, Lk, kbs, khs, rs, 0, stream));
    return MG_OK;
}

// ------------------------------------------------------------------------------------ per-token glue
// dtable[r, c] = sum over tokens (b, l) with ids[b, l] == r (and valid, when given) of dout[b, c, l]; row skip_row
// (nn.Embedding's padding_idx, or -1) stays zero.  A thread per (row, channel) walks the tokens in order.
__global__ __launch_bounds__(256) void lt_embed_bwd_kernel(const int64_t *__restrict__ ids, const float *__restrict__ dout,
                                                           const uint8_t *__restrict__ valid, float *__restrict__ dtable,
                                                           int B, int L, int C, int skip_row)
{
    const int r = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    float acc = 0.f;
    if (r != skip_row) {
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l)
                if (ids[(size_t)b * L + l] == r && (!valid || valid[(size_t)b * L + l]))
                    acc += dout[((size_t)b * C + c) * L + l];
    }
    dtable[(size_t)r * C + c] = acc;
}

extern "C" int mg_embed_cm_bwd(const int64_t *ids, const float *dout, const uint8_t *valid, float *dtable, int B, int L,
                               int C, int n_rows, int skip_row, void *stream)
{
    if (!ids || !dout || !dtable) return MG_ERR_ARG;
    if (B <= 0 || L <= 0 || C <= 0 || n_rows <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(lt_embed_bwd_kernel, dim3(n_rows, mg_cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, ids, dout,
                       valid, dtable, B, L, C, skip_row);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// g[b,l] = dpred * valid * scale:  dh[b,c,l] = w[c] g[b,l] (blocks x >= C+1 of the grid), dw[c] = sum h[b,c,l] g[b,l]
// and db = sum g (blocks 0..C: a fixed-order strided sum and LDS tree per block).
__global__ __launch_bounds__(256) void lt_variance_head_bwd_kernel(const float *__restrict__ h, const float *__restrict__ wt,
                                                                   const uint8_t *__restrict__ valid, float scale,
                                                                   const float *__restrict__ dpred, float *__restrict__ dh,
                                                                   float *__restrict__ dw, float *__restrict__ db, int B,
                                                                   int C, int L)
{
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int n = B * L;
    if ((int)blockIdx.x > C) {
        const size_t e = (size_t)(blockIdx.x - C - 1) * 256 + tid;
        if (e >= (size_t)B * C * L) return;
        const int l = (int)(e % L), c = (int)((e / L) % C), b = (int)(e / ((size_t)C * L));
        const size_t t = (size_t)b * L + l;
        dh[e] = wt[c] * (valid[t] ? dpred[t] * scale : 0.f);
        return;
    }
    const int c = blockIdx.x;
    float acc = 0.f;
    for (int t = tid; t < n; t += 256) {
        const float g = valid[t] ? dpred[t] * scale : 0.f;
        const int b = t / L, l = t % L;
        acc = fmaf(c < C ? h[((size_t)b * C + c) * L + l] : 1.f, g, acc);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        if (c < C) dw[c] = red[0];
        else db[0] = red[0];
    }
}

extern "C" int mg_variance_head_bwd(const float *h, const float *weight, const uint8_t *valid, float scale,
                                    const float *dpred, float *dh, float *dweight, float *dbias, int B, int C, int L,
                                    void *stream)
{
    if (!h || !weight || !valid || !dpred || !dh || !dweight || !dbias) return MG_ERR_ARG;
    if (B <= 0 || C <= 0 || L <= 0) return MG_ERR_SHAPE;
    const int nb = C + 1 + mg_cdiv(B * C * L, 256);
    hipLaunchKernelGGL(lt_variance_head_bwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, h, weight, valid, scale,
                       dpred, dh, dweight, dbias, B, C, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// A thread per phoneme: dlogp[b,p] = dlogw[b,w] exp(logp[b,p] - logw[b,w]) for the word w < min(W, src_w_len) that
// holds p, 0 for phonemes outside every counted word.
__global__ __launch_bounds__(256) void lt_duration_head_bwd_kernel(const float *__restrict__ logp,
                                                                   const float *__restrict__ logw,
                                                                   const float *__restrict__ dlogw,
                                                                   const int64_t *__restrict__ wb,
                                                                   const int64_t *__restrict__ src_w_len,
                                                                   float *__restrict__ dlogp, int Tp, int Tw, int W)
{
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= Tp) return;
    const int64_t *wr = wb + (size_t)b * Tw;
    const int nw = (int)min((int64_t)min(Tw, W), src_w_len[b]);
    float g = 0.f;
    int64_t p0 = 0;
    for (int wi = 0; wi < nw; ++wi) {
        const int64_t p1 = p0 + wr[wi];
        if (p >= p0 && p < p1) {
            const size_t o = (size_t)b * W + wi;
            g = dlogw[o] * expf(logp[(size_t)b * Tp + p] - logw[o]);
            break;
        }
        p0 = p1;
    }
    dlogp[(size_t)b * Tp + p] = g;
}

extern "C" int mg_duration_head_bwd(const float *logp, const float *logw, const float *dlogw, const int64_t *wb,
                                    const int64_t *src_w_len, float *dlogp, int B, int Tp, int Tw, int W, void *stream)
{
    if (!logp || !logw || !dlogw || !wb || !src_w_len || !dlogp) return MG_ERR_ARG;
    if (B <= 0 || Tp <= 0 || Tw <= 0 || W <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(lt_duration_head_bwd_kernel, dim3(mg_cdiv(Tp, 256), B), dim3(256), 0, (hipStream_t)stream, logp,
                       logw, dlogw, wb, src_w_len, dlogp, Tp, Tw, W);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// 32 frames x 32 channels per workgroup: the batch sum in registers (b in order), transposed through LDS so that the
// [L, C] table gradient is written channel-contiguous.
__global__ __launch_bounds__(256) void lt_posenc_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ coef,
                                                            float *__restrict__ dtable, int B, int C, int L)
{
    __shared__ float t[32][33];
    const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tid = threadIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + u * 256, rc = e >> 5, rl = e & 31;      // channel-major read (l contiguous)
            const int l = l0 + rl, c = c0 + rc;
            if (l < L && c < C) acc[u] = fmaf(coef[(size_t)b * L + l], dout[((size_t)b * C + c) * L + l], acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + u * 256;
        t[e >> 5][e & 31] = acc[u];
    }
    __syncthreads();
    for (int e = tid; e < 1024; e += 256) {
        const int rl = e >> 5, rc = e & 31;                              // frame-major write (c contiguous)
        const int l = l0 + rl, c = c0 + rc;
        if (l < L && c < C) dtable[(size_t)l * C + c] = t[rc][rl];
    }
}

extern "C" int mg_posenc_add_bwd(const float *dout, const float *coef, float *dtable, int B, int C, int L, void *stream)
{
    if (!dout || !coef || !dtable) return MG_ERR_ARG;
    if (B <= 0 || C <= 0 || L <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(lt_posenc_bwd_kernel, dim3(mg_cdiv(L, 32), mg_cdiv(C, 32)), dim3(256), 0, (hipStream_t)stream,
                       dout, coef, dtable, B, C, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

__global__ __launch_bounds__(256) void lt_dropout_kernel(const float *__restrict__ x, const uint8_t *__restrict__ keep,
                                                         float scale, float *__restrict__ out, size_t n)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = keep[e] ? x[e] * scale : 0.f;
}

extern "C" int mg_dropout_apply(const float *x, const uint8_t *keep, float scale, float *out, size_t n, void *stream)
{
    if (!x || !keep || !out) return MG_ERR_ARG;
    if (n == 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(lt_dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, keep,
                       scale, out, n);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
