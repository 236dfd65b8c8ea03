// Inference kernels of the LinguisticEncoder (model/linguistic_encoder.py, model/blocks.py) that the
// generic library kernels do not cover:
//   mg_rel_attention_fwd   RelativeSelfAttention.attention (blocks.py:1016-1123): windowed relative keys/values
//                          (mg_rel_attention_train_fwd: the same with attention dropout and the probabilities saved)
//   mg_w2p_attention_fwd   ScaledDotProductAttention inside WordToPhonemeAttention (blocks.py:695-768)
//   mg_embed_cm            nn.Embedding gather straight into the channel-major layout, pads zeroed
//   mg_variance_head       VariancePredictor.linear_layer + mask + control + bucketize + embedding add
//                          (linguistic_encoder.py:163-183, 419-478)
//   mg_duration_head       exp -> word sum -> log -> clamp(round(exp - 1) * d_control, 0) (linguistic_encoder.py:294-316)
//   mg_posenc_add          x + coef[:, :, None] * table[:L]                        (linguistic_encoder.py:201-220)
// The two attentions share one kernel: a workgroup owns ROWS queries of one (batch, head), keeps their full score
// rows in LDS (the key counts here are phonemes or words: hundreds, not thousands), takes an exact two-pass
// softmax per row (one wave per row) and streams V through LDS in 32-key chunks for the P.V product.
#include "common.h"

#define LE_D 128      // head width (encoder_hidden 256 / encoder_head 2)
#define LE_WMAX 8     // largest encoder_window_size
#define LE_VCH 32     // keys per V chunk staged in LDS
#define LE_LDS_MAX (64 * 1024)

static size_t le_lds_bytes(int rows, int Lk)
{
    return sizeof(float) * ((size_t)rows * LE_D + (size_t)rows * Lk + (size_t)LE_D * (LE_VCH + 1) +
                            (size_t)rows * (2 * LE_WMAX + 1));
}

// REL: RelativeSelfAttention (q, k, v are slices of one qkv tensor; x_mask in kvalid; -1e4 masking; relative terms
//      within |j - i| <= w).  !REL: word-to-phoneme attention (-inf key masking, optional ctc prior, query and
//      mapping masks, the three [H, B, Lq, Lk] probability / log-probability tensors written head-major).
// TRAIN (REL only): the softmax probabilities go to psave [B, H, L, L] (when not NULL) and the P of both products is
//      dropout(P) with the uint8 keep-mask [B, H, L, L] (when not NULL) -- `self.drop(p_attn)`, model/blocks.py:1059.
//      The inference instantiation (TRAIN = false) never reads the three extra arguments.
template <bool REL, int ROWS, bool TRAIN = false>
__global__ __launch_bounds__(256) void le_attention_kernel(
    const float *__restrict__ q, long q_bs, const float *__restrict__ k, const float *__restrict__ v, long kv_bs,
    int Lq, int Lk, int B, const uint8_t *__restrict__ qvalid, const uint8_t *__restrict__ kvalid,
    const float *__restrict__ emb_k, const float *__restrict__ emb_v, int w, const uint8_t *__restrict__ mapping,
    const float *__restrict__ prior, float *__restrict__ out, long out_bs, float *__restrict__ attn,
    float *__restrict__ attn_raw, float *__restrict__ logprob, const uint8_t *__restrict__ keep, float keep_scale,
    float *__restrict__ psave)
{
    static_assert(REL || !TRAIN, "the train form is the relative self-attention's");
    static_assert(ROWS % 4 == 0, "one softmax wave per row, four waves");
    extern __shared__ float le_sm[];
    float *qs = le_sm;                        // [D][ROWS]
    float *S = qs + ROWS * LE_D;              // [ROWS][Lk]: scores, then probabilities
    float *vs = S + (size_t)ROWS * Lk;        // [D][VCH + 1]
    float *rk = vs + LE_D * (LE_VCH + 1);     // [ROWS][2 WMAX + 1]: q . E_k / sqrt(d)
    const int tid = threadIdx.x, i0 = blockIdx.x * ROWS, h = blockIdx.y, b = blockIdx.z;
    const float temp = sqrtf((float)LE_D);    // the reference divides by sqrt(d_k), it does not multiply
    const int nrel = 2 * w + 1;

    const float *qb = q + (size_t)b * q_bs + (size_t)h * LE_D * Lq;
    for (int e = tid; e < ROWS * LE_D; e += 256) {
        const int d = e / ROWS, r = e % ROWS, i = i0 + r;
        qs[e] = i < Lq ? qb[(size_t)d * Lq + i] : 0.f;
    }
    __syncthreads();
    if (REL) {
        for (int e = tid; e < ROWS * nrel; e += 256) {
            const int r = e / nrel, m = e % nrel;
            float a = 0.f;
            for (int d = 0; d < LE_D; ++d) a = fmaf(qs[d * ROWS + r], emb_k[m * LE_D + d], a);
            rk[r * (2 * LE_WMAX + 1) + m] = a / temp;
        }
        __syncthreads();
    }

    // scores: a thread per key, ROWS accumulators
    const float *kb = k + (size_t)b * kv_bs + (size_t)h * LE_D * Lk;
    for (int j = tid; j < Lk; j += 256) {
        float acc[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
        for (int d = 0; d < LE_D; ++d) {
            const float kv = kb[(size_t)d * Lk + j];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) acc[r] = fmaf(qs[d * ROWS + r], kv, acc[r]);
        }
        const bool kval = kvalid[(size_t)b * Lk + j] != 0;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int i = i0 + r;
            float s = acc[r] / temp;
            if (REL) {
                const int m = j - i + w;
                if (m >= 0 && m < nrel) s += rk[r * (2 * LE_WMAX + 1) + m];
                if (i >= Lq || !kval || !qvalid[(size_t)b * Lq + i]) s = -1e4f;
            } else if (!kval) {
                s = -INFINITY;
            }
            S[(size_t)r * Lk + j] = s;
        }
    }
    __syncthreads();

    // softmax: wave r%4 takes row r
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < ROWS; r += 4) {
        const int i = i0 + r;
        if (i >= Lq) break;
        float *Sr = S + (size_t)r * Lk;
        float mx = -INFINITY;
        if (!REL && prior) {    // log_softmax(scores) + log(prior^T + 1e-8)
            for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, Sr[j]);
            mx = mg_wave_max(mx);
            float sum = 0.f;
            for (int j = lane; j < Lk; j += 64) sum += expf(Sr[j] - mx);
            const float lsum = logf(mg_wave_sum(sum));
            const float *pb = prior + (size_t)b * Lk * Lq + i;
            for (int j = lane; j < Lk; j += 64) Sr[j] = ((Sr[j] - mx) - lsum) + logf(pb[(size_t)j * Lq] + 1e-8f);
            mx = -INFINITY;
        }
        const size_t ob = (((size_t)h * B + b) * Lq + i) * Lk;
        for (int j = lane; j < Lk; j += 64) {
            const float s = Sr[j];
            if (!REL) logprob[ob + j] = s;
            mx = fmaxf(mx, s);
        }
        mx = mg_wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < Lk; j += 64) {
            const float e = expf(Sr[j] - mx);
            Sr[j] = e;
            sum += e;
        }
        sum = mg_wave_sum(sum);
        if (REL && TRAIN) {
            const size_t pb = (((size_t)b * gridDim.y + h) * Lq + i) * Lk;
            for (int j = lane; j < Lk; j += 64) {
                float p = Sr[j] / sum;
                if (psave) psave[pb + j] = p;
                if (keep) p = keep[pb + j] ? p * keep_scale : 0.f;
                Sr[j] = p;
            }
        } else if (REL) {
            for (int j = lane; j < Lk; j += 64) Sr[j] = Sr[j] / sum;
        } else {
            const float qm = qvalid[(size_t)b * Lq + i] ? 1.f : 0.f;
            const uint8_t *mp = mapping + ((size_t)b * Lq + i) * Lk;
            for (int j = lane; j < Lk; j += 64) {
                const float p = (Sr[j] / sum) * qm;
                const float a = p * (mp[j] ? 1.f : 0.f);
                attn_raw[ob + j] = p;
                attn[ob + j] = a;
                Sr[j] = a;
            }
        }
    }
    __syncthreads();

    // out[d, i] = sum_j P[i, j] V[d, j] (+ the band of P against E_v): a thread per (d, half of the rows)
    constexpr int RH = ROWS / 2;
    const int d = tid & (LE_D - 1), rg = tid >> 7;
    float acc[RH];
#pragma unroll
    for (int r = 0; r < RH; ++r) acc[r] = 0.f;
    const float *vb = v + (size_t)b * kv_bs + (size_t)h * LE_D * Lk;
    for (int j0 = 0; j0 < Lk; j0 += LE_VCH) {
        for (int e = tid; e < LE_D * LE_VCH; e += 256) {
            const int dd = e / LE_VCH, jj = e % LE_VCH, j = j0 + jj;
            vs[dd * (LE_VCH + 1) + jj] = j < Lk ? vb[(size_t)dd * Lk + j] : 0.f;
        }
        __syncthreads();
        const int jn = min(LE_VCH, Lk - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const float vv = vs[d * (LE_VCH + 1) + jj];
#pragma unroll
            for (int r = 0; r < RH; ++r) acc[r] = fmaf(S[(size_t)(rg * RH + r) * Lk + j0 + jj], vv, acc[r]);
        }
        __syncthreads();
    }
    float *obase = out + (size_t)b * out_bs + (size_t)(h * LE_D + d) * Lq;
#pragma unroll
    for (int r = 0; r < RH; ++r) {
        const int rr = rg * RH + r, i = i0 + rr;
        if (i >= Lq) continue;
        float o = acc[r];
        if (REL) {
            float rel = 0.f;
            for (int m = 0; m < nrel; ++m) {
                const int j = i + m - w;
                if (j >= 0 && j < Lk) rel = fmaf(S[(size_t)rr * Lk + j], emb_v[m * LE_D + d], rel);
            }
            o += rel;
        }
        obase[i] = o;
    }
}

// The one place the kernel's form is chosen (le_attention_launch switches on it): 16 query rows per workgroup while
// their score rows fit LE_LDS_MAX (Lk <= 615), else 4 (Lk <= 2895), else 0: no form, MG_ERR_SHAPE.
extern "C" int mg_le_attention_rows(int Lk)
{
    if (Lk <= 0) return 0;
    if (le_lds_bytes(16, Lk) <= LE_LDS_MAX) return 16;
    if (le_lds_bytes(4, Lk) <= LE_LDS_MAX) return 4;
    return 0;
}

template <bool REL, bool TRAIN = false>
static int le_attention_launch(const float *q, long q_bs, const float *k, const float *v, long kv_bs, int Lq, int Lk,
                               int B, int H, const uint8_t *qvalid, const uint8_t *kvalid, const float *emb_k,
                               const float *emb_v, int w, const uint8_t *mapping, const float *prior, float *out,
                               long out_bs, float *attn, float *attn_raw, float *logprob, hipStream_t st,
                               const uint8_t *keep = nullptr, float keep_scale = 1.f, float *psave = nullptr)
{
    const int rows = mg_le_attention_rows(Lk);
    if (rows == 16) {
        hipLaunchKernelGGL((le_attention_kernel<REL, 16, TRAIN>), dim3(mg_cdiv(Lq, 16), H, B), dim3(256),
                           le_lds_bytes(16, Lk), st, q, q_bs, k, v, kv_bs, Lq, Lk, B, qvalid, kvalid, emb_k, emb_v, w,
                           mapping, prior, out, out_bs, attn, attn_raw, logprob, keep, keep_scale, psave);
    } else if (rows == 4) {
        hipLaunchKernelGGL((le_attention_kernel<REL, 4, TRAIN>), dim3(mg_cdiv(Lq, 4), H, B), dim3(256),
                           le_lds_bytes(4, Lk), st, q, q_bs, k, v, kv_bs, Lq, Lk, B, qvalid, kvalid, emb_k, emb_v, w,
                           mapping, prior, out, out_bs, attn, attn_raw, logprob, keep, keep_scale, psave);
    } else {
        return MG_ERR_SHAPE;
    }
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_rel_attention_fwd(const float *qkv, const uint8_t *valid, const float *emb_k, const float *emb_v,
                                    float *out, int B, int L, int n_head, int d_head, int window, void *stream)
{
    if (!qkv || !valid || !emb_k || !emb_v || !out) return MG_ERR_ARG;
    if (B <= 0 || L <= 0 || n_head <= 0 || d_head != LE_D || window < 0 || window > LE_WMAX) return MG_ERR_SHAPE;
    const long HD = (long)n_head * LE_D;
    return le_attention_launch<true>(qkv, 3 * HD * L, qkv + HD * L, qkv + 2 * HD * L, 3 * HD * L, L, L, B, n_head,
                                     valid, valid, emb_k, emb_v, window, nullptr, nullptr, out, HD * L, nullptr,
                                     nullptr, nullptr, (hipStream_t)stream);
}

// Train form: keep [B, H, L, L] uint8 or NULL (no dropout), P [B, H, L, L] (the softmax before dropout) or NULL
// (nothing saved: a train-mode forward under no_grad).
extern "C" int mg_rel_attention_train_fwd(const float *qkv, const uint8_t *valid, const float *emb_k,
                                          const float *emb_v, const uint8_t *keep, float keep_scale, float *out,
                                          float *P, int B, int L, int n_head, int d_head, int window, void *stream)
{
    if (!qkv || !valid || !emb_k || !emb_v || !out) return MG_ERR_ARG;
    if (B <= 0 || L <= 0 || n_head <= 0 || d_head != LE_D || window < 0 || window > LE_WMAX) return MG_ERR_SHAPE;
    const long HD = (long)n_head * LE_D;
    return le_attention_launch<true, true>(qkv, 3 * HD * L, qkv + HD * L, qkv + 2 * HD * L, 3 * HD * L, L, L, B,
                                           n_head, valid, valid, emb_k, emb_v, window, nullptr, nullptr, out, HD * L,
                                           nullptr, nullptr, nullptr, (hipStream_t)stream, keep, keep_scale, P);
}

extern "C" int mg_w2p_attention_fwd(const float *q, const float *kv, const uint8_t *key_valid,
                                    const uint8_t *query_valid, const uint8_t *mapping, const float *prior, float *out,
                                    float *attn, float *attn_raw, float *logprob, int B, int Lq, int Lk, int n_head,
                                    int d_head, void *stream)
{
    if (!q || !kv || !key_valid || !query_valid || !mapping || !out || !attn || !attn_raw || !logprob) return MG_ERR_ARG;
    if (B <= 0 || Lq <= 0 || Lk <= 0 || n_head <= 0 || d_head != LE_D) return MG_ERR_SHAPE;
    const long HD = (long)n_head * LE_D;
    return le_attention_launch<false>(q, HD * Lq, kv, kv + HD * Lk, 2 * HD * Lk, Lq, Lk, B, n_head, query_valid,
                                      key_valid, nullptr, nullptr, 0, mapping, prior, out, HD * Lq, attn, attn_raw,
                                      logprob, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ per-token glue
__global__ __launch_bounds__(256) void le_embed_cm_kernel(const int64_t *__restrict__ ids, const float *__restrict__ table,
                                                          const uint8_t *__restrict__ valid, float *__restrict__ out,
                                                          int C, int L, int n_rows)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (e >= (size_t)C * L) return;
    const int c = (int)(e / L), l = (int)(e % L);
    const int64_t id = ids[(size_t)b * L + l];
    const bool ok = valid[(size_t)b * L + l] && id >= 0 && id < n_rows;
    out[(size_t)b * C * L + e] = ok ? table[(size_t)id * C + c] : 0.f;
}

extern "C" int mg_embed_cm(const int64_t *ids, const float *table, const uint8_t *valid, float *out, int B, int L,
                           int C, int n_rows, void *stream)
{
    if (!ids || !table || !valid || !out) return MG_ERR_ARG;
    if (B <= 0 || L <= 0 || C <= 0 || n_rows <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(le_embed_cm_kernel, dim3(mg_cdiv(C * L, 256), B), dim3(256), 0, (hipStream_t)stream, ids, table,
                       valid, out, C, L, n_rows);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// a thread per frame: pred = (w . h + bias) * valid (* control without a target); bucketize the target or the
// prediction (right=False: the count of bins strictly below the value); x[:, l] += emb[bucket]
__global__ __launch_bounds__(256) void le_variance_head_kernel(
    const float *__restrict__ hcm, const float *__restrict__ wt, const float *__restrict__ bias,
    const uint8_t *__restrict__ valid, float control, const float *__restrict__ target, const float *__restrict__ bins,
    int n_bounds, const float *__restrict__ emb, float *__restrict__ pred, float *__restrict__ x, int C, int L)
{
    const int l = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (l >= L) return;
    const float *hb = hcm + (size_t)b * C * L + l;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(wt[c], hb[(size_t)c * L], a);
    float p = (a + bias[0]) * (valid[(size_t)b * L + l] ? 1.f : 0.f);
    if (!target) p = p * control;
    pred[(size_t)b * L + l] = p;
    if (!emb) return;
    const float val = target ? target[(size_t)b * L + l] : p;
    int lo = 0, hi = n_bounds;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (bins[mid] < val) lo = mid + 1;
        else hi = mid;
    }
    const float *er = emb + (size_t)lo * C;
    float *xb = x + (size_t)b * C * L + l;
    for (int c = 0; c < C; ++c) xb[(size_t)c * L] += er[c];
}

extern "C" int mg_variance_head(const float *h, const float *weight, const float *bias, const uint8_t *valid,
                                float control, const float *target, const float *bins, int n_bounds, const float *emb,
                                float *pred, float *x, int B, int C, int L, void *stream)
{
    if (!h || !weight || !bias || !valid || !pred || (emb && (!bins || !x))) return MG_ERR_ARG;
    if (B <= 0 || C <= 0 || L <= 0 || (emb && n_bounds <= 0)) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(le_variance_head_kernel, dim3(mg_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream, h, weight,
                       bias, valid, control, target, bins, n_bounds, emb, pred, x, C, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// a thread per word: log_w = log(sum over the word's phonemes of exp(log_p)) (-inf for words past src_w_len);
// dur = the word sum of the integer target, or long(max(rint(exp(log_w) - 1) * d_control, 0))
__global__ __launch_bounds__(256) void le_duration_head_kernel(const float *__restrict__ logp,
                                                               const int64_t *__restrict__ target,
                                                               const int64_t *__restrict__ wb,
                                                               const int64_t *__restrict__ src_w_len, float d_control,
                                                               float *__restrict__ logw, int64_t *__restrict__ dur,
                                                               int Tp, int Tw, int W)
{
    const int b = blockIdx.y, wi = blockIdx.x * 256 + threadIdx.x;
    if (wi >= W) return;
    const int64_t *wr = wb + (size_t)b * Tw;
    const int nw = (int)min((int64_t)min(Tw, W), src_w_len[b]);
    float s = 0.f;
    int64_t ts = 0;
    if (wi < nw) {
        int64_t p0 = 0;
        for (int i = 0; i < wi; ++i) p0 += wr[i];
        const int64_t p1 = min(p0 + wr[wi], (int64_t)Tp);
        for (int64_t p = p0; p < p1; ++p) {
            s += expf(logp[(size_t)b * Tp + p]);
            if (target) ts += target[(size_t)b * Tp + p];
        }
    }
    const float lw = logf(s);
    logw[(size_t)b * W + wi] = lw;
    if (target) {
        dur[(size_t)b * W + wi] = ts;
    } else {
        const float r = rintf(expf(lw) - 1.f) * d_control;
        dur[(size_t)b * W + wi] = (int64_t)fmaxf(r, 0.f);
    }
}

extern "C" int mg_duration_head(const float *logp, const int64_t *target, const int64_t *wb, const int64_t *src_w_len,
                                float d_control, float *logw, int64_t *dur, int B, int Tp, int Tw, int W, void *stream)
{
    if (!logp || !wb || !src_w_len || !logw || !dur) return MG_ERR_ARG;
    if (B <= 0 || Tp <= 0 || Tw <= 0 || W <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(le_duration_head_kernel, dim3(mg_cdiv(W, 256), B), dim3(256), 0, (hipStream_t)stream, logp,
                       target, wb, src_w_len, d_control, logw, dur, Tp, Tw, W);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// 32 frames x 32 channels per workgroup through LDS: out[b, c, l] = x[b, l, c] (or x[b, c, l]) + coef[b, l] * table[l, c]
__global__ __launch_bounds__(256) void le_posenc_add_kernel(const float *__restrict__ x, int x_rowmajor,
                                                            const float *__restrict__ coef,
                                                            const float *__restrict__ table, float *__restrict__ out,
                                                            int C, int L)
{
    __shared__ float tx[32][33], tt[32][33];
    const int l0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z, tid = threadIdx.x;
    for (int e = tid; e < 1024; e += 256) {
        const int rl = e >> 5, rc = e & 31;     // frame-major read (c contiguous)
        const int l = l0 + rl, c = c0 + rc;
        const bool in = l < L && c < C;
        tt[rl][rc] = in ? table[(size_t)l * C + c] : 0.f;
        if (x_rowmajor) tx[rl][rc] = in ? x[((size_t)b * L + l) * C + c] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < 1024; e += 256) {
        const int rc = e >> 5, rl = e & 31;     // channel-major write (l contiguous)
        const int l = l0 + rl, c = c0 + rc;
        if (l >= L || c >= C) continue;
        const size_t o = ((size_t)b * C + c) * L + l;
        const float xv = x_rowmajor ? tx[rl][rc] : x[o];
        out[o] = xv + coef[(size_t)b * L + l] * tt[rl][rc];
    }
}

extern "C" int mg_posenc_add(const float *x, int x_rowmajor, const float *coef, const float *table, float *out, int B,
                             int C, int L, void *stream)
{
    if (!x || !coef || !table || !out) return MG_ERR_ARG;
    if (B <= 0 || C <= 0 || L <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(le_posenc_add_kernel, dim3(mg_cdiv(L, 32), mg_cdiv(C, 32), B), dim3(256), 0,
                       (hipStream_t)stream, x, x_rowmajor, coef, table, out, C, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
