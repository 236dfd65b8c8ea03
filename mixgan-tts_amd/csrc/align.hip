// Forced aligner (mixgan_tts_amd/aligner.py; stands where the corpus chain calls the Montreal Forced Aligner, with no
// claim of parity with it): Gaussian emission scores, a left-to-right Viterbi pass per utterance, and the per-Gaussian
// moments of the hard-EM update.  tests/align_oracle.py states all three in float64 numpy.  No atomics anywhere: every
// output element is written by one thread, in an order fixed by its own row.
#include "common.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------ emissions
// ll[row, g] = sum_d (A[g, d] x^2 + Bm[g, d] x) + c[g]: the [rows, 2 D] x [2 D, G] product on v_mfma_f32_32x32x2f32.
// A workgroup owns ER x EC outputs, each of its four waves one 32 x 32 accumulator.  D is walked in chunks of EK: the
// chunk of the feature tile and of both tables is staged in LDS (row stride EK + 1: the 32 rows a wave reads at one k
// fall into 32 banks), zero where the row is past its utterance's frames, d >= D or g >= G, so an odd D and a ragged
// last column tile are padded here and not in the caller's arrays.  A k-step of the MFMA takes two d: the [x^2, x]
// operand is squared in registers, one MFMA against the A rows and one against the Bm rows.  An output element is one
// chain of fused multiply-adds in a fixed order (per pair of d, ascending: the two A x^2 terms, then the two Bm x terms)
// whatever else its tile holds, so a row's bits do not depend on its place.
constexpr int ER = 64, EC = 64, EK = 32, ELD = EK + 1;
static_assert(ER == EC && ER * EK % 256 == 0, "one staging loop fills the feature tile and both table tiles");

__global__ __launch_bounds__(256) void align_emissions_kernel(const float *__restrict__ x,
                                                              const int *__restrict__ n_frames, int B, int T, int D,
                                                              const float *__restrict__ A, const float *__restrict__ Bm,
                                                              const float *__restrict__ c, int G, float *__restrict__ ll)
{
    __shared__ float xs[ER * ELD];
    __shared__ float as[EC * ELD];
    __shared__ float bs[EC * ELD];
    __shared__ int valid[ER];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, hh = lane >> 5, r = lane & 31;
    const long rows = (long)B * T;
    const long row0 = (long)blockIdx.y * ER;
    const int g0 = blockIdx.x * EC;

    if (tid < ER) {
        const long row = row0 + tid;
        int ok = 0;
        if (row < rows) {
            const int b = (int)(row / T), t = (int)(row - (long)b * T);
            ok = t < n_frames[b];
        }
        valid[tid] = ok;
    }
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    for (int d0 = 0; d0 < D; d0 += EK) {
        // EK consecutive d of one row are consecutive in memory, in x and in both tables
#pragma unroll
        for (int i = 0; i < ER * EK / 256; ++i) {
            const int idx = tid + 256 * i, rr = idx / EK, dk = idx % EK;
            const int d = d0 + dk;
            float xv = 0.f, av = 0.f, bv = 0.f;
            if (d < D) {
                if (valid[rr]) xv = x[(size_t)(row0 + rr) * D + d];
                if (g0 + rr < G) {
                    av = A[(size_t)(g0 + rr) * D + d];
                    bv = Bm[(size_t)(g0 + rr) * D + d];
                }
            }
            xs[rr * ELD + dk] = xv;
            as[rr * ELD + dk] = av;
            bs[rr * ELD + dk] = bv;
        }
        __syncthreads();
        const float *xw = xs + (wm * 32 + r) * ELD + hh, *aw = as + (wn * 32 + r) * ELD + hh,
                    *bw = bs + (wn * 32 + r) * ELD + hh;
#pragma unroll
        for (int s = 0; s < EK / 2; ++s) {
            const float xv = xw[2 * s];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv * xv, aw[2 * s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, bw[2 * s], acc, 0, 0, 0);
        }
        __syncthreads();
    }

    const int g = g0 + wn * 32 + r;
    if (g < G) {
        const float cg = c[g];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rr = wm * 32 + 8 * (e >> 2) + 4 * hh + (e & 3);
            const long row = row0 + rr;
            if (row < rows) ll[(size_t)row * G + g] = valid[rr] ? acc[e] + cg : 0.f;
        }
    }
}

// ------------------------------------------------------------------ Viterbi
// Every float64 operation below is one addition or one comparison, in the order tests/align_oracle.py states, so the
// path equals the oracle's bit for bit: no contraction from here on.
#pragma clang fp contract(off)

constexpr int VS = 8;                            // consecutive states of one thread
constexpr int VMAXT = MG_ALIGN_MAX_S / VS;       // threads at the largest S
constexpr int BT_F = 12, BT_W = 5;               // backtrace: frames per block, half-words per frame (2 BT_F <= 8 (BT_W - 1))

__host__ __device__ inline int viterbi_words(int S) { return (S + VS - 1) / VS; }

// One workgroup per utterance, thread i owns the states 8 i .. 8 i + 7 and keeps their delta in registers.  Of the
// previous frame it needs, beyond its own, the last two delta of thread i - 1: those cross through LDS, in two buffers
// taken in turn, so one barrier per frame separates a frame's reads from the next frame's writes.  The eight
// back-pointers of a thread (0 stay, 1 advance, 2 skip; two bits each) are one half-word of the workspace,
// [B, T, ceil(S / 8)].  The emission scores of frame t + 1 are loaded before frame t is worked.
// Backtrace, by the first wave: a path falls by at most two states a frame, so the BT_F frames below frame hi can only
// need the half-words of the BT_W groups at and below the current state's; lane 5 f + q loads group top - q of frame
// hi - f, and the walk takes them from the lanes.
__global__ __launch_bounds__(VMAXT) void align_viterbi_kernel(const float *__restrict__ ll, const int *__restrict__ seq,
                                                              const uint8_t *__restrict__ skip,
                                                              const int *__restrict__ n_frames,
                                                              const int *__restrict__ n_states, int T, int S, int G,
                                                              int *__restrict__ durations, double *__restrict__ score,
                                                              int *__restrict__ ok, unsigned short *__restrict__ ws)
{
    __shared__ double edge[2][VMAXT][2];
    __shared__ double last[MG_ALIGN_MAX_S];
    __shared__ int dur[MG_ALIGN_MAX_S];
    __shared__ int end_state;
    const int tid = threadIdx.x, b = blockIdx.x, nthr = blockDim.x;
    const int SW = viterbi_words(S);
    int nf = n_frames[b], ns = n_states[b];
    nf = nf < 0 ? 0 : (nf > T ? T : nf);
    ns = ns < 0 ? 0 : (ns > S ? S : ns);
    const float *lrow = ll + (size_t)b * T * G;
    unsigned short *bp = ws + (size_t)b * T * SW;
    const double NEG = -INFINITY;

    for (int s = tid; s < MG_ALIGN_MAX_S; s += nthr) dur[s] = 0;
    if (nf == 0 || ns == 0) {      // block-uniform
        for (int s = tid; s < S; s += nthr) durations[(size_t)b * S + s] = 0;
        if (tid == 0) {
            score[b] = NEG;
            ok[b] = 0;
        }
        return;
    }

    int gid[VS];
    bool sk1[VS];      // skip[s - 1]: state s may be entered from s - 2
    const int s0 = tid * VS;
#pragma unroll
    for (int j = 0; j < VS; ++j) {
        const int s = s0 + j;
        int g = s < ns ? seq[(size_t)b * S + s] : 0;
        gid[j] = g < 0 ? 0 : (g >= G ? G - 1 : g);
        sk1[j] = s >= 1 && s < ns && skip[(size_t)b * S + s - 1] != 0;
    }

    float en[VS];
    double dl[VS];
#pragma unroll
    for (int j = 0; j < VS; ++j) en[j] = s0 + j < ns ? lrow[gid[j]] : 0.f;
#pragma unroll
    for (int j = 0; j < VS; ++j) {
        const int s = s0 + j;
        const bool open = s < ns && (s == 0 || (s == 1 && sk1[j]));
        dl[j] = open ? (double)en[j] : NEG;
    }
    if (nf > 1)
#pragma unroll
        for (int j = 0; j < VS; ++j) en[j] = s0 + j < ns ? lrow[(size_t)G + gid[j]] : 0.f;
    edge[0][tid][0] = dl[VS - 2];
    edge[0][tid][1] = dl[VS - 1];
    __syncthreads();

    for (int t = 1; t < nf; ++t) {
        float e[VS];
#pragma unroll
        for (int j = 0; j < VS; ++j) e[j] = en[j];
        if (t + 1 < nf)
#pragma unroll
            for (int j = 0; j < VS; ++j) en[j] = s0 + j < ns ? lrow[(size_t)(t + 1) * G + gid[j]] : 0.f;
        double p[VS + 2];
        p[0] = tid > 0 ? edge[(t - 1) & 1][tid - 1][0] : NEG;
        p[1] = tid > 0 ? edge[(t - 1) & 1][tid - 1][1] : NEG;
#pragma unroll
        for (int j = 0; j < VS; ++j) p[j + 2] = dl[j];
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < VS; ++j) {
            double best = p[j + 2];      // ties: stay, then advance, then skip
            unsigned arg = 0;
            if (p[j + 1] > best) {
                best = p[j + 1];
                arg = 1;
            }
            if (sk1[j] && p[j] > best) {
                best = p[j];
                arg = 2;
            }
            dl[j] = (double)e[j] + best;
            w |= arg << (2 * j);
        }
        if (tid < SW) bp[(size_t)t * SW + tid] = (unsigned short)w;
        edge[t & 1][tid][0] = dl[VS - 2];
        edge[t & 1][tid][1] = dl[VS - 1];
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < VS; ++j) last[s0 + j] = dl[j];
    __threadfence();      // the back-pointer half-words, read below by the first wave
    __syncthreads();
    if (tid == 0) {
        int se = ns - 1;
        if (ns >= 2 && skip[(size_t)b * S + ns - 1] != 0 && last[ns - 2] > last[ns - 1]) se = ns - 2;
        const double v = last[se];
        const int good = v > NEG;
        score[b] = v;
        ok[b] = good;
        end_state = good ? se : -1;
    }
    __syncthreads();
    int s = end_state;
    if (s >= 0 && tid < 64) {
        const int lane = tid;
        const int f = lane / BT_W, q = lane % BT_W;
        for (int hi = nf - 1; hi >= 1; hi -= BT_F) {
            const int top = s >> 3;
            const int tt = hi - f, grp = top - q;
            unsigned w = 0;
            if (f < BT_F && tt >= 1 && grp >= 0) w = bp[(size_t)tt * SW + grp];
            const int steps = hi < BT_F ? hi : BT_F;
            for (int i = 0; i < steps; ++i) {      // frame hi - i: count it, then the state of frame hi - i - 1
                if (lane == 0) dur[s] += 1;
                const unsigned wi = __shfl(w, i * BT_W + (top - (s >> 3)));
                s -= (int)(wi >> (2 * (s & 7)) & 3u);
                if (s < 0) s = 0;      // not reached on a finite path
            }
        }
        if (lane == 0) dur[s] += 1;      // frame 0
    }
    __syncthreads();
    for (int i = tid; i < S; i += nthr) durations[(size_t)b * S + i] = dur[i];
}

// ------------------------------------------------------------------ statistics
// One workgroup per Gaussian, thread d sums component d of the rows of the Gaussian's segment in list order: float64,
// the square of a float32 is exact in it, every sum is one chain.  Four rows are loaded ahead of their additions.
__global__ __launch_bounds__(MG_ALIGN_MAX_D) void align_stats_kernel(const float *__restrict__ x,
                                                                     const int *__restrict__ frame_index,
                                                                     const int *__restrict__ offsets, int D,
                                                                     double *__restrict__ sum,
                                                                     double *__restrict__ sumsq)
{
    const int g = blockIdx.x, d = threadIdx.x;
    if (d >= D) return;
    const int lo = offsets[g], hi = offsets[g + 1];
    double s1 = 0.0, s2 = 0.0;
    int i = lo;
    for (; i + 4 <= hi; i += 4) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = x[(size_t)frame_index[i + u] * D + d];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double dv = (double)v[u];
            s1 = s1 + dv;
            s2 = s2 + dv * dv;
        }
    }
    for (; i < hi; ++i) {
        const double dv = (double)x[(size_t)frame_index[i] * D + d];
        s1 = s1 + dv;
        s2 = s2 + dv * dv;
    }
    sum[(size_t)g * D + d] = s1;
    sumsq[(size_t)g * D + d] = s2;
}

}  // namespace

extern "C" int mg_align_emissions(const float *x, const int *n_frames, int B, int T, int D, const float *A,
                                  const float *Bm, const float *c, int G, float *ll, void *stream)
{
    if (!x || !n_frames || !A || !Bm || !c || !ll) return MG_ERR_ARG;
    if (B <= 0 || T <= 0 || D < 1 || D > MG_ALIGN_MAX_D || G < 1 || G > MG_ALIGN_MAX_G) return MG_ERR_SHAPE;
    const long tiles = ((long)B * T + ER - 1) / ER;
    if (tiles > 65535) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(align_emissions_kernel, dim3(mg_cdiv(G, EC), (unsigned)tiles), dim3(256), 0, (hipStream_t)stream,
                       x, n_frames, B, T, D, A, Bm, c, G, ll);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_align_viterbi_workspace_bytes(int B, int T, int S)
{
    if (B <= 0 || T <= 0 || S <= 0) return 0;
    return (size_t)B * (size_t)T * (size_t)viterbi_words(S) * sizeof(unsigned short);
}

extern "C" int mg_align_viterbi(const float *ll, const int *seq, const uint8_t *skip, const int *n_frames,
                                const int *n_states, int B, int T, int S, int G, int *durations, double *score, int *ok,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ll || !seq || !skip || !n_frames || !n_states || !durations || !score || !ok) return MG_ERR_ARG;
    if (B <= 0 || T < 1 || T > MG_ALIGN_MAX_T || S < 1 || S > MG_ALIGN_MAX_S || G < 1 || G > MG_ALIGN_MAX_G)
        return MG_ERR_SHAPE;
    if (!workspace || workspace_bytes < mg_align_viterbi_workspace_bytes(B, T, S)) return MG_ERR_WORKSPACE;
    const int threads = mg_cdiv(viterbi_words(S), 64) * 64;
    hipLaunchKernelGGL(align_viterbi_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, ll, seq, skip, n_frames,
                       n_states, T, S, G, durations, score, ok, (unsigned short *)workspace);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_align_stats(const float *x, const int *frame_index, const int *offsets, int G, int D, double *sum,
                              double *sumsq, void *stream)
{
    if (!x || !frame_index || !offsets || !sum || !sumsq) return MG_ERR_ARG;
    if (D < 1 || D > MG_ALIGN_MAX_D || G < 1 || G > MG_ALIGN_MAX_G) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(align_stats_kernel, dim3(G), dim3(MG_ALIGN_MAX_D), 0, (hipStream_t)stream, x, frame_index,
                       offsets, D, sum, sumsq);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
