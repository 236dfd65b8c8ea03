// Objective synthesis metrics (mixgan_tts_amd/metrics.py): the cepstra of a log-mel and a
// dynamic-time-warping pass with its back-trace.  tests/metrics_ref.py states all of it in float64 numpy.  No atomics
// anywhere: every output element is written by one thread, in an order fixed by its own pair, so a pair's bits do not
// depend on its place in the batch or on the padding around it.
#include "common.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------ cepstra
// out[b, t, k - 1] = sqrt(2 / M) sum_m mel[b, t, m] cos(pi / M (m + 1/2) k), k = 1 .. n_coef.  A workgroup takes
// CEP_FRAMES frames of one row.  The cosine table sits in LDS bin-major, [M][n_coef]: the lanes of a wave hold
// consecutive k of one frame, so they read consecutive table words and one mel value between them.  The angle is
// reduced in integers, (2 m + 1) k mod 4 M, before the float64 cosine: the table is the float32 rounding of the exact
// value whatever M and k.
constexpr int CEP_FRAMES = 64;

__global__ __launch_bounds__(256) void mel_cepstra_kernel(const float *__restrict__ mel,
                                                          const int *__restrict__ n_frames, int T, int M, int n_coef,
                                                          float *__restrict__ out)
{
    extern __shared__ float tab[];
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * CEP_FRAMES;
    int nf = n_frames[b];
    nf = nf < 0 ? 0 : (nf > T ? T : nf);
    if (t0 < nf)      // block-uniform
        for (int e = tid; e < M * n_coef; e += 256) {
            const int m = e / n_coef, k = e % n_coef + 1;
            const int r = (2 * m + 1) * k % (4 * M);
            tab[e] = (float)cos(M_PI * (double)r / (double)(2 * M));
        }
    __syncthreads();
    const float scale = (float)sqrt(2.0 / (double)M);
    for (int o = tid; o < CEP_FRAMES * n_coef; o += 256) {
        const int t = t0 + o / n_coef, k = o % n_coef;
        if (t >= T) break;
        float acc = 0.f;
        if (t < nf) {
            const float *row = mel + ((size_t)b * T + t) * M;
            for (int m = 0; m < M; ++m) acc = fmaf(row[m], tab[m * n_coef + k], acc);
            acc *= scale;
        }
        out[((size_t)b * T + t) * n_coef + k] = acc;
    }
}

// ------------------------------------------------------------------ DTW
// Workspace of a batch, in 4-byte words: the back-pointers [B][ceil(Tb / 16)][Ta], sixteen two-bit codes of one row i
// per word (0: from (i-1, j-1), 1: from (i-1, j), 2: from (i, j-1)); then the operands feature-major,
// aT [B][MG_DTW_MAX_D][Ta] and bT [B][MG_DTW_MAX_D][Tb], of which a pair fills its first D planes.
constexpr int DTW_THREADS = 1024;
constexpr int DTW_ROWS = MG_DTW_MAX_T / DTW_THREADS;      // rows i of one thread at the largest Ta
static_assert(DTW_ROWS * DTW_THREADS == MG_DTW_MAX_T, "a thread's rows cover the largest Ta");

__host__ __device__ inline size_t dtw_bp_words(int Ta, int Tb) { return (size_t)((Tb + 15) / 16) * (size_t)Ta; }

// One workgroup per pair sweeps the anti-diagonals i + j = d.  Thread tid owns the rows i = tid + r blockDim.x, so on
// diagonal d its column is j = d - i: one step to the right per diagonal, and the sixteen codes of a back-pointer word
// are gathered in a register and stored once.  Three diagonals of Dacc roll through LDS indexed by i: diagonal d is
// written while d - 1 and d - 2 are read, and d + 1 overwrites d - 2, so one barrier per diagonal separates them.
// The local costs are computed from the feature-major copies the workgroup makes first -- lanes of consecutive i read
// consecutive a and (descending) consecutive b, where the row-major operands would be read with a stride of D floats
// -- and DTW_U diagonals at a time: the costs of a thread's next DTW_U cells do not depend on the recurrence, so their
// loads are in flight together and a diagonal's step is LDS reads, two comparisons and a barrier.  A cost is the
// same chain of operations whatever the batch.  A cell with one predecessor takes it whatever the values, so the
// back-trace cannot leave the grid on NaN input.
constexpr int DTW_U = 8;

__global__ __launch_bounds__(DTW_THREADS) void dtw_forward_kernel(const float *__restrict__ a,
                                                                  const float *__restrict__ b,
                                                                  const int *__restrict__ a_len,
                                                                  const int *__restrict__ b_len, int Ta, int Tb, int D,
                                                                  float *__restrict__ total, unsigned *__restrict__ bp,
                                                                  float *__restrict__ aT, float *__restrict__ bT)
{
    __shared__ float diag[3][MG_DTW_MAX_T];
    const int tid = threadIdx.x, nthr = blockDim.x, pair = blockIdx.x;
    int n = a_len[pair], m = b_len[pair];
    n = n < 0 ? 0 : (n > Ta ? Ta : n);
    m = m < 0 ? 0 : (m > Tb ? Tb : m);
    if (n == 0 || m == 0) {      // block-uniform
        if (tid == 0) total[pair] = 0.f;
        return;
    }
    a += (size_t)pair * Ta * D;
    b += (size_t)pair * Tb * D;
    aT += (size_t)pair * MG_DTW_MAX_D * Ta;
    bT += (size_t)pair * MG_DTW_MAX_D * Tb;
    bp += (size_t)pair * dtw_bp_words(Ta, Tb);
    for (int e = tid; e < n * D; e += nthr) aT[(size_t)(e % D) * Ta + e / D] = a[e];
    for (int e = tid; e < m * D; e += nthr) bT[(size_t)(e % D) * Tb + e / D] = b[e];
    __threadfence_block();
    __syncthreads();

    unsigned w[DTW_ROWS];
    float c[DTW_ROWS][DTW_U];
#pragma unroll
    for (int r = 0; r < DTW_ROWS; ++r) w[r] = 0u;

    const int nd = n + m - 1;
    for (int d0 = 0; d0 < nd; d0 += DTW_U) {
        // the costs of the cells (i, d0 - i) .. (i, d0 + DTW_U - 1 - i); a column outside [0, m) is clamped into it
        // for the loads and its cost is never used
#pragma unroll
        for (int r = 0; r < DTW_ROWS; ++r) {
            const int i = tid + r * nthr, jlo = d0 - i;
            if (i < n && jlo + DTW_U > 0 && jlo < m) {
                int jc[DTW_U];
                float s[DTW_U];
#pragma unroll
                for (int u = 0; u < DTW_U; ++u) {
                    const int j = jlo + u;
                    jc[u] = j < 0 ? 0 : (j > m - 1 ? m - 1 : j);
                    s[u] = 0.f;
                }
                for (int k = 0; k < D; ++k) {
                    const float av = aT[(size_t)k * Ta + i];
                    const float *bk = bT + (size_t)k * Tb;
#pragma unroll
                    for (int u = 0; u < DTW_U; ++u) {
                        const float df = av - bk[jc[u]];
                        s[u] = fmaf(df, df, s[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < DTW_U; ++u) c[r][u] = sqrtf(s[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < DTW_U; ++u) {
            const int d = d0 + u;      // past the last diagonal no cell is in range
            float *cur = diag[d % 3];
            const float *p1 = diag[(d + 2) % 3], *p2 = diag[(d + 1) % 3];      // diagonals d - 1 and d - 2
#pragma unroll
            for (int r = 0; r < DTW_ROWS; ++r) {
                const int i = tid + r * nthr, j = d - i;
                if (i < n && j >= 0 && j < m) {
                    float best = 0.f;
                    unsigned code = 0u;
                    if (i == 0) {
                        if (j > 0) {
                            best = p1[0];
                            code = 2u;
                        }
                    } else if (j == 0) {
                        best = p1[i - 1];
                        code = 1u;
                    } else {      // ties: the diagonal, then (i - 1, j), then (i, j - 1)
                        best = p2[i - 1];
                        const float up = p1[i - 1], left = p1[i];
                        if (up < best) {
                            best = up;
                            code = 1u;
                        }
                        if (left < best) {
                            best = left;
                            code = 2u;
                        }
                    }
                    const float v = c[r][u] + best;
                    cur[i] = v;
                    w[r] |= code << (2 * (j & 15));
                    if ((j & 15) == 15 || j == m - 1) {
                        bp[(size_t)(j >> 4) * Ta + i] = w[r];
                        w[r] = 0u;
                    }
                    if (i == n - 1 && j == m - 1) total[pair] = v;
                }
            }
            __syncthreads();
        }
    }
}

// One wave per pair walks back from (a_len - 1, b_len - 1), every lane holding the same cell.  A step goes up by at
// most one row and left by at most one column, so the next 16 steps at least stay inside the 32 rows at and above the
// cell and the two word columns at and left of it: lane 2 q + p loads the word of row i - q, word column (j >> 4) - p,
// and the walk takes its words from the lanes until it leaves that window -- one round trip to memory per window, not
// per step.  Lane 0 writes the cells from the end of the pair's path rows; then the wave moves them to the front, 64 at
// a time (a chunk's destination lies below every later chunk's source, and a chunk is loaded whole before it is
// stored), and fills the rest with -1.
__global__ __launch_bounds__(64) void dtw_backtrace_kernel(const int *__restrict__ a_len, const int *__restrict__ b_len,
                                                           int Ta, int Tb, const unsigned *__restrict__ bp,
                                                           int *__restrict__ path_len, int *path)
{
    const int lane = threadIdx.x, pair = blockIdx.x;
    const int P = Ta + Tb - 1;
    int n = a_len[pair], m = b_len[pair];
    n = n < 0 ? 0 : (n > Ta ? Ta : n);
    m = m < 0 ? 0 : (m > Tb ? Tb : m);
    int *prow = path ? path + (size_t)pair * P * 2 : nullptr;
    int len = 0;
    if (n > 0 && m > 0) {      // block-uniform, and so is everything in the walk
        bp += (size_t)pair * dtw_bp_words(Ta, Tb);
        int i = n - 1, j = m - 1;
        bool done = false;
        while (!done) {
            const int i0 = i, w0 = j >> 4;
            const int ri = i0 - (lane >> 1), rw = w0 - (lane & 1);
            unsigned held = 0u;
            if (ri >= 0 && rw >= 0) held = bp[(size_t)rw * Ta + ri];
            for (;;) {
                if (prow && lane == 0) {
                    prow[2 * (P - 1 - len)] = i;
                    prow[2 * (P - 1 - len) + 1] = j;
                }
                ++len;
                if (i == 0 && j == 0) {
                    done = true;
                    break;
                }
                const unsigned word = __shfl(held, 2 * (i0 - i) + (w0 - (j >> 4)));
                unsigned code = (word >> (2 * (j & 15))) & 3u;
                if (i == 0) code = 2u;      // what the forward pass wrote there; kept so that no word can lead outside
                else if (j == 0) code = 1u;
                if (code != 2u) --i;
                if (code != 1u) --j;
                if (i0 - i >= 32 || w0 - (j >> 4) >= 2) break;      // the next cell's word is outside the window
            }
        }
    }
    if (lane == 0) path_len[pair] = len;
    if (!prow) return;
    __threadfence();      // lane 0's cells, read below by the whole wave
    const int off = P - len;
    if (off > 0)
        for (int base = 0; base < len; base += 64) {
            const int k = base + lane;
            int vi = -1, vj = -1;
            if (k < len) {
                vi = prow[2 * (off + k)];
                vj = prow[2 * (off + k) + 1];
            }
            __threadfence_block();
            if (k < len) {
                prow[2 * k] = vi;
                prow[2 * k + 1] = vj;
            }
        }
    for (int k = 2 * len + lane; k < 2 * P; k += 64) prow[k] = -1;
}

}  // namespace

extern "C" int mg_mel_cepstra(const float *mel, const int *n_frames, int B, int T, int M, int n_coef, float *out,
                              void *stream)
{
    if (!mel || !n_frames || !out) return MG_ERR_ARG;
    if (B <= 0 || B > 65535 || T <= 0 || M < 2 || M > MG_CEPSTRA_MAX_M || n_coef < 1 || n_coef >= M) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(mel_cepstra_kernel, dim3(mg_cdiv(T, CEP_FRAMES), B), dim3(256),
                       (size_t)M * n_coef * sizeof(float), (hipStream_t)stream, mel, n_frames, T, M, n_coef, out);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_dtw_workspace_bytes(int B, int Ta, int Tb)
{
    if (B <= 0 || Ta <= 0 || Tb <= 0) return 0;
    return (size_t)B * (dtw_bp_words(Ta, Tb) + (size_t)MG_DTW_MAX_D * ((size_t)Ta + (size_t)Tb)) * 4;
}

extern "C" int mg_dtw(const float *a, const float *b, const int *a_len, const int *b_len, int B, int Ta, int Tb, int D,
                      float *total, int *path_len, int *path, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!a || !b || !a_len || !b_len || !total || !path_len) return MG_ERR_ARG;
    if (B <= 0 || Ta < 1 || Ta > MG_DTW_MAX_T || Tb < 1 || Tb > MG_DTW_MAX_T || D < 1 || D > MG_DTW_MAX_D)
        return MG_ERR_SHAPE;
    if (!workspace || workspace_bytes < mg_dtw_workspace_bytes(B, Ta, Tb)) return MG_ERR_WORKSPACE;
    unsigned *bp = (unsigned *)workspace;
    float *aT = (float *)(bp + (size_t)B * dtw_bp_words(Ta, Tb));
    float *bT = aT + (size_t)B * MG_DTW_MAX_D * Ta;
    const int threads = Ta >= DTW_THREADS ? DTW_THREADS : mg_cdiv(Ta, 64) * 64;
    hipLaunchKernelGGL(dtw_forward_kernel, dim3(B), dim3(threads), 0, (hipStream_t)stream, a, b, a_len, b_len, Ta, Tb, D,
                       total, bp, aT, bT);
    MG_LAUNCH_CHECK();
    hipLaunchKernelGGL(dtw_backtrace_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a_len, b_len, Ta, Tb,
                       (const unsigned *)bp, path_len, path);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
