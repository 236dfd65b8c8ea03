// HiFi-GAN multi-scale discriminator (Kong et al. 2020, DiscriminatorS): grouped strided K = 41 convolutions on
// v_mfma_f32_32x32x2_f32 (forward, polyphase data gradient, weight gradient), the one-input-channel first layer on the
// VALU, and AvgPool1d(4, 2, 2).  C ABI: include/mixgan_hip.h, "HiFi-GAN multi-scale discriminator".
//
// MFMA operand maps (32x32x2, f32): lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]; result register
// r of lane l is C[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col l & 31].  Every kernel below puts FRAMES (or weight
// columns) on the B / C columns, so that a wave's 32 lanes read 32 consecutive floats of LDS and store 128 contiguous
// bytes.
#include "common.h"
#include "gconv_c4.h"

namespace {

constexpr int GC_K = 41;
static_assert(GC_K == C4_K, "one kernel size for every grouped form");

__device__ __forceinline__ int gc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// ---------------------------------------------------------------------------------------------------------------
// forward.  One workgroup = (frame tile, group, n), four waves.  The group's input window is staged once,
// deinterleaved by phase: sample p of the window (global position t0 s - pad + p) of channel ci sits at
// win[ci][p % S][p / S], so the B fragment of tap k (frames j = 0..31 -> p = j S + k) is 32 consecutive floats of phase
// row k % S from offset k / S.  Weights stream from L2 in fragment order.  NT frames per workgroup: 128 (each wave 32
// frames, all row blocks) unless the window would pass 64 KB of LDS, then 64 (two frame blocks x two row blocks).
// ---------------------------------------------------------------------------------------------------------------
template <int CIG, int S>
constexpr int gc_fwd_nt() { return CIG * S * (128 + (GC_K - 1) / S) * 4 <= 65536 ? 128 : 64; }

template <int CIG, int COG, int S>
__global__ __launch_bounds__(256) void gc_fwd_kernel(const float *__restrict__ in, const float *__restrict__ packed,
                                                     const float *__restrict__ bias, float *__restrict__ out, int Ci,
                                                     int Lin, int Co, int Lout, int pad, int act, float slope)
{
    constexpr int NT = gc_fwd_nt<CIG, S>(), MB = (COG + 31) / 32, NB = NT / 32, MBW = MB * NB / 4;
    constexpr int WP = NT + (GC_K - 1) / S, SPAN = S * WP, QT = CIG / 2;
    static_assert(MB * NB % 4 == 0 && MBW >= 1 && CIG % 2 == 0, "four waves share the tile evenly");
    __shared__ float win[CIG * SPAN];
    const int g = blockIdx.y, n = blockIdx.z, t0 = blockIdx.x * NT;
    const long g0 = (long)t0 * S - pad;
    const float *src = in + ((long)n * Ci + (long)g * CIG) * Lin;
    for (int e = threadIdx.x; e < CIG * SPAN; e += 256) {
        const int ci = e / SPAN, p = e % SPAN;
        const long gp = g0 + p;
        win[ci * SPAN + (p % S) * WP + p / S] = (gp >= 0 && gp < Lin) ? src[(long)ci * Lin + gp] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int nb = wave % NB, mb0 = (wave / NB) * MBW;
    f32x16 acc[MBW];
#pragma unroll
    for (int m = 0; m < MBW; ++m)
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    const float *wp = packed + ((long)g * MB + mb0) * (GC_K * QT * 64) + lane;
    const float *bw = win + h * SPAN + nb * 32 + r;
    for (int k = 0; k < GC_K; ++k) {
        const float *bk = bw + (k % S) * WP + k / S;
        const float *wk = wp + k * QT * 64;
#pragma unroll 8
        for (int q = 0; q < QT; ++q) {
            const float b = bk[q * 2 * SPAN];
#pragma unroll
            for (int m = 0; m < MBW; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wk[(m * GC_K * QT + q) * 64], b, acc[m], 0, 0, 0);
        }
    }
    const int t = t0 + nb * 32 + r;
    if (t >= Lout) return;
#pragma unroll
    for (int m = 0; m < MBW; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = (mb0 + m) * 32 + gc_row(i, lane);
            if (co < COG) {
                const int c = g * COG + co;
                float v = acc[m][i] + (bias ? bias[c] : 0.f);
                if (act == MG_ACT_LRELU) v = v > 0.f ? v : v * slope;
                out[((long)n * Co + c) * Lout + t] = v;
            }
        }
}

// fragment-order packs (layouts: the header)
__global__ void gc_pack_fwd_kernel(const float *__restrict__ w, float *__restrict__ packed, int CIG, int COG, int G)
{
    const int QT = CIG / 2, MB = (COG + 31) / 32;
    const long total = (long)G * MB * GC_K * QT * 64;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += gridDim.x * 256l) {
        const int lane = i % 64;
        long j = i / 64;
        const int q = j % QT;
        j /= QT;
        const int k = j % GC_K;
        j /= GC_K;
        const int mb = j % MB, g = j / MB;
        const int co = mb * 32 + (lane & 31), ci = 2 * q + (lane >> 5);
        packed[i] = co < COG ? w[((long)(g * COG + co) * CIG + ci) * GC_K + k] : 0.f;
    }
}

// taps of phase f are k = f + S j, j < gc_jn(f); the dgrad pack orders taps by (f, j)
__host__ __device__ inline int gc_jn(int f, int S) { return f < GC_K ? (GC_K - f + S - 1) / S : 0; }
__host__ __device__ inline int gc_tap_base(int f, int S)
{
    int b = 0;
    for (int i = 0; i < f; ++i) b += gc_jn(i, S);
    return b;
}

__global__ void gc_pack_dgrad_kernel(const float *__restrict__ w, float *__restrict__ packed, int CIG, int COG, int S, int G)
{
    const int QD = COG / 2, MB = (CIG + 31) / 32;
    const long total = (long)G * MB * GC_K * QD * 64;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += gridDim.x * 256l) {
        const int lane = i % 64;
        long j = i / 64;
        const int q = j % QD;
        j /= QD;
        int tp = j % GC_K;      // position in (phase, j) order
        j /= GC_K;
        const int mb = j % MB, g = j / MB;
        int f = 0;
        while (tp >= gc_jn(f, S)) tp -= gc_jn(f++, S);
        const int k = f + S * tp;
        const int ci = mb * 32 + (lane & 31), co = 2 * q + (lane >> 5);
        packed[i] = ci < CIG ? w[((long)(g * COG + co) * CIG + ci) * GC_K + k] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// data gradient, polyphase.  With m + pad = S u + f, dx_f[ci, u] = sum_{co, j} w[co, ci, f + S j] dy[co, u - j]: a stride-1
// convolution over dy per phase f.  One workgroup = 128 consecutive input positions of (group, n) = 128 / S values of u x S
// phases; wave w takes phase w % S and the 32-u block w / S.  dy rows are staged once: dyw[co][i] = dy[co, u0 - (J - 1) + i],
// J = ceil(K / S).
// ---------------------------------------------------------------------------------------------------------------
template <int CIG, int COG, int S>
__global__ __launch_bounds__(256) void gc_dgrad_kernel(const float *__restrict__ dy, const float *__restrict__ packed,
                                                       const float *__restrict__ map, const float *__restrict__ add,
                                                       float *__restrict__ dx, int Ci, int Lin, int Co, int Lout, int pad,
                                                       float slope)
{
    constexpr int NU = 128 / S, J = (GC_K + S - 1) / S, WD = NU + J - 1, QD = COG / 2, MB = (CIG + 31) / 32;
    static_assert(COG % 2 == 0 && (S == 1 || S == 2 || S == 4), "");
    __shared__ float dyw[COG * WD];
    const int g = blockIdx.y, n = blockIdx.z, u0 = blockIdx.x * NU;
    const float *src = dy + ((long)n * Co + (long)g * COG) * Lout;
    for (int e = threadIdx.x; e < COG * WD; e += 256) {
        const int co = e / WD, l = u0 - (J - 1) + e % WD;
        dyw[e] = (l >= 0 && l < Lout) ? src[(long)co * Lout + l] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int f = wave % S, ub = wave / S;
    const int jn = gc_jn(f, S), tb = gc_tap_base(f, S);
    f32x16 acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
        for (int i = 0; i < 16; ++i) acc[m][i] = 0.f;
    const float *wp = packed + (long)g * MB * (GC_K * QD * 64) + lane;
    const float *bw = dyw + h * WD + ub * 32 + r + (J - 1);
    for (int j = 0; j < jn; ++j) {
        const float *wk = wp + (tb + j) * QD * 64;
#pragma unroll 8
        for (int q = 0; q < QD; ++q) {
            const float b = bw[q * 2 * WD - j];
#pragma unroll
            for (int m = 0; m < MB; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(wk[(m * GC_K * QD + q) * 64], b, acc[m], 0, 0, 0);
        }
    }
    const long mpos = (long)S * (u0 + ub * 32 + r) + f - pad;
    if (mpos < 0 || mpos >= Lin) return;
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ci = m * 32 + gc_row(i, lane);
            if (ci < CIG) {
                const long idx = ((long)n * Ci + g * CIG + ci) * Lin + mpos;
                float v = acc[m][i];
                if (add) v += add[idx];
                if (map) v *= map[idx] > 0.f ? 1.f : slope;
                dx[idx] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient.  Per group a GEMM dw[co][c] = sum_{n,l} dy[co, l] x[ci(c), l S + k(c) - pad] over the flat weight
// column c = ci K + k.  A workgroup owns 16 column blocks of 32 (wave w: blocks 4 w .. 4 w + 3), all row blocks, and a
// range of (n, 64-frame) chunks.  Per chunk it stages dy [Cog][64] (row stride 65: the A fragment walks rows) and the x
// window of the <= 14 channels its columns touch, row stride ROW = 64 S + 41.  ROW = 41 mod 32, so the B fragment's address
// (ci - ci_lo) ROW + k + l S maps the 32 consecutive columns of a block onto 32 consecutive banks whatever (ci, k) they
// straddle: the tap is an address offset, and no read conflicts.
// ---------------------------------------------------------------------------------------------------------------
constexpr int GW_LT = 64, GW_CBW = 16, GW_XR = 14;

template <int CIG, int COG, int S>
__global__ __launch_bounds__(256) void gc_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                       float *__restrict__ scratch, int N, int Ci, int Lin, int Co, int Lout,
                                                       int pad, int cps)
{
    constexpr int MB = (COG + 31) / 32, ROW = GW_LT * S + GC_K, NC = CIG * GC_K, NCBT = (NC + 31) / 32;
    constexpr int XR = CIG < GW_XR ? CIG : GW_XR, DR = GW_LT + 1;
    __shared__ float dyl[MB * 32 * DR];
    __shared__ float xl[XR * ROW];
    const int g = blockIdx.y, z = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int ci_lo = blockIdx.x * (GW_CBW * 32) / GC_K;
    const int cb0 = blockIdx.x * GW_CBW + wave * 4;
    int boff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = (cb0 + i) * 32 + r;
        c = c < NC ? c : NC - 1;
        boff[i] = (c / GC_K - ci_lo) * ROW + c % GC_K + h * S;
    }
    f32x16 acc[MB][4];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            for (int e = 0; e < 16; ++e) acc[m][i][e] = 0.f;
    const int lchunks = (Lout + GW_LT - 1) / GW_LT, total = N * lchunks;
    const int c_end = min(total, (z + 1) * cps);
    for (int ch = z * cps; ch < c_end; ++ch) {
        const int n = ch / lchunks, l0 = (ch % lchunks) * GW_LT;
        const float *dsrc = dy + ((long)n * Co + (long)g * COG) * Lout;
        for (int e = threadIdx.x; e < MB * 32 * GW_LT; e += 256) {
            const int co = e / GW_LT, i = e % GW_LT;
            dyl[co * DR + i] = (co < COG && l0 + i < Lout) ? dsrc[(long)co * Lout + l0 + i] : 0.f;
        }
        const float *xsrc = x + ((long)n * Ci + (long)g * CIG) * Lin;
        const long gp0 = (long)l0 * S - pad;
        for (int e = threadIdx.x; e < XR * ROW; e += 256) {
            const int ci = ci_lo + e / ROW;
            const long gp = gp0 + e % ROW;
            xl[e] = (ci < CIG && gp >= 0 && gp < Lin) ? xsrc[(long)ci * Lin + gp] : 0.f;
        }
        __syncthreads();
        if (cb0 < NCBT) {
#pragma unroll 4
            for (int st = 0; st < GW_LT / 2; ++st) {
                float a[MB], b[4];
#pragma unroll
                for (int m = 0; m < MB; ++m) a[m] = dyl[(m * 32 + r) * DR + 2 * st + h];
#pragma unroll
                for (int i = 0; i < 4; ++i) b[i] = xl[boff[i] + 2 * st * S];
#pragma unroll
                for (int m = 0; m < MB; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[m][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[i], acc[m][i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float *dst = scratch + (long)z * Co * NC + (long)g * COG * NC;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = (cb0 + i) * 32 + r;
        if (c >= NC) continue;
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = m * 32 + gc_row(e, lane);
                if (co < COG) dst[(long)co * NC + c] = acc[m][i][e];
            }
    }
}

// out[i] = sum_z part[z][i], z ascending
__global__ void gc_sum_splits_kernel(const float *__restrict__ part, float *__restrict__ out, long n, int nsplit)
{
    for (long i = blockIdx.x * 256l + threadIdx.x; i < n; i += gridDim.x * 256l) {
        float s = part[i];
        for (int z = 1; z < nsplit; ++z) s += part[(long)z * n + i];
        out[i] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the first layer: Conv1d(1, Co, K <= 16, stride 1)
// ---------------------------------------------------------------------------------------------------------------
constexpr int C1_KMAX = 16, C1_CO_PER_BLOCK = 32;

// thread = one frame, blockIdx.z = 32 output rows: the K input samples sit in registers, the weights are wave-uniform
__global__ __launch_bounds__(256) void c1_fwd_kernel(const float *__restrict__ in, const float *__restrict__ w,
                                                     const float *__restrict__ bias, float *__restrict__ out, int L, int Lout,
                                                     int Co, int K, int pad, int act, float slope)
{
    const int n = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Lout) return;
    float xs[C1_KMAX];
#pragma unroll
    for (int k = 0; k < C1_KMAX; ++k) {
        const int p = t + k - pad;
        xs[k] = (k < K && p >= 0 && p < L) ? in[(long)n * L + p] : 0.f;
    }
    const int co_end = min(Co, (int)(blockIdx.z + 1) * C1_CO_PER_BLOCK);
    for (int co = blockIdx.z * C1_CO_PER_BLOCK; co < co_end; ++co) {
        float v = bias ? bias[co] : 0.f;
#pragma unroll
        for (int k = 0; k < C1_KMAX; ++k)
            if (k < K) v = fmaf(w[co * K + k], xs[k], v);
        if (act == MG_ACT_LRELU) v = v > 0.f ? v : v * slope;
        out[((long)n * Co + co) * Lout + t] = v;
    }
}

// a workgroup = C1_DG_TILE consecutive samples of one n: each of its four waves takes all of them, four per lane, and a
// quarter of every 32-row slab of dy; the four partial sums are added in wave order at the end.  A slab passes through LDS
// with each element loaded once: tile[r][i] = dy[co0 + r, m0 + i + pad - (C1_KMAX - 1)], so that sample m0 + 4 lane + o takes
// tap k from i = 4 lane + o + (C1_KMAX - 1) - k -- 20 consecutive floats per lane and row, five aligned ds_read_b128, indexed
// at compile time whatever K is.  Small tiles on purpose: the whole job is a few hundred thousand samples, and 8 KB of
// loads per wave and slab in flight at once is what hides their latency.
constexpr int C1_DG_TILE = 256, C1_DG_ROWS = 32, C1_DG_STRIDE = C1_DG_TILE + 16;
static_assert(C1_DG_ROWS * C1_DG_STRIDE % 256 == 0 && 4 * C1_DG_TILE <= C1_DG_ROWS * C1_DG_STRIDE, "");

__global__ __launch_bounds__(256) void c1_dgrad_kernel(const float *__restrict__ dy, const float *__restrict__ w,
                                                       float *__restrict__ dx, int L, int Lout, int Co, int K, int pad)
{
    __shared__ __attribute__((aligned(16))) float tile[C1_DG_ROWS * C1_DG_STRIDE];
    const int n = blockIdx.y, m0 = blockIdx.x * C1_DG_TILE, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long l0 = (long)m0 + pad - (C1_KMAX - 1);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int co0 = 0; co0 < Co; co0 += C1_DG_ROWS) {
#pragma unroll
        for (int it = 0; it < C1_DG_ROWS * C1_DG_STRIDE / 256; ++it) {
            const int e = it * 256 + t, r = e / C1_DG_STRIDE;
            const long l = l0 + e % C1_DG_STRIDE;
            tile[e] = (co0 + r < Co && l >= 0 && l < Lout) ? dy[((long)n * Co + co0 + r) * Lout + l] : 0.f;
        }
        __syncthreads();
        for (int rr = 0; rr < C1_DG_ROWS / 4; ++rr) {
            const int r = wave * (C1_DG_ROWS / 4) + rr;
            if (co0 + r >= Co) break;      // wave-uniform
            float v[20];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                const f32x4 x4 = *reinterpret_cast<const f32x4 *>(&tile[r * C1_DG_STRIDE + 4 * lane + 4 * q]);
                v[4 * q] = x4[0], v[4 * q + 1] = x4[1], v[4 * q + 2] = x4[2], v[4 * q + 3] = x4[3];
            }
            const float *wr = w + (co0 + r) * K;
#pragma unroll
            for (int k = 0; k < C1_KMAX; ++k)
                if (k < K) {
                    const float wk = wr[k];
#pragma unroll
                    for (int o = 0; o < 4; ++o) s[o] = fmaf(wk, v[o + (C1_KMAX - 1) - k], s[o]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) tile[wave * C1_DG_TILE + 4 * lane + o] = s[o];
    __syncthreads();
    const int m = m0 + t;
    if (m < L)
        dx[(long)n * L + m] = ((tile[t] + tile[C1_DG_TILE + t]) + tile[2 * C1_DG_TILE + t]) + tile[3 * C1_DG_TILE + t];
}

// blockIdx.x = output row, blockIdx.y = split of the (n, l) range; each thread keeps K + 1 sums (taps and the bias), the
// block adds them by a fixed tree; part[split][co][C1_KMAX + 1]
__global__ __launch_bounds__(256) void c1_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                       float *__restrict__ part, int N, int L, int Lout, int Co, int K,
                                                       int pad, int per)
{
    __shared__ float red[4][C1_KMAX + 1];
    const int co = blockIdx.x, z = blockIdx.y;
    const long total = (long)N * Lout, end = min(total, (long)(z + 1) * per);
    float s[C1_KMAX + 1];
#pragma unroll
    for (int k = 0; k <= C1_KMAX; ++k) s[k] = 0.f;
    for (long e = (long)z * per + threadIdx.x; e < end; e += 256) {
        const int n = e / Lout, l = e % Lout;
        const float d = dy[((long)n * Co + co) * Lout + l];
        s[C1_KMAX] += d;
#pragma unroll
        for (int k = 0; k < C1_KMAX; ++k) {
            const int p = l + k - pad;
            if (k < K && p >= 0 && p < L) s[k] = fmaf(d, x[(long)n * L + p], s[k]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= C1_KMAX; ++k) {
        float v = s[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x <= C1_KMAX)
        part[((long)z * Co + co) * (C1_KMAX + 1) + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void c1_wgrad_finalize_kernel(const float *__restrict__ part, float *__restrict__ dw, float *__restrict__ db,
                                         int Co, int K, int nsplit)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Co * (C1_KMAX + 1)) return;
    const int co = i / (C1_KMAX + 1), k = i % (C1_KMAX + 1);
    float s = 0.f;
    for (int z = 0; z < nsplit; ++z) s += part[(long)z * Co * (C1_KMAX + 1) + i];
    if (k < K) dw[co * K + k] = s;
    else if (k == C1_KMAX && db) db[co] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// AvgPool1d(4, 2, padding PAD): window i = samples 2 i - PAD .. 2 i - PAD + 3 within [0, L).  COUNT_PAD: a window
// divides by 4 (HiFi-GAN, PAD 2); otherwise by its in-range count (MelGAN, PAD 1, count_include_pad=False)
// ---------------------------------------------------------------------------------------------------------------
template <int PAD, bool COUNT_PAD>
__device__ __forceinline__ float pool_rcp(int i, int L)
{
    if constexpr (COUNT_PAD) return 0.25f;
    const int lo = 2 * i - PAD < 0 ? 0 : 2 * i - PAD, hi = 2 * i - PAD + 3 > L - 1 ? L - 1 : 2 * i - PAD + 3;
    return 1.f / (float)(hi - lo + 1);
}

template <int PAD, bool COUNT_PAD>
__global__ void avgpool_fwd_kernel(const float *__restrict__ in, float *__restrict__ out, long rows, int L, int Lout)
{
    const long total = rows * Lout;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const long rrow = e / Lout;
        const int i = e % Lout;
        const float *src = in + rrow * L;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int p = 2 * i - PAD + t;
            if (p >= 0 && p < L) s += src[p];
        }
        out[e] = s * pool_rcp<PAD, COUNT_PAD>(i, L);
    }
}

// Sample m lies in windows i - 1 and i, i = (m + PAD) / 2.  COUNT_PAD scales the SUM of the two taps, once: the
// results are pinned bit for bit, and 0.25f * (a + b) and a * 0.25f + b * 0.25f differ where a product is subnormal
template <int PAD, bool COUNT_PAD>
__global__ void avgpool_bwd_kernel(const float *__restrict__ dy, float *__restrict__ dx, long rows, int L, int Lout)
{
    const long total = rows * L;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const long rrow = e / L;
        const int m = e % L, i = (m + PAD) / 2;
        const float *src = dy + rrow * Lout;
        float s = 0.f;
        if (i >= 1 && i - 1 < Lout) s += COUNT_PAD ? src[i - 1] : src[i - 1] * pool_rcp<PAD, false>(i - 1, L);
        if (i < Lout) s += COUNT_PAD ? src[i] : src[i] * pool_rcp<PAD, false>(i, L);
        dx[e] = COUNT_PAD ? 0.25f * s : s;
    }
}

int blocks_for(long n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

// ---------------------------------------------------------------------------------------------------------------
// ReflectionPad1d(p) and its fold-back
// ---------------------------------------------------------------------------------------------------------------
__global__ void reflect_pad_fwd_kernel(const float *__restrict__ in, float *__restrict__ out, long rows, int T, int p)
{
    const int Tp = T + 2 * p;
    const long total = rows * Tp;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const long rrow = e / Tp;
        int j = (int)(e % Tp) - p;
        j = j < 0 ? -j : (j >= T ? 2 * (T - 1) - j : j);
        out[e] = in[rrow * T + j];
    }
}

__global__ void reflect_pad_bwd_kernel(const float *__restrict__ dy, float *__restrict__ dx, long rows, int T, int p)
{
    const int Tp = T + 2 * p;
    const long total = rows * T;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const long rrow = e / T;
        const int m = e % T;
        const float *src = dy + rrow * Tp;
        float s = src[m + p];
        if (m >= 1 && m <= p) s += src[p - m];
        if (m >= T - 1 - p && m <= T - 2) s += src[p + 2 * (T - 1) - m];
        dx[e] = s;
    }
}

// ---- which (Cig, Cog, K, s) exist: one list for the size queries, the checks and the launchers.  Cig = 4 forms run the
// kernels of gconv_c4.h, the others the MFMA kernels above.
#define GC_FORMS(X) X(32, 32, 2) X(8, 16, 2) X(16, 32, 4) X(32, 64, 4) X(64, 64, 1) X(4, 16, 4) X(4, 4, 4)

template <int CIG, int COG, int S>
void gc_launch_fwd(hipStream_t st, const float *in, const float *packed, const float *bias, float *out, int N, int Ci,
                   int Lin, int Co, int Lout, int pad, int groups, int act, float slope)
{
    if constexpr (CIG == C4_CIG) {
        static_assert(S == C4_S, "");
        hipLaunchKernelGGL((c4_fwd_kernel<COG>), dim3(mg_cdiv(Lout, C4F_NT), mg_cdiv(groups, c4_gpb<COG>()), N), dim3(256),
                           0, st, in, packed, bias, out, Ci, Lin, Co, Lout, pad, groups, act, slope);
    } else {
        hipLaunchKernelGGL((gc_fwd_kernel<CIG, COG, S>), dim3(mg_cdiv(Lout, gc_fwd_nt<CIG, S>()), groups, N), dim3(256), 0,
                           st, in, packed, bias, out, Ci, Lin, Co, Lout, pad, act, slope);
    }
}

template <int CIG, int COG, int S>
void gc_launch_dgrad(hipStream_t st, const float *dy, const float *packed, const float *map, const float *add, float *dx,
                     int N, int Ci, int Lin, int Co, int Lout, int pad, int groups, float slope)
{
    // m + pad = s u + f for m in [0, Lin): u up to (Lin - 1 + pad) / s
    const int umax = (int)(((long)Lin - 1 + pad) / S);
    if constexpr (CIG == C4_CIG) {
        hipLaunchKernelGGL((c4_dgrad_kernel<COG>), dim3(umax / c4d_nu<COG>() + 1, mg_cdiv(groups, c4_gpb<COG>()), N),
                           dim3(256), 0, st, dy, packed, map, add, dx, Ci, Lin, Co, Lout, pad, groups, slope);
    } else {
        // a workgroup takes 128 / s values of u
        hipLaunchKernelGGL((gc_dgrad_kernel<CIG, COG, S>), dim3(umax / (128 / S) + 1, groups, N), dim3(256), 0, st, dy,
                           packed, map, add, dx, Ci, Lin, Co, Lout, pad, slope);
    }
}

bool gc_form_ok(int Cig, int Cog, int K, int s)
{
    if (K != GC_K) return false;
#define X(a, b, c) \
    if (Cig == a && Cog == b && s == c) return true;
    GC_FORMS(X)
#undef X
    return false;
}

// common argument checks of the three grouped entry points; MG_OK when (Ci, Co, K, s, G, Lin, Lout, pad) is a launchable form
int gc_check(int N, int Ci, int Lin, int Co, int Lout, int K, int s, int pad, int G)
{
    if (N <= 0 || N > 65535 || Ci <= 0 || Co <= 0 || Lin <= 0 || Lout <= 0 || pad < 0 || G <= 0 || G > 65535 || s <= 0)
        return MG_ERR_SHAPE;
    if (Ci % G || Co % G || !gc_form_ok(Ci / G, Co / G, K, s)) return MG_ERR_SHAPE;
    if ((long)Lin + 2l * pad < K || (long)Lout != ((long)Lin + 2l * pad - K) / s + 1) return MG_ERR_SHAPE;
    if ((long)N * Ci * Lin >= (1l << 40) || (long)Lin * s >= (1l << 30)) return MG_ERR_SHAPE;
    return MG_OK;
}

int gw_colchunks(int Cig) { return mg_cdiv(mg_cdiv(Cig * GC_K, 32), GW_CBW); }

// splits of the (n, 64-frame chunk) range of the weight gradient: about 1024 workgroups, at most 64 partial copies
int gw_nsplit(int N, int Lout, int Cig, int Cog, int G)
{
    if (Cig == C4_CIG) return c4w_nsplit(N, Lout, Cog, G);
    const long chunks = (long)N * mg_cdiv(Lout, GW_LT);
    long n = 1024 / ((long)G * gw_colchunks(Cig));
    n = n < 1 ? 1 : n > 64 ? 64 : n;
    return (int)(n > chunks ? chunks : n);
}

template <int CIG, int COG, int S>
void gc_launch_wgrad(hipStream_t st, const float *dy, const float *x, float *scratch, int N, int Ci, int Lin, int Co,
                     int Lout, int pad, int groups, int nsplit)
{
    if constexpr (CIG == C4_CIG) {
        hipLaunchKernelGGL((c4_wgrad_kernel<COG>), dim3(mg_cdiv(groups, c4_gpb<COG>()), nsplit), dim3(256), 0, st, dy, x,
                           scratch, N, Ci, Lin, Co, Lout, pad, groups, mg_cdiv(N * mg_cdiv(Lout, C4W_LT), nsplit));
    } else {
        hipLaunchKernelGGL((gc_wgrad_kernel<CIG, COG, S>), dim3(gw_colchunks(CIG), groups, nsplit), dim3(256), 0, st, dy, x,
                           scratch, N, Ci, Lin, Co, Lout, pad, mg_cdiv(N * mg_cdiv(Lout, GW_LT), nsplit));
    }
}

int c1_nsplit(int N, int Lout)
{
    const long n = ((long)N * Lout + 8191) / 8192;
    return (int)(n < 1 ? 1 : n > 32 ? 32 : n);
}

}   // namespace

extern "C" size_t mg_gconv_packed_floats(int Ci, int Co, int K, int stride, int groups, int mode)
{
    if (groups <= 0 || Ci <= 0 || Co <= 0 || Ci % groups || Co % groups) return 0;
    const int Cig = Ci / groups, Cog = Co / groups;
    if (!gc_form_ok(Cig, Cog, K, stride)) return 0;
    if (Cig == C4_CIG) return mode == MG_GCONV_FWD || mode == MG_GCONV_DGRAD ? (size_t)Co * Cig * GC_K : 0;
    if (mode == MG_GCONV_FWD) return (size_t)groups * mg_cdiv(Cog, 32) * GC_K * (Cig / 2) * 64;
    if (mode == MG_GCONV_DGRAD) return (size_t)groups * mg_cdiv(Cig, 32) * GC_K * (Cog / 2) * 64;
    return 0;
}

extern "C" int mg_gconv_pack(const float *w, float *packed, int Ci, int Co, int K, int stride, int groups, int mode,
                             void *stream)
{
    if (!w || !packed) return MG_ERR_ARG;
    if (mode != MG_GCONV_FWD && mode != MG_GCONV_DGRAD) return MG_ERR_ARG;
    const size_t n = mg_gconv_packed_floats(Ci, Co, K, stride, groups, mode);
    if (!n) return MG_ERR_SHAPE;
    const int Cig = Ci / groups, Cog = Co / groups;
    if (Cig == C4_CIG)
        hipLaunchKernelGGL(c4_pack_kernel, dim3(blocks_for((long)n)), dim3(256), 0, (hipStream_t)stream, w, packed, Cog,
                           groups, mode);
    else if (mode == MG_GCONV_FWD)
        hipLaunchKernelGGL(gc_pack_fwd_kernel, dim3(blocks_for((long)n)), dim3(256), 0, (hipStream_t)stream, w, packed, Cig,
                           Cog, groups);
    else
        hipLaunchKernelGGL(gc_pack_dgrad_kernel, dim3(blocks_for((long)n)), dim3(256), 0, (hipStream_t)stream, w, packed, Cig,
                           Cog, stride, groups);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_gconv1d_fwd(const float *in, const float *packed, const float *bias, float *out, int N, int Ci, int Lin,
                              int Co, int Lout, int K, int stride, int pad, int groups, int act, float slope, void *stream)
{
    if (!in || !packed || !out) return MG_ERR_ARG;
    if (act != MG_ACT_NONE && act != MG_ACT_LRELU) return MG_ERR_ARG;
    MG_TRY(gc_check(N, Ci, Lin, Co, Lout, K, stride, pad, groups));
    const int Cig = Ci / groups, Cog = Co / groups;
    hipStream_t st = (hipStream_t)stream;
#define X(a, b, c)                           \
    if (Cig == a && Cog == b && stride == c) \
        gc_launch_fwd<a, b, c>(st, in, packed, bias, out, N, Ci, Lin, Co, Lout, pad, groups, act, slope);
    GC_FORMS(X)
#undef X
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_gconv1d_dgrad(const float *dy, const float *packed, const float *map, const float *add, float *dx, int N,
                                int Ci, int Lin, int Co, int Lout, int K, int stride, int pad, int groups, float slope,
                                void *stream)
{
    if (!dy || !packed || !dx) return MG_ERR_ARG;
    MG_TRY(gc_check(N, Ci, Lin, Co, Lout, K, stride, pad, groups));
    const int Cig = Ci / groups, Cog = Co / groups;
    hipStream_t st = (hipStream_t)stream;
#define X(a, b, c)                           \
    if (Cig == a && Cog == b && stride == c) \
        gc_launch_dgrad<a, b, c>(st, dy, packed, map, add, dx, N, Ci, Lin, Co, Lout, pad, groups, slope);
    GC_FORMS(X)
#undef X
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_gconv1d_wgrad_scratch_floats(int N, int Ci, int Co, int Lout, int K, int stride, int groups)
{
    if (N <= 0 || Lout <= 0 || groups <= 0 || Ci <= 0 || Co <= 0 || Ci % groups || Co % groups) return 0;
    if (!gc_form_ok(Ci / groups, Co / groups, K, stride)) return 0;
    return (size_t)gw_nsplit(N, Lout, Ci / groups, Co / groups, groups) * Co * (Ci / groups) * GC_K;
}

extern "C" int mg_gconv1d_wgrad(const float *dy, const float *x, float *dw, float *scratch, size_t scratch_floats, int N,
                                int Ci, int Lin, int Co, int Lout, int K, int stride, int pad, int groups, void *stream)
{
    if (!dy || !x || !dw || !scratch) return MG_ERR_ARG;
    MG_TRY(gc_check(N, Ci, Lin, Co, Lout, K, stride, pad, groups));
    const int Cig = Ci / groups, Cog = Co / groups;
    const int nsplit = gw_nsplit(N, Lout, Cig, Cog, groups);
    const long nw = (long)Co * Cig * GC_K;
    if (scratch_floats < (size_t)nsplit * nw) return MG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
#define X(a, b, c)                           \
    if (Cig == a && Cog == b && stride == c) \
        gc_launch_wgrad<a, b, c>(st, dy, x, scratch, N, Ci, Lin, Co, Lout, pad, groups, nsplit);
    GC_FORMS(X)
#undef X
    MG_LAUNCH_CHECK();
    hipLaunchKernelGGL(gc_sum_splits_kernel, dim3(blocks_for(nw)), dim3(256), 0, st, scratch, dw, nw, nsplit);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

static int c1_check(int N, int L, int Co, int K, int pad)
{
    if (N <= 0 || N > 65535 || L <= 0 || Co <= 0 || K <= 0 || K > C1_KMAX || pad < 0) return MG_ERR_SHAPE;
    if ((long)L + 2l * pad < K || (long)N * Co * ((long)L + 2l * pad) >= (1l << 40)) return MG_ERR_SHAPE;
    return MG_OK;
}

extern "C" int mg_conv1d_c1_fwd(const float *in, const float *w, const float *bias, float *out, int N, int L, int Co, int K,
                                int pad, int act, float slope, void *stream)
{
    if (!in || !w || !out) return MG_ERR_ARG;
    if (act != MG_ACT_NONE && act != MG_ACT_LRELU) return MG_ERR_ARG;
    MG_TRY(c1_check(N, L, Co, K, pad));
    const int Lout = L + 2 * pad - K + 1;
    hipLaunchKernelGGL(c1_fwd_kernel, dim3(mg_cdiv(Lout, 256), N, mg_cdiv(Co, C1_CO_PER_BLOCK)), dim3(256), 0,
                       (hipStream_t)stream, in, w, bias, out, L, Lout, Co, K, pad, act, slope);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_conv1d_c1_dgrad(const float *dy, const float *w, float *dx, int N, int L, int Co, int K, int pad,
                                  void *stream)
{
    if (!dy || !w || !dx) return MG_ERR_ARG;
    MG_TRY(c1_check(N, L, Co, K, pad));
    hipLaunchKernelGGL(c1_dgrad_kernel, dim3(mg_cdiv(L, C1_DG_TILE), N), dim3(256), 0, (hipStream_t)stream, dy, w, dx, L,
                       L + 2 * pad - K + 1, Co, K, pad);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_conv1d_c1_wgrad_scratch_floats(int N, int L, int Co, int K)
{
    if (N <= 0 || L <= 0 || Co <= 0 || K <= 0 || K > C1_KMAX) return 0;
    return (size_t)c1_nsplit(N, L + C1_KMAX) * Co * (C1_KMAX + 1);
}

extern "C" int mg_conv1d_c1_wgrad(const float *dy, const float *x, float *dw, float *db, float *scratch,
                                  size_t scratch_floats, int N, int L, int Co, int K, int pad, void *stream)
{
    if (!dy || !x || !dw || !scratch) return MG_ERR_ARG;
    MG_TRY(c1_check(N, L, Co, K, pad));
    const int Lout = L + 2 * pad - K + 1;
    if (Lout > L + C1_KMAX) return MG_ERR_SHAPE;      // the scratch query sizes for pad <= (K + 15) / 2
    const int nsplit = c1_nsplit(N, Lout);
    if (scratch_floats < (size_t)nsplit * Co * (C1_KMAX + 1)) return MG_ERR_WORKSPACE;
    const int per = (int)(((long)N * Lout + nsplit - 1) / nsplit);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(c1_wgrad_kernel, dim3(Co, nsplit), dim3(256), 0, st, dy, x, scratch, N, L, Lout, Co, K, pad, per);
    MG_LAUNCH_CHECK();
    hipLaunchKernelGGL(c1_wgrad_finalize_kernel, dim3(mg_cdiv(Co * (C1_KMAX + 1), 256)), dim3(256), 0, st, scratch, dw, db,
                       Co, K, nsplit);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_avgpool4s2_fwd(const float *in, float *out, int rows, int L, void *stream)
{
    if (!in || !out) return MG_ERR_ARG;
    if (rows <= 0 || L <= 0) return MG_ERR_SHAPE;
    const int Lout = L / 2 + 1;
    hipLaunchKernelGGL((avgpool_fwd_kernel<2, true>), dim3(blocks_for((long)rows * Lout)), dim3(256), 0,
                       (hipStream_t)stream, in, out, (long)rows, L, Lout);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_avgpool4s2_bwd(const float *dy, float *dx, int rows, int L, void *stream)
{
    if (!dy || !dx) return MG_ERR_ARG;
    if (rows <= 0 || L <= 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL((avgpool_bwd_kernel<2, true>), dim3(blocks_for((long)rows * L)), dim3(256), 0,
                       (hipStream_t)stream, dy, dx, (long)rows, L, L / 2 + 1);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_avgpool4s2p1_fwd(const float *in, float *out, int rows, int L, void *stream)
{
    if (!in || !out) return MG_ERR_ARG;
    if (rows <= 0 || L < 2) return MG_ERR_SHAPE;
    const int Lout = (L - 2) / 2 + 1;
    hipLaunchKernelGGL((avgpool_fwd_kernel<1, false>), dim3(blocks_for((long)rows * Lout)), dim3(256), 0,
                       (hipStream_t)stream, in, out, (long)rows, L, Lout);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_avgpool4s2p1_bwd(const float *dy, float *dx, int rows, int L, void *stream)
{
    if (!dy || !dx) return MG_ERR_ARG;
    if (rows <= 0 || L < 2) return MG_ERR_SHAPE;
    hipLaunchKernelGGL((avgpool_bwd_kernel<1, false>), dim3(blocks_for((long)rows * L)), dim3(256), 0,
                       (hipStream_t)stream, dy, dx, (long)rows, L, (L - 2) / 2 + 1);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_reflect_pad1d_fwd(const float *in, float *out, int rows, int T, int p, void *stream)
{
    if (!in || !out) return MG_ERR_ARG;
    if (rows <= 0 || p < 0 || T <= p || (long)T + 2l * p >= (1l << 30)) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(reflect_pad_fwd_kernel, dim3(blocks_for((long)rows * (T + 2 * p))), dim3(256), 0,
                       (hipStream_t)stream, in, out, (long)rows, T, p);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_reflect_pad1d_bwd(const float *dy, float *dx, int rows, int T, int p, void *stream)
{
    if (!dy || !dx) return MG_ERR_ARG;
    if (rows <= 0 || p < 0 || T <= p || (long)T + 2l * p >= (1l << 30)) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(reflect_pad_bwd_kernel, dim3(blocks_for((long)rows * T)), dim3(256), 0, (hipStream_t)stream, dy, dx,
                       (long)rows, T, p);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
