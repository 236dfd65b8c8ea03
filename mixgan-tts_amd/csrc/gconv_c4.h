// Grouped K = 41, stride 4 convolutions with FOUR input channels per group (MelGAN's discriminator, Kumar et al. 2019):
// (Cig, Cog) = (4, 16) and (4, 4).  Included by msd.hip, which dispatches to these kernels from the one form list.
//
// A group is a 4 x 164 (or 16 x 164) matrix: a 32-row MFMA tile would be 7/8 (1/2) zeros.  These kernels run on the VALU
// with several groups side by side in every wave: 16 lanes walk the frames of one group, the wave's four 16-lane
// quarters are four groups (or four groups x one row quad each).  A lane keeps a 4-row x 2-frame block of sums; one
// 16-byte weight load (four rows of one (ci, tap), L1/L2-resident: a group's weights are 2.6 - 10.5 KB) feeds four
// packed FMAs.  The input window sits in LDS deinterleaved by phase as in gc_fwd_kernel, so a lane's taps of one phase
// are consecutive floats.  DESIGN.md 4.16 has the reasoning and the measurements.
#pragma once
#include "common.h"

namespace {

constexpr int C4_K = 41, C4_S = 4, C4_CIG = 4;
constexpr int C4_J = (C4_K + C4_S - 1) / C4_S;      // taps of phase 0; the other phases have C4_J - 1

// groups per workgroup: 16 lanes x 16 slots, a slot = (group, quad of output rows)
template <int COG>
constexpr int c4_gpb() { return 64 / COG; }

__device__ __forceinline__ f32x2 c4_fma(f32x2 w, float x, f32x2 acc)
{
    return __builtin_elementwise_fma(w, (f32x2){x, x}, acc);      // v_pk_fma_f32
}

// ---------------------------------------------------------------------------------------------------------------
// forward: workgroup = (32 frames, c4_gpb groups, n).  win[group][ci][phase][pos]: sample p of the window (global
// position 4 t0 - pad + p) at phase p % 4, pos p / 4; frame l takes tap 4 j + f from phase f, pos l + j.
// ---------------------------------------------------------------------------------------------------------------
constexpr int C4F_NT = 32, C4F_WP = C4F_NT + C4_J - 1, C4F_CH = C4_S * C4F_WP, C4F_GS = C4_CIG * C4F_CH + 16;
static_assert(C4F_WP % 2 == 0 && C4F_GS % 2 == 0, "8-byte LDS reads");

template <int COG>
__global__ __launch_bounds__(256) void c4_fwd_kernel(const float *__restrict__ in, const float *__restrict__ packed,
                                                     const float *__restrict__ bias, float *__restrict__ out, int Ci,
                                                     int Lin, int Co, int Lout, int pad, int G, int act, float slope)
{
    constexpr int GPB = c4_gpb<COG>();
    __shared__ __attribute__((aligned(16))) float win[GPB * C4F_GS];
    const int t0 = blockIdx.x * C4F_NT, g0 = blockIdx.y * GPB, n = blockIdx.z;
    const long p0 = (long)t0 * C4_S - pad;
    for (int e = threadIdx.x; e < GPB * C4_CIG * C4F_CH; e += 256) {
        const int row = e / C4F_CH, p = e % C4F_CH, gi = row / C4_CIG, ci = row % C4_CIG;
        const long gp = p0 + p;
        float v = 0.f;
        if (g0 + gi < G && gp >= 0 && gp < Lin) v = in[((long)n * Ci + (long)(g0 + gi) * C4_CIG + ci) * Lin + gp];
        win[gi * C4F_GS + ci * C4F_CH + (p % C4_S) * C4F_WP + p / C4_S] = v;
    }
    __syncthreads();
    const int fs = threadIdx.x & 15, slot = threadIdx.x >> 4, gi = slot % GPB, coq = slot / GPB;
    const int g = g0 + gi, gw = g < G ? g : G - 1;      // lanes past the last group read a valid group's weights, store nothing
    f32x2 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[i][0] = acc[i][1] = (f32x2){0.f, 0.f};
    const float *wp = packed + (long)gw * C4_CIG * C4_K * COG + coq * 4;
    const float *xw = win + gi * C4F_GS + fs * 2;
#pragma unroll 1
    for (int ci = 0; ci < C4_CIG; ++ci) {
#pragma unroll 1
        for (int f = 0; f < C4_S; ++f) {      // eleven 16-byte weight loads in flight per pass; more would spill
            float xv[C4_J + 1];
#pragma unroll
            for (int i = 0; i < C4_J + 1; i += 2) {
                const f32x2 x2 = *reinterpret_cast<const f32x2 *>(xw + ci * C4F_CH + f * C4F_WP + i);
                xv[i] = x2[0], xv[i + 1] = x2[1];
            }
#pragma unroll
            for (int j = 0; j < C4_J; ++j) {
                const int k = C4_S * j + f;
                if (k < C4_K) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wp + (ci * C4_K + k) * COG);
#pragma unroll
                    for (int fr = 0; fr < 2; ++fr) {
                        acc[fr][0] = c4_fma((f32x2){w4[0], w4[1]}, xv[fr + j], acc[fr][0]);
                        acc[fr][1] = c4_fma((f32x2){w4[2], w4[3]}, xv[fr + j], acc[fr][1]);
                    }
                }
            }
        }
    }
    if (g >= G) return;
#pragma unroll
    for (int fr = 0; fr < 2; ++fr) {
        const int t = t0 + fs * 2 + fr;
        if (t >= Lout) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ch = g * COG + coq * 4 + c;
            float v = acc[fr][c >> 1][c & 1] + (bias ? bias[ch] : 0.f);
            if (act == MG_ACT_LRELU) v = v > 0.f ? v : v * slope;
            out[((long)n * Co + ch) * Lout + t] = v;
        }
    }
}

// mode MG_GCONV_FWD: [G][ci][K][COG]; MG_GCONV_DGRAD: [G][COG][K][ci]
__global__ void c4_pack_kernel(const float *__restrict__ w, float *__restrict__ packed, int COG, int G, int mode)
{
    const long total = (long)G * COG * C4_CIG * C4_K;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += gridDim.x * 256l) {
        long j = i;
        int co, ci, k;
        if (mode == MG_GCONV_FWD) {
            co = j % COG, j /= COG;
            k = j % C4_K, j /= C4_K;
            ci = j % C4_CIG, j /= C4_CIG;
        } else {
            ci = j % C4_CIG, j /= C4_CIG;
            k = j % C4_K, j /= C4_K;
            co = j % COG, j /= COG;
        }
        packed[i] = w[((j * COG + co) * C4_CIG + ci) * C4_K + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// data gradient, polyphase as gc_dgrad_kernel: with m + pad = 4 u + f, dx[ci, m] = sum_{co, j} w[co, ci, f + 4 j] dy[co, u - j].
// A lane owns two values of u of one group: 4 ci x 4 phases x 2 = 32 sums, and walks (co, tap) with one 16-byte load of
// the four input channels' weights per step.  A wave is four groups x 16 lanes.  Cog = 4: the four waves are sixteen
// groups over the same 32 u; Cog = 16: the four waves are four 32-u ranges of the same four groups, so that the first
// layer (G = 4) fills the workgroup.  dyw[group][co][i] = dy[co, u0 - (J - 1) + i].
// ---------------------------------------------------------------------------------------------------------------
template <int COG>
constexpr int c4d_nu() { return COG == 4 ? 32 : 128; }

template <int COG>
__global__ __launch_bounds__(256) void c4_dgrad_kernel(const float *__restrict__ dy, const float *__restrict__ packed,
                                                       const float *__restrict__ map, const float *__restrict__ add,
                                                       float *__restrict__ dx, int Ci, int Lin, int Co, int Lout, int pad,
                                                       int G, float slope)
{
    constexpr int GPB = c4_gpb<COG>(), NU = c4d_nu<COG>(), WD = NU + C4_J - 1;
    static_assert(WD % 2 == 0, "8-byte LDS reads");
    __shared__ __attribute__((aligned(16))) float dyw[GPB * COG * WD];
    const int u0 = blockIdx.x * NU, g0 = blockIdx.y * GPB, n = blockIdx.z;
    for (int e = threadIdx.x; e < GPB * COG * WD; e += 256) {
        const int row = e / WD, l = u0 - (C4_J - 1) + e % WD;      // row = gi COG + co: consecutive channels from g0 COG
        float v = 0.f;
        if (g0 + row / COG < G && l >= 0 && l < Lout) v = dy[((long)n * Co + (long)g0 * COG + row) * Lout + l];
        dyw[e] = v;
    }
    __syncthreads();
    const int lane16 = threadIdx.x & 15, quarter = (threadIdx.x >> 4) & 3, wave = threadIdx.x >> 6;
    const int gi = COG == 4 ? wave * 4 + quarter : quarter;
    const int ul = (COG == 4 ? 0 : wave * 32) + lane16 * 2;
    const int g = g0 + gi, gw = g < G ? g : G - 1;
    f32x2 acc[2][C4_S][2];
#pragma unroll
    for (int ur = 0; ur < 2; ++ur)
#pragma unroll
        for (int f = 0; f < C4_S; ++f) acc[ur][f][0] = acc[ur][f][1] = (f32x2){0.f, 0.f};
    const float *wp = packed + (long)gw * COG * C4_K * C4_CIG;
    const float *dw = dyw + gi * COG * WD + ul;
#pragma unroll 1
    for (int co = 0; co < COG; ++co) {
        float dv[C4_J + 1];
#pragma unroll
        for (int i = 0; i < C4_J + 1; i += 2) {
            const f32x2 d2 = *reinterpret_cast<const f32x2 *>(dw + co * WD + i);
            dv[i] = d2[0], dv[i + 1] = d2[1];
        }
#pragma unroll
        for (int k = 0; k < C4_K; ++k) {
            const int f = k % C4_S, j = k / C4_S;
            const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wp + (co * C4_K + k) * C4_CIG);
#pragma unroll
            for (int ur = 0; ur < 2; ++ur) {
                const float d = dv[ur + (C4_J - 1) - j];
                acc[ur][f][0] = c4_fma((f32x2){w4[0], w4[1]}, d, acc[ur][f][0]);
                acc[ur][f][1] = c4_fma((f32x2){w4[2], w4[3]}, d, acc[ur][f][1]);
            }
        }
    }
    if (g >= G) return;
#pragma unroll
    for (int ur = 0; ur < 2; ++ur)
#pragma unroll
        for (int f = 0; f < C4_S; ++f) {
            const long mpos = (long)C4_S * (u0 + ul + ur) + f - pad;
            if (mpos < 0 || mpos >= Lin) continue;
#pragma unroll
            for (int ci = 0; ci < C4_CIG; ++ci) {
                const long idx = ((long)n * Ci + (long)g * C4_CIG + ci) * Lin + mpos;
                float v = acc[ur][f][ci >> 1][ci & 1];
                if (add) v += add[idx];
                if (map) v *= map[idx] > 0.f ? 1.f : slope;
                dx[idx] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// weight gradient: dw[co, ci, 4 j + f] = sum_{n, l} dy[co, l] x[ci, 4 (l + j) + f - pad].  A lane owns (group, quad of
// output rows, ci, phase f): 4 x 11 sums, over the workgroup's range of (n, 16-frame) chunks; 16 lanes are the 16
// (ci, f) of one slot, a wave is four slots.  Per chunk the x window is staged phase-deinterleaved (a lane's 11 taps of
// frame l are pos l .. l + 10 of its own row) and dy as [group][co][16].  Partial tiles go to scratch [split][Co][4][41];
// gc_sum_splits_kernel adds them in ascending order.
// ---------------------------------------------------------------------------------------------------------------
constexpr int C4W_LT = 16, C4W_WP = C4W_LT + C4_J;

template <int COG>
__global__ __launch_bounds__(256) void c4_wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                       float *__restrict__ scratch, int N, int Ci, int Lin, int Co, int Lout,
                                                       int pad, int G, int cps)
{
    constexpr int GPB = c4_gpb<COG>(), XROW = C4_S * C4W_WP;
    __shared__ __attribute__((aligned(16))) float xw[GPB * C4_CIG * XROW];
    __shared__ __attribute__((aligned(16))) float dyl[GPB * COG * C4W_LT];
    const int g0 = blockIdx.x * GPB, z = blockIdx.y;
    const int item = threadIdx.x & 15, slot = threadIdx.x >> 4, gi = slot % GPB, coq = slot / GPB;
    const int ci = item >> 2, f = item & 3, g = g0 + gi;
    float acc[4][C4_J];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < C4_J; ++j) acc[c][j] = 0.f;
    const int lchunks = (Lout + C4W_LT - 1) / C4W_LT, total = N * lchunks;
    const int c_end = min(total, (z + 1) * cps);
    const float *xr = xw + ((gi * C4_CIG + ci) * C4_S + f) * C4W_WP;
    const float *dr = dyl + (gi * COG + coq * 4) * C4W_LT;
    for (int ch = z * cps; ch < c_end; ++ch) {
        const int n = ch / lchunks, l0 = (ch % lchunks) * C4W_LT;
        const long p0 = (long)l0 * C4_S - pad;
        for (int e = threadIdx.x; e < GPB * C4_CIG * XROW; e += 256) {
            const int row = e / XROW, p = e % XROW;      // row = gi 4 + ci: consecutive channels from g0 4
            const long gp = p0 + p;
            float v = 0.f;
            if (g0 + row / C4_CIG < G && gp >= 0 && gp < Lin) v = x[((long)n * Ci + (long)g0 * C4_CIG + row) * Lin + gp];
            xw[(row * C4_S + p % C4_S) * C4W_WP + p / C4_S] = v;
        }
        for (int e = threadIdx.x; e < GPB * COG * C4W_LT; e += 256) {
            const int row = e / C4W_LT, i = e % C4W_LT;
            float v = 0.f;
            if (g0 + row / COG < G && l0 + i < Lout) v = dy[((long)n * Co + (long)g0 * COG + row) * Lout + l0 + i];
            dyl[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int lq = 0; lq < C4W_LT / 4; ++lq) {
            float xs[C4_J + 3];
#pragma unroll
            for (int i = 0; i < C4_J + 3; ++i) xs[i] = xr[4 * lq + i];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 d4 = *reinterpret_cast<const f32x4 *>(dr + c * C4W_LT + 4 * lq);
#pragma unroll
                for (int li = 0; li < 4; ++li)
#pragma unroll
                    for (int j = 0; j < C4_J; ++j) acc[c][j] = fmaf(d4[li], xs[li + j], acc[c][j]);
            }
        }
        __syncthreads();
    }
    if (g >= G) return;
    float *dst = scratch + ((long)z * Co + (long)g * COG + coq * 4) * (C4_CIG * C4_K) + ci * C4_K;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < C4_J; ++j)
            if (C4_S * j + f < C4_K) dst[c * (C4_CIG * C4_K) + C4_S * j + f] = acc[c][j];
}

// splits of the (n, 16-frame chunk) range: about 512 workgroups, at most 256 partial copies
inline int c4w_nsplit(int N, int Lout, int Cog, int G)
{
    const long chunks = (long)N * mg_cdiv(Lout, C4W_LT);
    long n = 512 / mg_cdiv(G, 64 / Cog);
    n = n < 1 ? 1 : n > 256 ? 256 : n;
    return (int)(n > chunks ? chunks : n);
}

}   // namespace
