// MelGAN generator (descriptinc/melgan-neurips mel2wav/modules.py: Generator(80, ngf=32, n_residual_layers=3)):
// the reflect-padded convolutions, the upsampler writing into a channel slice, and the fused residual stack of the
// 32- and 64-channel stages.  The general form of a ResnetBlock(dim, d) is two launches:
//     t = lrelu(W1 (*)_d reflect_d(lrelu(x)) + b1)      -> channels [C, 2C) of a [B, 2C, L] buffer whose [0, C) is x
//     y = [Ws | W2] [x ; t] + (bs + b2)                  -> one K = 1 GEMM with Ci = 2C (mg_conv1x1_fwd_strided)
// which moves about 15 activation passes per stage through HBM.  The fused stack (mg_melgan_stack_fwd) reads a
// stage's input once and writes its output once.
//
// Fused stack.  Workgroup = 4 waves, one tile of T = 128 NNB - 24 output samples of one batch element (C = 32:
// NNB = 2, T = 232; C = 64: NNB = 1, T = 104 -- both hold two workgroups per CU without spilling; the next larger
// tiles need 350+ registers, i.e. one wave per SIMD).  LDS holds one [C][S] fp32 image of the stage input over the
// window [l0 - 13, l0 + T + 13) (13 = 1 + 3 + 9: every block shrinks the valid window by its dilation per side;
// neighbouring tiles recompute the halo).  Block k computes 128 NNB columns starting (sum of the later blocks'
// dilations) columns in from the window edge; each wave owns NNB 32-column tiles of them and all C rows:
//   conv1  t = lrelu(W1 (*)_d lrelu(x) + b1)   3C-deep reduction, B operand = the LDS image (lrelu on the read),
//                                              result in the MFMA accumulators
//   conv2  y = Ws x + W2 t + bs + b2           2C-deep; the x half reads the wave's own columns of the image, the t
//                                              half takes the accumulators as the B operand with no lane movement:
//                                              accumulator register r of lane (h = lane >> 5) holds row
//                                              8 (r >> 2) + 4 h + (r & 3), so k-step r pairs rows (8 (r>>2) + (r&3),
//                                              that + 4), and W2's columns are permuted to match before packing
//   y overwrites x in place (one barrier: every wave has read its conv1 halo), then positions outside [0, L) of the
//   block output are filled with its mirror image up to the next block's dilation -- each block reflects its own
//   input, as ReflectionPad1d does in the reference.  The last block stores straight from the accumulators.
// Both GEMMs run on v_mfma_f32_32x32x2_f32 with the weight stream of mg_conv_pack (K = 3, plain) and mg_conv_pack_at
// ([Ws | W2 permuted], K = 1), read global/L2 -> VGPR one k-group ahead, as in conv_mfma.h.
#include "conv_mfma.h"

// ---------------------------------------------------------------------------------------------
// Reflect-padded convolution and the slice-writing upsampler, each with a case list of its own (conv_mfma.h, ConvCases)
// ---------------------------------------------------------------------------------------------
struct EpiReflect : EpiBiasAct {};
template <>
struct EpiReflectPad<EpiReflect> { static constexpr bool value = true; };

// EpiBiasAct::run_phases with the batch stride out_bs (0 -> Co * u * Lin): the upsampler of a general-form stage writes
// channels [0, C) of the first block's [B, 2C, L] buffer.
struct EpiPhasesSlice {
    using Params = EpiBiasAct::Params;
    template <int WM, int NNB>
    static __device__ __forceinline__ void run(const Params &p, f32x16 (&acc)[WM][NNB], int b, int mrow0, int l0w,
                                               int lane, int Lm)
    {
        const int h = lane >> 5, c = lane & 31, u = p.phase_u;
        const int Mrows = p.Co * u;
        const size_t Lfull = (size_t)Lm * u;
        float *outb = p.out + (size_t)b * (p.out_bs ? (size_t)p.out_bs : (size_t)p.Co * Lfull);
#pragma unroll
        for (int i = 0; i < WM; ++i) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int row0 = mrow0 + i * 32 + 8 * rq + 4 * h;
                if (row0 >= Mrows) continue;
#pragma unroll
                for (int j = 0; j < NNB; ++j) {
                    const int m = l0w + j * 32 + c;
                    if (m >= Lm) continue;
                    if (u >= 4) {
                        const int co = row0 / u, r0 = row0 - co * u;
                        const float bv = p.bias ? p.bias[co] : 0.f;
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][rq * 4 + e] * p.alpha + bv;
                        *reinterpret_cast<f32x4 *>(outb + (size_t)co * Lfull + (size_t)m * u + r0) = v;
                    } else {   // u == 2
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const int co = (row0 >> 1) + e2;
                            const float bv = p.bias ? p.bias[co] : 0.f;
                            float2 v;
                            v.x = acc[i][j][rq * 4 + 2 * e2] * p.alpha + bv;
                            v.y = acc[i][j][rq * 4 + 2 * e2 + 1] * p.alpha + bv;
                            *reinterpret_cast<float2 *>(outb + (size_t)co * Lfull + (size_t)m * 2) = v;
                        }
                    }
                }
            }
        }
    }
};

extern "C" int mg_conv1d_reflect_fwd(const float *in, long in_bs, const float *packed, const float *bias, float *out,
                                     long out_bs, int B, int Ci, int L, int Co, int K, int dil, float in_slope, int act,
                                     float act_slope, float alpha, void *stream)
{
    if (!in || !packed || !out) return MG_ERR_ARG;
    if (act < 0 || act > MG_ACT_LRELU) return MG_ERR_ARG;
    if (B <= 0 || Ci <= 0 || Co <= 0 || dil < 1 || in_bs < 0 || out_bs < 0) return MG_ERR_SHAPE;
    if (!((K == 3 && dil <= 9) || (K == 7 && dil == 1))) return MG_ERR_SHAPE;
    const int pad = dil * (K - 1) / 2;
    if (L <= pad) return MG_ERR_SHAPE;   // ReflectionPad1d needs pad < L
    ConvShape s{B, Ci, L, L, K, 1, pad, Co, in_bs, 0, dil, in_slope};
    EpiBiasAct::Params ep{out, bias, nullptr, alpha, Co, act, 0, out_bs, nullptr, act_slope};
    return conv_launch<EpiReflect, CONV_CASES_REFLECT>(s, in, nullptr, packed, ep, (hipStream_t)stream);
}

extern "C" int mg_conv_transpose1d_fwd_slice(const float *in, const float *packed, const float *bias, float *out,
                                             long out_bs, int B, int Ci, int Lin, int Co, int u, float in_slope,
                                             float alpha, void *stream)
{
    if (!in || !packed || !out) return MG_ERR_ARG;
    if (B <= 0 || Ci <= 0 || Co <= 0 || Lin <= 0 || out_bs < 0) return MG_ERR_SHAPE;
    if (!(u == 2 || u == 4 || u == 8) || (Co * u) % 4 != 0) return MG_ERR_SHAPE;
    if (out_bs != 0 && out_bs < (long)Co * u * Lin) return MG_ERR_SHAPE;
    ConvShape s{B, Ci, Lin, Lin, 3, 1, 1, Co * u, 0, 0, 1, in_slope};
    EpiBiasAct::Params ep{out, bias, nullptr, alpha, Co, MG_ACT_NONE, 0, out_bs, nullptr, 0.f, u};
    return conv_launch<EpiPhasesSlice, CONV_CASES_SLICE>(s, in, nullptr, packed, ep, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Fused residual stack
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int MS_HALO = 13;   // 1 + 3 + 9

struct MelStackArgs {
    const float *in;   // [B, C, L]
    float *out;        // [B, C, L]
    const float *w1[3], *b1[3], *w2[3], *b2[3];
    int L, ntiles;
};

template <int C, int NNB>
struct MelStackGeom {
    static constexpr int MB = C / 32;                  // 32-row blocks
    static constexpr int NCOL = 4 * 32 * NNB;          // columns one block computes (4 waves x NNB 32-column tiles)
    static constexpr int T = NCOL - 2 * (MS_HALO - 1); // output samples per tile: block 1 computes T + 24 columns
    static constexpr int W = T + 2 * MS_HALO;          // staged window
    static constexpr int S = NCOL + 24;                // LDS row stride: block 3 reads up to column NCOL + 21
};

// One ResnetBlock on the LDS image: D = dilation, C0 = first column computed, LAST = store to `out` (else in place).
template <int C, int NNB, int D, int C0, bool LAST>
__device__ __forceinline__ void ms_block(float *lds, const MelStackArgs &a, int k, int b, int l0, int wave, int lane)
{
    using G = MelStackGeom<C, NNB>;
    constexpr int MB = G::MB, S = G::S;
    constexpr int Q1 = 3 * C / 8, QX = C / 8, Q2 = 2 * C / 8;   // k-groups: conv1, shortcut half, conv2
    const int h = lane >> 5, c32 = lane & 31;
    const int cb = C0 + wave * 32 * NNB + c32;   // this lane's column in n-tile 0

    // conv1: t = lrelu(W1 (*)_D lrelu(x) + b1); packed [mb][q = chunk*12 + tap*4 + g][lane] (mg_conv_pack, K = 3)
    f32x16 t[MB][NNB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NNB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) t[i][j][r] = 0.f;
    const f32x4 *A1 = reinterpret_cast<const f32x4 *>(a.w1[k]) + lane;
    f32x4 ac[MB], an[MB];
#pragma unroll
    for (int i = 0; i < MB; ++i) ac[i] = A1[(size_t)(i * Q1) * 64];
#pragma unroll
    for (int q = 0; q < Q1; ++q) {
        const int chunk = q / 12, tap = (q % 12) / 4, g = q % 4;
#pragma unroll
        for (int i = 0; i < MB; ++i) an[i] = A1[(size_t)(i * Q1 + (q + 1 < Q1 ? q + 1 : q)) * 64];
        float bv[4][NNB];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < NNB; ++j) {
                const float v = lds[(chunk * 32 + g * 8 + 2 * e + h) * S + cb + j * 32 + (tap - 1) * D];
                bv[e][j] = v > 0.f ? v : 0.2f * v;
            }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NNB; ++j)
                    t[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i][e], bv[e][j], t[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MB; ++i) ac[i] = an[i];
    }
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float bias = a.b1[k][i * 32 + 8 * (r >> 2) + 4 * h + (r & 3)];
#pragma unroll
            for (int j = 0; j < NNB; ++j) {
                const float v = t[i][j][r] + bias;
                t[i][j][r] = v > 0.f ? v : 0.2f * v;
            }
        }

    // conv2: y = [Ws | W2'] [x ; t] + (bs + b2); packed [mb][q][lane] with q < QX the shortcut (x from LDS, own
    // columns) and q >= QX W2 (B operand = the conv1 accumulators: k-step 4 g + e of 32-row block `chunk` is t[chunk][.][4 g + e])
    f32x16 y[MB][NNB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NNB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) y[i][j][r] = 0.f;
    const f32x4 *A2 = reinterpret_cast<const f32x4 *>(a.w2[k]) + lane;
#pragma unroll
    for (int i = 0; i < MB; ++i) ac[i] = A2[(size_t)(i * Q2) * 64];
#pragma unroll
    for (int q = 0; q < Q2; ++q) {
#pragma unroll
        for (int i = 0; i < MB; ++i) an[i] = A2[(size_t)(i * Q2 + (q + 1 < Q2 ? q + 1 : q)) * 64];
        float bv[4][NNB];
        if (q < QX) {
            const int chunk = q / 4, g = q % 4;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < NNB; ++j) bv[e][j] = lds[(chunk * 32 + g * 8 + 2 * e + h) * S + cb + j * 32];
        } else {
            const int chunk = (q - QX) / 4, g = (q - QX) % 4;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < NNB; ++j) bv[e][j] = t[chunk][j][4 * g + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NNB; ++j)
                    y[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[i][e], bv[e][j], y[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MB; ++i) ac[i] = an[i];
    }

    if (LAST) {   // columns [13, 13 + T) are the tile's outputs l0 .. l0 + T - 1
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                const float bias = a.b2[k][row];
                float *orow = a.out + ((size_t)b * C + row) * a.L;
#pragma unroll
                for (int j = 0; j < NNB; ++j) {
                    const int c = cb + j * 32 - MS_HALO, p = l0 + c;
                    if (c < G::T && p < a.L) orow[p] = y[i][j][r] + bias;
                }
            }
        return;
    }
    __syncthreads();   // every wave has read its conv1 halo: the block output may replace x
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
            const float bias = a.b2[k][row];
#pragma unroll
            for (int j = 0; j < NNB; ++j) lds[row * S + cb + j * 32] = y[i][j][r] + bias;
        }
    __syncthreads();
}

// Positions -1 .. -DN and L .. L-1+DN of the block output just written take the mirror image about 0 and L - 1 (the
// next block's ReflectionPad1d(DN)); only tiles whose window reaches an end have any.
template <int C, int NNB, int DN>
__device__ __forceinline__ void ms_mirror(float *lds, int l0, int L, int tid)
{
    using G = MelStackGeom<C, NNB>;
    const bool left = l0 == 0, right = l0 + G::T + MS_HALO - 1 >= L;
    if (!left && !right) return;   // workgroup-uniform
    for (int i = tid; i < C * DN; i += 256) {
        const int ci = i / DN, j = i - ci * DN + 1;
        float *row = lds + ci * G::S;
        if (left) row[MS_HALO - j] = row[MS_HALO + j];
        if (right) {
            const int cs = L - 1 - j - l0 + MS_HALO;
            row[cs + 2 * j] = row[cs];
        }
    }
    __syncthreads();
}

template <int C, int NNB>
__global__ __launch_bounds__(256, 2) void melgan_stack_kernel(MelStackArgs a)
{
    using G = MelStackGeom<C, NNB>;
    __shared__ float lds[C * G::S];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / a.ntiles, l0 = (blockIdx.x % a.ntiles) * G::T;
    const float *inb = a.in + (size_t)b * C * a.L;
    // stage x over [l0 - 13, l0 + T + 13), reflected about 0 and L - 1 (clamped where a second reflection would be
    // needed: those positions feed no stored output); the columns past the window are zero
#pragma unroll 8
    for (int i = tid; i < C * G::S; i += 256) {
        const int ci = i / G::S, c = i - ci * G::S;
        float v = 0.f;
        if (c < G::W) {
            int p = l0 - MS_HALO + c;
            p = p < 0 ? -p : p;
            p = p >= a.L ? 2 * (a.L - 1) - p : p;
            p = p < 0 ? 0 : (p >= a.L ? a.L - 1 : p);
            v = inb[(size_t)ci * a.L + p];
        }
        lds[i] = v;
    }
    __syncthreads();
    ms_block<C, NNB, 1, MS_HALO - 12, false>(lds, a, 0, b, l0, wave, lane);
    ms_mirror<C, NNB, 3>(lds, l0, a.L, tid);
    ms_block<C, NNB, 3, MS_HALO - 9, false>(lds, a, 1, b, l0, wave, lane);
    ms_mirror<C, NNB, 9>(lds, l0, a.L, tid);
    ms_block<C, NNB, 9, MS_HALO, true>(lds, a, 2, b, l0, wave, lane);
}

template <int C, int NNB>
int ms_launch(MelStackArgs &a, int B, hipStream_t st)
{
    a.ntiles = mg_cdiv(a.L, MelStackGeom<C, NNB>::T);
    const long grid = (long)B * a.ntiles;
    if (grid > 0x7fffffffL) return MG_ERR_SHAPE;
    hipLaunchKernelGGL((melgan_stack_kernel<C, NNB>), dim3((unsigned)grid), dim3(256), 0, st, a);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

}  // namespace

extern "C" int mg_melgan_stack_fwd(const float *in, float *out, const float *const *w1, const float *const *b1,
                                   const float *const *wmix, const float *const *bmix, int B, int C, int L, void *stream)
{
    if (!in || !out || in == out || !w1 || !b1 || !wmix || !bmix) return MG_ERR_ARG;
    MelStackArgs a;
    for (int k = 0; k < 3; ++k) {
        if (!w1[k] || !b1[k] || !wmix[k] || !bmix[k]) return MG_ERR_ARG;
        a.w1[k] = w1[k];
        a.b1[k] = b1[k];
        a.w2[k] = wmix[k];
        a.b2[k] = bmix[k];
    }
    if (B <= 0 || !(C == 32 || C == 64) || L <= 9) return MG_ERR_SHAPE;   // ReflectionPad1d(9) needs L > 9
    a.in = in;
    a.out = out;
    a.L = L;
    return C == 32 ? ms_launch<32, 2>(a, B, (hipStream_t)stream) : ms_launch<64, 1>(a, B, (hipStream_t)stream);
}

extern "C" int mg_melgan_stack_tile(int C)
{
    if (C == 32) return MelStackGeom<32, 2>::T;
    if (C == 64) return MelStackGeom<64, 1>::T;
    return 0;
}
