// HiFi-GAN multi-period discriminator (Kong et al. 2020, DiscriminatorP) on a slotted flat axis: every layer is one plain
// 1-D convolution of conv_mfma_kernel (CONV_CASES_PERIOD), all period arithmetic lives in the geometry function, the fold
// kernels and the epilogue below.  C ABI and the construction: include/mixgan_hip.h, "HiFi-GAN multi-period discriminator".
#include "conv_mfma.h"

// ---------------------------------------------------------------------------------------------------------------
// geometry: the single source of H[0..6] and S[0..6] for C and Python
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mg_period_geometry(int T, int p, int *H, int *S)
{
    if (!H || !S) return MG_ERR_ARG;
    if (T < 1 || p < 1) return MG_ERR_SHAPE;
    const int rpad = p - 1 - (T - 1) % p;   // reflect pad on the right up to a multiple of p
    if (T <= rpad) return MG_ERR_SHAPE;
    const long h0 = ((long)T + rpad) / p;
    long h[7];
    h[0] = h0;
    for (int j = 0; j < 4; ++j) h[j + 1] = (h[j] - 1) / 3 + 1;
    h[5] = h[6] = h[4];
    const long s4 = h[4] + 2;
    if (81 * s4 >= (1l << 30)) return MG_ERR_SHAPE;
    long s = s4;
    for (int j = 6; j >= 0; --j) {
        if (j < 4) s *= 3;
        S[j] = (int)s;
        H[j] = (int)h[j];
    }
    return MG_OK;
}

namespace {

// ---------------------------------------------------------------------------------------------------------------
// The epilogue of every period launch.  GEMM row `row`, column l of a launch with u = 1 is out[row, l]; with u = 3 (the
// polyphase data gradient) row = c 3 + f is phase f of channel c and the element goes to out[c, 3 l + f].  Position
// u l + f of a row of u Lout columns is live iff u (l mod Sq) + f < H (slot width u Sq); the slack is written as 0.
// Loads (add, map) of 8 rows x NNB columns go out at clamped addresses before any is used; only the store is predicated.
// ---------------------------------------------------------------------------------------------------------------
struct EpiPeriod {
    struct Params {
        float *out;         // [C, u Lout]
        const float *bias;  // [C] or null
        const float *add;   // as out, or null: added after the activation
        const float *map;   // as out, or null: result *= map > 0 ? 1 : map_slope
        float act_slope;    // leaky ReLU on acc + bias when act == MG_ACT_LRELU
        float map_slope;
        int rows;           // GEMM rows: C u
        int act;
        int u;              // 1 or 3
        int Sq, H;
    };
    template <int WM, int NNB>
    static __device__ __forceinline__ void run(const Params &p, f32x16 (&acc)[WM][NNB], int b, int mrow0, int l0w,
                                               int lane, int Lout)
    {
        const int h = lane >> 5, c = lane & 31, u = p.u;
        const size_t Lfull = (size_t)Lout * u;
        int lc[NNB], lm[NNB];
        bool lok[NNB];
#pragma unroll
        for (int j = 0; j < NNB; ++j) {
            const int l = l0w + j * 32 + c;
            lok[j] = l < Lout;
            lc[j] = lok[j] ? l : Lout - 1;
            lm[j] = u * (lc[j] % p.Sq);
        }
        const bool has_add = p.add != nullptr, has_map = p.map != nullptr;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            if (mrow0 + i * 32 >= p.rows) continue;   // wave-uniform
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float av[8][NNB], mv[8][NNB], bv[8];
                size_t rbase[8];
                int ph[8];
                bool rok[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int rr = half * 8 + r;
                    const int row = mrow0 + i * 32 + 8 * (rr >> 2) + 4 * h + (rr & 3);
                    rok[r] = row < p.rows;
                    const int rc = rok[r] ? row : p.rows - 1;
                    const int ch = rc / u;
                    ph[r] = rc - ch * u;
                    rbase[r] = (size_t)ch * Lfull + ph[r];
                    bv[r] = p.bias ? p.bias[ch] : 0.f;
                }
                if (has_add) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
#pragma unroll
                        for (int j = 0; j < NNB; ++j) av[r][j] = p.add[rbase[r] + (size_t)u * lc[j]];
                }
                if (has_map) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
#pragma unroll
                        for (int j = 0; j < NNB; ++j) mv[r][j] = p.map[rbase[r] + (size_t)u * lc[j]];
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) {
#pragma unroll
                    for (int j = 0; j < NNB; ++j) {
                        float v = acc[i][j][half * 8 + r] + bv[r];
                        if (p.act == MG_ACT_LRELU) v = v > 0.f ? v : p.act_slope * v;
                        if (has_add) v += av[r][j];
                        if (has_map) v *= mv[r][j] > 0.f ? 1.f : p.map_slope;
                        v = lm[j] + ph[r] < p.H ? v : 0.f;
                        if (rok[r] && lok[j]) p.out[rbase[r] + (size_t)u * lc[j]] = v;
                    }
                }
            }
        }
    }
};

// [Co, Ci, 5] -> the PLAIN-layout pack (conv_mfma.h header) of the two-tap GEMM with 3 Ci rows and Co reduction channels:
// tap 0 multiplies d[q] (k = f + 2), tap 1 d[q + 1] (k = f - 1; absent for f = 0).  CK = 32 for K = 2.
__global__ void period_pack3_kernel(const float *__restrict__ w, float *__restrict__ wp, int Co, int Ci, int Q, size_t total)
{
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        const size_t gq = idx >> 8;
        const int q = (int)(gq % Q), mb = (int)(gq / Q);
        const int chunk = q / 8, rem = q % 8, tap = rem / 4, g = rem % 4;
        const int co = chunk * 32 + g * 8 + 2 * e + (lane >> 5), row = mb * 32 + (lane & 31);
        float v = 0.f;
        if (row < 3 * Ci && co < Co) {
            const int ci = row / 3, f = row - ci * 3;
            const int k = tap == 0 ? f + 2 : f - 1;
            if (k >= 0) v = w[((size_t)co * Ci + ci) * 5 + k];
        }
        wp[idx] = v;
    }
}

// thread = one column of in0
__global__ void period_fold_fwd_kernel(const float *__restrict__ y, float *__restrict__ in0, int N, int T, int p, int H0,
                                       int S0)
{
    const long total = (long)N * p * S0;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const int r = (int)(e / S0), hh = (int)(e % S0);
        const int n = r / p, w = r - n * p;
        float v = 0.f;
        if (hh < H0) {
            int t = hh * p + w;
            t = t >= T ? 2 * (T - 1) - t : t;
            v = y[(long)n * T + t];
        }
        in0[e] = v;
    }
}

// thread = one sample: its own column, then the column of the pad sample that mirrors it (t' = 2 (T - 1) - t in [T, H0 p))
__global__ void period_fold_bwd_kernel(const float *__restrict__ din0, float *__restrict__ dy, int N, int T, int p, int H0,
                                       int S0)
{
    const long total = (long)N * T;
    for (long e = blockIdx.x * 256l + threadIdx.x; e < total; e += gridDim.x * 256l) {
        const int n = (int)(e / T), t = (int)(e % T);
        float s = din0[((long)n * p + t % p) * S0 + t / p];
        const int tm = 2 * (T - 1) - t;
        if (tm >= T && tm < H0 * p) s += din0[((long)n * p + tm % p) * S0 + tm / p];
        dy[e] = s;
    }
}

int blocks_for(long n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

int fold_check(int N, int T, int p, int *H0, int *S0)
{
    int H[7], S[7];
    if (N < 1) return MG_ERR_SHAPE;
    MG_TRY(mg_period_geometry(T, p, H, S));
    if ((long)N * p * S[0] >= (1l << 30) || (long)N * T >= (1l << 30)) return MG_ERR_SHAPE;
    *H0 = H[0], *S0 = S[0];
    return MG_OK;
}

// the checks the two convolution entry points share; Hm / Sm: the slot mask's height and width
int period_check(int R, int Ci, int Lin, int S_in, int Co, int Lout, int S_out, int K, int stride, int Hm, int Sm)
{
    if (R < 1 || Ci < 1 || Co < 1 || S_in < 1 || S_out < 1) return MG_ERR_SHAPE;
    if (!((K == 5 && (stride == 3 || stride == 1)) || (K == 3 && stride == 1))) return MG_ERR_SHAPE;
    if ((long)R * S_in >= (1l << 30)) return MG_ERR_SHAPE;
    if ((long)Lin != (long)R * S_in || (long)Lout != (long)R * S_out || (long)S_in != (long)stride * S_out)
        return MG_ERR_SHAPE;
    if (Hm < 1 || Hm > Sm - 2) return MG_ERR_SHAPE;
    if ((long)Ci * Lin >= (1l << 40) || (long)Co * Lout >= (1l << 40)) return MG_ERR_SHAPE;
    return MG_OK;
}

}   // namespace

extern "C" int mg_period_fold_fwd(const float *y, float *in0, int N, int T, int p, void *stream)
{
    if (!y || !in0) return MG_ERR_ARG;
    int H0, S0;
    MG_TRY(fold_check(N, T, p, &H0, &S0));
    hipLaunchKernelGGL(period_fold_fwd_kernel, dim3(blocks_for((long)N * p * S0)), dim3(256), 0, (hipStream_t)stream, y, in0,
                       N, T, p, H0, S0);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_period_fold_bwd(const float *din0, float *dy, int N, int T, int p, void *stream)
{
    if (!din0 || !dy) return MG_ERR_ARG;
    int H0, S0;
    MG_TRY(fold_check(N, T, p, &H0, &S0));
    hipLaunchKernelGGL(period_fold_bwd_kernel, dim3(blocks_for((long)N * T)), dim3(256), 0, (hipStream_t)stream, din0, dy, N,
                       T, p, H0, S0);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_period_conv_fwd(const float *in, const float *packed, const float *bias, float *out, int R, int Ci, int Lin,
                                  int S_in, int Co, int Lout, int S_out, int H_out, int K, int stride, int act, float slope,
                                  float *scratch, size_t scratch_floats, void *stream)
{
    if (!in || !packed || !out) return MG_ERR_ARG;
    if (act != MG_ACT_NONE && act != MG_ACT_LRELU) return MG_ERR_ARG;
    MG_TRY(period_check(R, Ci, Lin, S_in, Co, Lout, S_out, K, stride, H_out, S_out));
    ConvShape s{1, Ci, Lin, Lout, K, stride, (K - 1) / 2, Co, 0, 0, 1, 1.f, scratch, scratch ? scratch_floats : 0};
    EpiPeriod::Params ep{out, bias, nullptr, nullptr, slope, 0.f, Co, act, 1, S_out, H_out};
    return conv_launch<EpiPeriod, CONV_CASES_PERIOD>(s, in, nullptr, packed, ep, (hipStream_t)stream);
}

extern "C" size_t mg_period_dgrad3_packed_floats(int Co, int Ci)
{
    if (Co < 1 || Ci < 1 || (long)Ci * 3 >= (1l << 24) || Co >= (1 << 24)) return 0;
    return (size_t)mg_conv_mblocks(3 * Ci) * mg_conv_qcount(mg_round_up(Co, mg_conv_ck(2)), 2) * 256;
}

extern "C" int mg_period_dgrad3_pack(const float *w, float *packed, int Co, int Ci, void *stream)
{
    if (!w || !packed) return MG_ERR_ARG;
    const size_t total = mg_period_dgrad3_packed_floats(Co, Ci);
    if (!total) return MG_ERR_SHAPE;
    const int Q = mg_conv_qcount(mg_round_up(Co, mg_conv_ck(2)), 2);
    hipLaunchKernelGGL(period_pack3_kernel, dim3(blocks_for((long)total)), dim3(256), 0, (hipStream_t)stream, w, packed, Co,
                       Ci, Q, total);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_period_conv_dgrad(const float *d, const float *packed, const float *map, const float *add, float *dx, int R,
                                    int Ci, int Lin, int S_in, int H_in, int Co, int Lout, int S_out, int K, int stride,
                                    float slope, float *scratch, size_t scratch_floats, void *stream)
{
    if (!d || !packed || !dx) return MG_ERR_ARG;
    MG_TRY(period_check(R, Ci, Lin, S_in, Co, Lout, S_out, K, stride, H_in, S_in));
    const size_t nscr = scratch ? scratch_floats : 0;
    if (stride == 3) {   // GEMM rows ci 3 + f over columns q < Lout; the epilogue interleaves the phases into dx
        ConvShape s{1, Co, Lout, Lout, 2, 1, 0, 3 * Ci, 0, 0, 1, 1.f, scratch, nscr};
        EpiPeriod::Params ep{dx, nullptr, add, map, 0.f, slope, 3 * Ci, MG_ACT_NONE, 3, S_out, H_in};
        return conv_launch<EpiPeriod, CONV_CASES_PERIOD>(s, d, nullptr, packed, ep, (hipStream_t)stream);
    }
    ConvShape s{1, Co, Lout, Lin, K, 1, (K - 1) / 2, Ci, 0, 0, 1, 1.f, scratch, nscr};
    EpiPeriod::Params ep{dx, nullptr, add, map, 0.f, slope, Ci, MG_ACT_NONE, 1, S_in, H_in};
    return conv_launch<EpiPeriod, CONV_CASES_PERIOD>(s, d, nullptr, packed, ep, (hipStream_t)stream);
}
