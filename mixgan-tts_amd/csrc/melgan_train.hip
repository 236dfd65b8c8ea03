// Backward of the MelGAN generator's reflect-padded convolutions (melgan.py forward_train; the forward is melgan.hip's
// mg_conv1d_reflect_fwd):   y = act(alpha * W (*)_dil reflect_p(lrelu(x, in_slope)) + b),   p = dil (K - 1) / 2,
// refl(j) = -j for j < 0, 2 (L - 1) - j for j >= L (p < L: one mirror is enough).
//
//   mg_conv1d_reflect_wgrad   dW[co,ci,k] = alpha * sum_{b,l} dy[b,co,l] lrelu(x)[b,ci, refl(l + k dil - p)]:
//                             wgrad_tile_kernel<.., REFLECT> (wgrad_mfma.h) -- the column operand's staging mirrors the
//                             frame index where the zero-padded gradient drops the value; same split walk, same
//                             finalize, so the bits repeat run to run
//   mg_conv1d_reflect_dgrad   (a) P = alpha * dy (*) W^T with the taps flipped, zero padding 2p, over the PADDED length
//                                 L + 2p: the forward conv kernel on the MG_PACK_DGRAD pack (K = 3 at dilation <= 9 has
//                                 its own case list, CONV_CASES_DIL9; K = 7 is mg_conv1d_fwd_ex's)
//                             (b) mg_reflect_fold_bwd
//   mg_reflect_fold_bwd       da[i] = P[i+p] + [1 <= i <= p] P[p-i] + [L-1-p <= i <= L-2] P[2(L-1)-i+p] (the gradient of
//                             each mirrored position returns to the sample it copied; for L <= 2p both mirrors can
//                             reach one i), dx = da * (x > 0 ? 1 : slope) (+ add).  One thread per output element, three
//                             loads in a fixed order, one store into the dense out.  With p = 0 it is mg_lrelu_bwd with batch strides, which
//                             is how the ResnetBlock masks dt inside its [B, 2C, L] gradient buffer.
//
// The ResnetBlock's backward (autograd.melgan_resblock) is launches of these and of the K = 1 data / weight gradients
// the library already has, over [B, 2C, L] buffers; nothing loops over batch items and nothing reads the device.
#include "conv_mfma.h"
#include "wgrad_mfma.h"

struct EpiDil9 : EpiBiasAct {};   // EpiBiasAct under the name this file's kernels carry; its cases are CONV_CASES_DIL9

namespace {

bool mt_case_ok(int K, int dil) { return dil >= 1 && ((K == 3 && dil <= 9) || (K == 7 && dil == 1)); }

struct FoldArgs {
    const float *P, *x, *add;
    float *out;
    long p_bs, x_bs, add_bs;
    int C, L, p;
    float slope;
    size_t n;   // B * C * L
};

__global__ __launch_bounds__(256) void mt_fold_kernel(FoldArgs a)
{
    const int Lp = a.L + 2 * a.p;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < a.n; idx += (size_t)gridDim.x * 256) {
        const int i = (int)(idx % a.L);
        const size_t row = idx / a.L;
        const int c = (int)(row % a.C);
        const size_t b = row / a.C;
        const float *pr = a.P + b * a.p_bs + (size_t)c * Lp;
        const size_t e = (size_t)c * a.L + i;
        float v = pr[i + a.p];
        if (i >= 1 && i <= a.p) v += pr[a.p - i];
        if (i >= a.L - 1 - a.p && i <= a.L - 2) v += pr[2 * (a.L - 1) - i + a.p];
        if (a.x) v *= a.x[b * a.x_bs + e] > 0.f ? 1.f : a.slope;
        if (a.add) v += a.add[b * a.add_bs + e];
        a.out[row * a.L + i] = v;
    }
}

}  // namespace

extern "C" int mg_reflect_fold_bwd(const float *P, long p_bs, const float *x, long x_bs, const float *add, long add_bs,
                                   float *out, int B, int C, int L, int p, float slope, void *stream)
{
    if (!P || !out) return MG_ERR_ARG;
    if (B <= 0 || C <= 0 || L <= 0 || p < 0 || L <= p) return MG_ERR_SHAPE;
    const long plane = (long)C * L, pplane = (long)C * (L + 2l * p);
    if (pplane >= (1l << 31)) return MG_ERR_SHAPE;
    if (p_bs < 0 || x_bs < 0 || add_bs < 0) return MG_ERR_SHAPE;
    if ((p_bs && p_bs < pplane) || (x_bs && x_bs < plane) || (add_bs && add_bs < plane)) return MG_ERR_SHAPE;
    FoldArgs a{P, x, add, out, p_bs ? p_bs : pplane, x_bs ? x_bs : plane, add_bs ? add_bs : plane, C, L, p, slope,
               (size_t)B * C * L};
    const size_t blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(mt_fold_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, a);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_conv1d_reflect_wgrad(const float *dy, long dy_bs, const float *x, long x_bs, float *dw, float *scratch,
                                       int B, int Co, int Ci, int L, int K, int dil, float in_slope, float alpha,
                                       int accumulate, void *stream)
{
    if (!dy || !x || !dw || !scratch) return MG_ERR_ARG;
    if (B <= 0 || Co <= 0 || Ci <= 0 || L <= 0 || dy_bs < 0 || x_bs < 0) return MG_ERR_SHAPE;
    if (!mt_case_ok(K, dil)) return MG_ERR_SHAPE;
    const int p = dil * (K - 1) / 2;
    if (L <= p) return MG_ERR_SHAPE;   // ReflectionPad1d needs p < L
    const long dbs = dy_bs ? dy_bs : (long)Co * L, xbs = x_bs ? x_bs : (long)Ci * L;
    if (dbs < (long)Co * L || xbs < (long)Ci * L) return MG_ERR_SHAPE;
    return wgrad_tile_launch<true>(dy, dbs, 1.f, x, xbs, in_slope, dw, scratch, B, Co, Ci, L, L, K, 1, dil, p, alpha,
                                   accumulate, (hipStream_t)stream);
}

extern "C" size_t mg_conv1d_reflect_dgrad_workspace_floats(int B, int Ci, int L, int K, int dil)
{
    if (B <= 0 || Ci <= 0 || L <= 0 || !mt_case_ok(K, dil)) return 0;
    return (size_t)B * Ci * ((size_t)L + (size_t)dil * (K - 1));
}

extern "C" int mg_conv1d_reflect_dgrad(const float *dy, const float *packed, const float *x, long x_bs, const float *add,
                                       long add_bs, float *dx, float *workspace, size_t workspace_floats, int B, int Co,
                                       int Ci, int L, int K, int dil, float in_slope, float alpha, void *stream)
{
    if (!dy || !packed || !x || !dx || !workspace) return MG_ERR_ARG;
    if (B <= 0 || Co <= 0 || Ci <= 0 || L <= 0 || x_bs < 0 || add_bs < 0) return MG_ERR_SHAPE;
    if (!mt_case_ok(K, dil)) return MG_ERR_SHAPE;
    const int p = dil * (K - 1) / 2;
    if (L <= p) return MG_ERR_SHAPE;
    const long plane = (long)Ci * L;
    if ((x_bs && x_bs < plane) || (add_bs && add_bs < plane) || (long)Ci * (L + 2l * p) >= (1l << 31)) return MG_ERR_SHAPE;
    if (workspace_floats < mg_conv1d_reflect_dgrad_workspace_floats(B, Ci, L, K, dil)) return MG_ERR_WORKSPACE;
    const int Lp = L + 2 * p;
    if (K == 3) {
        ConvShape s{B, Co, L, Lp, 3, 1, 2 * p, Ci, 0, 0, dil, 1.f};
        EpiBiasAct::Params ep{workspace, nullptr, nullptr, alpha, Ci, MG_ACT_NONE, 0, 0, nullptr, 0.f};
        MG_TRY((conv_launch<EpiDil9, CONV_CASES_DIL9>(s, dy, nullptr, packed, ep, (hipStream_t)stream)));
    } else {
        MG_TRY(mg_conv1d_fwd_ex(dy, nullptr, packed, nullptr, nullptr, workspace, B, Co, L, Ci, Lp, K, 1, 2 * p, 1, 1.f,
                                MG_ACT_NONE, 0.f, alpha, 0, stream));
    }
    return mg_reflect_fold_bwd(workspace, 0, x, x_bs, add, add_bs, dx, B, Ci, L, p, in_slope, stream);
}
