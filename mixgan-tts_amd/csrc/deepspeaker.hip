// DeepSpeaker ResCNN speaker embedder (reference deepspeaker/audio_ds.py, batcher.py, conv_models.py): the fbank
// front end of the 160 cropped frames, the NHWC 2-D convolutions of the four ResCNN stages with folded BatchNorm and
// clipped-ReLU epilogues, and the head (time mean, Dense 2048 -> 512, l2 normalisation).
//
// Front end (grid: frame pairs x batch, one wave): frame f = offset + t of item b covers trimmed samples
// [f step, f step + frame_len) of audio[b, start : end), zero past the end; pre-emphasis y[i] = x[i] - 0.97 x[i-1]
// (y[0] = x[0]) is applied on the fly.  Two frames go through one 1024-point complex FFT (stft_pair.h), the power
// spectrum |X|^2 / 1024 through the banded triangular filters (lane m owns filter m), exact zeros become DBL_EPSILON
// and each frame is normalised over its filters by its population std (floored at 1e-12).  Rows at or past the
// item's frame count are zeros, as sample_from_mfcc pads.
//
// Convolution: activations NHWC, weights packed [K = (kh KS + kw) Ci + ci][Co] (the Keras HWIO kernel flattened, BN
// folded in).  An implicit GEMM: rows are output positions flattened over (n, oh, ow) across the whole batch, columns
// are output channels, K runs over the taps.  A workgroup of four waves owns a BM x BN tile (128 x 128, or 256 x 64
// when Co is not a multiple of 128), each wave a 64 x 64 quarter as 2 x 2 tiles of v_mfma_f32_32x32x2_f32.  Per
// 32-wide K step (one tap, 32 input channels: Ci % 32 == 0) the A tile is gathered straight from the input with TF
// 'same' padding (zeros outside), the B tile is 32 contiguous weight rows; both go through registers into LDS while
// the previous step's MFMAs run.  Inside a K step, MFMA s takes k = 16 h + s from lane half h, so a lane reads its
// 16 A values with four 16-byte LDS reads.  The sum order over K is fixed per output element, so an utterance's
// output does not depend on the batch around it.  Epilogue: + bias, clip to [0, 20], then optionally + residual and
// clip again.  Layers with Ci % 32 != 0 (the Ci = 1 first conv) take a direct VALU kernel.
#include "common.h"
#include "stft_pair.h"

#include <float.h>

namespace {

constexpr int N = MG_STFT_N;  // 1024-point FFT
constexpr int NB = N / 2 + 1;
constexpr float CLIP = 20.f;

struct FbankArgs {
    const float *x;
    long x_bs;
    const int *start, *end, *offset;
    int frames, frame_len, frame_step, nfilt;
    const float2 *tw;
    const int *band;  // start [nfilt], length [nfilt], offset into band_w [nfilt]
    const float *band_w;
    float *out;  // [B, frames, nfilt]
};

__device__ __forceinline__ float ds_preemph(const float *x, int i, int slen)
{
    if (i >= slen) return 0.f;
    return i == 0 ? x[0] : x[i] - 0.97f * x[i - 1];
}

__global__ __launch_bounds__(64) void ds_fbank_kernel(FbankArgs a)
{
    __shared__ float2 d[N];
    __shared__ float pw[2 * NB];
    const int lane = threadIdx.x, b = blockIdx.y, t0 = 2 * blockIdx.x;
    const int st = a.start[b], slen = a.end[b] - st;
    const int nfr = slen <= a.frame_len ? 1 : 1 + (slen - a.frame_len + a.frame_step - 1) / a.frame_step;
    const int f0 = a.offset[b] + t0;
    const bool va = f0 < nfr, vb = f0 + 1 < nfr && t0 + 1 < a.frames;
    float *out = a.out + ((size_t)b * a.frames + t0) * a.nfilt;
    if (!va) {
        for (int m = lane; m < a.nfilt; m += 64) {
            out[m] = 0.f;
            if (t0 + 1 < a.frames) out[a.nfilt + m] = 0.f;
        }
        return;
    }
    const float *x = a.x + (size_t)b * a.x_bs + st;
    const int ia = f0 * a.frame_step, ib = ia + a.frame_step;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = lane + 64 * i;
        float2 z = make_float2(0.f, 0.f);
        if (n < a.frame_len) {
            z.x = ds_preemph(x, ia + n, slen);
            if (vb) z.y = ds_preemph(x, ib + n, slen);
        }
        d[n] = z;
    }
    __syncthreads();
    mg_fft1024(d, a.tw, lane);
    for (int k = lane; k < NB; k += 64) {
        float ar, ai, br, bi;
        mg_pair_split(d, k, ar, ai, br, bi);
        pw[k] = (ar * ar + ai * ai) * (1.f / N);
        pw[NB + k] = (br * br + bi * bi) * (1.f / N);
    }
    __syncthreads();
    float s0 = 0.f, s1 = 0.f;
    const bool own = lane < a.nfilt;
    if (own) {
        mg_pair_band_sum(a.band, a.band_w, a.nfilt, lane, pw, s0, s1);
        s0 = s0 == 0.f ? (float)DBL_EPSILON : s0;
        s1 = s1 == 0.f ? (float)DBL_EPSILON : s1;
    }
    // population mean / std over the filters of each frame (lanes past nfilt contribute nothing)
    float m0 = own ? s0 : 0.f, m1 = own ? s1 : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m0 += __shfl_xor(m0, off);
        m1 += __shfl_xor(m1, off);
    }
    m0 /= a.nfilt;
    m1 /= a.nfilt;
    float v0 = own ? (s0 - m0) * (s0 - m0) : 0.f, v1 = own ? (s1 - m1) * (s1 - m1) : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v0 += __shfl_xor(v0, off);
        v1 += __shfl_xor(v1, off);
    }
    const float sd0 = fmaxf(sqrtf(v0 / a.nfilt), 1e-12f), sd1 = fmaxf(sqrtf(v1 / a.nfilt), 1e-12f);
    if (own) {
        out[lane] = (s0 - m0) / sd0;
        if (t0 + 1 < a.frames) out[a.nfilt + lane] = vb ? (s1 - m1) / sd1 : 0.f;
    }
}

struct ConvArgs {
    const float *x;     // [Nb, H, W, Ci]
    const float *w;     // [KS KS Ci, Co]
    const float *bias;  // [Co]
    const float *res;   // [P, Co] or null
    float *y;           // [P, Co], P = Nb Ho Wo
    int H, W, Ci, Ho, Wo, Co, ks, stride, pt, pl, P;
};

__device__ __forceinline__ float ds_epilogue(float v, const float *res, size_t o)
{
    v = fminf(fmaxf(v, 0.f), CLIP);
    if (res) v = fminf(fmaxf(v + res[o], 0.f), CLIP);
    return v;
}

constexpr int BK = 32, APAD = 4, THREADS = 256;

// WM waves along the positions, 4 / WM along the channels; each wave owns 64 x 64.
template <int WM>
__global__ __launch_bounds__(THREADS) void ds_conv2d_mfma_kernel(ConvArgs a)
{
    constexpr int WN = 4 / WM, BM = 64 * WM, BN = 64 * WN;
    constexpr int AJ = BM / 32;                   // A float4 loads per thread (8 threads per position row)
    constexpr int BC4 = BN / 4, BJ = BK * BC4 / THREADS;  // B float4 loads per thread
    __shared__ float As[BM][BK + APAD];
    __shared__ float Bs[BK][BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int wm = wave % WM, wn = wave / WM;
    const int HWo = a.Ho * a.Wo;

    // per-thread A rows: position p = m0 + (tid >> 3) + 32 j, float4 chunk tid & 7 of the 32-wide K step
    const int ac = tid & 7;
    int abase[AJ], aih[AJ], aiw[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int p = m0 + (tid >> 3) + 32 * j;
        if (p < a.P) {
            const int n = p / HWo, r = p - n * HWo, oh = r / a.Wo, ow = r - oh * a.Wo;
            abase[j] = n * a.H * a.W;
            aih[j] = oh * a.stride - a.pt;
            aiw[j] = ow * a.stride - a.pl;
        } else {
            abase[j] = 0;
            aih[j] = -(1 << 20);  // never inside the image
            aiw[j] = 0;
        }
    }
    const int bc = tid % BC4, br = tid / BC4;

    const int K = a.ks * a.ks * a.Ci, nK = K / BK;
    float4 ra[AJ], rb[BJ];
    auto load = [&](int kt) {
        const int k0 = kt * BK, tap = k0 / a.Ci, ci0 = k0 - tap * a.Ci;
        const int kh = tap / a.ks, kw = tap - kh * a.ks;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int ih = aih[j] + kh, iw = aiw[j] + kw;
            if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
                ra[j] = *(const float4 *)(a.x + ((size_t)(abase[j] + ih * a.W + iw) * a.Ci + ci0 + 4 * ac));
            else
                ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j)
            rb[j] = *(const float4 *)(a.w + ((size_t)(k0 + br + (THREADS / BC4) * j) * a.Co + n0 + 4 * bc));
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < AJ; ++j) *(float4 *)&As[(tid >> 3) + 32 * j][4 * ac] = ra[j];
#pragma unroll
        for (int j = 0; j < BJ; ++j) *(float4 *)&Bs[br + (THREADS / BC4) * j][4 * bc] = rb[j];
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int l32 = lane & 31, h = lane >> 5;
    load(0);
    store();
    __syncthreads();
    for (int kt = 0; kt < nK; ++kt) {
        if (kt + 1 < nK) load(kt + 1);
        float av[2][16];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *(const float4 *)&As[wm * 64 + i * 32 + l32][16 * h + 4 * q];
                av[i][4 * q] = v.x;
                av[i][4 * q + 1] = v.y;
                av[i][4 * q + 2] = v.z;
                av[i][4 * q + 3] = v.w;
            }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float b0 = Bs[16 * h + s][wn * 64 + l32], b1 = Bs[16 * h + s][wn * 64 + 32 + l32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][s], b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][s], b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < nK) {
            store();
            __syncthreads();
        }
    }

    // C/D map of 32x32: column lane & 31 (channel), row (r & 3) + 8 (r >> 2) + 4 h (position)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = n0 + wn * 64 + j * 32 + l32;
        const float bv = a.bias[co];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (p < a.P) {
                    const size_t o = (size_t)p * a.Co + co;
                    a.y[o] = ds_epilogue(acc[i][j][r] + bv, a.res, o);
                }
            }
    }
}

// Direct convolution for layers whose Ci is not a multiple of 32 (the Ci = 1 first conv): one thread per output
// element, taps in (kh, kw, ci) order.
__global__ __launch_bounds__(256) void ds_conv2d_direct_kernel(ConvArgs a)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)a.P * a.Co) return;
    const int co = (int)(e % a.Co), p = (int)(e / a.Co);
    const int HWo = a.Ho * a.Wo;
    const int n = p / HWo, r = p - n * HWo, oh = r / a.Wo, ow = r - oh * a.Wo;
    const float *x = a.x + (size_t)n * a.H * a.W * a.Ci;
    float s = 0.f;
    for (int kh = 0; kh < a.ks; ++kh) {
        const int ih = oh * a.stride - a.pt + kh;
        if (ih < 0 || ih >= a.H) continue;
        for (int kw = 0; kw < a.ks; ++kw) {
            const int iw = ow * a.stride - a.pl + kw;
            if (iw < 0 || iw >= a.W) continue;
            const float *xp = x + ((size_t)ih * a.W + iw) * a.Ci;
            const float *wp = a.w + ((size_t)(kh * a.ks + kw) * a.Ci) * a.Co + co;
            for (int ci = 0; ci < a.Ci; ++ci) s = fmaf(xp[ci], wp[(size_t)ci * a.Co], s);
        }
    }
    a.y[e] = ds_epilogue(s + a.bias[co], a.res, (size_t)e);
}

// Head: one workgroup of O threads per utterance.  m = mean over the `rows` rows of x[b] ([rows, D], NHWC order, so
// column w C + c as Keras's Reshape), out = l2_normalize(m W + bias).
__global__ __launch_bounds__(512) void ds_head_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                      const float *__restrict__ bias, float *__restrict__ out, int rows,
                                                      int D, int O)
{
    extern __shared__ float sm[];  // [D] mean, then [O / 64] partial sums
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *xb = x + (size_t)b * rows * D;
    for (int k = tid; k < D; k += blockDim.x) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += xb[(size_t)r * D + k];
        sm[k] = s / rows;
    }
    __syncthreads();
    float v = 0.f;
    if (tid < O) {
        v = bias[tid];
        for (int k = 0; k < D; ++k) v = fmaf(sm[k], w[(size_t)k * O + tid], v);
    }
    float ss = tid < O ? v * v : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    float *part = sm + D;
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    float tot = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) tot += part[i];
    if (tid < O) out[(size_t)b * O + tid] = v * rsqrtf(fmaxf(tot, 1e-12f));
}

}  // namespace

// TF 'same': out = ceil(n / stride), pad_total = max((out - 1) stride + k - n, 0), pad_total / 2 before.
static void ds_same_padding(int n, int k, int stride, int *out_size, int *pad_before, int *pad_after)
{
    const int o = (n + stride - 1) / stride;
    int total = (o - 1) * stride + k - n;
    total = total < 0 ? 0 : total;
    *out_size = o;
    *pad_before = total / 2;
    *pad_after = total - total / 2;
}

extern "C" int mg_ds_fbank(const float *audio, long x_bs, const int *start, const int *end, const int *offset, int B,
                           int frames, int frame_len, int frame_step, const float *twiddle, const int *band,
                           const float *band_w, int nfilt, float *out, void *stream)
{
    if (!audio || !start || !end || !offset || !twiddle || !band || !band_w || !out) return MG_ERR_ARG;
    if (B <= 0 || frames <= 0 || frame_len <= 0 || frame_len > N || frame_step <= 0 || nfilt <= 0 || nfilt > 64)
        return MG_ERR_SHAPE;
    FbankArgs a;
    a.x = audio;
    a.x_bs = x_bs;
    a.start = start;
    a.end = end;
    a.offset = offset;
    a.frames = frames;
    a.frame_len = frame_len;
    a.frame_step = frame_step;
    a.nfilt = nfilt;
    a.tw = (const float2 *)twiddle;
    a.band = band;
    a.band_w = band_w;
    a.out = out;
    hipLaunchKernelGGL(ds_fbank_kernel, dim3(mg_cdiv(frames, 2), B), dim3(64), 0, (hipStream_t)stream, a);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_ds_conv2d(const float *x, const float *w, const float *bias, const float *res, float *y, int Nb,
                            int H, int W, int Ci, int Co, int ks, int stride, void *stream)
{
    if (!x || !w || !bias || !y) return MG_ERR_ARG;
    if (Nb <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || Co % 64 || ks <= 0 || stride <= 0) return MG_ERR_SHAPE;
    ConvArgs a;
    int pb;
    a.x = x;
    a.w = w;
    a.bias = bias;
    a.res = res;
    a.y = y;
    a.H = H;
    a.W = W;
    a.Ci = Ci;
    a.Co = Co;
    a.ks = ks;
    a.stride = stride;
    ds_same_padding(H, ks, stride, &a.Ho, &a.pt, &pb);
    ds_same_padding(W, ks, stride, &a.Wo, &a.pl, &pb);
    const long P = (long)Nb * a.Ho * a.Wo;
    if (P * (long)(Co > Ci ? Co : Ci) >= (1L << 31) || (long)Nb * H * W * Ci >= (1L << 31)) return MG_ERR_SHAPE;
    a.P = (int)P;
    hipStream_t s = (hipStream_t)stream;
    if (Ci % BK) {
        hipLaunchKernelGGL(ds_conv2d_direct_kernel, dim3((unsigned)((P * Co + 255) / 256)), dim3(256), 0, s, a);
    } else if (Co % 128 == 0) {
        hipLaunchKernelGGL(ds_conv2d_mfma_kernel<2>, dim3(mg_cdiv(a.P, 128), Co / 128), dim3(THREADS), 0, s, a);
    } else {
        hipLaunchKernelGGL(ds_conv2d_mfma_kernel<4>, dim3(mg_cdiv(a.P, 256), Co / 64), dim3(THREADS), 0, s, a);
    }
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_ds_head(const float *x, const float *w, const float *bias, float *out, int B, int rows, int D, int O,
                          void *stream)
{
    if (!x || !w || !bias || !out) return MG_ERR_ARG;
    if (B <= 0 || rows <= 0 || D <= 0 || O <= 0 || O > 512 || O % 64 || D > 8192) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(ds_head_kernel, dim3(B), dim3(O), (D + O / 64) * sizeof(float), (hipStream_t)stream, x, w, bias,
                       out, rows, D, O);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
