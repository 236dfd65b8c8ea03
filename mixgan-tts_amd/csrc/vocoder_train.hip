// Backward of the HiFi-GAN generator (vocoder.py forward_train) and of the log-mel (audio.py mel_spectrogram_diff).
//
//   mg_lrelu_bwd                  out = dy * (x > 0 ? 1 : slope) (+ add): the data gradient's mask and the residual add
//   mg_conv_transpose1d_dgrad     dy read as u phases of length L -> 3-tap implicit GEMM with Ci rows over Co*u
//                                 channels on the forward conv kernel (K = 3 case), then the mask
//   mg_stft_mel_bwd               gradient of mg_stft_mel's mel with respect to the signal: per frame pair, recompute
//                                 the spectrum, band-form basis^T, the ADJOINT of the one-sided windowed DFT (one
//                                 complex FFT for two frames), windowed frame gradients into a workspace; a gather pass
//                                 overlap-adds them and folds the reflect padding, frames in ascending order
//
// Every result is reproducible run to run: no atomics, fixed summation orders.
//
// The two weight gradients (mg_conv1d_wgrad_ex, mg_conv_transpose1d_wgrad) are in conv_api.hip, on wgrad_tile_kernel of
// wgrad_mfma.h.
#include "common.h"
#include "stft_pair.h"

namespace {

bool vt_u_ok(int u) { return u == 2 || u == 4 || u == 8; }

// ---------------------------------------------------------------------------------------------
// elementwise pieces
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_lrelu_bwd_kernel(const float *dy, const float *__restrict__ x, const float *add,
                                                           float *out, float slope, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v = dy[i] * (x[i] > 0.f ? 1.f : slope);
        if (add) v += add[i];
        out[i] = v;
    }
}

// w [Ci, Co, 2u] -> w3 [Ci, Co*u, 3]: w3[ci, co*u + p, t] = w[ci, co, u*(t-1) + p + u/2] where that tap exists
__global__ __launch_bounds__(256) void vt_tpose_w3_kernel(const float *__restrict__ w, float *__restrict__ w3, size_t n, int u)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % 3);
        const size_t q = i / 3;                 // (ci*Co + co)*u + p
        const int p = (int)(q % u);
        const size_t cc = q / u;                // ci*Co + co
        const int k = u * (t - 1) + p + u / 2;
        w3[i] = (k >= 0 && k < 2 * u) ? w[cc * 2 * u + k] : 0.f;
    }
}

// dy [rows, u*L] -> dyp [rows*u, L]: dyp[r*u + p, t] = dy[r, u*t + p]
__global__ __launch_bounds__(256) void vt_phase_split_kernel(const float *__restrict__ dy, float *__restrict__ dyp, size_t n,
                                                             int u, int L)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % L);
        const size_t q = i / L;                 // r*u + p
        const int p = (int)(q % u);
        const size_t r = q / u;
        dyp[i] = dy[(r * L + t) * u + p];
    }
}

int vt_blocks(size_t n) { return (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192); }

size_t vt_tpose_packed_floats(int Ci, int Co, int u) { return mg_conv_packed_floats(Ci, Co * u, 3, MG_PACK_PLAIN); }

// ---------------------------------------------------------------------------------------------
// log-mel backward
// ---------------------------------------------------------------------------------------------
constexpr int N = MG_STFT_N;
constexpr int NB = N / 2 + 1;

struct MelBwdArgs {
    const float *x;
    long x_bs;
    int L, hop, T;
    const float *window;
    const float2 *tw;
    const int *band;
    const float *band_w;
    int n_mels;
    const float *dmel;   // [B, n_mels, T]
    float *frames;       // [B, T, N] windowed frame gradients
};

// One wave, two frames: the forward's spectrum and band sums (stft_pair.h's staging, split and sum, as stft_fwd_body
// calls them), then the chain rule down to the frame samples.
__global__ __launch_bounds__(64) void stft_mel_bwd_frames_kernel(MelBwdArgs a)
{
    __shared__ float2 d[N];
    __shared__ float2 spa[NB], spb[NB];          // A[k], B[k] of the two frames
    __shared__ float mags[2 * NB];
    __shared__ float dm[2 * MG_STFT_MAX_MELS];
    const int lane = threadIdx.x, b = blockIdx.y, t0 = 2 * blockIdx.x;
    const int Lb = a.L;
    const bool fb = t0 + 1 < 1 + Lb / a.hop;   // the forward transforms frame t0 + 1 whenever the signal has it
    const bool vb = t0 + 1 < a.T;              // ... but only T frames carry a gradient

    mg_pair_stage(d, a.x + (size_t)b * a.x_bs, Lb, a.hop, t0, a.window, fb, lane);
    __syncthreads();
    mg_fft1024(d, a.tw, lane);

    for (int k = lane; k < NB; k += 64) {
        float ar, ai, br, bi;
        mg_pair_split(d, k, ar, ai, br, bi);
        spa[k] = make_float2(ar, ai);
        spb[k] = make_float2(br, bi);
        mags[k] = sqrtf(ar * ar + ai * ai);
        mags[NB + k] = sqrtf(br * br + bi * bi);
    }
    __syncthreads();

    // dm = dmel * [m >= 1e-5] / m, m = basis |X| summed as in the forward
    const float *dmel = a.dmel + (size_t)b * a.n_mels * a.T;
    for (int m = lane; m < a.n_mels; m += 64) {
        float s0, s1;
        mg_pair_band_sum(a.band, a.band_w, a.n_mels, m, mags, s0, s1);
        dm[m] = s0 >= 1e-5f ? dmel[(size_t)m * a.T + t0] / s0 : 0.f;
        dm[MG_STFT_MAX_MELS + m] = (vb && s1 >= 1e-5f) ? dmel[(size_t)m * a.T + t0 + 1] / s1 : 0.f;
    }
    __syncthreads();

    // d|X|[k] = sum_m basis[m, k] dm[m] over the rows whose band holds k (ascending m), dX = d|X| X / |X|, then the
    // Hermitian halves of both one-sided gradients packed as conj(Ga' + i Gb') for one forward FFT
    for (int k = lane; k < NB; k += 64) {
        float ga = 0.f, gb = 0.f;
        for (int m = 0; m < a.n_mels; ++m) {
            const int st = a.band[m], len = a.band[a.n_mels + m];
            if (k >= st && k < st + len) {
                const float w = a.band_w[a.band[2 * a.n_mels + m] + (k - st)];
                ga = fmaf(w, dm[m], ga);
                gb = fmaf(w, dm[MG_STFT_MAX_MELS + m], gb);
            }
        }
        const float ma = mags[k], mb = mags[NB + k];
        const float sa = ma > 0.f ? ga / ma : 0.f, sb = mb > 0.f ? gb / mb : 0.f;
        const bool edge = k == 0 || k == N / 2;
        const float h = edge ? 1.f : 0.5f;       // an interior bin splits over k and N - k; the adjoint doubles nothing
        const float ra = h * sa * spa[k].x, ia = edge ? 0.f : h * sa * spa[k].y;
        const float rb = h * sb * spb[k].x, ib = edge ? 0.f : h * sb * spb[k].y;
        d[k] = make_float2(ra - ib, -(ia + rb));
        if (!edge) d[N - k] = make_float2(ra + ib, -(rb - ia));
    }
    __syncthreads();
    mg_fft1024(d, a.tw, lane);
    // frame t0's sample gradient is Re(d), frame t0 + 1's is -Im(d); no 1/N: this is the adjoint, not the inverse
    float *fa = a.frames + ((size_t)b * a.T + t0) * N;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = lane + 64 * i;
        const float w = a.window[n];
        fa[n] = w * d[n].x;
        if (vb) fa[N + n] = w * -d[n].y;
    }
}

// dx[b, j] = sum over the padded positions q that read sample j (itself, its left reflection, its right reflection,
// in that order), and per position over the frames that cover it in ascending order.
__global__ __launch_bounds__(256) void stft_mel_bwd_gather_kernel(const float *__restrict__ frames, float *__restrict__ dx,
                                                                  long dx_bs, int L, int hop, int T)
{
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= L) return;
    const float *fr = frames + (size_t)b * T * N;
    const int q3[3] = {j + N / 2, N / 2 - j, 2 * (L - 1) - j + N / 2};
    const bool ok3[3] = {true, j >= 1 && j <= N / 2, j <= L - 2};
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (!ok3[s]) continue;
        const int q = q3[s];
        int t_lo, t_hi;
        mg_pair_frame_range(q, hop, T, t_lo, t_hi);
        for (int t = t_lo; t <= t_hi; ++t) acc += fr[(size_t)t * N + (q - t * hop)];
    }
    dx[(size_t)b * dx_bs + j] = acc;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" int mg_lrelu_bwd(const float *dy, const float *x, const float *add, float *out, float slope, size_t n,
                            void *stream)
{
    if (!dy || !x || !out) return MG_ERR_ARG;
    if (n == 0) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(vt_lrelu_bwd_kernel, dim3(vt_blocks(n)), dim3(256), 0, (hipStream_t)stream, dy, x, add, out, slope, n);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_conv_transpose1d_dgrad_workspace_floats(int B, int Ci, int L, int Co, int u)
{
    if (B <= 0 || Ci <= 0 || Co <= 0 || L <= 0 || !vt_u_ok(u)) return 0;
    const size_t packed = vt_tpose_packed_floats(Ci, Co, u);
    if (!packed) return 0;
    // [phase view of dy | w3 | pack of w3], each rounded up to 16 bytes
    return mg_align_up((size_t)B * Co * u * L, 4) + mg_align_up((size_t)Ci * Co * u * 3, 4) + mg_align_up(packed, 4);
}

extern "C" int mg_conv_transpose1d_dgrad(const float *dy, const float *w, const float *x, float *dx, float *workspace,
                                         size_t workspace_floats, int B, int Ci, int L, int Co, int u, float in_slope,
                                         float alpha, void *stream)
{
    if (!dy || !w || !x || !dx || !workspace) return MG_ERR_ARG;
    if (B <= 0 || Ci <= 0 || Co <= 0 || L <= 0 || !vt_u_ok(u)) return MG_ERR_SHAPE;
    const size_t need = mg_conv_transpose1d_dgrad_workspace_floats(B, Ci, L, Co, u);
    if (!need) return MG_ERR_SHAPE;
    if (workspace_floats < need) return MG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t n_dyp = (size_t)B * Co * u * L, n_w3 = (size_t)Ci * Co * u * 3;
    float *dyp = workspace, *w3 = dyp + mg_align_up(n_dyp, 4), *packed = w3 + mg_align_up(n_w3, 4);
    hipLaunchKernelGGL(vt_tpose_w3_kernel, dim3(vt_blocks(n_w3)), dim3(256), 0, st, w, w3, n_w3, u);
    MG_LAUNCH_CHECK();
    MG_TRY(mg_conv_pack(w3, packed, Ci, Co * u, 3, MG_PACK_PLAIN, stream));
    hipLaunchKernelGGL(vt_phase_split_kernel, dim3(vt_blocks(n_dyp)), dim3(256), 0, st, dy, dyp, n_dyp, u, L);
    MG_LAUNCH_CHECK();
    MG_TRY(mg_conv1d_fwd_ex(dyp, nullptr, packed, nullptr, nullptr, dx, B, Co * u, L, Ci, L, 3, 1, 1, 1, 1.f, MG_ACT_NONE,
                            0.f, alpha, 0, stream));
    const size_t n = (size_t)B * Ci * L;
    hipLaunchKernelGGL(vt_lrelu_bwd_kernel, dim3(vt_blocks(n)), dim3(256), 0, st, dx, x, (const float *)nullptr, dx,
                       in_slope, n);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_stft_mel_bwd_workspace_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (size_t)B * T * N * sizeof(float);
}

extern "C" int mg_stft_mel_bwd(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                               const float *twiddle, const int *band, const float *band_w, int n_mels, const float *dmel,
                               int T, float *dx, long dx_bs, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !window || !twiddle || !band || !band_w || !dmel || !dx || !workspace) return MG_ERR_ARG;
    if (lengths) return MG_ERR_SHAPE;   // ragged items are not differentiated
    if (B <= 0 || !mg_stft_hop_ok(hop) || L <= N / 2 || T <= 0 || T > 1 + L / hop || x_bs < L || dx_bs < L || n_mels <= 0 ||
        n_mels > MG_STFT_MAX_MELS)
        return MG_ERR_SHAPE;
    if (workspace_bytes < mg_stft_mel_bwd_workspace_bytes(B, T)) return MG_ERR_WORKSPACE;
    MelBwdArgs a = {};
    a.x = x;
    a.x_bs = x_bs;
    a.L = L;
    a.hop = hop;
    a.T = T;
    a.window = window;
    a.tw = (const float2 *)twiddle;
    a.band = band;
    a.band_w = band_w;
    a.n_mels = n_mels;
    a.dmel = dmel;
    a.frames = (float *)workspace;
    hipLaunchKernelGGL(stft_mel_bwd_frames_kernel, dim3(mg_cdiv(T, 2), B), dim3(64), 0, (hipStream_t)stream, a);
    MG_LAUNCH_CHECK();
    hipLaunchKernelGGL(stft_mel_bwd_gather_kernel, dim3(mg_cdiv(L, 256), B), dim3(256), 0, (hipStream_t)stream,
                       (const float *)workspace, dx, dx_bs, L, hop, T);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
