// Audio front end (reference audio/stft.py, audio/audio_processing.py): the 1024-point STFT with its magnitude /
// phase, log-mel / energy and Griffin-Lim phase epilogues, and the inverse STFT with window-sum normalisation.
//
// The reference runs the STFT as conv1d against a [1026, 1, 1024] windowed real-DFT basis and the inverse as
// conv_transpose1d against its pseudo-inverse.  That basis is exactly the windowed real DFT, and the pseudo-inverse
// is the windowed inverse real DFT over n_fft / hop (DC and Nyquist weighted 1/N, the other bins 2/N, the imaginary
// rows of DC and Nyquist zero), so an FFT computes the same sums with less rounding.
//
// Both kernels are one wave per workgroup.  A wave transforms two frames at once as z = a + i b: one 1024-point
// complex FFT (radix-4 Stockham, five passes through an 8 KB LDS buffer, twiddles from a host-built fp32 table), with
// the forward split and the inverse packing of stft_pair.h; the inverse is conj(FFT(conj Z)) / N.
//
// Forward (grid: frame pairs x batch): frame t covers samples [t hop - N/2, t hop + N/2) of the item, reflected at
// both of the item's own ends (its length comes from `lengths`, so ragged items of one batch get exactly what a call
// on that item alone gets); frames at or past the item's frame count are written as zeros.
//
// Inverse (grid: output tiles x batch): a workgroup owns `tile` output samples and recomputes every frame that
// overlaps them (at most (tile + N - hop) / tile times the frame count), adding the windowed frames in ascending frame
// order into registers: no atomics, and the result does not depend on the tiling.  The window sum-square envelope is
// computed per sample in the same order and arithmetic as the reference's numpy loop (a float32 accumulator, each add
// done in float64 from the float64 squared window), then divides where it exceeds FLT_MIN.  The reference's
// 1 / (n_fft / hop) in its pseudo-inverse and its * (n_fft / hop) after the division are powers of two that cancel
// exactly, so neither is applied.
#include "common.h"
#include "stft_pair.h"

#include <float.h>

namespace {

constexpr int N = MG_STFT_N;   // 1024
constexpr int NB = N / 2 + 1;  // 513 bins
constexpr int MAX_TILE = 1024;

struct FwdArgs {
    const float *x;
    long x_bs;
    const int *lengths;  // [B] or null (every item has L samples)
    int L, hop, T;
    const float *window;
    const float2 *tw;
    // magnitude / phase: element (b, k, t) at b s_bs + k s_ks + t s_ts (mag null: phase only)
    float *mag, *phase;
    long s_bs, s_ks, s_ts;
    // log-mel / energy: band[m] = start, band[n_mels + m] = length, band[2 n_mels + m] = offset into band_w
    const int *band;
    const float *band_w;
    int n_mels;
    float *mel, *energy;
};

constexpr int EPI_MAG_PHASE = 0, EPI_MEL = 1, EPI_PHASE = 2;

template <int EPI>
__device__ __forceinline__ void stft_fwd_body(const FwdArgs &a)
{
    __shared__ float2 d[N];
    __shared__ float mags[EPI == EPI_MEL ? 2 * NB : 1];
    const int lane = threadIdx.x, b = blockIdx.y, t0 = 2 * blockIdx.x;
    int Lb = a.lengths ? a.lengths[b] : a.L;
    Lb = Lb < 1 ? 1 : (Lb > a.L ? a.L : Lb);  // in-bounds reads whatever the caller passed (the host validates)
    const int Tb = 1 + Lb / a.hop;
    const bool va = t0 < Tb, vb = t0 + 1 < Tb, wa = t0 < a.T, wb = t0 + 1 < a.T;

    if (!va) {  // both frames past this item's end: zeros, as data.pad_2D pads
        if (EPI == EPI_MEL) {
            float *mel = a.mel + (size_t)b * a.n_mels * a.T;
            for (int m = lane; m < a.n_mels; m += 64) {
                if (wa) mel[(size_t)m * a.T + t0] = 0.f;
                if (wb) mel[(size_t)m * a.T + t0 + 1] = 0.f;
            }
            if (lane == 0 && wa) a.energy[(size_t)b * a.T + t0] = 0.f;
            if (lane == 0 && wb) a.energy[(size_t)b * a.T + t0 + 1] = 0.f;
        } else {
            for (int k = lane; k < NB; k += 64) {
                const size_t o = (size_t)b * a.s_bs + (size_t)k * a.s_ks + (size_t)t0 * a.s_ts;
                if (wa) {
                    if (EPI == EPI_MAG_PHASE) a.mag[o] = 0.f;
                    a.phase[o] = 0.f;
                }
                if (wb) {
                    if (EPI == EPI_MAG_PHASE) a.mag[o + a.s_ts] = 0.f;
                    a.phase[o + a.s_ts] = 0.f;
                }
            }
        }
        return;
    }

    mg_pair_stage(d, a.x + (size_t)b * a.x_bs, Lb, a.hop, t0, a.window, vb, lane);
    __syncthreads();
    mg_fft1024(d, a.tw, lane);

    float e0 = 0.f, e1 = 0.f;
#pragma unroll
    for (int jj = 0; jj < 9; ++jj) {
        const int k = lane + 64 * jj;
        if (k >= NB) break;
        float ar, ai, br, bi;
        mg_pair_split(d, k, ar, ai, br, bi);
        const float ma = sqrtf(ar * ar + ai * ai), mb = sqrtf(br * br + bi * bi);
        if (EPI == EPI_MEL) {
            mags[k] = ma;
            mags[NB + k] = mb;
            e0 += ma * ma;
            e1 += mb * mb;
        } else {
            const size_t o = (size_t)b * a.s_bs + (size_t)k * a.s_ks + (size_t)t0 * a.s_ts;
            if (wa) {
                if (EPI == EPI_MAG_PHASE) a.mag[o] = ma;
                a.phase[o] = atan2f(ai, ar);
            }
            if (wb) {
                if (EPI == EPI_MAG_PHASE) a.mag[o + a.s_ts] = vb ? mb : 0.f;
                a.phase[o + a.s_ts] = vb ? atan2f(bi, br) : 0.f;
            }
        }
    }
    if (EPI != EPI_MEL) return;

    // energy = ||magnitude||_2 over the bins (a fixed butterfly order), log-mel over each row's nonzero band
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        e0 += __shfl_xor(e0, off);
        e1 += __shfl_xor(e1, off);
    }
    __syncthreads();
    float *mel = a.mel + (size_t)b * a.n_mels * a.T;
    for (int m = lane; m < a.n_mels; m += 64) {
        float s0, s1;
        mg_pair_band_sum(a.band, a.band_w, a.n_mels, m, mags, s0, s1);
        // spectral_normalize: log(clamp(x, 1e-5) * 1)
        if (wa) mel[(size_t)m * a.T + t0] = logf(fmaxf(s0, 1e-5f));
        if (wb) mel[(size_t)m * a.T + t0 + 1] = vb ? logf(fmaxf(s1, 1e-5f)) : 0.f;
    }
    if (lane == 0) {
        if (wa) a.energy[(size_t)b * a.T + t0] = sqrtf(e0);
        if (wb) a.energy[(size_t)b * a.T + t0 + 1] = vb ? sqrtf(e1) : 0.f;
    }
}

// Distinct entry points, so that a kernel trace tells the three epilogues apart.
__global__ __launch_bounds__(64) void stft_magphase_kernel(FwdArgs a) { stft_fwd_body<EPI_MAG_PHASE>(a); }
__global__ __launch_bounds__(64) void stft_phase_kernel(FwdArgs a) { stft_fwd_body<EPI_PHASE>(a); }
__global__ __launch_bounds__(64) void stft_logmel_kernel(FwdArgs a) { stft_fwd_body<EPI_MEL>(a); }

struct InvArgs {
    const float *mag, *phase;
    long s_bs, s_ks, s_ts;
    int T, hop, tile, Lout;
    const float *window;
    const double *wsq;
    const float2 *tw;
    float *out;
};

__global__ __launch_bounds__(64) void istft_ola_kernel(InvArgs a)
{
    __shared__ float2 d[N];
    constexpr int ACC = MAX_TILE / 64;
    const int lane = threadIdx.x, b = blockIdx.y, hop = a.hop;
    const int p0 = blockIdx.x * a.tile + N / 2;  // first output sample, in padded coordinates
    const int nacc = a.tile / 64;
    // the frames that cover the tile: from the first position's lowest to the last position's highest (written out: as
    // a call of mg_pair_frame_range it compiles to other code, and so does the packing below)
    const int num = p0 - (N - 1);
    const int t_lo = num <= 0 ? 0 : (num + hop - 1) / hop;
    int t_hi = (p0 + a.tile - 1) / hop;
    t_hi = t_hi > a.T - 1 ? a.T - 1 : t_hi;
    const size_t sb = (size_t)b * a.s_bs;

    float acc[ACC];
#pragma unroll
    for (int j = 0; j < ACC; ++j) acc[j] = 0.f;

    for (int ta = t_lo; ta <= t_hi; ta += 2) {
        const bool hb = ta + 1 <= t_hi;
        // recombine mag cos(phase), mag sin(phase) and pack conj(A + i B) over the Hermitian extensions
        for (int k = lane; k < NB; k += 64) {
            const size_t o = sb + (size_t)k * a.s_ks + (size_t)ta * a.s_ts;
            float sa, ca, sbv = 0.f, cb = 0.f;
            sincosf(a.phase[o], &sa, &ca);
            const float mga = a.mag[o];
            float ra = mga * ca, ia = mga * sa, rb = 0.f, ib = 0.f;
            if (hb) {
                sincosf(a.phase[o + a.s_ts], &sbv, &cb);
                const float mgb = a.mag[o + a.s_ts];
                rb = mgb * cb;
                ib = mgb * sbv;
            }
            if (k == 0 || k == N / 2) ia = ib = 0.f;  // the reference basis has no sine row at DC and Nyquist
            d[k] = make_float2(ra - ib, -(ia + rb));
            if (k != 0 && k != N / 2) d[N - k] = make_float2(ra + ib, -(rb - ia));
        }
        __syncthreads();
        mg_fft1024(d, a.tw, lane);
        // frame ta is Re(d) / N, frame ta + 1 is -Im(d) / N; add them in that order
        const int ba = ta * hop, bb = ba + hop;
#pragma unroll
        for (int j = 0; j < ACC; ++j) {
            if (j >= nacc) continue;
            const int p = p0 + lane + 64 * j;
            const int na = p - ba, nb = p - bb;
            if (na >= 0 && na < N) acc[j] += a.window[na] * (d[na].x * (1.f / N));
            if (hb && nb >= 0 && nb < N) acc[j] += a.window[nb] * (-d[nb].y * (1.f / N));
        }
        __syncthreads();
    }

    float *out = a.out + (size_t)b * a.Lout;
#pragma unroll
    for (int j = 0; j < ACC; ++j) {
        const int p = p0 + lane + 64 * j;
        if (j >= nacc || p - N / 2 >= a.Lout) continue;
        // window_sumsquare: frames in ascending order, float32 accumulator, each add in float64
        int w_lo, w_hi;
        mg_pair_frame_range(p, hop, a.T, w_lo, w_hi);
        float ws = 0.f;
        for (int t = w_lo; t <= w_hi; ++t) ws = (float)((double)ws + a.wsq[p - t * hop]);
        float v = acc[j];
        if (ws > FLT_MIN) v /= ws;
        out[p - N / 2] = v;
    }
}

}  // namespace

static int stft_fwd_launch(int epi, const FwdArgs &a, int B, hipStream_t stream)
{
    const dim3 grid(mg_cdiv(a.T, 2), B);
    if (epi == EPI_MAG_PHASE) hipLaunchKernelGGL(stft_magphase_kernel, grid, dim3(64), 0, stream, a);
    else if (epi == EPI_PHASE) hipLaunchKernelGGL(stft_phase_kernel, grid, dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(stft_logmel_kernel, grid, dim3(64), 0, stream, a);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_stft_fwd(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                           const float *twiddle, float *mag, float *phase, long s_bs, long s_ks, long s_ts, int T,
                           void *stream)
{
    if (!x || !window || !twiddle || !phase) return MG_ERR_ARG;
    if (B <= 0 || !mg_stft_hop_ok(hop) || L <= N / 2 || T <= 0 || T > 1 + L / hop || x_bs < L) return MG_ERR_SHAPE;
    FwdArgs a = {};
    a.x = x;
    a.x_bs = x_bs;
    a.lengths = lengths;
    a.L = L;
    a.hop = hop;
    a.T = T;
    a.window = window;
    a.tw = (const float2 *)twiddle;
    a.mag = mag;
    a.phase = phase;
    a.s_bs = s_bs;
    a.s_ks = s_ks;
    a.s_ts = s_ts;
    return stft_fwd_launch(mag ? EPI_MAG_PHASE : EPI_PHASE, a, B, (hipStream_t)stream);
}

extern "C" int mg_stft_mel(const float *x, long x_bs, const int *lengths, int B, int L, int hop, const float *window,
                           const float *twiddle, const int *band, const float *band_w, int n_mels, float *mel,
                           float *energy, int T, void *stream)
{
    if (!x || !window || !twiddle || !band || !band_w || !mel || !energy) return MG_ERR_ARG;
    if (B <= 0 || !mg_stft_hop_ok(hop) || L <= N / 2 || T <= 0 || T > 1 + L / hop || x_bs < L || n_mels <= 0 ||
        n_mels > MG_STFT_MAX_MELS)
        return MG_ERR_SHAPE;
    FwdArgs a = {};
    a.x = x;
    a.x_bs = x_bs;
    a.lengths = lengths;
    a.L = L;
    a.hop = hop;
    a.T = T;
    a.window = window;
    a.tw = (const float2 *)twiddle;
    a.band = band;
    a.band_w = band_w;
    a.n_mels = n_mels;
    a.mel = mel;
    a.energy = energy;
    return stft_fwd_launch(EPI_MEL, a, B, (hipStream_t)stream);
}

extern "C" int mg_istft(const float *mag, const float *phase, long s_bs, long s_ks, long s_ts, int B, int T, int hop,
                        const float *window, const double *wsq, const float *twiddle, float *out, int tile,
                        void *stream)
{
    if (!mag || !phase || !window || !wsq || !twiddle || !out) return MG_ERR_ARG;
    if (B <= 0 || T < 2 || !mg_stft_hop_ok(hop) || tile <= 0 || tile % 64 || tile > MAX_TILE) return MG_ERR_SHAPE;
    InvArgs a;
    a.mag = mag;
    a.phase = phase;
    a.s_bs = s_bs;
    a.s_ks = s_ks;
    a.s_ts = s_ts;
    a.T = T;
    a.hop = hop;
    a.tile = tile;
    a.Lout = (T - 1) * hop;
    a.window = window;
    a.wsq = wsq;
    a.tw = (const float2 *)twiddle;
    a.out = out;
    hipLaunchKernelGGL(istft_ola_kernel, dim3(mg_cdiv(a.Lout, tile), B), dim3(64), 0, (hipStream_t)stream, a);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
