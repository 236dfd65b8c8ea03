// Two real frames through one 1024-point complex FFT (fft1024.h), z = a + i b: what audio.hip (STFT, inverse STFT),
// vocoder_train.hip (log-mel backward) and deepspeaker.hip (split and band sum only) share.  The log-mel backward
// recomputes the forward's spectrum and band sums and compares them with the forward's clamp: its mask is the forward's
// because both call this code.  LDS arrays are declared by the kernels; the helpers take pointers.
#pragma once
#include "fft1024.h"

// d[n] = (frame t0, frame t0 + 1)[n] * window[n] of x[0, Lb), frame t covering [t hop - N/2, t hop + N/2) reflected at
// both ends, then clamped: in-bounds reads whatever hop and Lb are.  The second frame is zeros unless `second`.
__device__ __forceinline__ void mg_pair_stage(float2 *d, const float *x, int Lb, int hop, int t0, const float *window,
                                              bool second, int lane)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = lane + 64 * i;
        const float w = window[n];
        float2 z;
        int j = t0 * hop + n - MG_STFT_N / 2;
        j = j < 0 ? -j : (j >= Lb ? 2 * (Lb - 1) - j : j);
        j = j < 0 ? 0 : (j >= Lb ? Lb - 1 : j);
        z.x = x[j] * w;
        if (second) {
            j = (t0 + 1) * hop + n - MG_STFT_N / 2;
            j = j < 0 ? -j : (j >= Lb ? 2 * (Lb - 1) - j : j);
            j = j < 0 ? 0 : (j >= Lb ? Lb - 1 : j);
            z.y = x[j] * w;
        } else {
            z.y = 0.f;
        }
        d[n] = z;
    }
}

// Forward split of bin k of the transformed d: A = (Z[k] + conj Z[N-k]) / 2, B = (Z[k] - conj Z[N-k]) / 2i
__device__ __forceinline__ void mg_pair_split(const float2 *d, int k, float &ar, float &ai, float &br, float &bi)
{
    const float2 zk = d[k], zm = d[(MG_STFT_N - k) & (MG_STFT_N - 1)];
    ar = 0.5f * (zk.x + zm.x);
    ai = 0.5f * (zk.y - zm.y);
    br = 0.5f * (zk.y + zm.y);
    bi = -0.5f * (zk.x - zm.x);
}

// Row m of a banded matrix (band[m] = first bin, band[rows + m] = length, band[2 rows + m] = offset into band_w) times
// v[0, NB) and v[NB, 2 NB): s0, s1, in ascending bin order.
__device__ __forceinline__ void mg_pair_band_sum(const int *band, const float *band_w, int rows, int m, const float *v,
                                                 float &s0, float &s1)
{
    const int st = band[m], len = band[rows + m];
    const float *w = band_w + band[2 * rows + m];
    s0 = s1 = 0.f;
    for (int i = 0; i < len; ++i) {
        s0 = fmaf(w[i], v[st + i], s0);
        s1 = fmaf(w[i], v[MG_STFT_N / 2 + 1 + st + i], s1);
    }
}

// Frames [t_lo, t_hi] of T that cover padded position q, frame t covering [t hop, t hop + N).
__host__ __device__ __forceinline__ void mg_pair_frame_range(int q, int hop, int T, int &t_lo, int &t_hi)
{
    const int num = q - (MG_STFT_N - 1);
    t_lo = num <= 0 ? 0 : (num + hop - 1) / hop;
    t_hi = q / hop;
    t_hi = t_hi > T - 1 ? T - 1 : t_hi;
}

// Hops the frame-pair kernels take: a power of two up to the FFT length.
inline bool mg_stft_hop_ok(int hop) { return hop >= 1 && hop <= MG_STFT_N && (hop & (hop - 1)) == 0; }
