// One-wave 1024-point complex FFT in LDS, shared by the audio front end (audio.hip), the log-mel backward
// (vocoder_train.hip) and the DeepSpeaker filterbank (deepspeaker.hip), which reach it through stft_pair.h, and by the
// pitch extractor (pitch.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ float2 mg_cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// In-place forward FFT of d[0, 1024) by one wave: radix-4 Stockham, pass s (Ns = 4^s) maps butterfly j, k = j mod Ns,
// from d[j + 256 r] (times W^(r k 256 / Ns)) to d[4 (j - k) + k + r Ns].  Every lane reads its 16 points before the
// barrier and writes after it.
__device__ __forceinline__ void mg_fft1024(float2 *d, const float2 *__restrict__ tw, int lane)
{
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int Ns = 1 << (2 * s), tws = 256 >> (2 * s);
        float2 v[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[q][r] = d[lane + 64 * q + 256 * r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q, k = j & (Ns - 1);
            if (s > 0) {
#pragma unroll
                for (int r = 1; r < 4; ++r) v[q][r] = mg_cmul(v[q][r], tw[r * k * tws]);
            }
            const float2 s02 = make_float2(v[q][0].x + v[q][2].x, v[q][0].y + v[q][2].y);
            const float2 d02 = make_float2(v[q][0].x - v[q][2].x, v[q][0].y - v[q][2].y);
            const float2 s13 = make_float2(v[q][1].x + v[q][3].x, v[q][1].y + v[q][3].y);
            const float2 d13 = make_float2(v[q][1].x - v[q][3].x, v[q][1].y - v[q][3].y);
            const int base = 4 * (j - k) + k;
            d[base] = make_float2(s02.x + s13.x, s02.y + s13.y);
            d[base + Ns] = make_float2(d02.x + d13.y, d02.y - d13.x);
            d[base + 2 * Ns] = make_float2(s02.x - s13.x, s02.y - s13.y);
            d[base + 3 * Ns] = make_float2(d02.x - d13.y, d02.y + d13.x);
        }
        __syncthreads();
    }
}
