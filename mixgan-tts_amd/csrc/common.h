// Shared device/host helpers for libmixgan_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/mixgan_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define MG_LAUNCH_CHECK()                          \
    do {                                           \
        hipError_t e__ = hipGetLastError();        \
        if (e__ != hipSuccess) return (int)e__;    \
    } while (0)

#define MG_TRY(expr)                \
    do {                            \
        int rc__ = (expr);          \
        if (rc__ != MG_OK) return rc__; \
    } while (0)

static inline int mg_cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t mg_align_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// number of frame splits for a [Co, Ci, K] weight gradient (both launchers of wgrad_mfma.h; the one count that they
// and the scratch sizes of the entry points use): two workgroups per CU are resident (66.5 KB LDS each), keep the grid within
// ONE round of 512 workgroups -- 560 workgroups take two rounds, i.e. twice the time of 504
static inline int wgrad_nsplit(int Co, int Ci, int K, int G = 1)
{
    const int tiles = mg_cdiv(Co, 128) * mg_cdiv(Ci, 128) * K * G;
    // measured sweep (B=8, L=1000): 512 workgroups is the optimum for every shape with more than 8 tiles; the small
    // k=1 gradients (<= 8 tiles: 512x256, 256x256) are 10-25 % faster with 256 -- their finalize pass, which reads
    // nsplit copies of the output, is as long as the GEMM itself
    const int target = tiles <= 8 ? 256 : 512;
    const int n = target / tiles;
    return n < 1 ? 1 : n;
}

// v_rcp_f32 (1 ulp) instead of the IEEE division sequence (~10 VALU instructions): the gate epilogue evaluates 64
// of these per lane per layer between two barriers, where nothing overlaps them.
__device__ __forceinline__ float mg_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// tanh via one exp: 1 - 2/(exp(2x)+1); exact limits at +-inf, abs err ~1e-7.
__device__ __forceinline__ float mg_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f); }

// Full 64-lane xor butterfly: every lane ends with the sum (the maximum) over the wave.  T: float, or double in pitch.hip.
template <typename T>
__device__ __forceinline__ T mg_wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float mg_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <int ACT>
__device__ __forceinline__ float mg_act(float v)
{
    if (ACT == MG_ACT_RELU) return v > 0.f ? v : 0.f;
    if (ACT == MG_ACT_LRELU02) return v > 0.f ? v : 0.2f * v;
    if (ACT == MG_ACT_TANH) return tanhf(v);
    return v;
}
