// One-wave probe of v_mfma_f32_4x4x1_16b_f32 (sixteen independent 4 x 4 x 1 outer products per instruction) on gfx950:
// (1) the A / B / C lane maps, pinned against a CPU product; (2) cycles per instruction of a dependent chain (one
// accumulator) and of an independent chain (eight accumulators), beside the same two chains of v_mfma_f32_32x32x2_f32 --
// 512 against 4096 FLOP per instruction, so equal FLOP/clk needs the small form eight times as often.
//     hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma_f32_4x4x1.hip -o tools/ubench/mfma_f32_4x4x1 && tools/ubench/mfma_f32_4x4x1
// Hypothesis tested: lane l holds A[block l >> 2][row l & 3] and B[block l >> 2][col l & 3]; result register r of lane l
// is C[block l >> 2][row r][col l & 3].  On a mismatch the map is searched: every product a[la] * b[lb] is unique.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void map_kernel(const float *a, const float *b, float *d)
{
    const int l = threadIdx.x;
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = __builtin_amdgcn_mfma_f32_4x4x1f32(a[l], b[l], c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) d[r * 64 + l] = c[r];
}

// NACC accumulators in rotation: 1 = dependent chain, 8 = independent
template <int NACC, bool SMALL>
__global__ __launch_bounds__(64) void chain_kernel(float *out, long long *cyc, int iters)
{
    const float a = 1.f + threadIdx.x * 1e-3f, b = 1.f - threadIdx.x * 1e-3f;
    f32x4 c4[NACC];
    f32x16 c16[NACC];
    for (int i = 0; i < NACC; ++i) {
        for (int r = 0; r < 4; ++r) c4[i][r] = 0.f;
        for (int r = 0; r < 16; ++r) c16[i][r] = 0.f;
    }
    const long long t0 = clock64();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8 / NACC; ++u)
#pragma unroll
            for (int i = 0; i < NACC; ++i) {
                if (SMALL) c4[i] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c4[i], 0, 0, 0);
                else c16[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c16[i], 0, 0, 0);
            }
    }
    const long long t1 = clock64();
    float s = 0.f;
    for (int i = 0; i < NACC; ++i) {
        for (int r = 0; r < 4; ++r) s += c4[i][r];
        for (int r = 0; r < 16; ++r) s += c16[i][r];
    }
    out[threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}

template <class K>
static double cycles_per_instruction(K kern)
{
    const int iters = 4000;
    float *out;
    long long *cyc, h = 0;
    hipMalloc(&out, 64 * 4);
    hipMalloc(&cyc, 8);
    for (int rep = 0; rep < 3; ++rep) hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, 0, out, cyc, iters);
    hipDeviceSynchronize();
    hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost);
    hipFree(out);
    hipFree(cyc);
    return (double)h / (iters * 8.0);
}

int main()
{
    float ha[64], hb[64], hd[256], *a, *b, *d;
    for (int l = 0; l < 64; ++l) {
        ha[l] = 1.f + l;              // 1 .. 64
        hb[l] = 1.f + 128.f * l;      // products a b are unique and exact in fp32
    }
    hipMalloc(&a, 256);
    hipMalloc(&b, 256);
    hipMalloc(&d, 1024);
    hipMemcpy(a, ha, 256, hipMemcpyHostToDevice);
    hipMemcpy(b, hb, 256, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(map_kernel, dim3(1), dim3(64), 0, 0, a, b, d);
    hipMemcpy(hd, d, 1024, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int r = 0; r < 4; ++r)
        for (int l = 0; l < 64; ++l) {
            const int blk = l >> 2, la = blk * 4 + r, lb = l;      // A[blk][row r] sits in lane 4 blk + r; B[blk][col l & 3] in lane l
            if (hd[r * 64 + l] != ha[la] * hb[lb]) ++bad;
        }
    printf("lane map hypothesis (A: lane = 4 block + row; B: lane = 4 block + col; C: reg = row, lane = 4 block + col): %s (%d of 256 differ)\n",
           bad ? "WRONG" : "confirmed", bad);
    if (bad)
        for (int r = 0; r < 4; ++r)
            for (int l = 0; l < 64; ++l)
                for (int la = 0; la < 64; ++la)
                    for (int lb = 0; lb < 64; ++lb)
                        if (hd[r * 64 + l] == ha[la] * hb[lb]) printf("C reg %d lane %2d = A lane %2d x B lane %2d\n", r, l, la, lb);
    const double d4 = cycles_per_instruction(chain_kernel<1, true>), i4 = cycles_per_instruction(chain_kernel<8, true>);
    const double d32 = cycles_per_instruction(chain_kernel<1, false>), i32 = cycles_per_instruction(chain_kernel<8, false>);
    printf("4x4x1   dependent chain %.2f cycles / instruction, independent (8 accumulators) %.2f -> %.1f FLOP / cycle / wave\n", d4,
           i4, 512.0 / i4);
    printf("32x32x2 dependent chain %.2f cycles / instruction, independent (8 accumulators) %.2f -> %.1f FLOP / cycle / wave\n", d32,
           i32, 4096.0 / i32);
    return bad != 0;
}
