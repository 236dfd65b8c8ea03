// prepare_align kernels (reference preprocessor/ljspeech.py, preprocessor/aishell3.py): the polyphase resampler that
// stands in for librosa.load(path, sr), and the peak normalisation to int16.
#include "common.h"

// ------------------------------------------------------------------ polyphase resampler
// One workgroup computes RS_TILE consecutive outputs of one utterance.  Output n reads the Kp inputs from
// q - Mh + 1 on, q = n down / up, against row r = n down % up of the tap table (layout: mixgan_hip.h), so the tile
// needs the inputs from q(first) - Mh + 1 to q(last) - Mh + Kp: they are staged in LDS once, zero outside
// [0, lengths[b]).  A thread owns the outputs first + tid + i RS_THREADS: neighbouring lanes store neighbouring
// samples, read LDS addresses that differ by about down / up, and read their tap rows as 16-byte vectors from L2
// (up > 1), or share one row through scalar loads (up == 1, UP1).  n down is formed in 64 bits.
#define RS_THREADS 256
#define RS_TILE MG_RESAMPLE_TILE

template <bool UP1>
__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(const float *__restrict__ x, long x_bs,
                                                                   const int *__restrict__ lengths, int N,
                                                                   const float *__restrict__ taps, int up, int down,
                                                                   int Kp, int Mh, float *__restrict__ y, long y_bs,
                                                                   int M, int span_max)
{
    extern __shared__ __attribute__((aligned(16))) float xs[];

    const int b = blockIdx.y, tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * RS_TILE;
    int len = lengths ? lengths[b] : N;
    len = len < 0 ? 0 : (len > N ? N : len);
    const long long out_len = ((long long)len * up + down - 1) / down;
    float *yrow = y + (size_t)b * y_bs;
    const int count = (int)(M - first < RS_TILE ? M - first : RS_TILE);      // outputs of this tile inside the row
    if (first >= out_len) {
        for (int i = tid; i < count; i += RS_THREADS) yrow[first + i] = 0.f;
        return;
    }
    const long long live = out_len - first < count ? out_len - first : count;      // of them, before out_len

    // the staged span: inputs k0 .. k0 + span - 1
    const long long q_first = UP1 ? first * down : first * down / up;
    const long long q_last = UP1 ? (first + live - 1) * down : (first + live - 1) * down / up;
    const long long k0 = q_first - Mh + 1;
    int span = (int)(q_last - q_first) + Kp;
    span = span > span_max ? span_max : span;      // cannot happen: the host sized span_max for a whole tile
    const float *xrow = x + (size_t)b * x_bs;
    for (int i = tid; i < span; i += RS_THREADS) {
        const long long k = k0 + i;
        xs[i] = (k >= 0 && k < len) ? xrow[k] : 0.f;
    }
    __syncthreads();

    for (int i = tid; i < count; i += RS_THREADS) {
        float r = 0.f;
        if (i < live) {
            const long long nd = (first + i) * down;
            const long long q = UP1 ? nd : nd / up;
            const int row = UP1 ? 0 : (int)(nd - q * up);
            const float *xp = xs + (int)(q - q_first);
            const f32x4 *tp = (const f32x4 *)(taps + (size_t)row * Kp);
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            for (int j = 0; j < Kp; j += 4) {
                const f32x4 t = tp[j >> 2];
                a0 = fmaf(t.x, xp[j], a0);
                a1 = fmaf(t.y, xp[j + 1], a1);
                a2 = fmaf(t.z, xp[j + 2], a2);
                a3 = fmaf(t.w, xp[j + 3], a3);
            }
            r = (a0 + a1) + (a2 + a3);
        }
        yrow[first + i] = r;
    }
}

__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(const float *__restrict__ x, long x_bs,
                                                                   const int *__restrict__ lengths, int N,
                                                                   float *__restrict__ y, long y_bs, int M)
{
    const int b = blockIdx.y;
    int len = lengths ? lengths[b] : N;
    len = len < 0 ? 0 : (len > N ? N : len);
    const float *xrow = x + (size_t)b * x_bs;
    float *yrow = y + (size_t)b * y_bs;
    const long long first = (long long)blockIdx.x * RS_TILE;
    for (long long n = first + threadIdx.x; n < first + RS_TILE && n < M; n += RS_THREADS)
        yrow[n] = n < len ? xrow[n] : 0.f;
}

extern "C" int mg_resample_poly(const float *x, long x_bs, const int *lengths, int B, int N, const float *taps, int up,
                                int down, int Kp, int half, float *y, long y_bs, int M, void *stream)
{
    if (!x || !y) return MG_ERR_ARG;
    if (B <= 0 || B > 65535 || N <= 0 || M <= 0 || up <= 0 || down <= 0 || x_bs < N || y_bs < M) return MG_ERR_SHAPE;
    const dim3 grid(mg_cdiv(M, RS_TILE), B), block(RS_THREADS);
    if (up == 1 && down == 1) {
        hipLaunchKernelGGL(resample_copy_kernel, grid, block, 0, (hipStream_t)stream, x, x_bs, lengths, N, y, y_bs, M);
        MG_LAUNCH_CHECK();
        return MG_OK;
    }
    if (!taps || (uintptr_t)taps % 16 != 0) return MG_ERR_ARG;
    if (half < 0 || up > MG_RESAMPLE_MAX_UP || Kp <= 0 || Kp > MG_RESAMPLE_MAX_TAPS || Kp % 4 != 0) return MG_ERR_SHAPE;
    const int Mh = half / up + 1;
    if (Kp < 2 * Mh) return MG_ERR_SHAPE;
    const long long span_max = (long long)(RS_TILE - 1) * down / up + Kp + 2;
    if (span_max > MG_RESAMPLE_MAX_SPAN) return MG_ERR_SHAPE;
    const size_t lds = (size_t)span_max * sizeof(float);
    if (up == 1)
        hipLaunchKernelGGL((resample_poly_kernel<true>), grid, block, lds, (hipStream_t)stream, x, x_bs, lengths, N,
                           taps, up, down, Kp, Mh, y, y_bs, M, (int)span_max);
    else
        hipLaunchKernelGGL((resample_poly_kernel<false>), grid, block, lds, (hipStream_t)stream, x, x_bs, lengths, N,
                           taps, up, down, Kp, Mh, y, y_bs, M, (int)span_max);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

// ------------------------------------------------------------------ peak normalisation to int16
// One workgroup per utterance: the row maximum of |x| (wave shuffles, then LDS across the waves), then
// q = trunc((x / max) max_wav_value), each operation rounded on its own as numpy's float32 expression is, saturated.
#define PN_THREADS 256

__global__ __launch_bounds__(PN_THREADS) void peak_normalize_i16_kernel(const float *__restrict__ x, long x_bs,
                                                                        const int *__restrict__ lengths, int N,
                                                                        float max_wav_value, int16_t *__restrict__ out,
                                                                        long out_bs)
{
    __shared__ float part[PN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int len = lengths ? lengths[b] : N;
    len = len < 0 ? 0 : (len > N ? N : len);
    const float *xrow = x + (size_t)b * x_bs;
    int16_t *orow = out + (size_t)b * out_bs;

    float m = 0.f;
    for (int k = tid; k < len; k += PN_THREADS) m = fmaxf(m, fabsf(xrow[k]));
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    m = part[0];
    for (int w = 1; w < PN_THREADS / 64; ++w) m = fmaxf(m, part[w]);

    for (int k = tid; k < N; k += PN_THREADS) {
        int q = 0;
        if (k < len && m > 0.f) {
            const float v = __fmul_rn(__fdiv_rn(xrow[k], m), max_wav_value);
            q = v >= 32767.f ? 32767 : (v <= -32768.f ? -32768 : (int)v);      // a NaN sample gives 0
        }
        orow[k] = (int16_t)q;
    }
}

extern "C" int mg_peak_normalize_i16(const float *x, long x_bs, const int *lengths, int B, int N, float max_wav_value,
                                     int16_t *out, long out_bs, void *stream)
{
    if (!x || !out) return MG_ERR_ARG;
    if (!(max_wav_value > 0.f)) return MG_ERR_ARG;
    if (B <= 0 || N <= 0 || x_bs < N || out_bs < N) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(peak_normalize_i16_kernel, dim3(B), dim3(PN_THREADS), 0, (hipStream_t)stream, x, x_bs, lengths,
                       N, max_wav_value, out, out_bs);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
