// Corpus builder kernels (reference preprocessor/preprocessor.py): the beta-binomial alignment prior
// (:384-393, called at :344-348) and the phoneme-level averaging of pitch / energy (:311-341).
#include "common.h"

#include <limits.h>

// ------------------------------------------------------------------ beta-binomial prior
// Row (b, i), i = 0 .. src_len - 1, frame k = 0 .. n - 1 with n = mel_len:
//   pmf(k) = C(n, k) B(k + a, n - k + bb) / B(a, bb),   a = s (i + 1),   bb = s (src_len - i).
// One wave writes one row.  A lane owns PR_CH consecutive frames: it evaluates log pmf at its first frame from
// float64 lgamma terms (the five that depend on the row only are computed by five lanes and summed), and walks
// the other frames with the ratio pmf(k + 1) / pmf(k) = (n - k)(k + a) / ((k + 1)(n - k - 1 + bb)) as a running
// product relative to the anchor, so a chain is PR_CH - 1 multiplications long.  The values go through an LDS tile
// so that the wave stores whole 16-byte vectors along L; padding (k >= mel_len, i >= src_len) is stored as zeros
// in the same pass.
#define PR_CH 16
#define PR_WAVES 4
// below this log the anchor is near the subnormal range: the lane then takes exp(log anchor + log product)
#define PR_SAFE_LOG (-690.0)

template <typename OutT> struct pr_vec;
template <> struct pr_vec<float> {
    typedef f32x4 type;
    static constexpr int N = 4;
};
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <> struct pr_vec<double> {
    typedef f64x2 type;
    static constexpr int N = 2;
};

template <typename OutT, bool VEC>
__global__ __launch_bounds__(64 * PR_WAVES) void betabinom_prior_kernel(const int *__restrict__ src_lens,
                                                                        const int *__restrict__ mel_lens, double s,
                                                                        OutT *__restrict__ out, int rows, int T, int L)
{
    constexpr int VN = pr_vec<OutT>::N;
    constexpr int PITCH = PR_CH + VN;      // one vector of padding per lane chunk keeps the vectors aligned
    typedef typename pr_vec<OutT>::type vec_t;
    __shared__ __attribute__((aligned(16))) OutT tile[PR_WAVES][64 * PITCH];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * PR_WAVES + wave;
    const bool row_ok = row < rows;
    const int b = row_ok ? row / T : 0, i = row_ok ? row % T : 0;
    int n = 0, src = 0;
    if (row_ok) {
        src = src_lens[b];
        n = mel_lens[b];
        n = n < 0 ? 0 : (n > L ? L : n);
        src = src > T ? T : src;
    }
    const bool live = row_ok && i < src && n > 0;
    const double a = s * (double)(i + 1), bb = s * (double)(src - i), dn = (double)n;

    double row_c = 0.0;
    if (live) {
        double t = 0.0;
        if (lane == 0) t = lgamma(dn + 1.0);
        if (lane == 1) t = -lgamma(dn + a + bb);
        if (lane == 2) t = -lgamma(a);
        if (lane == 3) t = -lgamma(bb);
        if (lane == 4) t = lgamma(a + bb);
        t += __shfl_xor(t, 1);
        t += __shfl_xor(t, 2);
        t += __shfl_xor(t, 4);
        row_c = __shfl(t, 0);
    }

    OutT *mine = tile[wave] + lane * PITCH;
    OutT *orow = out + (size_t)(row_ok ? row : 0) * L;
    for (int base = 0; base < L; base += 64 * PR_CH) {
        const int k0 = base + lane * PR_CH;
        if (live && k0 < n) {
            const double dk = (double)k0;
            const double lp = row_c - lgamma(dk + 1.0) - lgamma(dn - dk + 1.0) + lgamma(dk + a) + lgamma(dn - dk + bb);
            const bool safe = lp > PR_SAFE_LOG;
            const double p0 = exp(lp);
            double r = 1.0;
            if (safe) {
#pragma unroll
                for (int j = 0; j < PR_CH; ++j) {
                    const double kk = (double)(k0 + j);
                    mine[j] = k0 + j < n ? (OutT)(p0 * r) : (OutT)0;
                    r *= ((dn - kk) * (kk + a)) / ((kk + 1.0) * (dn - kk - 1.0 + bb));
                }
            } else {
                for (int j = 0; j < PR_CH; ++j) {
                    const double kk = (double)(k0 + j);
                    mine[j] = k0 + j < n ? (OutT)exp(lp + log(r)) : (OutT)0;
                    r *= ((dn - kk) * (kk + a)) / ((kk + 1.0) * (dn - kk - 1.0 + bb));
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < PR_CH; ++j) mine[j] = (OutT)0;
        }
        __syncthreads();
        if (row_ok) {
            if (VEC) {
#pragma unroll
                for (int it = 0; it < PR_CH / VN; ++it) {
                    const int e = (it * 64 + lane) * VN;      // element of this tile, a multiple of VN
                    if (base + e < L)                        // L % VN == 0: the whole vector is inside the row
                        *(vec_t *)(orow + base + e) = *(const vec_t *)(tile[wave] + (e / PR_CH) * PITCH + e % PR_CH);
                }
            } else {
#pragma unroll
                for (int it = 0; it < PR_CH; ++it) {
                    const int e = it * 64 + lane;
                    if (base + e < L) orow[base + e] = tile[wave][(e / PR_CH) * PITCH + e % PR_CH];
                }
            }
        }
        __syncthreads();
    }
}

template <typename OutT>
static int launch_prior(const int *src_lens, const int *mel_lens, double s, OutT *out, int B, int T, int L,
                        hipStream_t stream)
{
    const int rows = B * T;
    const dim3 grid(mg_cdiv(rows, PR_WAVES)), block(64 * PR_WAVES);
    const bool vec = L % pr_vec<OutT>::N == 0 && (uintptr_t)out % 16 == 0;
    if (vec)
        hipLaunchKernelGGL((betabinom_prior_kernel<OutT, true>), grid, block, 0, stream, src_lens, mel_lens, s, out,
                           rows, T, L);
    else
        hipLaunchKernelGGL((betabinom_prior_kernel<OutT, false>), grid, block, 0, stream, src_lens, mel_lens, s, out,
                           rows, T, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" int mg_betabinom_prior(const int *src_lens, const int *mel_lens, const double *scaling, void *out, int B,
                                  int T, int L, int out_f64, void *stream)
{
    if (!src_lens || !mel_lens || !scaling || !out) return MG_ERR_ARG;
    if (out_f64 != 0 && out_f64 != 1) return MG_ERR_ARG;
    if (B <= 0 || T <= 0 || L <= 0 || (long)B * T > (long)INT_MAX / 2) return MG_ERR_SHAPE;
    const double s = *scaling;
    if (!(s > 0.0) || s > 1e6) return MG_ERR_ARG;
    if (out_f64) return launch_prior<double>(src_lens, mel_lens, s, (double *)out, B, T, L, (hipStream_t)stream);
    return launch_prior<float>(src_lens, mel_lens, s, (float *)out, B, T, L, (hipStream_t)stream);
}

// ------------------------------------------------------------------ phoneme-level averages
// One workgroup per utterance.  pos[i] is the exclusive prefix sum of the durations; out[i] is the mean of
// value[pos[i] : pos[i] + d_i) cut at n_frames as a numpy slice is, or 0 for d_i == 0.  Pitch mode first replaces the
// zero frames by scipy's linear interp1d (numpy's interp) over the non-zero ones: the previous / next non-zero frame
// come from two block scans, and the first / last non-zero value holds outside them.  The reference averages in
// place (pitch[i] = mean(pitch[pos : pos + d])), so a segment with pos[i] < i reads entries that earlier segments
// have overwritten; an utterance with such a segment is redone by one thread in the reference's order.
#define PA_THREADS 256
#define PA_MAXT 2048
#define PA_MAXL 4096

// Exclusive block scan of one int per thread (op: 0 sum, 1 max); `part` is PA_THREADS ints of LDS.
template <int OP>
__device__ __forceinline__ int pa_scan_excl(int v, int identity, int *part)
{
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    int acc = identity;
    for (int t = 0; t < (int)threadIdx.x; ++t) acc = OP == 0 ? acc + part[t] : max(acc, part[t]);
    return acc;
}

template <typename ValT, bool PITCH>
struct pa_reader {
    const ValT *v;
    const int *prev, *next;      // PITCH: last non-zero frame < k (-1: none), first non-zero frame >= k (INT_MAX: none)
    int n;
    __device__ __forceinline__ double at(int k) const
    {
        if (!PITCH || v[k] != (ValT)0) return (double)v[k];      // a non-zero frame is a knot: np.interp returns it as is
        const int hi = next[k], lo = prev[k];
        if (hi == INT_MAX) return lo >= 0 ? (double)v[lo] : 0.0;      // after the last non-zero frame
        if (lo < 0) return (double)v[hi];                              // before the first one
        // interp1d: slope * (x - x_lo) + y_lo, each operation rounded on its own
        const double ylo = (double)v[lo], yhi = (double)v[hi];
        const double slope = __ddiv_rn(__dsub_rn(yhi, ylo), (double)(hi - lo));
        return __dadd_rn(__dmul_rn(slope, (double)(k - lo)), ylo);
    }
};

template <typename ValT, bool PITCH>
__global__ __launch_bounds__(PA_THREADS) void phoneme_average_kernel(const ValT *__restrict__ values,
                                                                     const int *__restrict__ durations,
                                                                     const int *__restrict__ n_frames,
                                                                     const int *__restrict__ n_phon,
                                                                     ValT *__restrict__ out, int T, int L)
{
    __shared__ int pos[PA_MAXT];
    __shared__ int part[PA_THREADS];
    __shared__ int prev[PITCH ? PA_MAXL : 1], next[PITCH ? PA_MAXL : 1];
    __shared__ int aliased;

    const int b = blockIdx.x, tid = threadIdx.x;
    const ValT *v = values + (size_t)b * L;
    const int *dur = durations + (size_t)b * T;
    ValT *o = out + (size_t)b * T;
    const int n = min(max(n_frames[b], 0), L), np = min(max(n_phon[b], 0), T);
    if (tid == 0) aliased = 0;

    // pos: each thread scans a contiguous chunk of phonemes
    {
        const int per = (np + PA_THREADS - 1) / PA_THREADS, i0 = min(tid * per, np), i1 = min(i0 + per, np);
        int sum = 0;
        for (int i = i0; i < i1; ++i) sum += max(dur[i], 0);
        int acc = pa_scan_excl<0>(sum, 0, part);
        for (int i = i0; i < i1; ++i) {
            pos[i] = acc;
            acc += max(dur[i], 0);
        }
    }
    if (PITCH) {
        const int per = (n + PA_THREADS - 1) / PA_THREADS, k0 = min(tid * per, n), k1 = min(k0 + per, n);
        int last = -1;
        for (int k = k0; k < k1; ++k)
            if (v[k] != (ValT)0) last = k;
        int acc = pa_scan_excl<1>(last, -1, part);
        for (int k = k0; k < k1; ++k) {
            prev[k] = acc;
            if (v[k] != (ValT)0) acc = k;
        }
        // first non-zero frame >= k: the same scan from the right, on negated indices
        int first = INT_MIN;
        for (int k = k1 - 1; k >= k0; --k)
            if (v[k] != (ValT)0) first = -k;
        __syncthreads();
        part[PA_THREADS - 1 - tid] = first;
        __syncthreads();
        acc = INT_MIN;
        for (int t = 0; t < PA_THREADS - 1 - tid; ++t) acc = max(acc, part[t]);
        for (int k = k1 - 1; k >= k0; --k) {
            if (v[k] != (ValT)0) acc = -k;
            next[k] = acc == INT_MIN ? INT_MAX : -acc;
        }
    }
    __syncthreads();

    const pa_reader<ValT, PITCH> rd = {v, prev, next, n};
    for (int i = tid; i < T; i += PA_THREADS) {
        double r = 0.0;
        if (i < np) {
            const int d = max(dur[i], 0);
            if (d > 0) {
                const int p0 = min(pos[i], n), p1 = min(pos[i] + d, n);
                if (pos[i] < i) aliased = 1;      // every writer stores the same value
                double sum = 0.0;
                for (int k = p0; k < p1; ++k) sum += rd.at(k);
                r = sum / (double)(p1 - p0);      // an empty slice is numpy's nan
            }
        }
        o[i] = (ValT)r;
    }
    __syncthreads();
    if (aliased && tid == 0) {
        // in place: entries below i hold the earlier segments' results, the others the (interpolated) input
        for (int i = 0; i < np; ++i) {
            const int d = max(dur[i], 0);
            double r = 0.0;
            if (d > 0) {
                const int p0 = min(pos[i], n), p1 = min(pos[i] + d, n);
                double sum = 0.0;
                for (int k = p0; k < p1; ++k) sum += k < i ? (double)o[k] : rd.at(k);
                r = sum / (double)(p1 - p0);
            }
            o[i] = (ValT)r;
        }
    }
}

extern "C" int mg_phoneme_average(const void *values, const int *durations, const int *n_frames, const int *n_phon,
                                  void *out, int B, int T, int L, int pitch, void *stream)
{
    if (!values || !durations || !n_frames || !n_phon || !out) return MG_ERR_ARG;
    if (pitch != 0 && pitch != 1) return MG_ERR_ARG;
    if (B <= 0 || T <= 0 || T > PA_MAXT || L <= 0 || L > PA_MAXL) return MG_ERR_SHAPE;
    if (pitch)
        hipLaunchKernelGGL((phoneme_average_kernel<double, true>), dim3(B), dim3(PA_THREADS), 0, (hipStream_t)stream,
                           (const double *)values, durations, n_frames, n_phon, (double *)out, T, L);
    else
        hipLaunchKernelGGL((phoneme_average_kernel<float, false>), dim3(B), dim3(PA_THREADS), 0, (hipStream_t)stream,
                           (const float *)values, durations, n_frames, n_phon, (float *)out, T, L);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
