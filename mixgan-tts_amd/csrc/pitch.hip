// Pitch extractor of the corpus builder (mixgan_tts_amd/pitch.py; stands where the reference calls pyworld's dio +
// stonemask, without any claim of parity with them): YIN candidates per frame, then a Viterbi track per utterance.
// tests/pitch_oracle.py states both stages in float64 numpy.
//
// Geometry: frame k of a row is the PN = 1024 samples from k hop - PN / 2 on, zero outside [0, lengths[b]) (nothing
// at or past the length is read), and the difference function integrates over PW = 512 samples:
//     d(tau) = sum_{j < PW} (x_j - x_{j + tau})^2 = e(0) + e(tau) - 2 r(tau),   0 <= tau <= tau_max + 1 <= PN - PW,
// e(tau) = sum_{j < PW} x_{j + tau}^2, r(tau) = sum_{j < PW} x_j x_{j + tau}.
#include "common.h"
#include "fft1024.h"

#include <limits.h>

namespace {

constexpr int PN = MG_PITCH_N, PW = MG_PITCH_W, PK = MG_PITCH_K;
constexpr int LPL = 9;      // lags per lane: lane l owns the lags 9 l .. 9 l + 8, 576 >= PN - PW + 1 in all
constexpr float EMPTY_COST = 1e30f;

// Exclusive prefix sum over the lanes of one wave.
__device__ __forceinline__ double wave_exclusive_scan(double v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    const double prev = __shfl_up(v, 1);
    return lane == 0 ? 0.0 : prev;
}

// ------------------------------------------------------------------ stage 1: candidates
// One wave per frame.  r comes from two FFTs: z = a + i b with a = x[0, PW) zero-padded and b = x[0, PN), the split
//     A[k] = (Z[k] + conj Z[N-k]) / 2,   B[k] = (Z[k] - conj Z[N-k]) / 2i,
// and r(tau) = Re FFT(A conj B)[tau] / N, which is the inverse transform of conj(A) B because r is real; tau <= PN - PW
// keeps the circular correlation from wrapping.  Everything after the FFT is float64, so the FFT's rounding is the
// only error of d that matters: e by a prefix scan of x_{t+PW-1}^2 - x_{t-1}^2 (products of floats are exact in
// float64), the running sum of d by a second scan, d' = d tau / sum.  The four deepest local minima are found by four
// wave arg-min reductions over (d', lag), the lower lag winning a tie, and leave in increasing lag.
__global__ __launch_bounds__(64) void yin_candidates_kernel(const float *__restrict__ x, long x_bs,
                                                            const int *__restrict__ lengths, int L, int hop,
                                                            int tau_min, int tau_max, const float2 *__restrict__ tw,
                                                            float *__restrict__ period, float *__restrict__ cost,
                                                            float *__restrict__ rms, int T)
{
    __shared__ __attribute__((aligned(16))) float2 d[PN];
    __shared__ float xs[PN];
    const int lane = threadIdx.x, b = blockIdx.y, k = blockIdx.x;
    int len = lengths ? lengths[b] : L;
    len = len < 0 ? 0 : (len > L ? L : len);
    const int Tb = len / hop + 1;
    const size_t o = (size_t)b * T + k;
    if (k >= Tb) {      // past this row's frames: zeros
        if (lane < PK) {
            period[o * PK + lane] = 0.f;
            cost[o * PK + lane] = 0.f;
        }
        if (lane == 0) rms[o] = 0.f;
        return;
    }

    const float *xrow = x + (size_t)b * x_bs;
    const long long s0 = (long long)k * hop - PN / 2;
    double sq = 0.0, sqa = 0.0;
#pragma unroll
    for (int i = 0; i < PN / 64; ++i) {
        const int n = lane + 64 * i;
        const long long s = s0 + n;
        const float v = (s >= 0 && s < len) ? xrow[s] : 0.f;
        xs[n] = v;
        d[n] = make_float2(n < PW ? v : 0.f, v);
        sq += (double)v * (double)v;
        if (n < PW) sqa += (double)v * (double)v;
    }
    sq = mg_wave_sum(sq);
    const double e0 = mg_wave_sum(sqa);
    if (lane == 0) rms[o] = (float)sqrt(sq * (1.0 / PN));
    __syncthreads();
    mg_fft1024(d, tw, lane);

    // P = A conj(B); P[N - k] = conj P[k] because a and b are real.  A lane owns both ends of its pairs.
#pragma unroll
    for (int jj = 0; jj < 9; ++jj) {
        const int kk = lane + 64 * jj;
        if (kk > PN / 2) break;
        const float2 zk = d[kk], zm = d[(PN - kk) & (PN - 1)];
        const float ar = 0.5f * (zk.x + zm.x), ai = 0.5f * (zk.y - zm.y);
        const float br = 0.5f * (zk.y + zm.y), bi = -0.5f * (zk.x - zm.x);
        const float pr = ar * br + ai * bi, pi = ai * br - ar * bi;
        d[kk] = make_float2(pr, pi);
        if (kk != 0 && kk != PN / 2) d[PN - kk] = make_float2(pr, -pi);
    }
    __syncthreads();
    mg_fft1024(d, tw, lane);

    // d over this lane's lags
    const int t0 = lane * LPL;
    double dv[LPL];
    double run = 0.0;
#pragma unroll
    for (int c = 0; c < LPL; ++c) {      // e(t) - e(0), inclusive within the lane
        const int t = t0 + c;
        if (t >= 1 && t <= PN - PW) {
            const double hi = (double)xs[t + PW - 1], lo = (double)xs[t - 1];
            run += hi * hi - lo * lo;
        }
        dv[c] = run;
    }
    const double ebase = e0 + wave_exclusive_scan(run, lane);
    run = 0.0;
#pragma unroll
    for (int c = 0; c < LPL; ++c) {
        const int t = t0 + c;
        double v = 0.0;
        if (t >= 1 && t <= tau_max + 1) {
            const double r = (double)d[t].x * (1.0 / PN);
            v = fmax(e0 + (ebase + dv[c]) - 2.0 * r, 0.0);
        }
        run += v;
        dv[c] = v;
    }
    double csum = wave_exclusive_scan(run, lane);
    __syncthreads();      // every lane has read r: d' takes over the buffer
    double *dp = reinterpret_cast<double *>(d);
#pragma unroll
    for (int c = 0; c < LPL; ++c) {
        const int t = t0 + c;
        csum += dv[c];
        dp[t] = (t >= 1 && csum > 0.0) ? dv[c] * (double)t / csum : 1.0;
    }
    __syncthreads();

    // local minima of this lane: strictly below the left neighbour, not above the right one
    unsigned open = 0;
#pragma unroll
    for (int c = 0; c < LPL; ++c) {
        const int t = t0 + c;
        if (t >= tau_min && t <= tau_max && dp[t] < dp[t - 1] && dp[t] <= dp[t + 1]) open |= 1u << c;
    }

    int sel_t[PK];
    float sel_p[PK], sel_c[PK];
#pragma unroll
    for (int i = 0; i < PK; ++i) {
        double bv = INFINITY;
        int bt = INT_MAX;
#pragma unroll
        for (int c = 0; c < LPL; ++c) {      // ascending lag: the first of equal values stays
            if ((open >> c & 1u) && dp[t0 + c] < bv) {
                bv = dp[t0 + c];
                bt = t0 + c;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off);
            const int ot = __shfl_xor(bt, off);
            if (ov < bv || (ov == bv && ot < bt)) {
                bv = ov;
                bt = ot;
            }
        }
        sel_t[i] = bt;
        sel_p[i] = 0.f;
        sel_c[i] = EMPTY_COST;
        if (bt != INT_MAX) {      // wave-uniform
            if (bt / LPL == lane) open &= ~(1u << (bt - t0));
            const double y0 = dp[bt - 1], y1 = dp[bt], y2 = dp[bt + 1];
            const double den = y0 - 2.0 * y1 + y2;
            double off = 0.0;
            if (den > 0.0) off = fmin(0.5, fmax(-0.5, 0.5 * (y0 - y2) / den));
            sel_p[i] = (float)((double)bt + off);
            sel_c[i] = (float)y1;
        }
    }
    // increasing lag; empty slots (INT_MAX) end up last
#define PITCH_CSWAP(i, j)                                                   \
    if (sel_t[j] < sel_t[i]) {                                              \
        const int tt = sel_t[i]; sel_t[i] = sel_t[j]; sel_t[j] = tt;        \
        const float tp = sel_p[i]; sel_p[i] = sel_p[j]; sel_p[j] = tp;      \
        const float tc = sel_c[i]; sel_c[i] = sel_c[j]; sel_c[j] = tc;      \
    }
    PITCH_CSWAP(0, 1) PITCH_CSWAP(2, 3) PITCH_CSWAP(0, 2) PITCH_CSWAP(1, 3) PITCH_CSWAP(1, 2)
#undef PITCH_CSWAP
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < PK; ++i) {
            period[o * PK + i] = sel_p[i];
            cost[o * PK + i] = sel_c[i];
        }
    }
}

// ------------------------------------------------------------------ stage 2: track
// Every float64 operation below is rounded on its own, in the order tests/pitch_oracle.py states, so the path equals
// the oracle's bit for bit: no contraction into fused multiply-adds from here on.
#pragma clang fp contract(off)

// log2 by operations that round alike everywhere (the library's log2 is not correctly rounded): frexp to
// m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), the odd series of 2 atanh(s) to s^21 by Horner.
__device__ double pitch_log2(double x)
{
    int e;
    double m = frexp(x, &e);
    if (m < 0.70710678118654757) {
        m = m * 2.0;
        e -= 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double p = 1.0 / 21.0;
    p = p * s2 + 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    return (double)e + (s * p) * 2.8853900817779268;
}

struct TrackParams {
    double sr, theta, beta, lam, sw, gate_lin, tau_max;
};

constexpr int S = PK + 1;      // states: PK candidate slots, then unvoiced

// One wave per row, sequential over its frames.  Lanes 0 .. 4 own the states (observation cost, log-period, delta);
// lane 5 b + a forms delta(a) + trans(a, b); lane b then takes the first minimum over a.  The five back-pointers of a
// frame are packed three bits each into one word of the workspace; the backtrace loads 64 words at a time and walks
// them through the wave.
__global__ __launch_bounds__(64) void pitch_track_kernel(const float *__restrict__ period,
                                                         const float *__restrict__ cost,
                                                         const float *__restrict__ rms,
                                                         const int *__restrict__ n_frames, int T, TrackParams p,
                                                         double *__restrict__ f0, unsigned *__restrict__ ws)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    int nf = n_frames[b];
    nf = nf < 0 ? 0 : (nf > T ? T : nf);
    const float *per = period + (size_t)b * T * PK, *cst = cost + (size_t)b * T * PK, *rm = rms + (size_t)b * T;
    double *out = f0 + (size_t)b * T;
    unsigned *bp = ws + (size_t)b * T;
    for (int t = nf + lane; t < T; t += 64) out[t] = 0.0;
    if (nf == 0) return;

    float mx = 0.f;
    for (int t = lane; t < nf; t += 64) mx = fmaxf(mx, rm[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const double gate = p.gate_lin * (double)mx;

    const int st = lane < S ? lane : S - 1;      // the state of lanes 0 .. 4
    const int tb = lane < S * S ? lane / S : 0, ta = lane < S * S ? lane % S : 0;
    const int slot = st < PK ? st : 0;
    float n_per = per[slot], n_cst = cst[slot], n_rms = rm[0];
    double delta = 0.0, Lprev = 0.0;
    for (int t = 0; t < nf; ++t) {
        const double pd = (double)n_per, cs = (double)n_cst, rs = (double)n_rms;
        if (t + 1 < nf) {      // the next frame's values, ahead of their use
            n_per = per[(size_t)(t + 1) * PK + slot];
            n_cst = cst[(size_t)(t + 1) * PK + slot];
            n_rms = rm[t + 1];
        }
        const bool valid = st < PK && pd > 0.0;
        double obs = INFINITY;
        if (valid && !(rs < gate)) obs = cs + (p.beta * pd) / p.tau_max;
        if (st == PK) obs = p.theta;
        const double Lc = valid ? pitch_log2(pd) : 0.0;
        if (t == 0) {
            delta = obs;
        } else {
            const double La = __shfl(Lprev, ta), Lb = __shfl(Lc, tb), da = __shfl(delta, ta);
            double trans;
            if (ta < PK && tb < PK) trans = p.lam * fabs(La - Lb);
            else trans = (ta == PK && tb == PK) ? 0.0 : p.sw;
            const double cand = da + trans;
            double best = __shfl(cand, st * S);
            int arg = 0;
#pragma unroll
            for (int a = 1; a < S; ++a) {
                const double v = __shfl(cand, st * S + a);
                if (v < best) {
                    best = v;
                    arg = a;
                }
            }
            delta = best + obs;
            unsigned w = lane < S ? (unsigned)arg << (3 * lane) : 0u;
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            if (lane == 0) bp[t] = w;
        }
        Lprev = Lc;
    }

    // the first minimal final state
    double best = __shfl(delta, 0);
    int s = 0;
#pragma unroll
    for (int a = 1; a < S; ++a) {
        const double v = __shfl(delta, a);
        if (v < best) {
            best = v;
            s = a;
        }
    }
    __threadfence();      // lane 0's back-pointer words, read below by the other lanes
    __syncthreads();
    for (int hi = nf - 1; hi >= 0; hi -= 64) {
        const int tt = hi - lane;
        const unsigned w = tt >= 1 ? bp[tt] : 0u;
        const int steps = hi + 1 < 64 ? hi + 1 : 64;
        int mine = PK;
        for (int i = 0; i < steps; ++i) {
            if (lane == i) mine = s;
            const unsigned wi = __shfl(w, i);
            s = (int)(wi >> (3 * s) & 7u);      // frame hi - i: state at hi - i - 1 (unused for frame 0)
        }
        if (tt >= 0) out[tt] = mine < PK ? p.sr / (double)per[(size_t)tt * PK + mine] : 0.0;
    }
}

}  // namespace

extern "C" int mg_yin_candidates(const float *x, long x_bs, const int *lengths, int B, int L, int hop, int tau_min,
                                 int tau_max, const float *twiddle, float *period, float *cost, float *rms, int T,
                                 void *stream)
{
    if (!x || !twiddle || !period || !cost || !rms) return MG_ERR_ARG;
    if (B <= 0 || B > 65535 || L <= 0 || hop <= 0 || T <= 0 || T > L / hop + 1 || x_bs < L) return MG_ERR_SHAPE;
    if (tau_min < 2 || tau_min > tau_max || tau_max + 1 > PN - PW) return MG_ERR_SHAPE;
    hipLaunchKernelGGL(yin_candidates_kernel, dim3(T, B), dim3(64), 0, (hipStream_t)stream, x, x_bs, lengths, L, hop,
                       tau_min, tau_max, (const float2 *)twiddle, period, cost, rms, T);
    MG_LAUNCH_CHECK();
    return MG_OK;
}

extern "C" size_t mg_pitch_track_workspace_bytes(int B, int T)
{
    if (B <= 0 || T <= 0) return 0;
    return (size_t)B * (size_t)T * sizeof(unsigned);
}

extern "C" int mg_pitch_track(const float *period, const float *cost, const float *rms, const int *n_frames, int B,
                              int T, const double *params, double *f0, void *workspace, size_t workspace_bytes,
                              void *stream)
{
    if (!period || !cost || !rms || !n_frames || !params || !f0) return MG_ERR_ARG;
    if (B <= 0 || T <= 0) return MG_ERR_SHAPE;
    TrackParams p;
    p.sr = params[MG_PITCH_P_SR];
    p.tau_max = params[MG_PITCH_P_TAU_MAX];
    p.theta = params[MG_PITCH_P_THETA];
    p.beta = params[MG_PITCH_P_BETA];
    p.lam = params[MG_PITCH_P_LAMBDA];
    p.sw = params[MG_PITCH_P_SWITCH];
    p.gate_lin = params[MG_PITCH_P_GATE];
    if (!(p.sr > 0.0) || !(p.tau_max >= 2.0) || p.tau_max + 1 > PN - PW) return MG_ERR_SHAPE;
    if (!workspace || workspace_bytes < mg_pitch_track_workspace_bytes(B, T)) return MG_ERR_WORKSPACE;
    hipLaunchKernelGGL(pitch_track_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, period, cost, rms, n_frames, T, p,
                       f0, (unsigned *)workspace);
    MG_LAUNCH_CHECK();
    return MG_OK;
}
