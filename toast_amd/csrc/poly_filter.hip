// poly_filter.hip -- the kernels behind toast.ops.PolyFilter and toast.ops.CommonModeFilter on the device.
//
// Reference: `filter_polynomial`, src/libtoast/src/toast_tod_filter.cpp:18-158 (binding
// src/toast/_libtoast/tod_filter.cpp:326-383), and `sum_detectors` / `subtract_mean`,
// src/toast/_libtoast/tod_filter.cpp:9-97.  The reference builds, per scan, a [norder][scanlen] template matrix on
// the host, compresses it and the signals to the unflagged samples and hands them to LAPACK's DGELSS; detectors with
// identical flags share one call.  Here every (detector, interval) is independent and no template matrix ever exists
// in memory: each lane evaluates the Legendre recurrence for its own samples and accumulates the Gram matrix
// T_good T_good^T and the projection T_good s in registers.
//
//   k_poly_single     one workgroup per (detector, interval): signal and flags are read ONCE into LDS (16-byte
//                     accesses), Gram + projection reduced (wave shuffles, then the 4 waves through LDS in a fixed
//                     order), the norder x norder system solved by Cholesky in fp64 on the first lanes of a wave, the
//                     fit subtracted from the LDS copy on the way back out: 17-18 B per detector-sample.
//   k_poly_partial    two-pass path, pass 1: several workgroups per (detector, interval), each writes the partial
//   k_poly_solve      Gram / projection of its kPolyChunk samples to a scratch buffer; one wave per (detector,
//   k_poly_subtract   interval) adds them up in chunk order (no atomics) and solves; pass 2 subtracts: 25-26 B.
//
// The normal equations square the condition number of the templates on the good samples, so they are only the FAST
// path: the Cholesky compares every pivot with the diagonal entry it started from, and when one falls below
// kPolyPivotFloor of it (good samples in a contiguous stretch: a detector cut for most of a scan) the job is fitted by
// `poly_forsythe` instead -- the polynomials orthogonal ON THE GOOD SAMPLES by their three-term recurrence, one
// projection and one subtraction per term, no linear system.  In the single pass it sweeps the LDS copy; in the two
// passes k_poly_solve leaves a mark in the scratch buffer and the workgroup of the interval's first chunk sweeps global
// memory in k_poly_subtract.  Status 3 is left for input that is not finite.
//
// The path is chosen per interval by ONE threshold: an interval of at most kPolyStageCap samples (what two workgroups
// per CU can stage in the 160 KB of LDS) takes the single pass, a longer one the two passes.
//
//   k_sum_detectors / k_subtract_mean / k_common_mode   one lane owns one sample and walks the detector list in list
//                     order -- the reference's summation order, so the results are bit-identical --; the fused form
//                     keeps the mean in a register between the two sweeps over the rows.

#include <algorithm>

#include "kernel_common.hpp"

namespace {

constexpr int kPolyMaxTerms = 16;      // order + 1 supported by the entry point
constexpr int kPolyStageCap = 7424;    // samples staged in LDS by one workgroup: 10 B each, two workgroups per CU
constexpr int kPolyChunk = 4096;       // samples per workgroup of the two-pass path

// kPolyNotFinite (3): a good sample is NaN or infinite; the interval is left untouched.
enum PolyStatus : int32_t { kPolyFitted = 0, kPolyNoGood = 1, kPolyReduced = 2, kPolyNotFinite = 3 };
enum PolySolve : int { kSolveDirect = 0, kSolveRobust = 1, kSolveNotFinite = 2 };

// A Cholesky pivot below this fraction of the diagonal entry it started from sends the job to poly_forsythe.  The
// normal equations lose about 1e-14 / ratio of max|signal| on ALL samples of the interval (host emulation on
// tests/golden/poly_filter_edges.npz: 5e-13 at a ratio of 0.015, 2e-14 at 0.036, 3e-15 at 0.25), and the bound of the
// suite is 1e-12: 0.05 keeps the direct solve a factor of five inside it.  Scattered flags never get there -- 10 % at
// random leave every ratio above 0.9 at all supported orders --, half an interval flagged in one block does.
constexpr double kPolyPivotFloor = 0.05;

template <int N>
struct PolyAcc {
    static constexpr int NP = N * (N + 1) / 2;
    static constexpr int NV = NP + N;     // packed upper Gram (row-major, r <= c), then the projection
    double v[NV];
    int ngood;
};

// toast_tod_filter.cpp:69-93: p[0] = 1, p[1] = x, p[k] = ((2k - 1) x p[k-1] - (k - 1) p[k-2]) * (1 / k)
template <int N>
__device__ __forceinline__ void legendre_terms(double x, double (&p)[N]) {
    p[0] = 1.0;
    if constexpr (N > 1) p[1] = x;
#pragma unroll
    for (int k = 2; k < N; ++k) {
        const double kinv = 1. / (double)k;
        p[k] = ((double)(2 * k - 1) * x * p[k - 1] - (double)(k - 1) * p[k - 2]) * kinv;
    }
}

template <int N>
__device__ __forceinline__ void poly_accumulate(PolyAcc<N> & a, double x, double s) {
    double p[N];
    legendre_terms<N>(x, p);
    int q = 0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = r; c < N; ++c) a.v[q++] += p[r] * p[c];
    }
#pragma unroll
    for (int r = 0; r < N; ++r) a.v[PolyAcc<N>::NP + r] += p[r] * s;
    ++a.ngood;
}

// Lane partials -> wave totals (xor butterflies: the same tree in every run) -> `out[wave][k]` in LDS.
template <int N>
__device__ __forceinline__ void poly_wave_totals(PolyAcc<N> & a, double * out /*[4][NV + 1]*/) {
    constexpr int NV = PolyAcc<N>::NV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double v = a.v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) out[wave * (NV + 1) + k] = v;
    }
    int g = a.ngood;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) g += __shfl_xor(g, off, 64);
    if (lane == 0) out[wave * (NV + 1) + NV] = (double)g;
}

// Solve the leading n x n block of the packed system `tot` (NV values: Gram upper triangle, projection) by Cholesky.
// Every wave that calls this does the same work in its own registers: lane r < N holds row r of the lower triangle,
// the columns travel by shuffles, nothing goes through memory.  kSolveDirect: lane k < n holds coefficient k in `x`;
// kSolveRobust: a pivot fell below kPolyPivotFloor of its diagonal entry (or is not positive); kSolveNotFinite: the
// projection holds a NaN or an infinity (the Gram matrix cannot: |x| < 1).
template <int N>
__device__ __forceinline__ PolySolve poly_cholesky(const double * tot, int n, double & x) {
    constexpr int NP = PolyAcc<N>::NP;
    const int lane = threadIdx.x & 63;
    double a[N], u[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        // A[lane][c], c <= lane: packed index of (c, lane) in the upper triangle
        const int r = (lane < N) ? lane : 0;
        const int lo = (c <= r) ? c : r, hi = (c <= r) ? r : c;
        a[c] = (lane < N) ? tot[lo * N - (lo * (lo - 1)) / 2 + (hi - lo)] : 0.0;
        u[c] = 0.0;
    }
    double b = (lane < N) ? tot[NP + lane] : 0.0;
    const bool finite = fabs(b) <= 1.7976931348623157e308;
    // this lane's diagonal entry as it was, and its pivot's square root: compared after the loop, off its chain
    const double diag = (lane < N) ? tot[lane * N - (lane * (lane - 1)) / 2] : 1.0;
    double lmine = 1.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k < n && ok) {
            const double akk = __shfl(a[k], k, 64);
            if (!(akk > 0.0)) {
                ok = false;
            } else {
                const double lkk = f_sqrt(akk);
                a[k] = (lane == k) ? lkk : a[k] / lkk;        // L[lane][k]
                if (lane == k) lmine = lkk;
#pragma unroll
                for (int c = k + 1; c < N; ++c) {
                    if (c < n) {
                        const double lck = __shfl(a[k], c, 64);   // L[c][k]
                        if (lane == k) u[c] = lck;                // column k of L, kept for the back substitution
                        if (c <= lane) a[c] -= a[k] * lck;
                    }
                }
            }
        }
    }
    if (__any(!finite)) return kSolveNotFinite;
    if (!ok || __any(lane < n && !(lmine * lmine > kPolyPivotFloor * diag))) return kSolveRobust;
    // L y = b
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k < n) {
            const double yk = __shfl(b / a[k], k, 64);
            if (lane == k) b = yk;
            if (lane > k) b -= a[k] * yk;
        }
    }
    // L^T x = y
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        if (k < n) {
            const double xk = __shfl(b / a[k], k, 64);
            if (lane == k) b = xk;
            if (lane < k) b -= u[k] * xk;
        }
    }
    x = b;
    return kSolveDirect;
}

__device__ __forceinline__ bool poly_good(uint8_t s, uint8_t smask, uint8_t d, uint8_t dmask) {
    return ((s & smask) == 0) && ((d & dmask) == 0);
}

// ------------------------------------------------------------------------------------ the robust fit
// The monic polynomials orthogonal on the good samples (Forsythe): p_-1 = 0, p_0 = 1,
// p_{k+1} = (x - a_k) p_k - b_k p_{k-1} with a_k = <x p_k, p_k> / <p_k, p_k>, b_k = <p_k, p_k> / <p_{k-1}, p_{k-1}>,
// the inner products over the good samples; c_k = <r, p_k> / <p_k, p_k> and r -= c_k p_k on ALL samples.  Sweep k
// subtracts term k - 1 and projects on p_k in one pass over r: n + 1 sweeps, three sums each, reduced in a fixed
// order (lanes by xor butterflies, the waves in wave order) so that two runs give the same bits.  No sample's p_k is
// stored: each lane runs the recurrence up to k from the a_j, b_j in LDS.  The coefficients come out in the Legendre
// basis of the direct solve: lanes 0..15 carry the Legendre expansion of p_k along (x P_j = ((j + 1) P_{j+1} +
// j P_{j-1}) / (2j + 1)) and add c_k times it to coefficient `lane`.
struct PolyRobustLds {
    double a[kPolyMaxTerms], b[kPolyMaxTerms];
    double q[3][kPolyMaxTerms];       // Legendre expansions of p_{k-1}, p_k, p_{k+1}, rotating
    double red[kThreads / 64][3];
    double c;                         // coefficient of the term the next sweep subtracts
    int stop;                         // <p_k, p_k> underflowed to zero: no further term is fitted
};

// All kThreads threads of a workgroup; `r`, `df`, `sf` point at the interval's first sample (LDS or global memory; `df`
// or `sf` may be null).  In place on r[0, len).  Threads 0..order write `crow`.
__device__ __forceinline__ void poly_forsythe(double * r, const uint8_t * df, uint8_t det_mask, const uint8_t * sf,
                                              uint8_t shared_mask, int64_t len, int n, int order, PolyRobustLds & w,
                                              double * __restrict__ crow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = threadIdx.x;
    const double dx = 2. / (double)len;
    const double xstart = 0.5 * dx - 1;
    if (t < kPolyMaxTerms) {
        w.q[0][t] = (t == 0) ? 1.0 : 0.0;
        w.q[2][t] = 0.0;                  // p_-1
    }
    if (t == 0) w.stop = 0, w.c = 0.0;
    __syncthreads();
    double g_prev = 1.0, coeff = 0.0;
    for (int k = 0; k <= n; ++k) {
        const double c_prev = w.c;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = t; i < len; i += kThreads) {
            const double x = xstart + (double)i * dx;
            double pm = 0.0, p = 1.0;
            for (int j = 0; j < k; ++j) {
                const double pn = (x - w.a[j]) * p - w.b[j] * pm;
                pm = p;
                p = pn;
            }
            double ri = r[i];
            if (k > 0) {
                ri -= c_prev * pm;
                r[i] = ri;
            }
            const uint8_t fd = (df != nullptr) ? df[i] : (uint8_t)0;
            const uint8_t fs = (sf != nullptr) ? sf[i] : (uint8_t)0;
            if (k < n && poly_good(fs, shared_mask, fd, det_mask)) {
                const double pp = p * p;
                s0 += pp;
                s1 += x * pp;
                s2 += ri * p;
            }
        }
        if (k == n) break;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s0 += __shfl_xor(s0, off, 64);
            s1 += __shfl_xor(s1, off, 64);
            s2 += __shfl_xor(s2, off, 64);
        }
        if (lane == 0) w.red[wave][0] = s0, w.red[wave][1] = s1, w.red[wave][2] = s2;
        __syncthreads();
        if (t < kPolyMaxTerms) {      // every one of these lanes adds the waves up in the same order
            double g = 0.0, xg = 0.0, rp = 0.0;
            for (int v = 0; v < kThreads / 64; ++v) g += w.red[v][0], xg += w.red[v][1], rp += w.red[v][2];
            if (!(g > 0.0)) {
                if (t == 0) w.stop = 1, w.c = 0.0;
            } else {
                const double ak = xg / g, bk = (k > 0) ? g / g_prev : 0.0, ck = rp / g;
                const double * qc = w.q[k % 3];
                const double * qp = w.q[(k + 2) % 3];
                coeff += ck * qc[t];
                // x * p_k in the Legendre basis, entry t
                const double below = (t > 0) ? qc[t - 1] * ((double)t / (double)(2 * t - 1)) : 0.0;
                const double above = (t + 1 < kPolyMaxTerms) ? qc[t + 1] * ((double)(t + 1) / (double)(2 * t + 3)) : 0.0;
                w.q[(k + 1) % 3][t] = (below + above) - ak * qc[t] - bk * qp[t];
                if (t == 0) w.a[k] = ak, w.b[k] = bk, w.c = ck;
                g_prev = g;
            }
        }
        __syncthreads();
        if (w.stop != 0) break;
    }
    if (t <= order) crow[t] = coeff;
}

// signal[i] -= sum_k coeff[k] P_k(x_i), one order after the other like toast_tod_filter.cpp:144-156
template <int N>
__device__ __forceinline__ double poly_subtract(double s, double x, const double (&coeff)[N]) {
    double p[N];
    legendre_terms<N>(x, p);
#pragma unroll
    for (int k = 0; k < N; ++k) s -= coeff[k] * p[k];
    return s;
}

struct PolyJob {
    int64_t first;   // clipped to [0, n_samp)
    int64_t last;
    int32_t view;    // index into the caller's interval list
    int32_t chunk0;  // two-pass: first slot of this interval in the chunk list
};

// Bytes [src, src + n) -> LDS dst[pad + i] with pad = src & 15, so that aligned 16-byte granules of global memory are
// aligned granules of LDS; partial granules at both ends go byte by byte.
__device__ __forceinline__ void stage_bytes(const uint8_t * __restrict__ src, int64_t n, uint8_t * dst, int pad) {
    const int64_t n_gran = (pad + n + 15) >> 4;
    const uint8_t * base = src - pad;
    for (int64_t g = threadIdx.x; g < n_gran; g += kThreads) {
        const int64_t b0 = g << 4;
        if (b0 >= pad && b0 + 16 <= pad + n) {
            *reinterpret_cast<uint4 *>(dst + b0) = *reinterpret_cast<const uint4 *>(base + b0);
        } else {
            for (int64_t b = b0; b < b0 + 16; ++b) {
                if (b >= pad && b < pad + n) dst[b] = base[b];
            }
        }
    }
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_poly_single(
    double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, const PolyJob * __restrict__ jobs, int order,
    int64_t n_interval, int stage_samples, double * __restrict__ coeff_out, int32_t * __restrict__ status_out) {
    constexpr int NV = PolyAcc<N>::NV;
    extern __shared__ double2 lds2[];
    __shared__ double wave_tot[4 * (NV + 1)];
    __shared__ double tot[NV + 1];
    __shared__ PolyRobustLds robust;
    // [stage_samples + 2 doubles][stage_samples + 32 bytes of detector flags][the same of shared flags]
    double * s_sig = reinterpret_cast<double *>(lds2);
    uint8_t * s_df = reinterpret_cast<uint8_t *>(s_sig + stage_samples + 2);
    uint8_t * s_sf = s_df + stage_samples + 32;

    const PolyJob job = jobs[blockIdx.x];
    const int64_t d = blockIdx.y;
    const int len = (int)(job.last - job.first);
    double * __restrict__ crow = coeff_out + (d * n_interval + job.view) * (order + 1);
    int32_t * __restrict__ srow = status_out + d * n_interval + job.view;
    if (len <= 0) {
        if (threadIdx.x == 0) *srow = kPolyNoGood;
        if ((int)threadIdx.x <= order) crow[threadIdx.x] = 0.0;
        return;
    }
    double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp + job.first;
    const uint8_t * __restrict__ df = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp + job.first : nullptr;
    const uint8_t * __restrict__ sf = (shared_flags != nullptr) ? shared_flags + job.first : nullptr;

    // ---- stage: doubles in aligned pairs (pad_s = 1 when the interval starts on an odd double)
    const int pad_s = (int)((reinterpret_cast<uintptr_t>(sig) >> 3) & 1);
    const int n_pair = (pad_s + len + 1) >> 1;
    for (int p = threadIdx.x; p < n_pair; p += kThreads) {
        const int i0 = 2 * p;    // index in the padded frame
        if (i0 >= pad_s && i0 + 2 <= pad_s + len) {
            lds2[p] = *reinterpret_cast<const double2 *>(sig - pad_s + i0);
        } else {
            if (i0 >= pad_s && i0 < pad_s + len) s_sig[i0] = sig[i0 - pad_s];
            if (i0 + 1 >= pad_s && i0 + 1 < pad_s + len) s_sig[i0 + 1] = sig[i0 + 1 - pad_s];
        }
    }
    const int pad_d = (df != nullptr) ? (int)(reinterpret_cast<uintptr_t>(df) & 15) : 0;
    const int pad_f = (sf != nullptr) ? (int)(reinterpret_cast<uintptr_t>(sf) & 15) : 0;
    if (df != nullptr) stage_bytes(df, len, s_df, pad_d);
    if (sf != nullptr) stage_bytes(sf, len, s_sf, pad_f);
    __syncthreads();

    // ---- Gram matrix and projection over the good samples
    const double dx = 2. / (double)len;
    const double xstart = 0.5 * dx - 1;
    PolyAcc<N> acc;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc.v[k] = 0.0;
    acc.ngood = 0;
    for (int i = threadIdx.x; i < len; i += kThreads) {
        const uint8_t fd = (df != nullptr) ? s_df[pad_d + i] : (uint8_t)0;
        const uint8_t fs = (sf != nullptr) ? s_sf[pad_f + i] : (uint8_t)0;
        if (poly_good(fs, shared_mask, fd, det_mask)) poly_accumulate<N>(acc, xstart + (double)i * dx, s_sig[pad_s + i]);
    }
    poly_wave_totals<N>(acc, wave_tot);
    __syncthreads();
    if ((int)threadIdx.x <= NV) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += wave_tot[w * (NV + 1) + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const int ngood = (int)tot[NV];
    if (ngood == 0) {
        if (threadIdx.x == 0) *srow = kPolyNoGood;
        if ((int)threadIdx.x <= order) crow[threadIdx.x] = 0.0;
        return;
    }
    const int n = (ngood < order + 1) ? ngood : order + 1;
    double xk = 0.0;
    const PolySolve solve = poly_cholesky<N>(tot, n, xk);
    if (solve == kSolveNotFinite) {
        if (threadIdx.x == 0) *srow = kPolyNotFinite;
        if ((int)threadIdx.x <= order) crow[threadIdx.x] = 0.0;
        return;
    }
    if (solve == kSolveRobust) {
        // the LDS copy becomes the residual; it goes back out as it is
        poly_forsythe(s_sig + pad_s, (df != nullptr) ? s_df + pad_d : nullptr, det_mask, (sf != nullptr) ? s_sf + pad_f : nullptr,
                      shared_mask, len, n, order, robust, crow);
        if (threadIdx.x == 0) *srow = (n < order + 1) ? kPolyReduced : kPolyFitted;
        __syncthreads();
        for (int p = threadIdx.x; p < n_pair; p += kThreads) {
            const int i0 = 2 * p;
            if (i0 >= pad_s && i0 + 2 <= pad_s + len) {
                *reinterpret_cast<double2 *>(sig - pad_s + i0) = lds2[p];
            } else {
                if (i0 >= pad_s && i0 < pad_s + len) sig[i0 - pad_s] = s_sig[i0];
                if (i0 + 1 >= pad_s && i0 + 1 < pad_s + len) sig[i0 + 1 - pad_s] = s_sig[i0 + 1];
            }
        }
        return;
    }
    double coeff[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double ck = __shfl(xk, k, 64);
        coeff[k] = (k < n) ? ck : 0.0;
    }
    if ((int)threadIdx.x <= order) crow[threadIdx.x] = (threadIdx.x < (unsigned)n) ? xk : 0.0;
    if (threadIdx.x == 0) *srow = (n < order + 1) ? kPolyReduced : kPolyFitted;

    // ---- subtract from ALL samples, on the way out
    for (int p = threadIdx.x; p < n_pair; p += kThreads) {
        const int i0 = 2 * p;
        if (i0 >= pad_s && i0 + 2 <= pad_s + len) {
            double2 v = lds2[p];
            v.x = poly_subtract<N>(v.x, xstart + (double)(i0 - pad_s) * dx, coeff);
            v.y = poly_subtract<N>(v.y, xstart + (double)(i0 + 1 - pad_s) * dx, coeff);
            *reinterpret_cast<double2 *>(sig - pad_s + i0) = v;
        } else {
            for (int i = i0; i < i0 + 2; ++i) {
                if (i >= pad_s && i < pad_s + len) {
                    sig[i - pad_s] = poly_subtract<N>(s_sig[i], xstart + (double)(i - pad_s) * dx, coeff);
                }
            }
        }
    }
}

struct PolyChunk {
    int32_t job;     // index into the two-pass job list
    int32_t chunk;   // chunk of that interval
};

template <int N>
__global__ __launch_bounds__(kThreads) void k_poly_partial(
    const double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, const PolyJob * __restrict__ jobs,
    const PolyChunk * __restrict__ chunks, int64_t n_chunk, double * __restrict__ partial) {
    constexpr int NV = PolyAcc<N>::NV;
    __shared__ double wave_tot[4 * (NV + 1)];
    const PolyChunk ch = chunks[blockIdx.x];
    const PolyJob job = jobs[ch.job];
    const int64_t d = blockIdx.y;
    const int64_t len = job.last - job.first;
    const int64_t i0 = (int64_t)ch.chunk * kPolyChunk;
    const int64_t i1 = (i0 + kPolyChunk < len) ? i0 + kPolyChunk : len;
    const double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp + job.first;
    const uint8_t * __restrict__ df = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp + job.first : nullptr;
    const uint8_t * __restrict__ sf = (shared_flags != nullptr) ? shared_flags + job.first : nullptr;
    const double dx = 2. / (double)len;
    const double xstart = 0.5 * dx - 1;
    PolyAcc<N> acc;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc.v[k] = 0.0;
    acc.ngood = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
        const uint8_t fd = (df != nullptr) ? df[i] : (uint8_t)0;
        const uint8_t fs = (sf != nullptr) ? sf[i] : (uint8_t)0;
        const double s = sig[i];
        if (poly_good(fs, shared_mask, fd, det_mask)) poly_accumulate<N>(acc, xstart + (double)i * dx, s);
    }
    poly_wave_totals<N>(acc, wave_tot);
    __syncthreads();
    if ((int)threadIdx.x <= NV) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += wave_tot[w * (NV + 1) + threadIdx.x];
        partial[(d * n_chunk + blockIdx.x) * (NV + 1) + threadIdx.x] = t;
    }
}

// One wave per (detector, two-pass interval): partial sums in chunk order, then the solve.
template <int N>
__global__ __launch_bounds__(64) void k_poly_solve(const PolyJob * __restrict__ jobs, int64_t n_chunk,
                                                   double * __restrict__ partial, int order, int64_t n_interval,
                                                   double * __restrict__ coeff_out, int32_t * __restrict__ status_out) {
    constexpr int NV = PolyAcc<N>::NV;
    __shared__ double tot[NV + 1];
    const PolyJob job = jobs[blockIdx.x];
    const int64_t d = blockIdx.y;
    const int64_t len = job.last - job.first;
    const int n_ch = (int)((len + kPolyChunk - 1) / kPolyChunk);
    double * __restrict__ crow = coeff_out + (d * n_interval + job.view) * (order + 1);
    int32_t * __restrict__ srow = status_out + d * n_interval + job.view;
    for (int k = threadIdx.x; k <= NV; k += 64) {
        double t = 0.0;
        for (int c = 0; c < n_ch; ++c) t += partial[(d * n_chunk + job.chunk0 + c) * (NV + 1) + k];
        tot[k] = t;
    }
    __syncthreads();
    const int ngood = (int)tot[NV];
    int32_t status = kPolyNoGood;
    double xk = 0.0;
    int n = 0;
    if (ngood > 0) {
        n = (ngood < order + 1) ? ngood : order + 1;
        const PolySolve solve = poly_cholesky<N>(tot, n, xk);
        status = (solve == kSolveNotFinite) ? kPolyNotFinite : ((n < order + 1) ? kPolyReduced : kPolyFitted);
        // The robust fit is left to k_poly_subtract: the good-sample count of the interval's first chunk, which has
        // been added up above, becomes -n.  That mark does not change while k_poly_subtract runs, so every workgroup
        // of the interval sees the same thing whenever it is scheduled (the status and the coefficients do change).
        if (solve == kSolveRobust) {
            if (threadIdx.x == 0) partial[(d * n_chunk + job.chunk0) * (NV + 1) + NV] = -(double)n;
            xk = 0.0;
        }
    }
    const bool fitted = (status == kPolyFitted || status == kPolyReduced);
    if ((int)threadIdx.x <= order) crow[threadIdx.x] = (fitted && (int)threadIdx.x < n) ? xk : 0.0;
    if (threadIdx.x == 0) *srow = status;
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_poly_subtract(
    double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, const PolyJob * __restrict__ jobs,
    const PolyChunk * __restrict__ chunks, int64_t n_chunk, const double * __restrict__ partial, int order,
    int64_t n_interval, double * __restrict__ coeff_io, const int32_t * __restrict__ status_in) {
    constexpr int NV = PolyAcc<N>::NV;
    __shared__ PolyRobustLds robust;
    const PolyChunk ch = chunks[blockIdx.x];
    const PolyJob job = jobs[ch.job];
    const int64_t d = blockIdx.y;
    const int32_t status = status_in[d * n_interval + job.view];
    if (status != kPolyFitted && status != kPolyReduced) return;
    const double mark = partial[(d * n_chunk + job.chunk0) * (NV + 1) + NV];
    if (mark < 0.0) {
        // k_poly_solve left the fit to poly_forsythe: the whole interval by the workgroup of its first chunk, which
        // alone writes the coefficients; the other workgroups of the interval have nothing to do
        if (ch.chunk != 0) return;
        const int n = (int)(-mark);
        double * __restrict__ r = signal + (int64_t)sig_index[d] * n_samp + job.first;
        const uint8_t * df = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp + job.first : nullptr;
        const uint8_t * sf = (shared_flags != nullptr) ? shared_flags + job.first : nullptr;
        poly_forsythe(r, df, det_mask, sf, shared_mask, job.last - job.first, n, order, robust,
                      coeff_io + (d * n_interval + job.view) * (order + 1));
        return;
    }
    const double * __restrict__ crow = coeff_io + (d * n_interval + job.view) * (order + 1);
    double coeff[N];
#pragma unroll
    for (int k = 0; k < N; ++k) coeff[k] = (k <= order) ? crow[k] : 0.0;
    const int64_t len = job.last - job.first;
    const int64_t i0 = (int64_t)ch.chunk * kPolyChunk;
    const int64_t i1 = (i0 + kPolyChunk < len) ? i0 + kPolyChunk : len;
    double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp + job.first;
    const double dx = 2. / (double)len;
    const double xstart = 0.5 * dx - 1;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) sig[i] = poly_subtract<N>(sig[i], xstart + (double)i * dx, coeff);
}

// ------------------------------------------------------------------------------------ common mode
constexpr int kCmUnroll = 8;   // detector rows loaded ahead of the (ordered) additions

// tod_filter.cpp:39-53 for sample i: the accumulator and the hit count start from `sum` / `hits`
__device__ __forceinline__ void common_mode_sum(const double * __restrict__ signal, int64_t n_samp,
                                                const int32_t * __restrict__ sig_index, const uint8_t * __restrict__ det_flags,
                                                const int32_t * __restrict__ flag_index, uint8_t det_mask, int64_t n_det,
                                                int64_t i, double & acc, int64_t & hits) {
    for (int64_t d0 = 0; d0 < n_det; d0 += kCmUnroll) {
        double v[kCmUnroll];
        uint8_t f[kCmUnroll];
#pragma unroll
        for (int k = 0; k < kCmUnroll; ++k) {
            const int64_t d = (d0 + k < n_det) ? d0 + k : n_det - 1;
            v[k] = signal[(int64_t)sig_index[d] * n_samp + i];
            f[k] = (det_flags != nullptr) ? det_flags[(int64_t)flag_index[d] * n_samp + i] : (uint8_t)0;
        }
#pragma unroll
        for (int k = 0; k < kCmUnroll; ++k) {
            if (d0 + k < n_det && (f[k] & det_mask) == 0) {
                acc += v[k];
                ++hits;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_sum_detectors(
    const double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, int64_t n_det, double * __restrict__ sum,
    int64_t * __restrict__ hits) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_samp; i += (int64_t)gridDim.x * kThreads) {
        if (shared_flags != nullptr && (shared_flags[i] & shared_mask) != 0) continue;
        double acc = sum[i];
        int64_t h = hits[i];
        common_mode_sum(signal, n_samp, sig_index, det_flags, flag_index, det_mask, n_det, i, acc, h);
        sum[i] = acc;
        hits[i] = h;
    }
}

// tod_filter.cpp:78-94: sum /= hits where hits != 0 (written back), then every listed row -= sum
__global__ __launch_bounds__(kThreads) void k_subtract_mean(double * __restrict__ signal, int64_t n_samp,
                                                            const int32_t * __restrict__ sig_index, int64_t n_det,
                                                            double * __restrict__ sum, const int64_t * __restrict__ hits) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_samp; i += (int64_t)gridDim.x * kThreads) {
        double mean = sum[i];
        const int64_t h = hits[i];
        if (h != 0) {
            mean /= (double)h;
            sum[i] = mean;
        }
        for (int64_t d = 0; d < n_det; ++d) signal[(int64_t)sig_index[d] * n_samp + i] -= mean;
    }
}

__global__ __launch_bounds__(kThreads) void k_common_mode(
    double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, int64_t n_det, double * __restrict__ mean_out,
    int64_t * __restrict__ hits_out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_samp; i += (int64_t)gridDim.x * kThreads) {
        double mean = 0.0;
        int64_t h = 0;
        if (shared_flags == nullptr || (shared_flags[i] & shared_mask) == 0) {
            common_mode_sum(signal, n_samp, sig_index, det_flags, flag_index, det_mask, n_det, i, mean, h);
        }
        if (h != 0) mean /= (double)h;
        if (mean_out != nullptr) mean_out[i] = mean;
        if (hits_out != nullptr) hits_out[i] = h;
        for (int64_t d = 0; d < n_det; ++d) signal[(int64_t)sig_index[d] * n_samp + i] -= mean;
    }
}

struct PolyArgs {
    int64_t order, n_samp, n_det, n_interval;
    const int32_t * signal_index;
    double * d_signal;
    const int32_t * flag_index;
    const uint8_t * d_det_flags;
    uint8_t det_mask;
    const uint8_t * d_shared_flags;
    uint8_t shared_mask;
    double * d_coeff;
    int32_t * d_status;
    std::vector<PolyJob> single, two;
    std::vector<PolyChunk> chunks;
    hipStream_t st;
};

template <int N>
void poly_launch(PolyArgs & a) {
    constexpr int NV = PolyAcc<N>::NV;
    ParamBlock pb;
    const size_t o_si = pb.push(a.signal_index, sizeof(int32_t) * a.n_det);
    std::vector<int32_t> no_flags(a.n_det, 0);
    const size_t o_fi = pb.push(a.d_det_flags != nullptr ? a.flag_index : no_flags.data(), sizeof(int32_t) * a.n_det);
    const size_t o_js = pb.push_vec(a.single);
    const size_t o_jt = pb.push_vec(a.two);
    const size_t o_ch = pb.push_vec(a.chunks);
    const char * dparam = pb.commit(a.st);
    const int32_t * sidx = (const int32_t *)(dparam + o_si);
    const int32_t * fidx = (const int32_t *)(dparam + o_fi);
    if (!a.single.empty()) {
        int64_t longest = 0;
        for (const PolyJob & j : a.single) longest = std::max(longest, j.last - j.first);
        const int stage = (int)((longest + 15) & ~int64_t(15));
        const size_t lds = sizeof(double) * (stage + 2) + 2 * (size_t)(stage + 32);
        // more than 64 KB of dynamic LDS needs the attribute; set on every call: it is per device and cheap
        TH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_poly_single<N>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const PolyJob * jobs = (const PolyJob *)(dparam + o_js);
        for (size_t j0 = 0; j0 < a.single.size(); j0 += 65535 * 16) {     // (grid.x is plenty; grid.y carries the detectors)
            const size_t nj = std::min(a.single.size() - j0, (size_t)65535 * 16);
            for (int64_t d0 = 0; d0 < a.n_det; d0 += 65535) {
                const int64_t nd = std::min<int64_t>(a.n_det - d0, 65535);
                hipLaunchKernelGGL(k_poly_single<N>, dim3((unsigned)nj, (unsigned)nd), dim3(kThreads), lds, a.st, a.d_signal,
                                   a.n_samp, sidx + d0, a.d_det_flags, fidx + d0, a.det_mask, a.d_shared_flags, a.shared_mask,
                                   jobs + j0, (int)a.order, a.n_interval, stage, a.d_coeff + d0 * a.n_interval * (a.order + 1),
                                   a.d_status + d0 * a.n_interval);
                check_launch();
            }
        }
    }
    if (!a.two.empty()) {
        const int64_t n_chunk = (int64_t)a.chunks.size();
        const PolyJob * jobs = (const PolyJob *)(dparam + o_jt);
        const PolyChunk * chunks = (const PolyChunk *)(dparam + o_ch);
        for (int64_t d0 = 0; d0 < a.n_det; d0 += 65535) {
            const int64_t nd = std::min<int64_t>(a.n_det - d0, 65535);
            double * partial = static_cast<double *>(Manager::get().scratch(
                Manager::kScratchPoly, sizeof(double) * (size_t)(nd * n_chunk * (NV + 1)), a.st));
            double * coeff = a.d_coeff + d0 * a.n_interval * (a.order + 1);
            int32_t * status = a.d_status + d0 * a.n_interval;
            hipLaunchKernelGGL(k_poly_partial<N>, dim3((unsigned)n_chunk, (unsigned)nd), dim3(kThreads), 0, a.st, a.d_signal,
                               a.n_samp, sidx + d0, a.d_det_flags, fidx + d0, a.det_mask, a.d_shared_flags, a.shared_mask, jobs,
                               chunks, n_chunk, partial);
            check_launch();
            hipLaunchKernelGGL(k_poly_solve<N>, dim3((unsigned)a.two.size(), (unsigned)nd), dim3(64), 0, a.st, jobs, n_chunk,
                               partial, (int)a.order, a.n_interval, coeff, status);
            check_launch();
            hipLaunchKernelGGL(k_poly_subtract<N>, dim3((unsigned)n_chunk, (unsigned)nd), dim3(kThreads), 0, a.st, a.d_signal,
                               a.n_samp, sidx + d0, a.d_det_flags, fidx + d0, a.det_mask, a.d_shared_flags, a.shared_mask,
                               jobs, chunks, n_chunk, partial, (int)a.order, a.n_interval, coeff, status);
            check_launch();
        }
    }
}

struct CmIndex {
    const int32_t * sidx;
    const int32_t * fidx;
};

CmIndex cm_index(const int32_t * signal_index, const int32_t * flag_index, bool have_flags, int64_t n_det, hipStream_t st) {
    ParamBlock pb;
    const size_t o_si = pb.push(signal_index, sizeof(int32_t) * n_det);
    std::vector<int32_t> no_flags(n_det, 0);
    const size_t o_fi = pb.push(have_flags && flag_index != nullptr ? flag_index : no_flags.data(), sizeof(int32_t) * n_det);
    const char * dparam = pb.commit(st);
    return CmIndex{(const int32_t *)(dparam + o_si), (const int32_t *)(dparam + o_fi)};
}

}  // namespace

extern "C" {

int toast_hip_filter_polynomial_stage_cap(void) { return kPolyStageCap; }

int toast_hip_filter_polynomial_dev(int64_t order, int64_t n_samp, const int32_t * signal_index, double * d_signal,
                                    const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                    const uint8_t * d_shared_flags, uint8_t shared_flag_mask, int64_t n_det,
                                    const int64_t * starts, const int64_t * stops, int64_t n_interval, double * d_coeff,
                                    int32_t * d_status, int path, void * stream) {
    return guarded([&] {
        if (order < 0 || n_det <= 0 || n_interval <= 0 || n_samp <= 0) return;   // toast_tod_filter.cpp:25
        if (order + 1 > kPolyMaxTerms) {
            fail_arg("filter_polynomial: order + 1 = " + std::to_string(order + 1) + " terms, at most " +
                     std::to_string(kPolyMaxTerms) + " are supported");
        }
        if (path < 0 || path > 2) fail_arg("filter_polynomial: path must be 0 (by the rule), 1 (single pass) or 2 (two passes)");
        if (d_coeff == nullptr || d_status == nullptr) fail_arg("filter_polynomial: the coefficient and status outputs are required");
        if ((reinterpret_cast<uintptr_t>(d_signal) & 7) != 0) fail_arg("filter_polynomial: the signal must be 8-byte aligned");
        PolyArgs a;
        a.order = order, a.n_samp = n_samp, a.n_det = n_det, a.n_interval = n_interval;
        a.signal_index = signal_index, a.d_signal = d_signal, a.flag_index = flag_index, a.d_det_flags = d_det_flags;
        a.det_mask = det_flag_mask, a.d_shared_flags = d_shared_flags, a.shared_mask = shared_flag_mask;
        a.d_coeff = d_coeff, a.d_status = d_status, a.st = as_stream(stream);
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("filter_polynomial: detector flags need their row indices");
        for (int64_t v = 0; v < n_interval; ++v) {
            // toast_tod_filter.cpp:40-45: clipped to [0, n_samp), stop exclusive
            int64_t first = starts[v] < 0 ? 0 : starts[v];
            int64_t last = stops[v] > n_samp ? n_samp : stops[v];
            if (last < first) last = first;
            const int64_t len = last - first;
            if (len >= (int64_t(1) << 31)) fail_arg("filter_polynomial: an interval of 2^31 samples or more");
            PolyJob job{first, last, (int32_t)v, 0};
            const bool single = (path == 1) || (path == 0 && len <= kPolyStageCap) || len == 0;
            if (single) {
                if (len > kPolyStageCap) {
                    fail_arg("filter_polynomial: the single-pass path stages at most " + std::to_string(kPolyStageCap) +
                             " samples, an interval has " + std::to_string(len));
                }
                a.single.push_back(job);
            } else {
                job.chunk0 = (int32_t)a.chunks.size();
                const int32_t n_ch = (int32_t)((len + kPolyChunk - 1) / kPolyChunk);
                for (int32_t c = 0; c < n_ch; ++c) a.chunks.push_back(PolyChunk{(int32_t)a.two.size(), c});
                a.two.push_back(job);
            }
        }
        if (a.chunks.size() > 0x7fffffffu || a.two.size() > 0x7fffffffu) fail_arg("filter_polynomial: too many chunks");
        const int64_t terms = order + 1;
        if (terms <= 2) {
            poly_launch<2>(a);
        } else if (terms <= 4) {
            poly_launch<4>(a);
        } else if (terms <= 6) {
            poly_launch<6>(a);
        } else if (terms <= 9) {
            poly_launch<9>(a);
        } else {
            poly_launch<16>(a);
        }
    });
}

int toast_hip_sum_detectors_dev(int64_t n_samp, const int32_t * signal_index, const double * d_signal,
                                const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                const uint8_t * d_shared_flags, uint8_t shared_flag_mask, int64_t n_det, double * d_sum,
                                int64_t * d_hits, void * stream) {
    return guarded([&] {
        if (n_samp <= 0 || n_det <= 0) return;
        hipStream_t st = as_stream(stream);
        const CmIndex ix = cm_index(signal_index, flag_index, d_det_flags != nullptr, n_det, st);
        hipLaunchKernelGGL(k_sum_detectors, flat_grid(n_samp), dim3(kThreads), 0, st, d_signal, n_samp, ix.sidx, d_det_flags,
                           ix.fidx, det_flag_mask, d_shared_flags, shared_flag_mask, n_det, d_sum, d_hits);
        check_launch();
    });
}

int toast_hip_subtract_mean_dev(int64_t n_samp, const int32_t * signal_index, double * d_signal, int64_t n_det,
                                double * d_sum, const int64_t * d_hits, void * stream) {
    return guarded([&] {
        if (n_samp <= 0) return;
        hipStream_t st = as_stream(stream);
        const CmIndex ix = cm_index(signal_index, nullptr, false, n_det, st);
        hipLaunchKernelGGL(k_subtract_mean, flat_grid(n_samp), dim3(kThreads), 0, st, d_signal, n_samp, ix.sidx, n_det, d_sum,
                           d_hits);
        check_launch();
    });
}

int toast_hip_common_mode_subtract_dev(int64_t n_samp, const int32_t * signal_index, double * d_signal,
                                       const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                       const uint8_t * d_shared_flags, uint8_t shared_flag_mask, int64_t n_det,
                                       double * d_mean, int64_t * d_hits, void * stream) {
    return guarded([&] {
        if (n_samp <= 0 || n_det <= 0) return;
        hipStream_t st = as_stream(stream);
        const CmIndex ix = cm_index(signal_index, flag_index, d_det_flags != nullptr, n_det, st);
        hipLaunchKernelGGL(k_common_mode, flat_grid(n_samp), dim3(kThreads), 0, st, d_signal, n_samp, ix.sidx, d_det_flags,
                           ix.fidx, det_flag_mask, d_shared_flags, shared_flag_mask, n_det, d_mean, d_hits);
        check_launch();
    });
}

}  // extern "C"
