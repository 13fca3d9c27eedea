// poly2d_filter.hip -- the kernels behind toast.ops.PolyFilter2D on the device.
//
// Reference: `filter_poly2D`, src/libtoast/src/toast_tod_filter.cpp:357-470 (binding src/toast/_libtoast/tod_filter.cpp,
// NumPy form src/toast/ops/polyfilter/kernels_numpy.py:86-97) and the operator around it,
// src/toast/ops/polyfilter/polyfilter.py:270-381.  At every sample of a view and for every detector group the reference
// fits the n_mode = (order + 1)^2 templates T[d][(i, j)] = theta_d^i phi_d^j to the unflagged detectors of the group:
// normal equations, DGELSS at rcond = 1e-6 -- a truncated pseudo-inverse --, and subtracts the fit from the unflagged
// detectors.  It works on [n_samp][n_det] copies made on the host.  Here the detector-major arrays are swept in place
// with one lane per (sample, group), the way k_common_mode and k_f2d_project do.
//
//   k_p2d_moments   lane per (sample, group): walks the detectors of the group in list order and accumulates, for the
//                   good ones, the (2 order + 1)^2 moments sum theta^p phi^q -- A[(i,j),(i',j')] depends only on
//                   (i + i', j + j') -- and the n_mode projections sum T[d][m] s_d: 13 / 34 / 65 doubles per lane at
//                   order 1 / 2 / 3.  The moment basis of every detector comes from the launcher:
//                   theta^p phi^q = T[d][(min(p, order), min(q, order))] * T[d][(the rest)], one rounded product.
//                   A flagged detector is selected out, never multiplied in.  9 B per detector-sample.
//   k_p2d_solve     a team of W = 1 / 4 / 16 / 16 lanes per system: lane r holds row r of A and of V in registers.
//                   Cyclic Jacobi in fp64, pairs (p, q) in row order; the 2 x 2 rotation is computed by every lane of
//                   the team from shuffled entries, columns are rotated in place, rows p and q are exchanged by
//                   shuffles.  A team stops sweeping when max |off-diagonal| <= 2^-60 max |diagonal| (at most
//                   kP2dMaxSweeps sweeps), whatever the other teams of its wave do.  Then
//                   c = sum_i [lambda_i > 1e-6 lambda_max] v_i (v_i . b) / lambda_i:  v_i . b by an xor butterfly over
//                   the team (offsets W/2 .. 1), the sum over i in ascending i.  lambda_max = 0 gives c = 0, never 0/0.
//                   A projection that is not finite (a NaN or an infinity among the good signals) gives c = 0 and
//                   status kP2dNotFinite.
//   k_p2d_subtract  lane per (sample, group), coefficients in registers: signal[d] -= sum_m c_m T[d][m] (ascending m,
//                   started from 0) for the good detectors; when detector flags are given and all c_m == 0,
//                   poly_flag_mask is OR-ed into the flag of every detector of the group (polyfilter.py:345-364).
//                   17 B per good detector-sample.  Optionally c goes to [n_samp][n_group][n_mode].
//
// The packed systems live in a grow-only scratch buffer of the manager, struct-of-arrays ([value][system]) so that
// all three kernels read and write it coalesced; the sample tiles are processed in batches so that it stays below
// kP2dScratchBytes.  No atomics and a fixed order of every sum: two runs give the same bits, and a system's result does
// not depend on which other systems share its wave.  There is one launch variant so far (path 1); path 0, the rule,
// chooses it.

#include <algorithm>
#include <cmath>

#include "kernel_common.hpp"

namespace {

constexpr int kP2dMaxOrder = 3;
constexpr int kP2dMaxSweeps = 24;
constexpr double kP2dRcond = 1.0e-6;                         // DGELSS's rcond in toast_tod_filter.cpp
constexpr double kP2dOffTol = 8.673617379884035e-19;         // 2^-60
constexpr size_t kP2dScratchBytes = size_t(96) << 20;

enum P2dStatus : int32_t { kP2dSolved = 0, kP2dNoGood = 1, kP2dTruncated = 2, kP2dNotFinite = 3 };

struct P2dJob {
    int64_t first;   // first sample of the view, clipped to [0, n_samp)
    int32_t len;
    int32_t tile0;   // first sample tile of this view
};

template <int ORDER>
struct P2d {
    static constexpr int NO = ORDER + 1;
    static constexpr int N = NO * NO;                        // modes
    static constexpr int NM = 2 * ORDER + 1;
    static constexpr int NM2 = NM * NM;                      // moments
    static constexpr int NV = NM2 + N;                       // doubles of a packed system
    static constexpr int W = (N == 1) ? 1 : ((N == 4) ? 4 : 16);   // lanes of a solving team
};

// the view of a sample tile: the last job with tile0 <= tile
__device__ __forceinline__ int p2d_job_of_tile(const P2dJob * __restrict__ jobs, int n_job, int tile) {
    int lo = 0, hi = n_job - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= tile) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

__device__ __forceinline__ bool p2d_good(const uint8_t * __restrict__ det_flags, int64_t row, int64_t n_samp, int64_t s,
                                         uint8_t det_mask, uint8_t & f) {
    f = (det_flags != nullptr) ? det_flags[row * n_samp + s] : (uint8_t)0;
    return (f & det_mask) == 0;
}

// Every kernel: grid (tiles of this batch, n_group); slot = (tile - tile_begin) * kThreads + thread; the system of
// (slot, group) is number group * n_slot + slot of n_sys = n_group * n_slot.
template <int ORDER>
__global__ __launch_bounds__(kThreads) void k_p2d_moments(
    const double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index,
    const uint8_t * __restrict__ det_flags, const int32_t * __restrict__ flag_index, uint8_t det_mask,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, const int32_t * __restrict__ group_start,
    const int32_t * __restrict__ group_dets, const double * __restrict__ tmpl, const double * __restrict__ mom,
    const P2dJob * __restrict__ jobs, int n_job, int tile_begin, int64_t n_slot, int64_t n_sys, double * __restrict__ sys) {
    using P = P2d<ORDER>;
    const int tile = tile_begin + (int)blockIdx.x;
    const P2dJob job = jobs[p2d_job_of_tile(jobs, n_job, tile)];
    const int i = (tile - job.tile0) * kThreads + (int)threadIdx.x;
    const int g = (int)blockIdx.y;
    const int64_t idx = (int64_t)g * n_slot + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double acc[P::NV];
#pragma unroll
    for (int k = 0; k < P::NV; ++k) acc[k] = 0.0;
    if (i < job.len) {
        const int64_t s = job.first + i;
        const bool shared_ok = (shared_flags == nullptr) || ((shared_flags[s] & shared_mask) == 0);
        if (shared_ok) {
            const int k0 = group_start[g], k1 = group_start[g + 1];
            for (int k = k0; k < k1; ++k) {
                const int d = group_dets[k];
                uint8_t f;
                if (!p2d_good(det_flags, flag_index[d], n_samp, s, det_mask, f)) continue;
                const double v = signal[(int64_t)sig_index[d] * n_samp + s];
                const double * __restrict__ md = mom + (int64_t)d * P::NM2;
                const double * __restrict__ td = tmpl + (int64_t)d * P::N;
#pragma unroll
                for (int m = 0; m < P::NM2; ++m) acc[m] += md[m];
#pragma unroll
                for (int m = 0; m < P::N; ++m) acc[P::NM2 + m] += td[m] * v;
            }
        }
    }
    // lanes past the end of a view write a system of zeros: the solve is then done at once
#pragma unroll
    for (int k = 0; k < P::NV; ++k) sys[(int64_t)k * n_sys + idx] = acc[k];
}

template <int W>
__device__ __forceinline__ double p2d_team_max(double x) {
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
        const double o = __shfl_xor(x, off, W);
        x = (o > x) ? o : x;
    }
    return x;
}

template <int W>
__device__ __forceinline__ double p2d_team_sum(double x) {
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, W);
    return x;
}

template <int ORDER>
__global__ __launch_bounds__(kThreads) void k_p2d_solve(const double * __restrict__ sys, int64_t n_sys,
                                                        double * __restrict__ coef, int32_t * __restrict__ status) {
    using P = P2d<ORDER>;
    constexpr int N = P::N, W = P::W;
    const int64_t gid = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t team = gid / W;
    const int r = (int)(gid % W);
    const bool valid = (team < n_sys) && (r < N);
    const int64_t idx = (team < n_sys) ? team : 0;
    const int ir = (r < N) ? r / P::NO : 0, jr = (r < N) ? r % P::NO : 0;
    // every lane of the wave stays until the end: the shuffles below need their partners
    double a[N], v[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const int m = (ir + c / P::NO) * P::NM + (jr + c % P::NO);
        a[c] = valid ? sys[(int64_t)m * n_sys + idx] : 0.0;
        v[c] = (c == r) ? 1.0 : 0.0;
    }
    const double b = valid ? sys[(int64_t)(P::NM2 + r) * n_sys + idx] : 0.0;

    if constexpr (N > 1) {
        bool done = false;
        for (int sweep = 0; sweep < kP2dMaxSweeps; ++sweep) {
            double off = 0.0, diag = 0.0;
#pragma unroll
            for (int c = 0; c < N; ++c) {
                const double x = fabs(a[c]);
                if (c == r) {
                    diag = x;
                } else {
                    off = (x > off) ? x : off;
                }
            }
            off = p2d_team_max<W>(off);
            diag = p2d_team_max<W>(diag);
            done = done || !(off > kP2dOffTol * diag);
            if (__all(done)) break;
#pragma unroll
            for (int p = 0; p < N - 1; ++p) {
#pragma unroll
                for (int q = p + 1; q < N; ++q) {
                    const double app = __shfl(a[p], p, W);
                    const double aqq = __shfl(a[q], q, W);
                    const double apq = __shfl(a[q], p, W);
                    const bool rot = !done && (apq != 0.0);
                    if (!__any(rot)) continue;
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + f_sqrt(theta * theta + 1.0));
                    const double cs = 1.0 / f_sqrt(t * t + 1.0);
                    const double sn = t * cs;
                    // columns p and q of A and V
                    const double ap = a[p], aq = a[q], vp = v[p], vq = v[q];
                    if (rot) {
                        a[p] = cs * ap - sn * aq;
                        a[q] = sn * ap + cs * aq;
                        v[p] = cs * vp - sn * vq;
                        v[q] = sn * vp + cs * vq;
                    }
                    // rows p and q of A
                    const int partner = (r == p) ? q : p;
#pragma unroll
                    for (int c = 0; c < N; ++c) {
                        const double o = __shfl(a[c], partner, W);
                        if (rot && r == p) a[c] = cs * a[c] - sn * o;
                        if (rot && r == q) a[c] = sn * o + cs * a[c];
                    }
                    if (rot && r == p) a[q] = 0.0;
                    if (rot && r == q) a[p] = 0.0;
                }
            }
        }
    }

    double lam = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        if (c == r) lam = a[c];
    }
    const double lmax = p2d_team_max<W>(valid ? lam : 0.0);
    const bool finite = fabs(b) <= 1.7976931348623157e308;
    const bool all_finite = p2d_team_max<W>(finite ? 0.0 : 1.0) == 0.0;
    double w[N];
    int rank = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double y = p2d_team_sum<W>(v[i] * b);
        const double li = __shfl(lam, i, W);
        const bool keep = (lmax > 0.0) && (li > kP2dRcond * lmax);
        w[i] = keep ? y / li : 0.0;
        rank += keep ? 1 : 0;
    }
    double c_r = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) c_r += v[i] * w[i];
    if (!all_finite) c_r = 0.0;
    if (valid) {
        coef[(int64_t)r * n_sys + idx] = c_r;
        if (r == 0) {
            status[idx] = !all_finite ? kP2dNotFinite : ((rank == 0) ? kP2dNoGood : ((rank < N) ? kP2dTruncated : kP2dSolved));
        }
    }
}

template <int ORDER>
__global__ __launch_bounds__(kThreads) void k_p2d_subtract(
    double * __restrict__ signal, int64_t n_samp, const int32_t * __restrict__ sig_index, uint8_t * __restrict__ det_flags,
    const int32_t * __restrict__ flag_index, uint8_t det_mask, const uint8_t * __restrict__ shared_flags,
    uint8_t shared_mask, uint8_t poly_mask, const int32_t * __restrict__ group_start,
    const int32_t * __restrict__ group_dets, const double * __restrict__ tmpl, const P2dJob * __restrict__ jobs, int n_job,
    int tile_begin, int64_t n_slot, int64_t n_sys, const double * __restrict__ coef, const int32_t * __restrict__ status,
    int n_group, double * __restrict__ coeff_out, int32_t * __restrict__ status_out) {
    using P = P2d<ORDER>;
    const int tile = tile_begin + (int)blockIdx.x;
    const P2dJob job = jobs[p2d_job_of_tile(jobs, n_job, tile)];
    const int i = (tile - job.tile0) * kThreads + (int)threadIdx.x;
    if (i >= job.len) return;
    const int g = (int)blockIdx.y;
    const int64_t idx = (int64_t)g * n_slot + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t s = job.first + i;
    double c[P::N];
    bool all_zero = true;
#pragma unroll
    for (int m = 0; m < P::N; ++m) {
        c[m] = coef[(int64_t)m * n_sys + idx];
        all_zero = all_zero && (c[m] == 0.0);
    }
    if (coeff_out != nullptr) {
        double * __restrict__ out = coeff_out + (s * n_group + g) * P::N;
#pragma unroll
        for (int m = 0; m < P::N; ++m) out[m] = c[m];
    }
    if (status_out != nullptr) status_out[s * n_group + g] = status[idx];
    const int k0 = group_start[g], k1 = group_start[g + 1];
    if (all_zero) {
        // nothing to subtract; the sample failed to filter for this group (polyfilter.py:359-364)
        if (det_flags == nullptr) return;
        for (int k = k0; k < k1; ++k) {
            uint8_t * __restrict__ pf = det_flags + (int64_t)flag_index[group_dets[k]] * n_samp + s;
            const uint8_t f = *pf;
            if ((f | poly_mask) != f) *pf = f | poly_mask;
        }
        return;
    }
    // a system with a coefficient that is not zero has a good detector, so the shared flag is clear here
    for (int k = k0; k < k1; ++k) {
        const int d = group_dets[k];
        uint8_t f;
        if (!p2d_good(det_flags, flag_index[d], n_samp, s, det_mask, f)) continue;
        const double * __restrict__ td = tmpl + (int64_t)d * P::N;
        double fit = 0.0;
#pragma unroll
        for (int m = 0; m < P::N; ++m) fit += c[m] * td[m];
        double * __restrict__ ps = signal + (int64_t)sig_index[d] * n_samp + s;
        *ps = *ps - fit;
    }
}

// toast_hip_filter_poly2d_profile: device-event times of the three phases, summed over the calls while it is on
bool g_p2d_profile = false;
double g_p2d_ms[3] = {0.0, 0.0, 0.0};

struct P2dArgs {
    int64_t n_samp, n_det, n_group;
    double * d_signal;
    uint8_t * d_det_flags;
    uint8_t det_mask;
    const uint8_t * d_shared_flags;
    uint8_t shared_mask, poly_mask;
    double * d_coeff;
    int32_t * d_status;
    std::vector<P2dJob> jobs;
    int64_t n_tile;
    const int32_t * sidx;
    const int32_t * fidx;
    const int32_t * gstart;
    const int32_t * gdets;
    const double * tmpl;
    const double * mom;
    const P2dJob * d_jobs;
    hipStream_t st;
};

// bytes of scratch per sample tile: for every slot and group the packed system, the coefficients, and the status (half a
// double)
template <int ORDER>
size_t p2d_tile_bytes(int64_t n_group) {
    using P = P2d<ORDER>;
    return (size_t)kThreads * (size_t)n_group * (sizeof(double) * (P::NV + P::N) + sizeof(int32_t));
}

// sample tiles per batch, before clipping to the tiles of the call: what keeps the scratch below kP2dScratchBytes
template <int ORDER>
int64_t p2d_batch_tiles(int64_t n_group) {
    const int64_t batch = (int64_t)(kP2dScratchBytes / p2d_tile_bytes<ORDER>(n_group));
    return (batch < 1) ? 1 : batch;
}

template <int ORDER>
void p2d_launch(const P2dArgs & a) {
    using P = P2d<ORDER>;
    const size_t per_tile = p2d_tile_bytes<ORDER>(a.n_group);
    int64_t batch = p2d_batch_tiles<ORDER>(a.n_group);
    if (batch > a.n_tile) batch = a.n_tile;
    const int64_t n_slot_max = batch * kThreads;
    char * scratch = static_cast<char *>(Manager::get().scratch(Manager::kScratchPoly, per_tile * (size_t)batch, a.st));
    for (int64_t t0 = 0; t0 < a.n_tile; t0 += batch) {
        const int64_t nt = std::min(batch, a.n_tile - t0);
        const int64_t n_slot = nt * kThreads;
        const int64_t n_sys = n_slot * a.n_group;
        double * sys = reinterpret_cast<double *>(scratch);
        double * coef = sys + (size_t)P::NV * (size_t)(n_slot_max * a.n_group);
        int32_t * status = reinterpret_cast<int32_t *>(coef + (size_t)P::N * (size_t)(n_slot_max * a.n_group));
        const dim3 grid((unsigned)nt, (unsigned)a.n_group);
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (g_p2d_profile) {
            for (auto & e : ev) TH_HIP(hipEventCreate(&e));
            TH_HIP(hipEventRecord(ev[0], a.st));
        }
        hipLaunchKernelGGL(k_p2d_moments<ORDER>, grid, dim3(kThreads), 0, a.st, (const double *)a.d_signal, a.n_samp, a.sidx,
                           (const uint8_t *)a.d_det_flags, a.fidx, a.det_mask, a.d_shared_flags, a.shared_mask, a.gstart,
                           a.gdets, a.tmpl, a.mom, a.d_jobs, (int)a.jobs.size(), (int)t0, n_slot, n_sys, sys);
        check_launch();
        if (g_p2d_profile) TH_HIP(hipEventRecord(ev[1], a.st));
        const int64_t n_thread = n_sys * P::W;
        hipLaunchKernelGGL(k_p2d_solve<ORDER>, dim3((unsigned)((n_thread + kThreads - 1) / kThreads)), dim3(kThreads), 0, a.st,
                           (const double *)sys, n_sys, coef, status);
        check_launch();
        if (g_p2d_profile) TH_HIP(hipEventRecord(ev[2], a.st));
        hipLaunchKernelGGL(k_p2d_subtract<ORDER>, grid, dim3(kThreads), 0, a.st, a.d_signal, a.n_samp, a.sidx, a.d_det_flags,
                           a.fidx, a.det_mask, a.d_shared_flags, a.shared_mask, a.poly_mask, a.gstart, a.gdets, a.tmpl,
                           a.d_jobs, (int)a.jobs.size(), (int)t0, n_slot, n_sys, (const double *)coef,
                           (const int32_t *)status, (int)a.n_group, a.d_coeff, a.d_status);
        check_launch();
        if (g_p2d_profile) {
            TH_HIP(hipEventRecord(ev[3], a.st));
            TH_HIP(hipEventSynchronize(ev[3]));
            for (int k = 0; k < 3; ++k) {
                float ms = 0.0f;
                TH_HIP(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
                g_p2d_ms[k] += (double)ms;
            }
            for (auto & e : ev) TH_HIP(hipEventDestroy(e));
        }
    }
}

}  // namespace

extern "C" {

int toast_hip_filter_poly2d_max_order(void) { return kP2dMaxOrder; }

int64_t toast_hip_filter_poly2d_batch_tiles(int64_t order, int64_t n_group) {
    if (order < 0 || order > kP2dMaxOrder || n_group < 1 || n_group > 65535) return 0;
    switch (order) {
        case 0: return p2d_batch_tiles<0>(n_group);
        case 1: return p2d_batch_tiles<1>(n_group);
        case 2: return p2d_batch_tiles<2>(n_group);
        default: return p2d_batch_tiles<3>(n_group);
    }
}

int toast_hip_filter_poly2d_profile(int on, double * ms_out) {
    return guarded([&] {
        if (ms_out != nullptr) {
            for (int k = 0; k < 3; ++k) ms_out[k] = g_p2d_ms[k];
        }
        for (double & v : g_p2d_ms) v = 0.0;
        g_p2d_profile = on != 0;
    });
}

int toast_hip_filter_poly2d_dev(int64_t order, int64_t n_samp, const int32_t * signal_index, double * d_signal,
                                const int32_t * flag_index, uint8_t * d_det_flags, uint8_t det_flag_mask,
                                const uint8_t * d_shared_flags, uint8_t shared_flag_mask, uint8_t poly_flag_mask,
                                const int32_t * det_group, int64_t n_group, const double * templates, int64_t n_det,
                                const int64_t * starts, const int64_t * stops, int64_t n_interval, double * d_coeff,
                                int32_t * d_status, int path, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_interval <= 0 || n_samp <= 0) return;
        if (order < 0 || order > kP2dMaxOrder) {
            fail_arg("filter_poly2d: order " + std::to_string(order) + "; 0 to " + std::to_string(kP2dMaxOrder) +
                     " are supported on the device");
        }
        if (path < 0 || path > 1) fail_arg("filter_poly2d: path must be 0 (by the rule) or 1 (three kernels)");
        if (n_group < 1 || n_group > 65535) fail_arg("filter_poly2d: 1 to 65535 detector groups");
        if (n_det >= (int64_t(1) << 24)) fail_arg("filter_poly2d: too many detectors");
        if (d_signal == nullptr || signal_index == nullptr || det_group == nullptr || templates == nullptr) {
            fail_arg("filter_poly2d: null buffer");
        }
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("filter_poly2d: detector flags need their row indices");
        const int no = (int)order + 1, n_mode = no * no, nm = 2 * (int)order + 1;
        P2dArgs a;
        a.n_samp = n_samp, a.n_det = n_det, a.n_group = n_group, a.d_signal = d_signal, a.d_det_flags = d_det_flags;
        a.det_mask = det_flag_mask, a.d_shared_flags = d_shared_flags, a.shared_mask = shared_flag_mask;
        a.poly_mask = poly_flag_mask, a.d_coeff = d_coeff, a.d_status = d_status, a.st = as_stream(stream);
        a.n_tile = 0;
        for (int64_t v = 0; v < n_interval; ++v) {
            const int64_t first = starts[v] < 0 ? 0 : starts[v];
            const int64_t last = stops[v] > n_samp ? n_samp : stops[v];
            const int64_t len = last - first;
            if (len <= 0) continue;
            if (len >= (int64_t(1) << 31) - kThreads) fail_arg("filter_poly2d: a view of 2^31 samples or more");
            a.jobs.push_back(P2dJob{first, (int32_t)len, (int32_t)a.n_tile});
            a.n_tile += (len + kThreads - 1) / kThreads;
            if (a.n_tile >= (int64_t(1) << 31) - 1) fail_arg("filter_poly2d: too many sample tiles");
        }
        if (a.jobs.empty()) return;
        // the detectors of every group, in list order
        std::vector<int32_t> gstart((size_t)n_group + 1, 0), gdets((size_t)n_det);
        for (int64_t d = 0; d < n_det; ++d) {
            if (det_group[d] < 0 || det_group[d] >= n_group) fail_arg("filter_poly2d: detector group out of range");
            ++gstart[(size_t)det_group[d] + 1];
        }
        for (int64_t g = 0; g < n_group; ++g) gstart[(size_t)g + 1] += gstart[(size_t)g];
        {
            std::vector<int32_t> fill(gstart.begin(), gstart.end() - 1);
            for (int64_t d = 0; d < n_det; ++d) gdets[(size_t)fill[(size_t)det_group[d]]++] = (int32_t)d;
        }
        // The moments stand for the Gram matrix only when T[d][(i, j)] = theta^i phi^j: checked, not assumed.
        std::vector<double> mom((size_t)(n_det * nm * nm));
        for (int64_t d = 0; d < n_det; ++d) {
            const double * t = templates + d * n_mode;
            const double theta = (order > 0) ? t[no] : 0.0, phi = (order > 0) ? t[1] : 0.0;
            for (int i = 0; i < no; ++i) {
                for (int j = 0; j < no; ++j) {
                    const double want = std::pow(theta, i) * std::pow(phi, j);
                    if (!(std::fabs(t[i * no + j] - want) <= 1e-12 * std::max(1.0, std::fabs(want)))) {
                        fail_arg("filter_poly2d: templates[d][i * (order + 1) + j] must be theta_d^i * phi_d^j");
                    }
                }
            }
            for (int p = 0; p < nm; ++p) {
                for (int q = 0; q < nm; ++q) {
                    const int i1 = std::min(p, (int)order), j1 = std::min(q, (int)order);
                    mom[(size_t)((d * nm + p) * nm + q)] = t[i1 * no + j1] * t[(p - i1) * no + (q - j1)];
                }
            }
        }
        ParamBlock pb;
        const size_t o_si = pb.push(signal_index, sizeof(int32_t) * n_det);
        std::vector<int32_t> no_flags((size_t)n_det, 0);
        const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : no_flags.data(), sizeof(int32_t) * n_det);
        const size_t o_gs = pb.push_vec(gstart);
        const size_t o_gd = pb.push_vec(gdets);
        const size_t o_j = pb.push_vec(a.jobs);
        const size_t o_t = pb.push(templates, sizeof(double) * (size_t)(n_det * n_mode));
        const size_t o_m = pb.push_vec(mom);
        const char * dp = pb.commit(a.st);
        a.sidx = (const int32_t *)(dp + o_si), a.fidx = (const int32_t *)(dp + o_fi);
        a.gstart = (const int32_t *)(dp + o_gs), a.gdets = (const int32_t *)(dp + o_gd);
        a.d_jobs = (const P2dJob *)(dp + o_j), a.tmpl = (const double *)(dp + o_t), a.mom = (const double *)(dp + o_m);
        switch (order) {
            case 0: p2d_launch<0>(a); break;
            case 1: p2d_launch<1>(a); break;
            case 2: p2d_launch<2>(a); break;
            default: p2d_launch<3>(a); break;
        }
    });
}

}  // extern "C"
