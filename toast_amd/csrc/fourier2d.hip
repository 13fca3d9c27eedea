// fourier2d.hip -- the kernels behind toast.templates.Fourier2D on the device.
//
// Reference: src/toast/templates/fourier2d.py:395-459, NumPy and SciPy, one detector at a time.  The template holds
// nmode amplitudes per SAMPLE of every view, shared by all detectors: a[s][m], and a tiny table T[d][m] of the
// focal-plane modes at each detector.  The sweeps contract over the detector axis of the timestream.
//
//   k_f2d_add       signal[d][s] += sum_m a[s][m] T[d][m] (fourier2d.py:395-414).  One lane per sample: the nmode
//                   amplitudes of the sample stay in registers while the lane walks down the detectors of its group;
//                   T[d][.] is wave-uniform; reads and writes along the sample axis are coalesced: 16 B per
//                   detector-sample, the amplitudes once per sample tile.  The sum over the modes is taken in the order
//                   of NumPy's reduction of a contiguous axis (its unrolled pairwise sum).
//   k_f2d_project   a[s][m] += signal[d][s] T[d][m], detector after detector, NO flags (fourier2d.py:416-435): the lane
//                   starts from the amplitude that is there and adds one rounded product per detector, which is the
//                   reference's own sequence: bit-identical.  8 B per detector-sample.
//                   When the sample tiles alone cannot fill the device the detectors are split over grid.y: every group
//                   writes its partial sums (started from 0) and k_f2d_combine adds them onto the amplitudes in group
//                   order.  No atomics anywhere: order-deterministic.
//   k_f2d_norms     norms[s][m] = 1 / sum_d good[d][s] (T[d][m]^2 w_d), 0 where the sum is 0 (fourier2d.py:342-365);
//                   the table (T * T) * w comes from the host; 1 B per detector-sample; never split: bit-identical.
//   k_f2d_precond   out = in * norms (fourier2d.py:457-459)
//
// Prior (fourier2d.py:437-455: scipy.signal.convolve(in[:, m], invcorr * scale_m, "same") per view and mode) as a
// circular convolution of length n_fft >= L + F - 1:
//   k_f2d_gather    the mode series (stride nmode) -> zero-padded rows [nmode][n_fft], transposed through LDS
//   toast_hip_fft_r1d_dev forward, k_f2d_spectrum (times the half-complex spectrum of invcorr and scale_m),
//   toast_hip_fft_r1d_dev backward
//   k_f2d_window    out[s][m] += row_m[s + (F - 1) / 2], transposed back through LDS

#include <algorithm>

#include "kernel_common.hpp"

extern "C" int toast_hip_fft_r1d_dev(int forward, int64_t length, int64_t count, const double * d_in, double * d_out,
                                     double scale, void * stream);

namespace {

// Most modes per sample: the accumulators of a lane (2 VGPRs each) plus one row of products leave four waves per SIMD.
// Orders 1 to 3 have 5 / 7, 17 / 19 and 37 / 39 modes; order 4 (65 / 67) runs on the host.
constexpr int kF2dMaxModes = 40;
constexpr int kF2dTile = 64;             // samples per LDS tile of the prior's two transposes
constexpr int kF2dFillBlocks = 1024;     // workgroups wanted before the detectors stay in one group (4 per CU)
// The rule makes at most ceil(n_det / 4) groups: about 4 detectors or more per group, below that the amplitudes dominate the
// traffic.  Not a floor: 5 detectors become groups of 3 and 2, 9 become three groups of 3.
constexpr int kF2dMinGroupDets = 4;

struct F2dJob {
    int64_t first;   // first sample of the view, clipped to [0, n_samp)
    int64_t amp;     // index of a[first][0] in the amplitude vector
    int64_t cum;     // samples of the views before this one
    int32_t len;
    int32_t tile0;   // first workgroup of this view
};

// the view of a workgroup: the last job with tile0 <= tile
__device__ __forceinline__ int f2d_job_of_tile(const F2dJob * __restrict__ jobs, int n_job, int tile) {
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

// the view of a sample counted through all views: the last job with cum <= s
__device__ __forceinline__ int f2d_job_of_sample(const F2dJob * __restrict__ jobs, int n_job, int64_t s) {
    int lo = 0, hi = n_job - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].cum <= s) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

// np.sum(a * t, 1) of fourier2d.py:410-414 for one row, in the order of NumPy's pairwise sum over a contiguous axis of
// N <= 128 elements: below 8 elements one after the other, otherwise eight running sums over blocks of 8, combined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail.
template <int N>
__device__ __forceinline__ double f2d_row_sum(const double (&a)[N], const double * __restrict__ t) {
    double p[N];
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = a[k] * t[k];
    double res;
    if constexpr (N < 8) {
        res = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) res += p[k];
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = p[j];
        constexpr int full = N - (N % 8);
#pragma unroll
        for (int i = 8; i < full; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += p[i + j];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = full; i < N; ++i) res += p[i];
    }
    return res;
}

template <int N>
__global__ __launch_bounds__(kThreads) void k_f2d_add(double * __restrict__ signal, int64_t n_samp,
                                                      const int32_t * __restrict__ sig_index,
                                                      const double * __restrict__ tmpl, int n_det, int det_per_group,
                                                      const double * __restrict__ amps,
                                                      const F2dJob * __restrict__ jobs, int n_job) {
    const F2dJob job = jobs[f2d_job_of_tile(jobs, n_job, blockIdx.x)];
    const int i = ((int)blockIdx.x - job.tile0) * kThreads + (int)threadIdx.x;
    if (i >= job.len) return;
    const double * __restrict__ arow = amps + job.amp + (int64_t)i * N;
    double a[N];
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = arow[k];
    const int d0 = (int)blockIdx.y * det_per_group;
    const int d1 = (d0 + det_per_group < n_det) ? d0 + det_per_group : n_det;
    for (int d = d0; d < d1; ++d) {
        double * __restrict__ p = signal + (int64_t)sig_index[d] * n_samp + job.first + i;
        *p = *p + f2d_row_sum<N>(a, tmpl + (int64_t)d * N);
    }
}

// PARTIAL = false: the whole sum of a sample in one lane, on top of the amplitude that is there
// PARTIAL = true:  group blockIdx.y writes its sums, started from 0, to partial[group][sample through all views][N]
template <int N, bool PARTIAL>
__global__ __launch_bounds__(kThreads) void k_f2d_project(const double * __restrict__ signal, int64_t n_samp,
                                                          const int32_t * __restrict__ sig_index,
                                                          const double * __restrict__ tmpl, int n_det, int det_per_group,
                                                          double * __restrict__ amps, double * __restrict__ partial,
                                                          int64_t n_total, const F2dJob * __restrict__ jobs, int n_job) {
    const F2dJob job = jobs[f2d_job_of_tile(jobs, n_job, blockIdx.x)];
    const int i = ((int)blockIdx.x - job.tile0) * kThreads + (int)threadIdx.x;
    if (i >= job.len) return;
    double * __restrict__ arow = PARTIAL ? partial + ((int64_t)blockIdx.y * n_total + job.cum + i) * N
                                         : amps + job.amp + (int64_t)i * N;
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = PARTIAL ? 0.0 : arow[k];
    const int d0 = (int)blockIdx.y * det_per_group;
    const int d1 = (d0 + det_per_group < n_det) ? d0 + det_per_group : n_det;
    for (int d = d0; d < d1; ++d) {
        const double s = signal[(int64_t)sig_index[d] * n_samp + job.first + i];
        const double * __restrict__ t = tmpl + (int64_t)d * N;
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += s * t[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) arow[k] = acc[k];
}

// one thread per amplitude of the observation: the partial sums of the groups, in group order, onto the amplitude
__global__ __launch_bounds__(kThreads) void k_f2d_combine(int n, int64_t n_total, int n_group,
                                                          const double * __restrict__ partial,
                                                          double * __restrict__ amps, const F2dJob * __restrict__ jobs,
                                                          int n_job) {
    const int64_t n_elem = n_total * n;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n_elem; e += (int64_t)gridDim.x * kThreads) {
        const int64_t s = e / n;
        const int k = (int)(e - s * n);
        const F2dJob job = jobs[f2d_job_of_sample(jobs, n_job, s)];
        double * __restrict__ a = amps + job.amp + (s - job.cum) * n + k;
        double t = *a;
        for (int g = 0; g < n_group; ++g) t += partial[(int64_t)g * n_elem + e];
        *a = t;
    }
}

// fourier2d.py:342-346 and :363-365; tw[d][m] = (T[d][m] * T[d][m]) * w_d
template <int N>
__global__ __launch_bounds__(kThreads) void k_f2d_norms(const uint8_t * __restrict__ det_flags, int64_t n_samp,
                                                        const int32_t * __restrict__ flag_index, uint8_t det_mask,
                                                        const double * __restrict__ tw, int n_det,
                                                        double * __restrict__ norms, const F2dJob * __restrict__ jobs,
                                                        int n_job) {
    const F2dJob job = jobs[f2d_job_of_tile(jobs, n_job, blockIdx.x)];
    const int i = ((int)blockIdx.x - job.tile0) * kThreads + (int)threadIdx.x;
    if (i >= job.len) return;
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (int d = 0; d < n_det; ++d) {
        if (det_flags != nullptr && (det_flags[(int64_t)flag_index[d] * n_samp + job.first + i] & det_mask) != 0) continue;
        const double * __restrict__ t = tw + (int64_t)d * N;
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += t[k];
    }
    double * __restrict__ out = norms + job.amp + (int64_t)i * N;
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = (acc[k] != 0.0) ? 1.0 / acc[k] : acc[k];
}

__global__ __launch_bounds__(kThreads) void k_f2d_precond(int64_t n_amp, const double * __restrict__ norms,
                                                          const double * __restrict__ amp_in, double * __restrict__ amp_out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_amp; i += (int64_t)gridDim.x * kThreads) {
        amp_out[i] = amp_in[i] * norms[i];
    }
}

// ------------------------------------------------------------------------------------ prior
// rows[m][i] = in[i][m] for i < len, 0 up to n_fft.  A workgroup moves kF2dTile samples: it reads their kF2dTile * n
// consecutive amplitudes, and every wave then writes whole rows of the tile (lds stride n: odd, no bank conflicts).
__global__ __launch_bounds__(kThreads) void k_f2d_gather(const double * __restrict__ in, int n, int64_t len, int64_t n_fft,
                                                         double * __restrict__ rows) {
    __shared__ double tile[kF2dTile * kF2dMaxModes];
    const int64_t i0 = (int64_t)blockIdx.x * kF2dTile;
    const int cnt = (i0 >= len) ? 0 : (int)((len - i0 < kF2dTile) ? len - i0 : kF2dTile);
    for (int e = threadIdx.x; e < cnt * n; e += kThreads) tile[e] = in[i0 * n + e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (i0 + lane >= n_fft) return;
    for (int m = wave; m < n; m += kThreads / 64) {
        rows[(int64_t)m * n_fft + i0 + lane] = (lane < cnt) ? tile[lane * n + m] : 0.0;
    }
}

// FFTW half-complex rows: r_0 .. r_{N/2}, i_{N/2-1} .. i_1.  row_m *= spectrum * scale[m]
__global__ __launch_bounds__(kThreads) void k_f2d_spectrum(double * __restrict__ rows, int64_t n_fft,
                                                           const double * __restrict__ spec,
                                                           const double * __restrict__ scale) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t half = n_fft / 2;
    if (k > half) return;
    double * __restrict__ row = rows + (int64_t)blockIdx.y * n_fft;
    const double sc = scale[blockIdx.y];
    if (k == 0 || 2 * k == n_fft) {
        row[k] = (row[k] * spec[k]) * sc;
    } else {
        const double re = row[k], im = row[n_fft - k];
        const double sr = spec[k], si = spec[n_fft - k];
        row[k] = (re * sr - im * si) * sc;
        row[n_fft - k] = (re * si + im * sr) * sc;
    }
}

// out[i][m] += rows[m][i + shift] for i < len (scipy's "same" window of the full convolution)
__global__ __launch_bounds__(kThreads) void k_f2d_window(const double * __restrict__ rows, int n, int64_t len, int64_t n_fft,
                                                         int64_t shift, double * __restrict__ out) {
    __shared__ double tile[kF2dTile * kF2dMaxModes];
    const int64_t i0 = (int64_t)blockIdx.x * kF2dTile;
    const int cnt = (i0 >= len) ? 0 : (int)((len - i0 < kF2dTile) ? len - i0 : kF2dTile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < cnt) {
        for (int m = wave; m < n; m += kThreads / 64) tile[lane * n + m] = rows[(int64_t)m * n_fft + i0 + lane + shift];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * n; e += kThreads) out[i0 * n + e] += tile[e];
}

// ------------------------------------------------------------------------------------ host side
struct F2dPlan {
    std::vector<F2dJob> jobs;
    int64_t n_tile = 0;
    int64_t n_total = 0;
};

// views clipped to [0, n_samp); a clipped start moves the first amplitude row along with it
F2dPlan f2d_plan(const toast_hip_interval * ivl, const int64_t * view_amp, int64_t n_view, int64_t n_samp, int64_t nmode,
                 const char * what) {
    F2dPlan p;
    for (int64_t v = 0; v < n_view; ++v) {
        const int64_t first = ivl[v].first < 0 ? 0 : ivl[v].first;
        const int64_t last = ivl[v].last > n_samp ? n_samp : ivl[v].last;
        const int64_t len = last - first;
        if (len <= 0) continue;
        if (len >= (int64_t(1) << 31) - kThreads) fail_arg(std::string(what) + ": a view of 2^31 samples or more");
        if (view_amp[v] < 0) fail_arg(std::string(what) + ": negative amplitude offset");
        p.jobs.push_back(F2dJob{first, view_amp[v] + (first - ivl[v].first) * nmode, p.n_total, (int32_t)len, (int32_t)p.n_tile});
        p.n_tile += (len + kThreads - 1) / kThreads;
        p.n_total += len;
        if (p.n_tile >= (int64_t(1) << 31) - 1) fail_arg(std::string(what) + ": too many sample tiles");
    }
    return p;
}

void f2d_check(int64_t nmode, const char * what) {
    switch (nmode) {
        case 5: case 7: case 17: case 19: case 37: case 39: return;
        default:
            fail_arg(std::string(what) + ": " + std::to_string(nmode) + " modes; (2 order)^2 + 1 (+ 2 with subharmonics) for "
                     "order 1 to 3 are supported: 5, 7, 17, 19, 37, 39");
    }
}

#define F2D_DISPATCH(nmode, CALL) \
    switch (nmode) {              \
        case 5: CALL(5); break;   \
        case 7: CALL(7); break;   \
        case 17: CALL(17); break; \
        case 19: CALL(19); break; \
        case 37: CALL(37); break; \
        default: CALL(39); break; \
    }

// how many detectors one group takes: all of them when the sample tiles fill the device (or n_group == 1 is asked for)
int64_t f2d_det_per_group(int64_t n_det, int64_t n_tile, int64_t n_group) {
    if (n_group <= 0) {
        n_group = (kF2dFillBlocks + n_tile - 1) / n_tile;
        const int64_t most = (n_det + kF2dMinGroupDets - 1) / kF2dMinGroupDets;
        if (n_group > most) n_group = most;
    }
    if (n_group > n_det) n_group = n_det;
    if (n_group > 65535) n_group = 65535;
    if (n_group < 1) n_group = 1;
    return (n_det + n_group - 1) / n_group;
}

}  // namespace

extern "C" {

int toast_hip_fourier2d_max_modes(void) { return kF2dMaxModes; }

int64_t toast_hip_fourier2d_groups(int64_t n_det, int64_t n_tile, int64_t n_group) {
    if (n_det < 1 || n_tile < 1) return 0;
    const int64_t dpg = f2d_det_per_group(n_det, n_tile, n_group);
    return (n_det + dpg - 1) / dpg;
}

int toast_hip_fourier2d_add_to_signal_dev(int64_t nmode, const double * d_templates, const int64_t * view_amp_offsets,
                                          const double * d_amplitudes, const int32_t * data_index, int64_t n_det,
                                          double * d_det_data, int64_t n_samp, const toast_hip_interval * intervals,
                                          int64_t n_view, int64_t n_group, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        f2d_check(nmode, "fourier2d_add_to_signal");
        if (n_det >= (int64_t(1) << 31)) fail_arg("fourier2d_add_to_signal: too many detectors");
        if (d_templates == nullptr || d_amplitudes == nullptr || d_det_data == nullptr) fail_arg("fourier2d_add_to_signal: null buffer");
        hipStream_t st = as_stream(stream);
        const F2dPlan plan = f2d_plan(intervals, view_amp_offsets, n_view, n_samp, nmode, "fourier2d_add_to_signal");
        if (plan.jobs.empty()) return;
        const int64_t dpg = f2d_det_per_group(n_det, plan.n_tile, n_group);
        const int64_t groups = (n_det + dpg - 1) / dpg;
        ParamBlock pb;
        const size_t o_si = pb.push(data_index, sizeof(int32_t) * n_det);
        const size_t o_j = pb.push_vec(plan.jobs);
        const char * dp = pb.commit(st);
#define CALL(NN)                                                                                                            \
    hipLaunchKernelGGL(k_f2d_add<NN>, dim3((unsigned)plan.n_tile, (unsigned)groups), dim3(kThreads), 0, st, d_det_data,      \
                       n_samp, (const int32_t *)(dp + o_si), d_templates, (int)n_det, (int)dpg, d_amplitudes,                 \
                       (const F2dJob *)(dp + o_j), (int)plan.jobs.size())
        F2D_DISPATCH(nmode, CALL);
#undef CALL
        check_launch();
    });
}

int toast_hip_fourier2d_project_signal_dev(int64_t nmode, const double * d_templates, const int64_t * view_amp_offsets,
                                           double * d_amplitudes, const int32_t * data_index, int64_t n_det,
                                           const double * d_det_data, int64_t n_samp, const toast_hip_interval * intervals,
                                           int64_t n_view, int64_t n_group, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        f2d_check(nmode, "fourier2d_project_signal");
        if (n_det >= (int64_t(1) << 31)) fail_arg("fourier2d_project_signal: too many detectors");
        if (d_templates == nullptr || d_amplitudes == nullptr || d_det_data == nullptr) fail_arg("fourier2d_project_signal: null buffer");
        hipStream_t st = as_stream(stream);
        const F2dPlan plan = f2d_plan(intervals, view_amp_offsets, n_view, n_samp, nmode, "fourier2d_project_signal");
        if (plan.jobs.empty()) return;
        const int64_t dpg = f2d_det_per_group(n_det, plan.n_tile, n_group);
        const int64_t groups = (n_det + dpg - 1) / dpg;
        ParamBlock pb;
        const size_t o_si = pb.push(data_index, sizeof(int32_t) * n_det);
        const size_t o_j = pb.push_vec(plan.jobs);
        const char * dp = pb.commit(st);
        const dim3 grid((unsigned)plan.n_tile, (unsigned)groups);
        if (groups == 1) {
#define CALL(NN)                                                                                                            \
    hipLaunchKernelGGL((k_f2d_project<NN, false>), grid, dim3(kThreads), 0, st, d_det_data, n_samp,                          \
                       (const int32_t *)(dp + o_si), d_templates, (int)n_det, (int)dpg, d_amplitudes, (double *)nullptr,      \
                       plan.n_total, (const F2dJob *)(dp + o_j), (int)plan.jobs.size())
            F2D_DISPATCH(nmode, CALL);
#undef CALL
            check_launch();
            return;
        }
        double * partial = static_cast<double *>(Manager::get().scratch(
            Manager::kScratchTemplate, sizeof(double) * (size_t)(groups * plan.n_total * nmode), st));
#define CALL(NN)                                                                                                            \
    hipLaunchKernelGGL((k_f2d_project<NN, true>), grid, dim3(kThreads), 0, st, d_det_data, n_samp,                           \
                       (const int32_t *)(dp + o_si), d_templates, (int)n_det, (int)dpg, d_amplitudes, partial, plan.n_total,  \
                       (const F2dJob *)(dp + o_j), (int)plan.jobs.size())
        F2D_DISPATCH(nmode, CALL);
#undef CALL
        check_launch();
        hipLaunchKernelGGL(k_f2d_combine, flat_grid(plan.n_total * nmode), dim3(kThreads), 0, st, (int)nmode, plan.n_total,
                           (int)groups, (const double *)partial, d_amplitudes, (const F2dJob *)(dp + o_j),
                           (int)plan.jobs.size());
        check_launch();
    });
}

int toast_hip_fourier2d_norms_dev(int64_t nmode, const double * d_weighted_squares, const int64_t * view_amp_offsets,
                                  const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                  int64_t n_det, int64_t n_samp, const toast_hip_interval * intervals, int64_t n_view,
                                  double * d_norms, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        f2d_check(nmode, "fourier2d_norms");
        if (n_det >= (int64_t(1) << 31)) fail_arg("fourier2d_norms: too many detectors");
        if (d_weighted_squares == nullptr || d_norms == nullptr) fail_arg("fourier2d_norms: null buffer");
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("fourier2d_norms: detector flags need their row indices");
        hipStream_t st = as_stream(stream);
        const F2dPlan plan = f2d_plan(intervals, view_amp_offsets, n_view, n_samp, nmode, "fourier2d_norms");
        if (plan.jobs.empty()) return;
        ParamBlock pb;
        std::vector<int32_t> no_flags(n_det, 0);
        const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : no_flags.data(), sizeof(int32_t) * n_det);
        const size_t o_j = pb.push_vec(plan.jobs);
        const char * dp = pb.commit(st);
#define CALL(NN)                                                                                                            \
    hipLaunchKernelGGL(k_f2d_norms<NN>, dim3((unsigned)plan.n_tile), dim3(kThreads), 0, st, d_det_flags, n_samp,             \
                       (const int32_t *)(dp + o_fi), det_flag_mask, d_weighted_squares, (int)n_det, d_norms,                  \
                       (const F2dJob *)(dp + o_j), (int)plan.jobs.size())
        F2D_DISPATCH(nmode, CALL);
#undef CALL
        check_launch();
    });
}

int toast_hip_fourier2d_apply_precond_dev(int64_t n_amp, const double * d_norms, const double * d_amp_in, double * d_amp_out,
                                          void * stream) {
    return guarded([&] {
        if (n_amp <= 0) return;
        hipLaunchKernelGGL(k_f2d_precond, flat_grid(n_amp), dim3(kThreads), 0, as_stream(stream), n_amp, d_norms, d_amp_in,
                           d_amp_out);
        check_launch();
    });
}

int toast_hip_fourier2d_add_prior_dev(int64_t nmode, int64_t view_len, const double * d_amp_in, double * d_amp_out,
                                      int64_t filter_len, int64_t n_fft, const double * d_spectrum, const double * scale,
                                      double * d_work, void * stream) {
    return guarded([&] {
        if (view_len <= 0) return;
        if (nmode < 1 || nmode > kF2dMaxModes) fail_arg("fourier2d_add_prior: 1 to " + std::to_string(kF2dMaxModes) + " modes are supported");
        if (filter_len < 1 || n_fft < view_len + filter_len - 1 || (n_fft & 1) != 0) {
            fail_arg("fourier2d_add_prior: n_fft must be even and at least view_len + filter_len - 1");
        }
        if (n_fft >= (int64_t(1) << 31)) fail_arg("fourier2d_add_prior: transforms of 2^31 points or more");
        if (d_amp_in == nullptr || d_amp_out == nullptr || d_spectrum == nullptr || scale == nullptr || d_work == nullptr) {
            fail_arg("fourier2d_add_prior: null buffer");
        }
        hipStream_t st = as_stream(stream);
        double * rows = d_work;
        double * freq = d_work + nmode * n_fft;
        ParamBlock pb;
        const size_t o_sc = pb.push(scale, sizeof(double) * nmode);
        const char * dp = pb.commit(st);
        hipLaunchKernelGGL(k_f2d_gather, dim3((unsigned)((n_fft + kF2dTile - 1) / kF2dTile)), dim3(kThreads), 0, st, d_amp_in,
                           (int)nmode, view_len, n_fft, rows);
        check_launch();
        int rc = toast_hip_fft_r1d_dev(1, n_fft, nmode, rows, freq, 1.0, st);
        if (rc != TOAST_HIP_OK) throw Error(rc, toast_hip_last_error());
        hipLaunchKernelGGL(k_f2d_spectrum, dim3((unsigned)((n_fft / 2 + 1 + kThreads - 1) / kThreads), (unsigned)nmode),
                           dim3(kThreads), 0, st, freq, n_fft, d_spectrum, (const double *)(dp + o_sc));
        check_launch();
        rc = toast_hip_fft_r1d_dev(0, n_fft, nmode, freq, rows, 1.0, st);
        if (rc != TOAST_HIP_OK) throw Error(rc, toast_hip_last_error());
        hipLaunchKernelGGL(k_f2d_window, dim3((unsigned)((view_len + kF2dTile - 1) / kF2dTile)), dim3(kThreads), 0, st,
                           (const double *)rows, (int)nmode, view_len, n_fft, (filter_len - 1) / 2, d_amp_out);
        check_launch();
    });
}

}  // extern "C"
