// filterbin.hip -- the joint template regression behind toast.ops.FilterBin on the device.
//
// Reference: src/toast/ops/filterbin.py.  There every detector builds its own copy of the sparse templates
// (`SparseTemplates.mask` :145-168), forms F^T diag(good) F in an O(n_template^2 n_samp) host loop
// (`build_template_covariance`, src/toast/_libtoast/ops_filterbin.cpp:276-382), inverts it and subtracts template by
// template (`fit` :94-97, `subtract` :109-114).
//
// Here the templates of an observation are split into
//   * Nd DENSE ones (HWP harmonics, ground polynomials): a [Nd][n_samp] matrix in HBM, built once per observation
//     (k_fourier_templates here, k_legendre / k_template_select of ground_filter.hip), and
//   * V intervals with K = poly_filter_order + 1 LOCAL Legendre polynomials each, never stored: a lane rebuilds
//     P_0..P_{K-1} at its sample from the recurrence of k_legendre,
// and the normal matrix of a detector is the arrowhead [[A, C], [C^T, diag(B_v)]].  A and the dense right-hand side come
// from toast_hip_template_fit_dev (ground_filter.hip); this file adds
//
//   k_fourier_templates       cos(k angle), sin(k angle) rows (src/toast/_libtoast/tod_filter.cpp:156-165)
//   k_template_spans          first / last non-zero sample of every dense row (`SparseTemplates.trim` :117-125)
//   k_good_counts             good samples per detector and good non-zero samples per (detector, dense row): the
//                             null-template test of `mask` :154 needs exact counts, a difference of sums cannot give them
//   k_flag_spans              OR a mask into stretches of detector-flag rows (filterbin.py:897-899, :945-946, :990)
//   k_interval_common         B_v = P_v^T W P_v (packed upper triangle), C_v = Dn^T W P_v over the shared-good samples
//   k_interval_accumulate     per detector: p_dv = P_v^T W_d s_d and the counts of good non-zero samples from every good
//                             sample; the corrections to B_v, C_v from the samples only that detector flags (the
//                             common-minus-flagged decomposition of k_template_gram_flagged)
//   k_filterbin_subtract      signal[d][i] -= sum_r a[d][r] Dn[r][i] + sum_j b[d][v(i)][j] P_j(x_i), one pass
//
// All of them stream: 9 B (signal + flag) per detector-sample for the accumulation, 16 B for the subtraction; no MFMA
// (K <= 8, Nd is 10-40, the reduction dimension is the long one).

#include <type_traits>

#include "kernel_common.hpp"

namespace {

constexpr int kFbTile = 256;      // samples per sub-tile: one per thread
constexpr int kFbChunk = 1024;    // samples of one interval per workgroup
constexpr int kFbGroup = 16;      // dense rows per launch of k_interval_accumulate / per LDS tile (kTmplGroup)
constexpr int kFbMaxK = 8;        // poly_filter_order <= 7

template <int K>
struct FbShape {
    static constexpr int kPairs = K * (K + 1) / 2;
    static constexpr int kDets = (K <= 4) ? 8 : 4;   // detectors per workgroup: kDets * K accumulators of p per lane
};

// The K normalised Legendre polynomials at x: the recurrence and the rounding of k_legendre (toast_tod_filter.cpp:269-331).
template <int K>
__device__ __forceinline__ void local_legendre(double x, double (&P)[K]) {
    P[0] = 1. / f_sqrt(2.);
    if constexpr (K > 1) P[1] = (1. / f_sqrt(2. / 3.)) * x;
    double val = x, prev = 1.0;
#pragma unroll
    for (int order = 2; order < K; ++order) {
        const double orderinv = 1. / (double)order;
        const double next = ((double)(2 * order - 1) * x * val - (double)(order - 1) * prev) * orderinv;
        prev = val;
        val = next;
        const double norm = 1. / f_sqrt(2. / (2. * (double)order + 1.));
        P[order] = val * norm;
    }
}

// filterbin.py:1395-1396: phase = (arange(L) + 0.5) * (2 / L) - 1
__device__ __forceinline__ double local_phase(int64_t i, int64_t start, double wbin) {
    return ((double)(i - start) + 0.5) * wbin - 1.0;
}

__global__ __launch_bounds__(kThreads) void k_fourier_templates(const double * __restrict__ angle, int64_t n_samp,
                                                                int64_t start_order, int64_t stop_order,
                                                                double * __restrict__ templates) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_samp; i += (int64_t)gridDim.x * kThreads) {
        const double a = angle[i];
        for (int64_t order = start_order; order < stop_order; ++order) {
            const double arg = (double)order * a;
            templates[(2 * (order - start_order)) * n_samp + i] = cos(arg);
            templates[(2 * (order - start_order) + 1) * n_samp + i] = sin(arg);
        }
    }
}

// first[r] = min i, last[r] = max i over templates[r][i] != 0; the caller presets n_samp and -1.
__global__ __launch_bounds__(kThreads) void k_template_spans(const double * __restrict__ templates, int64_t n_samp,
                                                             int64_t slice, long long * __restrict__ first,
                                                             long long * __restrict__ last) {
    const int64_t r = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.x * slice;
    const int64_t i1 = (i0 + slice < n_samp) ? i0 + slice : n_samp;
    const double * __restrict__ row = templates + r * n_samp;
    long long lo = n_samp, hi = -1;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
        if (row[i] != 0.0) {
            if (i < lo) lo = i;
            if (i > hi) hi = i;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long olo = __shfl_xor(lo, off, 64), ohi = __shfl_xor(hi, off, 64);
        lo = (olo < lo) ? olo : lo;
        hi = (ohi > hi) ? ohi : hi;
    }
    if ((threadIdx.x & 63) == 0 && hi >= 0) {
        atomicMin(&first[r], lo);
        atomicMax(&last[r], hi);
    }
}

// n_good[d] = #good samples, nnz[d][r] = #good samples with templates[r][i] != 0.  One wave per (slice, detector).
__global__ __launch_bounds__(kThreads) void k_good_counts(
    const double * __restrict__ templates, int64_t n_template, int64_t n_samp, const int32_t * __restrict__ flag_index,
    const uint8_t * __restrict__ det_flags, uint8_t det_mask, const uint8_t * __restrict__ shared_flags, uint8_t shared_mask,
    int64_t n_det, int64_t slice, unsigned long long * __restrict__ n_good, unsigned long long * __restrict__ nnz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t d = (int64_t)blockIdx.x * 4 + wave;
    if (d >= n_det) return;
    const int64_t i0 = (int64_t)blockIdx.y * slice;
    const int64_t i1 = (i0 + slice < n_samp) ? i0 + slice : n_samp;
    const uint8_t * __restrict__ df = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp : nullptr;
    for (int64_t t0 = 0; t0 == 0 || t0 < n_template; t0 += kFbGroup) {
        const int nt = (n_template - t0 < kFbGroup) ? (int)(n_template - t0) : kFbGroup;
        unsigned int cnt[kFbGroup];
#pragma unroll
        for (int r = 0; r < kFbGroup; ++r) cnt[r] = 0;
        unsigned int good_cnt = 0;
        for (int64_t i = i0 + lane; i < i1; i += 64) {
            const bool good = ((shared_flags == nullptr) || ((shared_flags[i] & shared_mask) == 0)) &&
                              ((df == nullptr) || ((df[i] & det_mask) == 0));
            if (!good) continue;
            ++good_cnt;
#pragma unroll
            for (int r = 0; r < kFbGroup; ++r) {
                if (r < nt && templates[(t0 + r) * n_samp + i] != 0.0) ++cnt[r];
            }
        }
        if (t0 == 0) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) good_cnt += __shfl_xor(good_cnt, off, 64);
            if (lane == 0 && good_cnt != 0) atomicAdd(&n_good[d], (unsigned long long)good_cnt);
        }
#pragma unroll
        for (int r = 0; r < kFbGroup; ++r) {
            if (r >= nt) continue;
            unsigned int v = cnt[r];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0 && v != 0) atomicAdd(&nnz[d * n_template + t0 + r], (unsigned long long)v);
        }
    }
}

struct FlagSpan {
    int64_t first, last;   // [first, last)
    int32_t row, pad;
};

__global__ __launch_bounds__(kThreads) void k_flag_spans(const FlagSpan * __restrict__ spans, int64_t n_samp,
                                                         uint8_t * __restrict__ det_flags, uint8_t mask) {
    const FlagSpan s = spans[blockIdx.x];
    uint8_t * __restrict__ row = det_flags + (int64_t)s.row * n_samp;
    for (int64_t i = s.first + (int64_t)blockIdx.y * kThreads + threadIdx.x; i < s.last; i += (int64_t)gridDim.y * kThreads)
        row[i] |= mask;
}

struct FbChunk {
    int64_t first, last;    // samples [first, last) of this chunk
    int64_t start;          // first sample of the (trimmed) interval
    double wbin;            // 2 / length of the interval
    int32_t interval, pad;
};

// B_v and C_v over the shared-good samples.  One workgroup per chunk; a lane keeps its sums over the chunk's sub-tiles,
// the waves reduce by DPP and add once per (entry, chunk).
template <int K>
__global__ __launch_bounds__(kThreads) void k_interval_common(
    const FbChunk * __restrict__ chunks, const double * __restrict__ dense, int64_t n_dense, int64_t n_samp,
    const uint8_t * __restrict__ shared_flags, uint8_t shared_mask, double * __restrict__ b_common,
    double * __restrict__ c_common) {
    constexpr int KP = FbShape<K>::kPairs;
    const FbChunk ch = chunks[blockIdx.x];
    const int lane = threadIdx.x & 63;
    double bacc[KP];
#pragma unroll
    for (int q = 0; q < KP; ++q) bacc[q] = 0.0;
    for (int64_t i = ch.first + threadIdx.x; i < ch.last; i += kThreads) {
        if (shared_flags != nullptr && (shared_flags[i] & shared_mask) != 0) continue;
        double P[K];
        local_legendre<K>(local_phase(i, ch.start, ch.wbin), P);
        int q = 0;
#pragma unroll
        for (int a = 0; a < K; ++a) {
#pragma unroll
            for (int b = a; b < K; ++b) bacc[q++] += P[a] * P[b];
        }
    }
#pragma unroll
    for (int q = 0; q < KP; ++q) {
        double v = bacc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && v != 0.0) atomicAdd(&b_common[(int64_t)ch.interval * KP + q], v);
    }
    for (int64_t r0 = 0; r0 < n_dense; r0 += 8) {
        const int nr = (n_dense - r0 < 8) ? (int)(n_dense - r0) : 8;
        double cacc[8][K];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
            for (int j = 0; j < K; ++j) cacc[r][j] = 0.0;
        }
        for (int64_t i = ch.first + threadIdx.x; i < ch.last; i += kThreads) {
            if (shared_flags != nullptr && (shared_flags[i] & shared_mask) != 0) continue;
            double P[K];
            local_legendre<K>(local_phase(i, ch.start, ch.wbin), P);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const double t = (r < nr) ? dense[(r0 + r) * n_samp + i] : 0.0;
#pragma unroll
                for (int j = 0; j < K; ++j) cacc[r][j] += t * P[j];
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r >= nr) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double v = cacc[r][j];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
                if (lane == 0 && v != 0.0) atomicAdd(&c_common[((int64_t)ch.interval * n_dense + r0 + r) * K + j], v);
            }
        }
    }
}

// One workgroup per (chunk, tile of kDets detectors, group of kFbGroup dense rows starting at g0).  Per sub-tile of 256
// samples: every lane rebuilds the K polynomials at its sample and leaves them in LDS; it then streams the detectors of
// the tile -- the launch for g0 == 0 reads the signal and adds to its p sums and counts, the others read the flags only
// -- and queues the samples that a detector alone flags.  Where something was queued the dense rows of the group are
// staged in LDS, and the threads, one per (detector, entry of B or C), walk that detector's queue.  The sums stay in
// registers over the sub-tiles of the chunk; the atomics at the end are one per (entry, chunk).
template <int K>
__global__ __launch_bounds__(kThreads) void k_interval_accumulate(
    const FbChunk * __restrict__ chunks, const double * __restrict__ dense, int64_t n_dense, int64_t g0, int64_t n_samp,
    const int32_t * __restrict__ sig_index, const double * __restrict__ signal, const int32_t * __restrict__ flag_index,
    const uint8_t * __restrict__ det_flags, uint8_t det_mask, const uint8_t * __restrict__ shared_flags, uint8_t shared_mask,
    int64_t n_det, int64_t n_interval, double * __restrict__ p_out, unsigned long long * __restrict__ nnz_out,
    double * __restrict__ b_flagged, double * __restrict__ c_flagged) {
    constexpr int KP = FbShape<K>::kPairs;
    constexpr int DT = FbShape<K>::kDets;
    constexpr int kBItems = DT * KP;                          // (detector, pair) entries of B
    constexpr int kCItems = DT * kFbGroup * K;                // (detector, dense row, polynomial) entries of C
    constexpr int kBPer = (kBItems + kThreads - 1) / kThreads;
    constexpr int kCPer = (kCItems + kThreads - 1) / kThreads;
    __shared__ double poly[K * kFbTile];
    __shared__ double tile[kFbGroup * kFbTile];
    __shared__ uint8_t queue[DT * kFbTile];
    __shared__ int n_queued[DT];
    const FbChunk ch = chunks[blockIdx.x];
    const int64_t d0 = (int64_t)blockIdx.y * DT;
    const bool first_group = (g0 == 0);
    const int nt = (n_dense - g0 < kFbGroup) ? (int)(n_dense - g0) : kFbGroup;    // may be <= 0 when n_dense == 0
    const int lane = threadIdx.x & 63;
    double pacc[DT][K];
    unsigned int ncnt[DT][K];
#pragma unroll
    for (int dd = 0; dd < DT; ++dd) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            pacc[dd][j] = 0.0;
            ncnt[dd][j] = 0;
        }
    }
    double bsum[kBPer], csum[kCPer];
#pragma unroll
    for (int q = 0; q < kBPer; ++q) bsum[q] = 0.0;
#pragma unroll
    for (int q = 0; q < kCPer; ++q) csum[q] = 0.0;
    for (int64_t base = ch.first; base < ch.last; base += kFbTile) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < ch.last;
        if (threadIdx.x < DT) n_queued[threadIdx.x] = 0;
        double P[K];
        local_legendre<K>(local_phase(valid ? i : ch.first, ch.start, ch.wbin), P);
#pragma unroll
        for (int j = 0; j < K; ++j) poly[j * kFbTile + threadIdx.x] = valid ? P[j] : 0.0;
        __syncthreads();
        const bool cgood = valid && ((shared_flags == nullptr) || ((shared_flags[i] & shared_mask) == 0));
#pragma unroll
        for (int dd = 0; dd < DT; ++dd) {
            const int64_t d = d0 + dd;
            if (d >= n_det) continue;                                    // uniform
            const bool dbad = (det_flags != nullptr) && cgood &&
                              ((det_flags[(int64_t)flag_index[d] * n_samp + i] & det_mask) != 0);
            if (cgood && dbad) queue[dd * kFbTile + atomicAdd(&n_queued[dd], 1)] = (uint8_t)threadIdx.x;
            if (first_group && cgood && !dbad) {
                const double sv = signal[(int64_t)sig_index[d] * n_samp + i];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    pacc[dd][j] += sv * P[j];
                    if (P[j] != 0.0) ++ncnt[dd][j];
                }
            }
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int dd = 0; dd < DT; ++dd) total += n_queued[dd];
        if (total > 0) {                                                 // uniform
            if (first_group) {
#pragma unroll
                for (int q = 0; q < kBPer; ++q) {
                    const int item = q * kThreads + threadIdx.x;
                    if (item >= kBItems) continue;
                    const int dd = item / KP, pair = item - dd * KP;
                    int a = 0, rem = pair;
                    while (rem >= K - a) {
                        rem -= K - a;
                        ++a;
                    }
                    const int b = a + rem;
                    const int nq = n_queued[dd];
                    double acc = 0.0;
                    for (int e = 0; e < nq; ++e) {
                        const int k = queue[dd * kFbTile + e];
                        acc += poly[a * kFbTile + k] * poly[b * kFbTile + k];
                    }
                    bsum[q] += acc;
                }
            }
            if (nt > 0) {
                for (int q = threadIdx.x; q < nt * kFbTile; q += kThreads) {
                    const int r = q / kFbTile, k = q - r * kFbTile;
                    tile[q] = (base + k < ch.last) ? dense[(g0 + r) * n_samp + base + k] : 0.0;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < kCPer; ++q) {
                    const int item = q * kThreads + threadIdx.x;
                    if (item >= kCItems) continue;
                    const int dd = item / (kFbGroup * K), rj = item - dd * (kFbGroup * K);
                    const int r = rj / K, j = rj - r * K;
                    if (r >= nt) continue;
                    const int nq = n_queued[dd];
                    double acc = 0.0;
                    for (int e = 0; e < nq; ++e) {
                        const int k = queue[dd * kFbTile + e];
                        acc += tile[r * kFbTile + k] * poly[j * kFbTile + k];
                    }
                    csum[q] += acc;
                }
            }
        }
        __syncthreads();
    }
    // ---- the chunk's sums leave the workgroup
    if (first_group) {
#pragma unroll
        for (int dd = 0; dd < DT; ++dd) {
            const int64_t d = d0 + dd;
            if (d >= n_det) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double v = pacc[dd][j];
                unsigned int c = ncnt[dd][j];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    v += __shfl_xor(v, off, 64);
                    c += __shfl_xor(c, off, 64);
                }
                const int64_t o = (d * n_interval + ch.interval) * K + j;
                if (lane == 0 && v != 0.0) atomicAdd(&p_out[o], v);
                if (lane == 0 && c != 0) atomicAdd(&nnz_out[o], (unsigned long long)c);
            }
        }
#pragma unroll
        for (int q = 0; q < kBPer; ++q) {
            const int item = q * kThreads + threadIdx.x;
            if (item >= kBItems) continue;
            const int dd = item / KP, pair = item - dd * KP;
            if (d0 + dd >= n_det || bsum[q] == 0.0) continue;
            atomicAdd(&b_flagged[((d0 + dd) * n_interval + ch.interval) * KP + pair], bsum[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < kCPer; ++q) {
        const int item = q * kThreads + threadIdx.x;
        if (item >= kCItems) continue;
        const int dd = item / (kFbGroup * K), rj = item - dd * (kFbGroup * K);
        const int r = rj / K, j = rj - r * K;
        if (r >= nt || d0 + dd >= n_det || csum[q] == 0.0) continue;
        atomicAdd(&c_flagged[(((d0 + dd) * n_interval + ch.interval) * n_dense + g0 + r) * K + j], csum[q]);
    }
}

// signal[d][i] -= sum_r a[d][r] Dn[r][i] + sum_j b[d][v(i)][j] P_j(x_i).  Block = (tile of samples, group of detectors),
// the dense tile staged in LDS as in k_template_subtract; a lane finds its interval by bisection over the sorted starts
// once and keeps the polynomials for all detectors of the block.  The fit is summed from zero, dense rows first, in
// template order.
template <int K>
__global__ __launch_bounds__(kThreads) void k_filterbin_subtract(
    const double * __restrict__ dense, int64_t n_dense, int64_t n_samp, const int32_t * __restrict__ sig_index,
    double * __restrict__ signal, int64_t n_det, int dets_per_block, const double * __restrict__ a_coeff,
    const int64_t * __restrict__ starts, const int64_t * __restrict__ stops, const double * __restrict__ wbins,
    int64_t n_interval, const double * __restrict__ b_coeff) {
    __shared__ double tile[kFbGroup * kFbTile];
    const int64_t base = (int64_t)blockIdx.x * kFbTile;
    const int64_t d0 = (int64_t)blockIdx.y * dets_per_block;
    const int64_t i = base + threadIdx.x;
    int64_t v = -1;
    double P[K];
#pragma unroll
    for (int j = 0; j < K; ++j) P[j] = 0.0;
    if (i < n_samp && n_interval > 0) {
        int64_t lo = 0, hi = n_interval;      // last interval with start <= i
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (starts[mid] <= i) lo = mid + 1; else hi = mid;
        }
        if (lo > 0 && i < stops[lo - 1]) {
            v = lo - 1;
            local_legendre<K>(local_phase(i, starts[v], wbins[v]), P);
        }
    }
    double fit[16];
    for (int64_t dpass = 0; dpass < dets_per_block; dpass += 16) {
#pragma unroll
        for (int dd = 0; dd < 16; ++dd) fit[dd] = 0.0;
        for (int64_t t0 = 0; t0 < n_dense; t0 += kFbGroup) {
            const int nt = (n_dense - t0 < kFbGroup) ? (int)(n_dense - t0) : kFbGroup;
            __syncthreads();
            for (int q = threadIdx.x; q < nt * kFbTile; q += kThreads) {
                const int r = q / kFbTile, k = q - r * kFbTile;
                tile[q] = (base + k < n_samp) ? dense[(t0 + r) * n_samp + base + k] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int dd = 0; dd < 16; ++dd) {
                const int64_t d = d0 + dpass + dd;
                if (d >= n_det || dpass + dd >= dets_per_block) continue;
                const double * __restrict__ cf = a_coeff + d * n_dense + t0;
                double f = fit[dd];
                for (int r = 0; r < nt; ++r) f += cf[r] * tile[r * kFbTile + threadIdx.x];
                fit[dd] = f;
            }
        }
        if (i < n_samp) {
#pragma unroll
            for (int dd = 0; dd < 16; ++dd) {
                const int64_t d = d0 + dpass + dd;
                if (d >= n_det || dpass + dd >= dets_per_block) continue;
                double f = fit[dd];
                if (v >= 0) {
                    const double * __restrict__ bc = b_coeff + (d * n_interval + v) * K;
#pragma unroll
                    for (int j = 0; j < K; ++j) f += bc[j] * P[j];
                }
                if (n_dense == 0 && v < 0) continue;      // outside every template: not touched
                double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp;
                sig[i] -= f;
            }
        }
    }
}

struct FbIntervals {
    std::vector<FbChunk> chunks;
    std::vector<double> wbins;
};

// The intervals as the kernels want them: sorted, disjoint, inside [0, n_samp) and at least K samples long.
FbIntervals fb_intervals(const int64_t * starts, const int64_t * stops, int64_t n_interval, int64_t n_samp, int K) {
    FbIntervals out;
    int64_t prev_stop = 0;
    for (int64_t v = 0; v < n_interval; ++v) {
        if (starts[v] < prev_stop || stops[v] > n_samp || stops[v] - starts[v] < K)
            fail_arg("filterbin: the intervals must be sorted, disjoint, inside the observation and not shorter than order + 1");
        prev_stop = stops[v];
        const double wbin = 2.0 / (double)(stops[v] - starts[v]);
        out.wbins.push_back(wbin);
        for (int64_t c0 = starts[v]; c0 < stops[v]; c0 += kFbChunk) {
            const int64_t c1 = (c0 + kFbChunk < stops[v]) ? c0 + kFbChunk : stops[v];
            out.chunks.push_back(FbChunk{c0, c1, starts[v], wbin, (int32_t)v, 0});
        }
    }
    return out;
}

template <typename F>
void fb_dispatch(int64_t order, F && f) {
    switch (order + 1) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        case 8: f(std::integral_constant<int, 8>()); break;
        default: fail_arg("filterbin: the polynomial order must be 0.." + std::to_string(kFbMaxK - 1));
    }
}

}  // namespace

extern "C" {

int toast_hip_fourier_templates_dev(const double * d_angle, int64_t n_samp, int64_t start_order, int64_t stop_order,
                                    double * d_templates, void * stream) {
    return guarded([&] {
        if (n_samp <= 0 || stop_order <= start_order) return;
        if (start_order < 0) fail_arg("fourier_templates: start_order must be >= 0");
        hipLaunchKernelGGL(k_fourier_templates, flat_grid(n_samp), dim3(kThreads), 0, as_stream(stream), d_angle, n_samp,
                           start_order, stop_order, d_templates);
        check_launch();
    });
}

int toast_hip_template_spans_dev(const double * d_templates, int64_t n_template, int64_t n_samp, int64_t * d_first,
                                 int64_t * d_last, void * stream) {
    return guarded([&] {
        if (n_template <= 0) return;
        if (n_template > 65535) fail_arg("template_spans: at most 65535 rows");
        hipStream_t st = as_stream(stream);
        std::vector<int64_t> init_first(n_template, n_samp > 0 ? n_samp : 0), init_last(n_template, -1);
        TH_HIP(hipMemcpyAsync(d_first, init_first.data(), sizeof(int64_t) * n_template, hipMemcpyHostToDevice, st));
        TH_HIP(hipMemcpyAsync(d_last, init_last.data(), sizeof(int64_t) * n_template, hipMemcpyHostToDevice, st));
        TH_HIP(hipStreamSynchronize(st));      // the initial values live on this stack frame
        if (n_samp <= 0) return;
        const int64_t slice = 65536;
        hipLaunchKernelGGL(k_template_spans, dim3((unsigned)((n_samp + slice - 1) / slice), (unsigned)n_template),
                           dim3(kThreads), 0, st, d_templates, n_samp, slice, reinterpret_cast<long long *>(d_first),
                           reinterpret_cast<long long *>(d_last));
        check_launch();
    });
}

int toast_hip_filterbin_good_counts_dev(const double * d_templates, int64_t n_template, int64_t n_samp,
                                        const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                        const uint8_t * d_shared_flags, uint8_t shared_flag_mask, int64_t n_det,
                                        int64_t * d_n_good, int64_t * d_nnz, void * stream) {
    return guarded([&] {
        if (n_det <= 0) return;
        if (n_template < 0) fail_arg("filterbin_good_counts: n_template must be >= 0");
        hipStream_t st = as_stream(stream);
        TH_HIP(hipMemsetAsync(d_n_good, 0, sizeof(int64_t) * n_det, st));
        if (n_template > 0) TH_HIP(hipMemsetAsync(d_nnz, 0, sizeof(int64_t) * n_det * n_template, st));
        if (n_samp <= 0) return;
        ParamBlock pb;
        std::vector<int32_t> no_flags(n_det, 0);
        const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : no_flags.data(), sizeof(int32_t) * n_det);
        const int32_t * fidx = (const int32_t *)(pb.commit(st) + o_fi);
        const int64_t slice = 16384;
        const int64_t n_slice = (n_samp + slice - 1) / slice;
        if (n_slice > 65535) fail_arg("filterbin_good_counts: n_samp too large");
        hipLaunchKernelGGL(k_good_counts, dim3((unsigned)((n_det + 3) / 4), (unsigned)n_slice), dim3(kThreads), 0, st,
                           d_templates, n_template, n_samp, fidx, d_det_flags, det_flag_mask, d_shared_flags,
                           shared_flag_mask, n_det, slice, reinterpret_cast<unsigned long long *>(d_n_good),
                           reinterpret_cast<unsigned long long *>(d_nnz));
        check_launch();
    });
}

int toast_hip_filterbin_flag_spans_dev(const int32_t * flag_rows, const int64_t * firsts, const int64_t * lasts,
                                       int64_t n_span, int64_t n_rows, int64_t n_samp, uint8_t * d_det_flags, uint8_t mask,
                                       void * stream) {
    return guarded([&] {
        if (n_span <= 0 || n_samp <= 0) return;
        std::vector<FlagSpan> spans;
        int64_t longest = 0;
        for (int64_t s = 0; s < n_span; ++s) {
            if (flag_rows[s] < 0 || flag_rows[s] >= n_rows || firsts[s] < 0 || lasts[s] > n_samp)
                fail_arg("filterbin_flag_spans: span outside the flag buffer");
            if (lasts[s] <= firsts[s]) continue;
            spans.push_back(FlagSpan{firsts[s], lasts[s], flag_rows[s], 0});
            longest = (lasts[s] - firsts[s] > longest) ? lasts[s] - firsts[s] : longest;
        }
        if (spans.empty()) return;
        hipStream_t st = as_stream(stream);
        ParamBlock pb;
        const size_t o_sp = pb.push_vec(spans);
        const FlagSpan * dsp = (const FlagSpan *)(pb.commit(st) + o_sp);
        int64_t gy = (longest + kThreads - 1) / kThreads;
        gy = (gy > 1024) ? 1024 : gy;
        // overlapping spans of one row would race on a byte: they are applied one launch per span then
        for (size_t base = 0; base < spans.size();) {
            size_t n = 1;
            auto overlaps = [&](size_t a, size_t b) {
                return spans[a].row == spans[b].row && spans[a].first < spans[b].last && spans[b].first < spans[a].last;
            };
            while (base + n < spans.size() && n < 65535) {
                bool clash = false;
                for (size_t k = base; k < base + n && !clash; ++k) clash = overlaps(k, base + n);
                if (clash) break;
                ++n;
            }
            hipLaunchKernelGGL(k_flag_spans, dim3((unsigned)n, (unsigned)gy), dim3(kThreads), 0, st, dsp + base, n_samp,
                               d_det_flags, mask);
            check_launch();
            base += n;
        }
    });
}

int toast_hip_filterbin_accumulate_dev(int64_t order, const double * d_dense, int64_t n_dense, int64_t n_samp,
                                       const int32_t * signal_index, const double * d_signal, const int32_t * flag_index,
                                       const uint8_t * d_det_flags, uint8_t det_flag_mask, const uint8_t * d_shared_flags,
                                       uint8_t shared_flag_mask, int64_t n_det, const int64_t * starts, const int64_t * stops,
                                       int64_t n_interval, double * d_p, int64_t * d_nnz, double * d_b_common,
                                       double * d_c_common, double * d_b_flagged, double * d_c_flagged, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_interval <= 0) return;
        if (n_dense < 0) fail_arg("filterbin_accumulate: n_dense must be >= 0");
        fb_dispatch(order, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            constexpr int KP = FbShape<K>::kPairs;
            constexpr int DT = FbShape<K>::kDets;
            hipStream_t st = as_stream(stream);
            const FbIntervals iv = fb_intervals(starts, stops, n_interval, n_samp, K);
            TH_HIP(hipMemsetAsync(d_p, 0, sizeof(double) * n_det * n_interval * K, st));
            TH_HIP(hipMemsetAsync(d_nnz, 0, sizeof(int64_t) * n_det * n_interval * K, st));
            TH_HIP(hipMemsetAsync(d_b_common, 0, sizeof(double) * n_interval * KP, st));
            TH_HIP(hipMemsetAsync(d_b_flagged, 0, sizeof(double) * n_det * n_interval * KP, st));
            if (n_dense > 0) {
                TH_HIP(hipMemsetAsync(d_c_common, 0, sizeof(double) * n_interval * n_dense * K, st));
                TH_HIP(hipMemsetAsync(d_c_flagged, 0, sizeof(double) * n_det * n_interval * n_dense * K, st));
            }
            ParamBlock pb;
            const size_t o_ch = pb.push_vec(iv.chunks);
            const size_t o_si = pb.push(signal_index, sizeof(int32_t) * n_det);
            std::vector<int32_t> no_flags(n_det, 0);
            const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : no_flags.data(), sizeof(int32_t) * n_det);
            const char * dparam = pb.commit(st);
            const FbChunk * dch = (const FbChunk *)(dparam + o_ch);
            const int32_t * sidx = (const int32_t *)(dparam + o_si);
            const int32_t * fidx = (const int32_t *)(dparam + o_fi);
            const int64_t n_chunk = (int64_t)iv.chunks.size();
            const int64_t n_tile = (n_det + DT - 1) / DT;
            if (n_tile > 65535) fail_arg("filterbin_accumulate: too many detectors for one call");
            hipLaunchKernelGGL(k_interval_common<K>, dim3((unsigned)n_chunk), dim3(kThreads), 0, st, dch, d_dense, n_dense,
                               n_samp, d_shared_flags, shared_flag_mask, d_b_common, d_c_common);
            check_launch();
            for (int64_t g0 = 0; g0 == 0 || g0 < n_dense; g0 += kFbGroup) {
                if (g0 > 0 && d_det_flags == nullptr) break;      // nothing but corrections in the later groups
                hipLaunchKernelGGL(k_interval_accumulate<K>, dim3((unsigned)n_chunk, (unsigned)n_tile), dim3(kThreads), 0, st,
                                   dch, d_dense, n_dense, g0, n_samp, sidx, d_signal, fidx, d_det_flags, det_flag_mask,
                                   d_shared_flags, shared_flag_mask, n_det, n_interval, d_p,
                                   reinterpret_cast<unsigned long long *>(d_nnz), d_b_flagged, d_c_flagged);
                check_launch();
            }
        });
    });
}

int toast_hip_filterbin_subtract_dev(int64_t order, const double * d_dense, int64_t n_dense, int64_t n_samp,
                                     const int32_t * signal_index, double * d_signal, int64_t n_det, const double * d_a,
                                     const int64_t * starts, const int64_t * stops, int64_t n_interval, const double * d_b,
                                     void * stream) {
    return guarded([&] {
        if (n_samp <= 0 || n_det <= 0 || (n_dense <= 0 && n_interval <= 0)) return;
        if (n_dense < 0 || n_interval < 0) fail_arg("filterbin_subtract: negative template counts");
        fb_dispatch(n_interval > 0 ? order : 0, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            hipStream_t st = as_stream(stream);
            const FbIntervals iv = fb_intervals(starts, stops, n_interval, n_samp, K);
            ParamBlock pb;
            const size_t o_si = pb.push(signal_index, sizeof(int32_t) * n_det);
            const size_t o_a = pb.push(starts, sizeof(int64_t) * n_interval);
            const size_t o_b = pb.push(stops, sizeof(int64_t) * n_interval);
            const size_t o_w = pb.push_vec(iv.wbins);
            const char * dparam = pb.commit(st);
            const int dets_per_block = 32;
            const dim3 grid((unsigned)((n_samp + kFbTile - 1) / kFbTile), (unsigned)((n_det + dets_per_block - 1) / dets_per_block));
            hipLaunchKernelGGL(k_filterbin_subtract<K>, grid, dim3(kThreads), 0, st, d_dense, n_dense, n_samp,
                               (const int32_t *)(dparam + o_si), d_signal, n_det, dets_per_block, d_a,
                               (const int64_t *)(dparam + o_a), (const int64_t *)(dparam + o_b),
                               (const double *)(dparam + o_w), n_interval, d_b);
            check_launch();
        });
    });
}

int toast_hip_filterbin_chunk(void) { return kFbChunk; }

int toast_hip_filterbin_det_tile(int64_t order) { return (order + 1 <= 4) ? 8 : 4; }

int toast_hip_filterbin_max_order(void) { return kFbMaxK - 1; }

}  // extern "C"
