// template_basis.hip -- the kernels behind toast.templates.SubHarmonic, toast.templates.GainTemplate and
// toast.templates.Periodic on the device.
//
// Reference: src/toast/templates/subharmonic.py:143-236, src/toast/templates/gaintemplate.py:56-238 and
// src/toast/templates/periodic.py:216-419.  The templates are pure NumPy there, one detector and one view at a time; here
// all detectors of an observation go in one launch.
//
// SubHarmonic and GainTemplate -- one family of Legendre sweeps.  The [norder][view_len] Legendre matrix the reference
// stores per view never exists: each lane evaluates r_i = i * (2 / (L - 1)) - 1 (np.linspace(-1, 1, L): the last sample is
// exactly 1) and the recurrence T_k = (((2k - 1) r) T_{k-1} - (k - 1) T_{k-2}) / k with a true division, the reference's
// own operation order, so the basis is the reference's bit for bit (-ffp-contract=off).  GainTemplate multiplies the same
// basis by a per-detector signal estimate, a second fp64 stream per sample with its own buffer and row list.  The two
// templates differ in six facts, stated by the policies SubHarmonicSweep and GainSweep and decided at compile time; chunks,
// pair loop, reductions and the Gram write exist once.
//   k_legendre_add      signal[d][view] += sum_k T_k a_k (GainTemplate: times the estimate); the amplitudes of a
//                       (detector, view) are wave-uniform; aligned pairs of samples move as 16 bytes: 16 B per
//                       detector-sample, 24 B with the estimate.
//   k_legendre_partial  pass 1 of the projection a_k = sum_i w_i T_k(r_i) (w: the signal, or estimate * signal: 17 B per
//                       detector-sample with estimate and flags) and of the Gram matrix sum_i T_r T_c: lane partials, xor
//                       butterflies, the four waves through LDS in wave order; one partial vector per chunk of kBasisChunk
//                       samples.
//   k_legendre_combine  one thread per output value adds the partials of a (detector, view) in chunk order and assigns or
//                       accumulates the amplitude (or writes the weighted Gram matrix).  No atomics anywhere:
//                       order-deterministic.
//   k_subh_precond      out[block] = P[block] in[block], one thread per output amplitude, for both templates.
//
// Periodic -- the bin of every sample is computed once per observation (k_periodic_index: int32((v - min) / incr) in
// fp64, truncated, clamped to nbins - 1; -1 outside the views and where the key's own flags are set) and cached as an
// int32 row: the three sweeps then read 4 B per sample, shared by all detectors when the key is a shared field.
//   k_periodic_hits     LDS histogram of the good samples per workgroup, merged with integer atomics (exact).
//   k_periodic_add      signal[d][i] += amps[d][index[i]]: a gather, bit-exact.
//   k_periodic_partial  amps[d][index[i]] += signal[d][i] over the unflagged samples: every wave owns a private copy of
//   k_periodic_combine  the detector's bins in LDS and adds 64 consecutive samples at a time into it, bin after bin, the
//                       lanes of one bin summed by xor butterflies (no atomics); the four copies are added in wave order
//                       into one partial histogram per chunk, the chunks in chunk order: order-deterministic by
//                       construction.
//   k_periodic_atomic   the same sums for more than kPeriodicLdsBins bins: fp64 vector atomics in global memory (NOT
//                       order-deterministic).
//   k_periodic_precond  out = in * hits where the amplitude is unflagged.

#include <algorithm>
#include <type_traits>

#include "kernel_common.hpp"

namespace {

constexpr int kSubhMaxTerms = 9;        // order + 1 supported: the Gram accumulators (45 doubles) stay in registers
constexpr int kBasisChunk = 4096;       // samples per workgroup of the SubHarmonic sweeps
constexpr int kPeriodicChunk = 16384;   // samples per workgroup of the Periodic sweeps
constexpr int kPeriodicLdsBins = 1024;  // four private fp64 copies of a detector's bins: 32 KB of LDS per workgroup

struct BasisJob {
    int64_t first;    // clipped to [0, n_samp)
    int32_t len;
    int32_t view;     // index into the caller's interval list
    int32_t chunk0;   // first slot of this view in the chunk list
    int32_t n_chunk;
};

struct BasisChunk {
    int32_t job;
    int32_t chunk;
};

// np.linspace(-1, 1, len)[i]: arange * step + start with step = 2 / (len - 1) (a single sample: 0 * 2 - 1), the last
// sample overwritten with the stop value
__device__ __forceinline__ double linspace_step(int len) { return (len > 1) ? 2.0 / (double)(len - 1) : 2.0; }

__device__ __forceinline__ double linspace_r(int i, int len, double step) {
    const double r = (double)i * step + (-1.0);
    return (len > 1 && i == len - 1) ? 1.0 : r;
}

// subharmonic.py:145-154
template <int N>
__device__ __forceinline__ void subh_terms(double r, double (&t)[N]) {
    t[0] = 1.0;
    if constexpr (N > 1) t[1] = r;
#pragma unroll
    for (int k = 2; k < N; ++k) {
        t[k] = (((double)(2 * k - 1) * r) * t[k - 1] - (double)(k - 1) * t[k - 2]) / (double)k;
    }
}

// ------------------------------------------------------------------------------------ the two Legendre templates
// The six facts in which SubHarmonic and GainTemplate differ, each the opposite of the other; every one is decided with
// `if constexpr` or inlined, so an instantiation neither tests nor reads what its template does not have.
struct SubHarmonicSweep {
    static constexpr bool kEstimate = false;          // 1. no estimate stream
    // 2. subharmonic.py:200-203: one order after the other, onto the signal itself
    template <int N>
    static __device__ __forceinline__ double add(double s, double, const double (&t)[N], const double (&amp)[N], int n) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (k < n) s += t[k] * amp[k];
        }
        return s;
    }
    static constexpr bool kProjectFlags = false;      // 3. the projection covers ALL samples (subharmonic.py:205-218)
    static constexpr bool kGramFlags = true;          // 4. sum_good T_r T_c, and the number of good samples (:157-179)
    static constexpr bool kGramTimesEstimate = false; // 5. the bare basis
    static constexpr bool kAccumulate = false;        // 6. the amplitude is ASSIGNED (subharmonic.py:217)
};

struct GainSweep {
    static constexpr bool kEstimate = true;           // 1. est[d][i], read next to the signal
    // 2. gaintemplate.py:182-197: the gain fluctuation sum_k T_k a_k (ascending k, from zero), times the estimate, onto
    // the signal
    template <int N>
    static __device__ __forceinline__ double add(double s, double e, const double (&t)[N], const double (&amp)[N], int n) {
        double g = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if (k < n) g += t[k] * amp[k];
        }
        return s + e * g;
    }
    static constexpr bool kProjectFlags = true;       // 3. sum_unflagged (est_i signal_i) T_k (gaintemplate.py:199-220)
    static constexpr bool kGramFlags = false;         // 4. ALL samples: the reference computes `good` for its
                                                      //    preconditioner and never uses it (gaintemplate.py:159-170)
    static constexpr bool kGramTimesEstimate = true;  // 5. sum (T_r est_i)(T_c est_i)
    static constexpr bool kAccumulate = true;         // 6. ONTO the amplitude already there (gaintemplate.py:220)
};

// values per chunk.  GRAM = false: the N amplitudes.  GRAM = true: the packed upper triangle of the N x N Gram matrix,
// then the number of good samples where the template counts them
template <int N, class P, bool GRAM>
constexpr int kSweepValues = GRAM ? N * (N + 1) / 2 + (P::kGramFlags ? 1 : 0) : N;

// The signal moves as aligned pairs.  The estimate row lies in another buffer with its own row index, so its pairs may
// start 8 bytes off a 16-byte boundary: it is read as two adjacent 8-byte values with no alignment promised.  gfx950
// takes wide loads at 8-byte alignment, and the compiler merges the two into one global_load_dwordx4 (seen in the ISA: one
// dwordx4 load per stream and one dwordx4 store per pair); either way a wave covers one contiguous range of the estimate.
template <int N, class P>
__global__ __launch_bounds__(kThreads) void k_legendre_add(double * __restrict__ signal, int64_t n_samp,
                                                           const int32_t * __restrict__ sig_index,
                                                           const double * __restrict__ estimate,
                                                           const int32_t * __restrict__ est_index,
                                                           const int64_t * __restrict__ amp_offsets,
                                                           const double * __restrict__ amplitudes,
                                                           const BasisJob * __restrict__ jobs,
                                                           const BasisChunk * __restrict__ chunks, int n) {
    const BasisChunk ch = chunks[blockIdx.x];
    const BasisJob job = jobs[ch.job];
    const int64_t d = blockIdx.y;
    const double * __restrict__ arow = amplitudes + amp_offsets[d] + (int64_t)job.view * n;
    double amp[N];
#pragma unroll
    for (int k = 0; k < N; ++k) amp[k] = (k < n) ? arow[k] : 0.0;
    const int i0 = ch.chunk * kBasisChunk;
    const int cnt = (i0 + kBasisChunk < job.len) ? kBasisChunk : job.len - i0;
    double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp + job.first + i0;
    const double * __restrict__ est = nullptr;
    if constexpr (P::kEstimate) est = estimate + (int64_t)est_index[d] * n_samp + job.first + i0;
    const double step = linspace_step(job.len);
    // one sample of the chunk (never read for SubHarmonic: its add() drops the estimate)
    auto at = [&](double s, int j) {
        double e = 0.0;
        if constexpr (P::kEstimate) e = est[j];
        double t[N];
        subh_terms<N>(linspace_r(i0 + j, job.len, step), t);
        return P::template add<N>(s, e, t, amp, n);
    };
    // aligned pairs: pad = 1 when the chunk starts on an odd double
    const int pad = (int)((reinterpret_cast<uintptr_t>(sig) >> 3) & 1);
    const int n_pair = (pad + cnt + 1) >> 1;
    for (int p = threadIdx.x; p < n_pair; p += kThreads) {
        const int j = 2 * p - pad;     // index inside the chunk of the pair's first sample
        if (j >= 0 && j + 2 <= cnt) {
            double2 v = *reinterpret_cast<const double2 *>(sig + j);
            v.x = at(v.x, j);
            v.y = at(v.y, j + 1);
            *reinterpret_cast<double2 *>(sig + j) = v;
        } else {
            if (j >= 0 && j < cnt) sig[j] = at(sig[j], j);
            if (j + 1 >= 0 && j + 1 < cnt) sig[j + 1] = at(sig[j + 1], j + 1);
        }
    }
}

// Lane partials -> wave totals (xor butterflies: the same tree in every run) -> the four waves in wave order -> out[NV]
template <int NV>
__device__ __forceinline__ void block_totals(const double (&v)[NV], double * wave_tot /*[4][NV]*/, double * __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
        if (lane == 0) wave_tot[wave * NV + k] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double t = 0.0;
        for (int w = 0; w < kThreads / 64; ++w) t += wave_tot[w * NV + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// GRAM = false: v[k] = sum w_i T_k(r_i) with w = the signal, or estimate * signal
// GRAM = true:  v = packed upper triangle of sum T_r T_c (the basis times the estimate first where the template says so),
//               then the number of good samples where it counts them
// over the samples of the chunk the template's flag facts admit
template <int N, class P, bool GRAM>
__global__ __launch_bounds__(kThreads) void k_legendre_partial(const double * __restrict__ signal, int64_t n_samp,
                                                               const int32_t * __restrict__ sig_index,
                                                               const double * __restrict__ estimate,
                                                               const int32_t * __restrict__ est_index,
                                                               const uint8_t * __restrict__ det_flags,
                                                               const int32_t * __restrict__ flag_index, uint8_t det_mask,
                                                               const BasisJob * __restrict__ jobs,
                                                               const BasisChunk * __restrict__ chunks, int64_t n_chunk,
                                                               double * __restrict__ partial) {
    constexpr int NV = kSweepValues<N, P, GRAM>;
    constexpr bool kFlags = GRAM ? P::kGramFlags : P::kProjectFlags;
    constexpr bool kEst = GRAM ? P::kGramTimesEstimate : P::kEstimate;
    __shared__ double wave_tot[4 * NV];
    const BasisChunk ch = chunks[blockIdx.x];
    const BasisJob job = jobs[ch.job];
    const int64_t d = blockIdx.y;
    const int i0 = ch.chunk * kBasisChunk;
    const int i1 = (i0 + kBasisChunk < job.len) ? i0 + kBasisChunk : job.len;
    const double step = linspace_step(job.len);
    const double * __restrict__ est = nullptr;
    if constexpr (kEst) est = estimate + (int64_t)est_index[d] * n_samp + job.first;
    const double * __restrict__ sig = nullptr;
    if constexpr (!GRAM) sig = signal + (int64_t)sig_index[d] * n_samp + job.first;
    const uint8_t * __restrict__ fl = nullptr;
    if constexpr (kFlags) fl = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp + job.first : nullptr;
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += kThreads) {
        if constexpr (kFlags) {
            if (fl != nullptr && (fl[i] & det_mask) != 0) continue;
        }
        double e = 0.0;
        if constexpr (kEst) e = est[i];
        double t[N];
        if constexpr (GRAM) {
            subh_terms<N>(linspace_r(i, job.len, step), t);
            if constexpr (kEst) {
#pragma unroll
                for (int k = 0; k < N; ++k) t[k] *= e;
            }
            int q = 0;
#pragma unroll
            for (int r = 0; r < N; ++r) {
#pragma unroll
                for (int c = r; c < N; ++c) v[q++] += t[r] * t[c];
            }
            if constexpr (kFlags) v[NV - 1] += 1.0;
        } else {
            double w = sig[i];
            if constexpr (kEst) w = e * w;
            subh_terms<N>(linspace_r(i, job.len, step), t);
#pragma unroll
            for (int k = 0; k < N; ++k) v[k] += w * t[k];
        }
    }
    block_totals<NV>(v, wave_tot, partial + ((int64_t)d * n_chunk + blockIdx.x) * NV);
}

// grid (views, detectors): thread k adds the partials of its value in chunk order.
// GRAM = false: amplitudes[amp_offsets[d] + view * n + k] = total, or += total: onto the value already there
// GRAM = true:  gram[(d * n_view + view)][r][c] = gram[..][c][r] = total * weight[d]; ngood[d * n_view + view] where counted
template <int N, class P, bool GRAM>
__global__ __launch_bounds__(64) void k_legendre_combine(const BasisJob * __restrict__ jobs, int64_t n_chunk,
                                                         const double * __restrict__ partial, int n, int64_t n_view,
                                                         const int64_t * __restrict__ amp_offsets,
                                                         double * __restrict__ amplitudes,
                                                         const double * __restrict__ weights, double * __restrict__ gram,
                                                         int64_t * __restrict__ ngood) {
    constexpr int NV = kSweepValues<N, P, GRAM>;
    const BasisJob job = jobs[blockIdx.x];
    const int64_t d = blockIdx.y;
    const double * __restrict__ p = partial + ((int64_t)d * n_chunk + job.chunk0) * NV;
    for (int k = threadIdx.x; k < NV; k += 64) {
        if constexpr (GRAM) {
            double t = 0.0;
            for (int c = 0; c < job.n_chunk; ++c) t += p[(int64_t)c * NV + k];
            const int64_t blk = d * n_view + job.view;
            bool count = false;
            if constexpr (P::kGramFlags) count = (k == NV - 1);
            if (count) {
                ngood[blk] = (int64_t)t;
            } else {
                // packed index k of the N x N upper triangle -> (r, c)
                int r = 0, rem = k;
                while (rem >= N - r) {
                    rem -= N - r;
                    ++r;
                }
                const int c = r + rem;
                if (c < n) {
                    const double g = t * weights[d];     // subharmonic.py:173-176: the dot product, then the weight
                    gram[blk * n * n + r * n + c] = g;
                    gram[blk * n * n + c * n + r] = g;
                }
            }
        } else {
            if (k < n) {
                double * __restrict__ a = amplitudes + amp_offsets[d] + (int64_t)job.view * n + k;
                double t = 0.0;
                if constexpr (P::kAccumulate) t = *a;
                for (int c = 0; c < job.n_chunk; ++c) t += p[(int64_t)c * NV + k];
                *a = t;
            }
        }
    }
}

// subharmonic.py:233-235
__global__ __launch_bounds__(kThreads) void k_subh_precond(int n, int64_t n_amp, const double * __restrict__ precond,
                                                           const double * __restrict__ amp_in, double * __restrict__ amp_out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_amp; i += (int64_t)gridDim.x * kThreads) {
        const int64_t blk = i / n;
        const int r = (int)(i - blk * n);
        const double * __restrict__ row = precond + (blk * n + r) * n;
        const double * __restrict__ x = amp_in + blk * n;
        double acc = 0.0;
        for (int c = 0; c < n; ++c) acc += row[c] * x[c];
        amp_out[i] = acc;
    }
}

// ------------------------------------------------------------------------------------ periodic
// periodic.py:311-317 for the samples of the views; the key's own flags folded in as index -1
__global__ __launch_bounds__(kThreads) void k_periodic_index(const double * __restrict__ key, int64_t key_stride,
                                                             const uint8_t * __restrict__ flags, uint8_t flag_mask,
                                                             int64_t n_samp, double obs_min, double incr, int32_t nbins,
                                                             const BasisJob * __restrict__ jobs,
                                                             const BasisChunk * __restrict__ chunks,
                                                             int32_t * __restrict__ index) {
    const BasisChunk ch = chunks[blockIdx.x];
    const BasisJob job = jobs[ch.job];
    const int64_t row = blockIdx.y;
    const int i0 = ch.chunk * kBasisChunk;
    const int i1 = (i0 + kBasisChunk < job.len) ? i0 + kBasisChunk : job.len;
    const double * __restrict__ krow = key + row * key_stride + job.first;
    const uint8_t * __restrict__ frow = (flags != nullptr) ? flags + row * key_stride + job.first : nullptr;
    int32_t * __restrict__ out = index + row * n_samp + job.first;
    for (int i = i0 + threadIdx.x; i < i1; i += kThreads) {
        int32_t b = -1;
        if (frow == nullptr || (frow[i] & flag_mask) == 0) {
            b = (int32_t)((krow[i] - obs_min) / incr);
            if (b >= nbins) b = nbins - 1;
        }
        out[i] = b;
    }
}

// a sample takes part when its cached index is a bin of THIS call (-1: outside the views or flagged by the key's flags)
__device__ __forceinline__ bool periodic_bin(int32_t b, int32_t nbins) { return (uint32_t)b < (uint32_t)nbins; }

__device__ __forceinline__ const int32_t * periodic_index_row(const int32_t * index, const int32_t * index_rows, int64_t d,
                                                              int64_t n_samp) {
    return (index_rows != nullptr) ? index + (int64_t)index_rows[d] * n_samp : index;
}

// periodic.py:257-269: hits[amp_offsets[d] + index[i]] += 1 over s0 <= i < s1 with a bin and clear detector flags
__global__ __launch_bounds__(kThreads) void k_periodic_hits(const int32_t * __restrict__ index,
                                                            const int32_t * __restrict__ index_rows, int64_t n_samp,
                                                            const uint8_t * __restrict__ det_flags,
                                                            const int32_t * __restrict__ flag_index, uint8_t det_mask,
                                                            const int64_t * __restrict__ amp_offsets, int32_t nbins,
                                                            int64_t s0, int64_t s1, int32_t * __restrict__ hits) {
    __shared__ int32_t hist[kPeriodicLdsBins];
    const int64_t d = blockIdx.y;
    const bool lds = nbins <= kPeriodicLdsBins;
    if (lds) {
        for (int b = threadIdx.x; b < nbins; b += kThreads) hist[b] = 0;
        __syncthreads();
    }
    const int32_t * __restrict__ irow = periodic_index_row(index, index_rows, d, n_samp);
    const uint8_t * __restrict__ fl = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp : nullptr;
    int32_t * __restrict__ hrow = hits + amp_offsets[d];
    const int64_t c0 = s0 + (int64_t)blockIdx.x * kPeriodicChunk;
    const int64_t c1 = (c0 + kPeriodicChunk < s1) ? c0 + kPeriodicChunk : s1;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += kThreads) {
        const int32_t b = irow[i];
        if (!periodic_bin(b, nbins) || (fl != nullptr && (fl[i] & det_mask) != 0)) continue;
        if (lds) {
            atomicAdd(&hist[b], 1);
        } else {
            atomicAdd(&hrow[b], 1);
        }
    }
    if (lds) {
        __syncthreads();
        for (int b = threadIdx.x; b < nbins; b += kThreads) {
            const int32_t h = hist[b];
            if (h != 0) atomicAdd(&hrow[b], h);
        }
    }
}

// periodic.py:339-349: the key's flags only (they are in the index), never the detector flags
__global__ __launch_bounds__(kThreads) void k_periodic_add(const int32_t * __restrict__ index,
                                                           const int32_t * __restrict__ index_rows, int64_t n_samp,
                                                           const int64_t * __restrict__ amp_offsets,
                                                           const double * __restrict__ amplitudes,
                                                           const int32_t * __restrict__ sig_index,
                                                           double * __restrict__ signal, int32_t nbins) {
    const int64_t d = blockIdx.y;
    const int32_t * __restrict__ irow = periodic_index_row(index, index_rows, d, n_samp);
    const double * __restrict__ arow = amplitudes + amp_offsets[d];
    double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp;
    const int64_t c0 = (int64_t)blockIdx.x * kPeriodicChunk;     // (even: pairs never straddle two chunks)
    const int64_t c1 = (c0 + kPeriodicChunk < n_samp) ? c0 + kPeriodicChunk : n_samp;
    // 16-byte signal and 8-byte index accesses need an even row start: n_samp even or row 0 (checked by the host)
    const bool pairs = ((reinterpret_cast<uintptr_t>(sig) & 15) == 0) && ((reinterpret_cast<uintptr_t>(irow) & 7) == 0);
    if (pairs) {
        for (int64_t i = c0 + 2 * (int64_t)threadIdx.x; i < c1; i += 2 * kThreads) {
            if (i + 1 < c1) {
                const int2 b = *reinterpret_cast<const int2 *>(irow + i);
                const bool gx = periodic_bin(b.x, nbins), gy = periodic_bin(b.y, nbins);
                if (gx && gy) {
                    double2 v = *reinterpret_cast<const double2 *>(sig + i);
                    v.x += arow[b.x];
                    v.y += arow[b.y];
                    *reinterpret_cast<double2 *>(sig + i) = v;
                } else if (gx) {
                    sig[i] += arow[b.x];
                } else if (gy) {
                    sig[i + 1] += arow[b.y];
                }
            } else {
                const int32_t b = irow[i];
                if (periodic_bin(b, nbins)) sig[i] += arow[b];
            }
        }
    } else {
        for (int64_t i = c0 + threadIdx.x; i < c1; i += kThreads) {
            const int32_t b = irow[i];
            if (periodic_bin(b, nbins)) sig[i] += arow[b];
        }
    }
}

// periodic.py:374-389, order-deterministic form.  dynamic LDS: [4 waves][nbins] doubles
__global__ __launch_bounds__(kThreads) void k_periodic_partial(const int32_t * __restrict__ index,
                                                               const int32_t * __restrict__ index_rows, int64_t n_samp,
                                                               const int32_t * __restrict__ sig_index,
                                                               const double * __restrict__ signal,
                                                               const uint8_t * __restrict__ det_flags,
                                                               const int32_t * __restrict__ flag_index, uint8_t det_mask,
                                                               int32_t nbins, double * __restrict__ partial) {
    extern __shared__ double bins[];
    const int64_t d = blockIdx.y;
    const int wave = threadIdx.x >> 6;
    for (int b = threadIdx.x; b < 4 * nbins; b += kThreads) bins[b] = 0.0;
    __syncthreads();
    const int32_t * __restrict__ irow = periodic_index_row(index, index_rows, d, n_samp);
    const double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp;
    const uint8_t * __restrict__ fl = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp : nullptr;
    double * mine = bins + wave * nbins;
    const int lane = threadIdx.x & 63;
    const int64_t c0 = (int64_t)blockIdx.x * kPeriodicChunk;
    const int64_t c1 = (c0 + kPeriodicChunk < n_samp) ? c0 + kPeriodicChunk : n_samp;
    // A wave takes 64 consecutive samples at a time and adds into its own copy only, one bin after the other: the lanes
    // of the lowest pending bin are summed by xor butterflies (the other lanes contribute zeros: the same tree in every
    // run) and the first of them adds the total with a plain read-modify-write.  No atomics: the order of every addition
    // is fixed by the program.  A slowly varying key meets one or two bins per step.
    for (int64_t base = c0 + (int64_t)wave * 64; base < c1; base += kThreads) {
        const int64_t i = base + lane;
        int32_t b = -1;
        double s = 0.0;
        if (i < c1) {
            b = irow[i];
            s = sig[i];
            if (!periodic_bin(b, nbins) || (fl != nullptr && (fl[i] & det_mask) != 0)) b = -1;
        }
        unsigned long long todo = __ballot(b >= 0);
        while (todo != 0ull) {
            const int leader = __ffsll((long long)todo) - 1;
            const int32_t lb = __shfl(b, leader, 64);
            const bool same = (b == lb);
            double v = same ? s : 0.0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == leader) mine[lb] += v;
            todo &= ~__ballot(same);
        }
    }
    __syncthreads();
    double * __restrict__ out = partial + ((int64_t)d * gridDim.x + blockIdx.x) * nbins;
    for (int b = threadIdx.x; b < nbins; b += kThreads) {
        double t = bins[b];
        for (int w = 1; w < kThreads / 64; ++w) t += bins[w * nbins + b];
        out[b] = t;
    }
}

__global__ __launch_bounds__(kThreads) void k_periodic_combine(const double * __restrict__ partial, int64_t n_chunk,
                                                               int32_t nbins, const int64_t * __restrict__ amp_offsets,
                                                               double * __restrict__ amplitudes) {
    const int64_t d = blockIdx.y;
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= nbins) return;
    const double * __restrict__ p = partial + d * n_chunk * nbins + b;
    double t = 0.0;
    for (int64_t c = 0; c < n_chunk; ++c) t += p[c * nbins];
    amplitudes[amp_offsets[d] + b] += t;
}

__global__ __launch_bounds__(kThreads) void k_periodic_atomic(const int32_t * __restrict__ index,
                                                              const int32_t * __restrict__ index_rows, int64_t n_samp,
                                                              const int32_t * __restrict__ sig_index,
                                                              const double * __restrict__ signal,
                                                              const uint8_t * __restrict__ det_flags,
                                                              const int32_t * __restrict__ flag_index, uint8_t det_mask,
                                                              const int64_t * __restrict__ amp_offsets,
                                                              int32_t nbins, double * __restrict__ amplitudes) {
    const int64_t d = blockIdx.y;
    const int32_t * __restrict__ irow = periodic_index_row(index, index_rows, d, n_samp);
    const double * __restrict__ sig = signal + (int64_t)sig_index[d] * n_samp;
    const uint8_t * __restrict__ fl = (det_flags != nullptr) ? det_flags + (int64_t)flag_index[d] * n_samp : nullptr;
    double * __restrict__ arow = amplitudes + amp_offsets[d];
    const int64_t c0 = (int64_t)blockIdx.x * kPeriodicChunk;
    const int64_t c1 = (c0 + kPeriodicChunk < n_samp) ? c0 + kPeriodicChunk : n_samp;
    for (int64_t i = c0 + threadIdx.x; i < c1; i += kThreads) {
        const int32_t b = irow[i];
        if (!periodic_bin(b, nbins) || (fl != nullptr && (fl[i] & det_mask) != 0)) continue;
        unsafeAtomicAdd(&arow[b], sig[i]);
    }
}

// periodic.py:411-417
__global__ __launch_bounds__(kThreads) void k_periodic_precond(int64_t n_amp, const int32_t * __restrict__ hits,
                                                               const uint8_t * __restrict__ amp_flags,
                                                               const double * __restrict__ amp_in, double * __restrict__ amp_out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_amp; i += (int64_t)gridDim.x * kThreads) {
        if (amp_flags[i] == 0) amp_out[i] = amp_in[i] * (double)hits[i];
    }
}

// ------------------------------------------------------------------------------------ host side
struct BasisPlan {
    std::vector<BasisJob> jobs;
    std::vector<BasisChunk> chunks;
    std::vector<int64_t> empty_views;     // views without a sample inside [0, n_samp): no job
};

BasisPlan basis_plan(const toast_hip_interval * ivl, int64_t n_view, int64_t n_samp, const char * what) {
    BasisPlan p;
    for (int64_t v = 0; v < n_view; ++v) {
        const int64_t first = ivl[v].first < 0 ? 0 : ivl[v].first;
        const int64_t last = ivl[v].last > n_samp ? n_samp : ivl[v].last;
        const int64_t len = last - first;
        if (len <= 0) {
            p.empty_views.push_back(v);
            continue;
        }
        if (len >= (int64_t(1) << 31)) fail_arg(std::string(what) + ": a view of 2^31 samples or more");
        BasisJob job{first, (int32_t)len, (int32_t)v, (int32_t)p.chunks.size(), (int32_t)((len + kBasisChunk - 1) / kBasisChunk)};
        for (int32_t c = 0; c < job.n_chunk; ++c) p.chunks.push_back(BasisChunk{(int32_t)p.jobs.size(), c});
        p.jobs.push_back(job);
    }
    if (p.chunks.size() > 0x7fffffffu) fail_arg(std::string(what) + ": too many chunks");
    return p;
}

void subh_check(int64_t norder, const char * what) {
    if (norder < 1 || norder > kSubhMaxTerms) {
        fail_arg(std::string(what) + ": order + 1 = " + std::to_string(norder) + " terms, 1 to " +
                 std::to_string(kSubhMaxTerms) + " are supported");
    }
}

// N = 2, 4 or 9 terms compiled; the runtime count n <= N
template <class F>
void dispatch_terms(int64_t norder, F && launch) {
    if (norder <= 2) {
        launch(std::integral_constant<int, 2>{});
    } else if (norder <= 4) {
        launch(std::integral_constant<int, 4>{});
    } else {
        launch(std::integral_constant<int, 9>{});
    }
}

// The per-detector lists of one call; a list the call does not have stays nullptr.
struct BasisRows {
    const int32_t * sig = nullptr;          // row of each detector in the signal buffer
    const int32_t * est = nullptr;          // ... in the estimate buffer
    const int32_t * flags = nullptr;        // ... in the flag buffer
    const int64_t * amp_offsets = nullptr;
    const double * weights = nullptr;
};

// One call of a kernel that walks the chunks of a view list: the stream, the plan, the device copies of the lists and the
// launches of the Legendre family.
struct BasisLaunch {
    hipStream_t st;
    int64_t n_det, n_samp, n_view;
    BasisPlan plan;
    BasisRows rows;                         // on the device, after upload()
    const BasisJob * jobs = nullptr;
    const BasisChunk * chunks = nullptr;
    std::vector<int32_t> zeros;             // storage of flag_rows()'s stand-in until upload()

    BasisLaunch(hipStream_t stream, const toast_hip_interval * ivl, int64_t n_view_, int64_t n_samp_, int64_t n_det_,
                const char * what)
        : st(stream), n_det(n_det_), n_samp(n_samp_), n_view(n_view_), plan(basis_plan(ivl, n_view_, n_samp_, what)) {}

    bool empty() const { return plan.chunks.empty(); }
    dim3 chunk_grid() const { return dim3((unsigned)plan.chunks.size(), (unsigned)n_det); }
    dim3 view_grid() const { return dim3((unsigned)plan.jobs.size(), (unsigned)n_det); }

    // the flag rows, or a stand-in when there are no flags: the kernels get a valid pointer they never follow
    const int32_t * flag_rows(const uint8_t * d_det_flags, const int32_t * flag_index) {
        if (d_det_flags != nullptr) return flag_index;
        zeros.assign((size_t)n_det, 0);
        return zeros.data();
    }

    void upload(const BasisRows & host) {
        ParamBlock pb;
        constexpr size_t none = ~size_t(0);
        auto push = [&](const auto * list) { return list != nullptr ? pb.push(list, sizeof(*list) * (size_t)n_det) : none; };
        const size_t o_si = push(host.sig), o_ei = push(host.est), o_fi = push(host.flags), o_ao = push(host.amp_offsets),
                     o_w = push(host.weights);
        const size_t o_j = pb.push_vec(plan.jobs), o_c = pb.push_vec(plan.chunks);
        const char * dp = pb.commit(st);
        auto at = [&](size_t off, auto & ptr) {
            ptr = (off != none) ? reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(dp + off) : nullptr;
        };
        at(o_si, rows.sig); at(o_ei, rows.est); at(o_fi, rows.flags); at(o_ao, rows.amp_offsets); at(o_w, rows.weights);
        at(o_j, jobs); at(o_c, chunks);
    }

    // signal += basis * amplitudes of template P
    template <class P>
    void add(int64_t norder, double * signal, const double * estimate, const double * amplitudes) {
        dispatch_terms(norder, [&](auto terms) {
            hipLaunchKernelGGL((k_legendre_add<decltype(terms)::value, P>), chunk_grid(), dim3(kThreads), 0, st, signal, n_samp,
                               rows.sig, estimate, rows.est, rows.amp_offsets, amplitudes, jobs, chunks, (int)norder);
        });
        check_launch();
    }

    // The two-pass reduction of template P.  GRAM = false: the projection of `signal` into `amplitudes`; GRAM = true: the
    // weighted Gram matrices into `gram` (and `ngood`).  A stream the pass does not have is nullptr.
    template <class P, bool GRAM>
    void reduce(int64_t norder, const double * signal, const double * estimate, const uint8_t * det_flags, uint8_t det_mask,
                double * amplitudes, double * gram, int64_t * ngood) {
        dispatch_terms(norder, [&](auto terms) {
            constexpr int N = decltype(terms)::value;
            const int64_t n_chunk = (int64_t)plan.chunks.size();
            double * partial = static_cast<double *>(Manager::get().scratch(
                Manager::kScratchTemplate, sizeof(double) * (size_t)(n_det * n_chunk * kSweepValues<N, P, GRAM>), st));
            hipLaunchKernelGGL((k_legendre_partial<N, P, GRAM>), chunk_grid(), dim3(kThreads), 0, st, signal, n_samp, rows.sig,
                               estimate, rows.est, det_flags, rows.flags, det_mask, jobs, chunks, n_chunk, partial);
            check_launch();
            hipLaunchKernelGGL((k_legendre_combine<N, P, GRAM>), view_grid(), dim3(64), 0, st, jobs, n_chunk,
                               (const double *)partial, (int)norder, n_view, rows.amp_offsets, amplitudes, rows.weights, gram,
                               ngood);
        });
        check_launch();
    }
};

inline dim3 periodic_grid(int64_t n_samp, int64_t n_det) {
    return dim3((unsigned)((n_samp + kPeriodicChunk - 1) / kPeriodicChunk), (unsigned)n_det);
}

void periodic_check(int64_t n_det, int64_t n_samp, int64_t nbins, const char * what) {
    if (n_det > 65535) fail_arg(std::string(what) + ": at most 65535 detectors per call");
    if (nbins < 1 || nbins >= (int64_t(1) << 31)) fail_arg(std::string(what) + ": the number of bins must be in [1, 2^31)");
    if ((n_samp + kPeriodicChunk - 1) / kPeriodicChunk >= (int64_t(1) << 31)) fail_arg(std::string(what) + ": too many samples");
}

}  // namespace

extern "C" {

int toast_hip_subharmonic_max_terms(void) { return kSubhMaxTerms; }
int toast_hip_periodic_lds_bins(void) { return kPeriodicLdsBins; }

int toast_hip_subharmonic_add_to_signal_dev(int64_t norder, const int64_t * amp_offsets, const double * d_amplitudes,
                                            const int32_t * data_index, int64_t n_det, double * d_det_data, int64_t n_samp,
                                            const toast_hip_interval * intervals, int64_t n_view, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "subharmonic_add_to_signal");
        if (n_det > 65535) fail_arg("subharmonic_add_to_signal: at most 65535 detectors per call");
        if ((reinterpret_cast<uintptr_t>(d_det_data) & 15) != 0) fail_arg("subharmonic_add_to_signal: the signal must be 16-byte aligned");
        BasisLaunch call(as_stream(stream), intervals, n_view, n_samp, n_det, "subharmonic_add_to_signal");
        if (call.empty()) return;
        BasisRows rows;
        rows.sig = data_index; rows.amp_offsets = amp_offsets;
        call.upload(rows);
        call.add<SubHarmonicSweep>(norder, d_det_data, nullptr, d_amplitudes);
    });
}

int toast_hip_subharmonic_project_signal_dev(int64_t norder, const int64_t * amp_offsets, double * d_amplitudes,
                                             const int32_t * data_index, int64_t n_det, const double * d_det_data,
                                             int64_t n_samp, const toast_hip_interval * intervals, int64_t n_view,
                                             void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "subharmonic_project_signal");
        if (n_det > 65535) fail_arg("subharmonic_project_signal: at most 65535 detectors per call");
        BasisLaunch call(as_stream(stream), intervals, n_view, n_samp, n_det, "subharmonic_project_signal");
        // a view without samples has no job: its amplitudes are the empty sum (np.dot of empty arrays), assigned like the rest
        for (const int64_t v : call.plan.empty_views) {
            for (int64_t d = 0; d < n_det; ++d) {
                TH_HIP(hipMemsetAsync(d_amplitudes + amp_offsets[d] + v * norder, 0, sizeof(double) * (size_t)norder, call.st));
            }
        }
        if (call.empty()) return;
        BasisRows rows;
        rows.sig = data_index; rows.amp_offsets = amp_offsets;
        call.upload(rows);
        call.reduce<SubHarmonicSweep, false>(norder, d_det_data, nullptr, nullptr, 0, d_amplitudes, nullptr, nullptr);
    });
}

int toast_hip_subharmonic_precond_build_dev(int64_t norder, const int32_t * flag_index, const uint8_t * d_det_flags,
                                            uint8_t det_flag_mask, const double * det_weights, int64_t n_det, int64_t n_samp,
                                            const toast_hip_interval * intervals, int64_t n_view, double * d_gram,
                                            int64_t * d_ngood, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "subharmonic_precond_build");
        if (n_det > 65535) fail_arg("subharmonic_precond_build: at most 65535 detectors per call");
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("subharmonic_precond_build: detector flags need their row indices");
        if (d_gram == nullptr || d_ngood == nullptr || det_weights == nullptr) fail_arg("subharmonic_precond_build: weights and outputs are required");
        hipStream_t st = as_stream(stream);
        TH_HIP(hipMemsetAsync(d_gram, 0, sizeof(double) * (size_t)(n_det * n_view * norder * norder), st));
        TH_HIP(hipMemsetAsync(d_ngood, 0, sizeof(int64_t) * (size_t)(n_det * n_view), st));     // (an empty view has no job)
        BasisLaunch call(st, intervals, n_view, n_samp, n_det, "subharmonic_precond_build");
        if (call.empty()) return;
        BasisRows rows;
        rows.flags = call.flag_rows(d_det_flags, flag_index); rows.weights = det_weights;
        call.upload(rows);
        call.reduce<SubHarmonicSweep, true>(norder, nullptr, nullptr, d_det_flags, det_flag_mask, nullptr, d_gram, d_ngood);
    });
}

int toast_hip_subharmonic_apply_precond_dev(int64_t norder, int64_t n_block, const double * d_precond, const double * d_amp_in,
                                            double * d_amp_out, void * stream) {
    return guarded([&] {
        if (n_block <= 0) return;
        subh_check(norder, "subharmonic_apply_precond");
        if (d_amp_in == d_amp_out) fail_arg("subharmonic_apply_precond: input and output must be different vectors");
        hipLaunchKernelGGL(k_subh_precond, flat_grid(n_block * norder), dim3(kThreads), 0, as_stream(stream), (int)norder,
                           n_block * norder, d_precond, d_amp_in, d_amp_out);
        check_launch();
    });
}

int toast_hip_gain_add_to_signal_dev(int64_t norder, const int64_t * amp_offsets, const double * d_amplitudes,
                                     const int32_t * data_index, double * d_det_data, const int32_t * est_index,
                                     const double * d_estimate, int64_t n_det, int64_t n_samp,
                                     const toast_hip_interval * intervals, int64_t n_view, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "gain_add_to_signal");
        if (n_det > 65535) fail_arg("gain_add_to_signal: at most 65535 detectors per call");
        if (d_det_data == nullptr || d_estimate == nullptr || d_amplitudes == nullptr) fail_arg("gain_add_to_signal: signal, estimate and amplitudes are required");
        if ((reinterpret_cast<uintptr_t>(d_det_data) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_estimate) & 7) != 0) fail_arg("gain_add_to_signal: signal and estimate must be 8-byte aligned");
        BasisLaunch call(as_stream(stream), intervals, n_view, n_samp, n_det, "gain_add_to_signal");
        if (call.empty()) return;
        BasisRows rows;
        rows.sig = data_index; rows.est = est_index; rows.amp_offsets = amp_offsets;
        call.upload(rows);
        call.add<GainSweep>(norder, d_det_data, d_estimate, d_amplitudes);
    });
}

int toast_hip_gain_project_signal_dev(int64_t norder, const int64_t * amp_offsets, double * d_amplitudes,
                                      const int32_t * data_index, const double * d_det_data, const int32_t * est_index,
                                      const double * d_estimate, const int32_t * flag_index, const uint8_t * d_det_flags,
                                      uint8_t det_flag_mask, int64_t n_det, int64_t n_samp,
                                      const toast_hip_interval * intervals, int64_t n_view, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "gain_project_signal");
        if (n_det > 65535) fail_arg("gain_project_signal: at most 65535 detectors per call");
        if (d_det_data == nullptr || d_estimate == nullptr || d_amplitudes == nullptr) fail_arg("gain_project_signal: signal, estimate and amplitudes are required");
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("gain_project_signal: detector flags need their row indices");
        // (a view without samples has no job: nothing is added to its amplitudes)
        BasisLaunch call(as_stream(stream), intervals, n_view, n_samp, n_det, "gain_project_signal");
        if (call.empty()) return;
        BasisRows rows;
        rows.sig = data_index; rows.est = est_index; rows.amp_offsets = amp_offsets;
        rows.flags = call.flag_rows(d_det_flags, flag_index);
        call.upload(rows);
        call.reduce<GainSweep, false>(norder, d_det_data, d_estimate, d_det_flags, det_flag_mask, d_amplitudes, nullptr, nullptr);
    });
}

int toast_hip_gain_precond_build_dev(int64_t norder, const int32_t * est_index, const double * d_estimate,
                                     const double * det_weights, int64_t n_det, int64_t n_samp,
                                     const toast_hip_interval * intervals, int64_t n_view, double * d_gram, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_view <= 0 || n_samp <= 0) return;
        subh_check(norder, "gain_precond_build");
        if (n_det > 65535) fail_arg("gain_precond_build: at most 65535 detectors per call");
        if (d_gram == nullptr || d_estimate == nullptr || det_weights == nullptr || est_index == nullptr) fail_arg("gain_precond_build: estimate, weights and output are required");
        hipStream_t st = as_stream(stream);
        TH_HIP(hipMemsetAsync(d_gram, 0, sizeof(double) * (size_t)(n_det * n_view * norder * norder), st));     // (an empty view has no job)
        BasisLaunch call(st, intervals, n_view, n_samp, n_det, "gain_precond_build");
        if (call.empty()) return;
        BasisRows rows;
        rows.est = est_index; rows.weights = det_weights;
        call.upload(rows);
        call.reduce<GainSweep, true>(norder, nullptr, d_estimate, nullptr, 0, nullptr, d_gram, nullptr);
    });
}

int toast_hip_periodic_index_dev(const double * d_key, const uint8_t * d_flags, uint8_t flag_mask, int64_t n_row, int64_t n_samp,
                                 double obs_min, double incr, int64_t nbins, const toast_hip_interval * intervals,
                                 int64_t n_view, int32_t * d_index, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n_samp <= 0) return;
        periodic_check(n_row, n_samp, nbins, "periodic_index");
        if (!(incr != 0.0)) fail_arg("periodic_index: the bin increment is zero");
        hipStream_t st = as_stream(stream);
        TH_HIP(hipMemsetAsync(d_index, 0xff, sizeof(int32_t) * (size_t)(n_row * n_samp), st));     // -1: no bin
        BasisLaunch call(st, intervals, n_view, n_samp, n_row, "periodic_index");
        if (call.empty()) return;
        call.upload(BasisRows{});
        hipLaunchKernelGGL(k_periodic_index, call.chunk_grid(), dim3(kThreads), 0, st, d_key, n_samp, d_flags, flag_mask, n_samp,
                           obs_min, incr, (int32_t)nbins, call.jobs, call.chunks, d_index);
        check_launch();
    });
}

int toast_hip_periodic_hits_dev(const int32_t * d_index, const int32_t * index_rows, const int32_t * flag_index,
                                const uint8_t * d_det_flags, uint8_t det_flag_mask, const int64_t * amp_offsets, int64_t n_det,
                                int64_t n_samp, int64_t nbins, int64_t first, int64_t last, int32_t * d_hits, void * stream) {
    return guarded([&] {
        if (first < 0) first = 0;
        if (last > n_samp) last = n_samp;
        if (n_det <= 0 || last <= first) return;
        periodic_check(n_det, n_samp, nbins, "periodic_hits");
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("periodic_hits: detector flags need their row indices");
        hipStream_t st = as_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> zeros(n_det, 0);
        const size_t o_ir = pb.push(index_rows != nullptr ? index_rows : zeros.data(), sizeof(int32_t) * n_det);
        const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : zeros.data(), sizeof(int32_t) * n_det);
        const size_t o_ao = pb.push(amp_offsets, sizeof(int64_t) * n_det);
        const char * dp = pb.commit(st);
        hipLaunchKernelGGL(k_periodic_hits, periodic_grid(last - first, n_det), dim3(kThreads), 0, st, d_index,
                           index_rows != nullptr ? (const int32_t *)(dp + o_ir) : (const int32_t *)nullptr, n_samp, d_det_flags,
                           (const int32_t *)(dp + o_fi), det_flag_mask, (const int64_t *)(dp + o_ao), (int32_t)nbins, first, last,
                           d_hits);
        check_launch();
    });
}

int toast_hip_periodic_add_to_signal_dev(const int32_t * d_index, const int32_t * index_rows, const int64_t * amp_offsets,
                                         const double * d_amplitudes, const int32_t * data_index, int64_t n_det,
                                         double * d_det_data, int64_t n_samp, int64_t nbins, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_samp <= 0) return;
        periodic_check(n_det, n_samp, nbins, "periodic_add_to_signal");
        hipStream_t st = as_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> zeros(n_det, 0);
        const size_t o_ir = pb.push(index_rows != nullptr ? index_rows : zeros.data(), sizeof(int32_t) * n_det);
        const size_t o_si = pb.push(data_index, sizeof(int32_t) * n_det);
        const size_t o_ao = pb.push(amp_offsets, sizeof(int64_t) * n_det);
        const char * dp = pb.commit(st);
        hipLaunchKernelGGL(k_periodic_add, periodic_grid(n_samp, n_det), dim3(kThreads), 0, st, d_index,
                           index_rows != nullptr ? (const int32_t *)(dp + o_ir) : (const int32_t *)nullptr, n_samp,
                           (const int64_t *)(dp + o_ao), d_amplitudes, (const int32_t *)(dp + o_si), d_det_data,
                           (int32_t)nbins);
        check_launch();
    });
}

int toast_hip_periodic_project_signal_dev(const int32_t * d_index, const int32_t * index_rows, const int32_t * data_index,
                                          const double * d_det_data, const int32_t * flag_index, const uint8_t * d_det_flags,
                                          uint8_t det_flag_mask, const int64_t * amp_offsets, double * d_amplitudes,
                                          int64_t n_det, int64_t n_samp, int64_t nbins, int path, void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_samp <= 0) return;
        periodic_check(n_det, n_samp, nbins, "periodic_project_signal");
        if (path < 0 || path > 2) fail_arg("periodic_project_signal: path must be 0 (by the rule), 1 (LDS copies) or 2 (global atomics)");
        if (path == 1 && nbins > kPeriodicLdsBins) {
            fail_arg("periodic_project_signal: the LDS path holds at most " + std::to_string(kPeriodicLdsBins) + " bins, asked for " +
                     std::to_string(nbins));
        }
        if (d_det_flags != nullptr && flag_index == nullptr) fail_arg("periodic_project_signal: detector flags need their row indices");
        hipStream_t st = as_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> zeros(n_det, 0);
        const size_t o_ir = pb.push(index_rows != nullptr ? index_rows : zeros.data(), sizeof(int32_t) * n_det);
        const size_t o_si = pb.push(data_index, sizeof(int32_t) * n_det);
        const size_t o_fi = pb.push(d_det_flags != nullptr ? flag_index : zeros.data(), sizeof(int32_t) * n_det);
        const size_t o_ao = pb.push(amp_offsets, sizeof(int64_t) * n_det);
        const char * dp = pb.commit(st);
        const int32_t * irows = index_rows != nullptr ? (const int32_t *)(dp + o_ir) : (const int32_t *)nullptr;
        const dim3 grid = periodic_grid(n_samp, n_det);
        const bool lds = (path == 1) || (path == 0 && nbins <= kPeriodicLdsBins);
        if (lds) {
            const int64_t n_chunk = grid.x;
            double * partial = static_cast<double *>(
                Manager::get().scratch(Manager::kScratchTemplate, sizeof(double) * (size_t)(n_det * n_chunk * nbins), st));
            hipLaunchKernelGGL(k_periodic_partial, grid, dim3(kThreads), sizeof(double) * 4 * (size_t)nbins, st, d_index, irows,
                               n_samp, (const int32_t *)(dp + o_si), d_det_data, d_det_flags, (const int32_t *)(dp + o_fi),
                               det_flag_mask, (int32_t)nbins, partial);
            check_launch();
            hipLaunchKernelGGL(k_periodic_combine, dim3((unsigned)((nbins + kThreads - 1) / kThreads), (unsigned)n_det),
                               dim3(kThreads), 0, st, (const double *)partial, n_chunk, (int32_t)nbins,
                               (const int64_t *)(dp + o_ao), d_amplitudes);
        } else {
            hipLaunchKernelGGL(k_periodic_atomic, grid, dim3(kThreads), 0, st, d_index, irows, n_samp,
                               (const int32_t *)(dp + o_si), d_det_data, d_det_flags, (const int32_t *)(dp + o_fi), det_flag_mask,
                               (const int64_t *)(dp + o_ao), (int32_t)nbins, d_amplitudes);
        }
        check_launch();
    });
}

int toast_hip_periodic_apply_precond_dev(int64_t n_amp, const int32_t * d_hits, const uint8_t * d_amp_flags,
                                         const double * d_amp_in, double * d_amp_out, void * stream) {
    return guarded([&] {
        if (n_amp <= 0) return;
        hipLaunchKernelGGL(k_periodic_precond, flat_grid(n_amp), dim3(kThreads), 0, as_stream(stream), n_amp, d_hits, d_amp_flags,
                           d_amp_in, d_amp_out);
        check_launch();
    });
}

}  // extern "C"
