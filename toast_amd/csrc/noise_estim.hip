// noise_estim.hip -- noise estimation from lagged covariance sums on gfx950.
//
// Counterpart of the reference's
//   * fod_autosums / fod_crosssums (src/libtoast/src/toast_fod_psd.cpp:12-93) -- host entries with the same sequential
//     loops (bit-identical sums) and a batched device entry,
//   * highpass_flagged_signal / flagged_running_average (src/toast/ops/noise_estimation_utils.py:13-101) -- a host
//     entry and a device entry,
// and the small device helpers of ops.NoiseEstim (the pair's good mask, strided decimation).
//
// Lagged sums on the device, per batch of pairs:
//   k_fod_partial   a workgroup owns (pair, chunk of 8192 samples of one segment, tile of 2048 lags).  It stages 1024
//                   samples of x and the matching 1024 + 2048 samples of y in LDS at a time; flagged samples, samples
//                   past the segment's end and (all_sums = 0) the x samples of the last lagmax are staged as zero, so
//                   the inner loop has no branch.  Every lane owns 8 consecutive lags in registers: x[i] is wave-uniform,
//                   the lane's window over y slides by one 8-byte LDS read per 8 FMAs (y is padded by one double per
//                   eight so that the 64-byte lane stride is free of bank conflicts).  The chunk's sums are written to
//                   scratch -- no atomics.
//   k_fod_reduce    the chunk sums of a (pair, realization, lag) are added in chunk order and accumulated into d_sums.
//   k_fod_pack / k_fod_hits   good flags packed into 64-bit words; hits[lag] = sum popcount(gx & (g >> lag)).
// Chunks are cut relative to their segment, so neither the batch size nor the order of the pairs changes one bit.
//
// High-pass on the device: sums of 64 and of 4096 samples in double-double (TwoSum), then every output adds the at
// most 4 x 63 + n / 4096 pieces that tile its window, also in double-double: the window sum carries one rounding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "runtime.hpp"

using namespace toast_hip;

namespace {

constexpr int kThreads = 256;
constexpr int kR = 8;                            // lags per lane
constexpr int kLagTile = kThreads * kR;          // lags per workgroup
constexpr int kStage = 1024;                     // x samples staged at a time
constexpr int kSumChunk = 8192;                  // samples per partial sum: part of the result's definition
constexpr int kYLen = kStage + kLagTile;         // y samples staged at a time
constexpr int kYPad = kYLen + kYLen / 8;
constexpr int kB1 = 64, kB2 = 4096;              // high-pass block sizes
constexpr int64_t kMaxGridY = 65535;

int g_timing = 0;                                // toast_hip_noise_estim_timing
double g_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};     // high-pass, sums, reduction, download

struct PhaseTimer {
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    explicit PhaseTimer(hipStream_t s) : st(s) {
        if (!g_timing) return;
        TH_HIP(hipEventCreate(&a));
        TH_HIP(hipEventCreate(&b));
        TH_HIP(hipEventRecord(a, st));
    }
    void stop(int phase) {
        if (!g_timing) return;
        TH_HIP(hipEventRecord(b, st));
        TH_HIP(hipEventSynchronize(b));
        float ms = 0.0f;
        TH_HIP(hipEventElapsedTime(&ms, a, b));
        g_phase_ms[phase] += (double)ms;
        TH_HIP(hipEventRecord(a, st));
    }
    ~PhaseTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// ------------------------------------------------------------------------------------ lagged sums
struct SumsArgs {
    const double * data;          // [row][stride]
    int64_t stride;
    const uint8_t * good;         // [row][good_stride], non-zero = use
    int64_t good_stride;
    const int32_t * row1;         // [n_pair]
    const int32_t * row2;
    const int32_t * good_row;
    const int64_t * seg_first;    // [n_seg], sorted by realization
    const int64_t * seg_len;
    const int32_t * seg_all;
    const int32_t * seg_real;
    const int64_t * seg_word;     // first packed word of the segment
    const int32_t * chunk_seg;    // [n_chunk]
    const int64_t * chunk_off;    // first sample of the chunk inside its segment
    const int32_t * real_chunk;   // [n_real + 1] chunks of a realization
    int64_t lagmax;
    int n_seg;
    int n_chunk;
    int n_real;
    int n_tile;
    int symmetric;
    int64_t n_word;               // packed words per pair
    double * partial;             // [batch pair][chunk][lagmax]
    uint64_t * bits;              // [batch pair][2][n_word]: x mask, y mask
};

__device__ __forceinline__ int ypad(int k) { return k + (k >> 3); }

__global__ __launch_bounds__(kThreads) void k_fod_partial(SumsArgs a, int pair0) {
    __shared__ double xs[kStage];
    __shared__ double ys[kYPad];
    const int p = pair0 + (int)blockIdx.y;
    const int c = (int)(blockIdx.x / a.n_tile), tile = (int)(blockIdx.x % a.n_tile);
    const int seg = a.chunk_seg[c];
    const int64_t first = a.seg_first[seg], n = a.seg_len[seg];
    const int64_t c0 = a.chunk_off[c];
    const int64_t cend = min(c0 + (int64_t)kSumChunk, n);
    // x[i] takes part for i < xcut: with all_sums the end of the segment (y is zero past it, i.e. i < n - lag); without,
    // the last lagmax samples are left to the neighbour
    const int64_t xcut = a.seg_all[seg] ? n : n - a.lagmax;
    const int r1 = a.row1[p], r2 = a.row2[p];
    const uint8_t * g = a.good + (int64_t)a.good_row[p] * a.good_stride + first;
    const int64_t l0 = (int64_t)tile * kLagTile;
    const int base = (int)threadIdx.x * kR;
    double acc[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = 0.0;
    const int n_pass = (a.symmetric && r1 != r2) ? 2 : 1;
    for (int pass = 0; pass < n_pass; ++pass) {
        const double * X = a.data + (int64_t)(pass == 0 ? r1 : r2) * a.stride + first;
        const double * Y = a.data + (int64_t)(pass == 0 ? r2 : r1) * a.stride + first;
        const double keep0 = acc[0];
        for (int64_t s0 = c0; s0 < cend; s0 += kStage) {
            __syncthreads();
            for (int k = (int)threadIdx.x; k < kStage; k += kThreads) {
                const int64_t i = s0 + k;
                xs[k] = (i < xcut && g[i] != 0) ? X[i] : 0.0;
            }
            for (int k = (int)threadIdx.x; k < kYLen; k += kThreads) {
                const int64_t j = s0 + l0 + k;
                ys[ypad(k)] = (j < n && g[j] != 0) ? Y[j] : 0.0;
            }
            __syncthreads();
            // w[(u + r) % kR] holds y[i + u + base + r]: the window slides without moving a register
            double w[kR];
#pragma unroll
            for (int r = 0; r < kR - 1; ++r) w[r] = ys[ypad(base + r)];
            for (int i = 0; i < kStage; i += kR) {
#pragma unroll
                for (int u = 0; u < kR; ++u) {
                    w[(u + kR - 1) % kR] = ys[ypad(i + u + base + kR - 1)];
                    const double xi = xs[i + u];
#pragma unroll
                    for (int r = 0; r < kR; ++r) acc[r] = __builtin_fma(xi, w[(u + r) % kR], acc[r]);
                }
            }
        }
        // the swapped products double the statistics of every lag except 0 (toast_fod_psd.cpp:81-87)
        if (pass == 1 && l0 + base == 0) acc[0] = keep0;
    }
    double * out = a.partial + ((int64_t)blockIdx.y * a.n_chunk + c) * a.lagmax;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        const int64_t lag = l0 + base + r;
        if (lag < a.lagmax) out[lag] = acc[r];
    }
}

__global__ __launch_bounds__(kThreads) void k_fod_reduce(SumsArgs a, int pair0, double * __restrict__ sums) {
    const int64_t lag = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (lag >= a.lagmax) return;
    const int b = (int)blockIdx.y;
    for (int r = 0; r < a.n_real; ++r) {
        const int c0 = a.real_chunk[r], c1 = a.real_chunk[r + 1];
        if (c0 == c1) continue;
        double s = 0.0;
        for (int c = c0; c < c1; ++c) s += a.partial[((int64_t)b * a.n_chunk + c) * a.lagmax + lag];
        sums[((int64_t)(pair0 + b) * a.n_real + r) * a.lagmax + lag] += s;
    }
}

__global__ __launch_bounds__(kThreads) void k_fod_pack(SumsArgs a, int pair0) {
    const int64_t w = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (w >= a.n_word) return;
    int lo = 0, hi = a.n_seg - 1;       // the segment that holds word w
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg_word[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int seg = lo;
    const int64_t first = a.seg_first[seg], n = a.seg_len[seg];
    const int64_t xcut = a.seg_all[seg] ? n : n - a.lagmax;
    const int p = pair0 + (int)blockIdx.y;
    const uint8_t * g = a.good + (int64_t)a.good_row[p] * a.good_stride + first;
    const int64_t i0 = (w - a.seg_word[seg]) * 64;
    uint64_t bx = 0, by = 0;
    for (int t = 0; t < 64; ++t) {
        const int64_t i = i0 + t;
        if (i < n && g[i] != 0) {
            by |= 1ull << t;
            if (i < xcut) bx |= 1ull << t;
        }
    }
    uint64_t * out = a.bits + (int64_t)blockIdx.y * 2 * a.n_word;
    out[w] = bx;
    out[a.n_word + w] = by;
}

__global__ __launch_bounds__(kThreads) void k_fod_hits(SumsArgs a, int pair0, int64_t * __restrict__ hits) {
    const int64_t lag = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (lag >= a.lagmax) return;
    const int b = (int)blockIdx.y, p = pair0 + b;
    const uint64_t * bx = a.bits + (int64_t)b * 2 * a.n_word;
    const uint64_t * by = bx + a.n_word;
    const int64_t q = lag >> 6;
    const int sft = (int)(lag & 63);
    const int64_t twice = (a.symmetric && a.row1[p] != a.row2[p] && lag != 0) ? 2 : 1;
    for (int seg = 0; seg < a.n_seg; ++seg) {
        const int64_t w0 = a.seg_word[seg], nw = (a.seg_len[seg] + 63) >> 6;
        int64_t count = 0;
        if (q < nw) {
            uint64_t lo = by[w0 + q];
            for (int64_t w = 0; w + q < nw; ++w) {
                const uint64_t hi = (w + q + 1 < nw) ? by[w0 + w + q + 1] : 0ull;
                const uint64_t shifted = sft ? ((lo >> sft) | (hi << (64 - sft))) : lo;
                count += __popcll(bx[w0 + w] & shifted);
                lo = hi;
            }
        }
        hits[((int64_t)p * a.n_real + a.seg_real[seg]) * a.lagmax + lag] += twice * count;
    }
}

// the register-only loop of k_fod_partial in the same launch shape: what the FP64 FMA pipes give this kernel at most
__global__ __launch_bounds__(kThreads) void k_fma_ceiling(int iterations, double seed, double * __restrict__ out) {
    double acc[kR], w[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        acc[r] = 0.0;
        w[r] = seed * (double)(threadIdx.x + r + 1);
    }
    double xi = seed;
    for (int i = 0; i < iterations; i += kR) {
#pragma unroll
        for (int u = 0; u < kR; ++u) {
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = __builtin_fma(xi, w[(u + r) % kR], acc[r]);
        }
        xi = -xi;
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < kR; ++r) s += acc[r];
    if (s == 12345.678) out[blockIdx.x] = s;      // never true for the seeds used: keeps the loop alive
}

// ------------------------------------------------------------------------------------ high-pass
struct DD {
    double hi, lo;
};
// s + v, error-free (Knuth's TwoSum; the library is built without contraction or reassociation)
__host__ __device__ __forceinline__ void dd_add(DD & s, double v) {
    const double t = s.hi + v;
    const double bb = t - s.hi;
    const double err = (s.hi - (t - bb)) + (v - bb);
    s.hi = t;
    s.lo += err;
}
__host__ __device__ __forceinline__ void dd_add(DD & s, const DD & v) {
    dd_add(s, v.hi);
    s.lo += v.lo;
}

struct HpArgs {
    const double * in;            // [row][in_stride]
    int64_t in_stride;
    const int32_t * in_row;       // [n_row]
    const uint8_t * good;
    int64_t good_stride;
    const int32_t * good_row;     // [n_row]
    int64_t n;
    int64_t window;
    int64_t nb1, nb2;
    DD * sum1;                    // [n_row][nb1]
    int32_t * cnt1;
    DD * sum2;                    // [n_row][nb2]
    int32_t * cnt2;
    double * out;                 // [n_row][out_stride]
    int64_t out_stride;
};

__global__ __launch_bounds__(kThreads) void k_hp_level1(HpArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= a.nb1) return;
    const int row = (int)blockIdx.y;
    const double * x = a.in + (int64_t)a.in_row[row] * a.in_stride;
    const uint8_t * g = a.good + (int64_t)a.good_row[row] * a.good_stride;
    DD s{0.0, 0.0};
    int cnt = 0;
    const int64_t i1 = min((b + 1) * kB1, a.n);
    for (int64_t i = b * kB1; i < i1; ++i) {
        if (g[i] != 0) {
            dd_add(s, x[i]);
            ++cnt;
        }
    }
    a.sum1[(int64_t)row * a.nb1 + b] = s;
    a.cnt1[(int64_t)row * a.nb1 + b] = cnt;
}

__global__ __launch_bounds__(kThreads) void k_hp_level2(HpArgs a) {
    const int64_t b = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= a.nb2) return;
    const int row = (int)blockIdx.y;
    DD s{0.0, 0.0};
    int cnt = 0;
    const int64_t k1 = min((b + 1) * (kB2 / kB1), a.nb1);
    for (int64_t k = b * (kB2 / kB1); k < k1; ++k) {
        dd_add(s, a.sum1[(int64_t)row * a.nb1 + k]);
        cnt += a.cnt1[(int64_t)row * a.nb1 + k];
    }
    a.sum2[(int64_t)row * a.nb2 + b] = s;
    a.cnt2[(int64_t)row * a.nb2 + b] = cnt;
}

__global__ __launch_bounds__(kThreads) void k_hp_out(HpArgs a) {
    __shared__ int64_t total;
    const int row = (int)blockIdx.y;
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int64_t b = 0; b < a.nb2; ++b) t += a.cnt2[(int64_t)row * a.nb2 + b];
        total = t;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const double * x = a.in + (int64_t)a.in_row[row] * a.in_stride;
    const uint8_t * g = a.good + (int64_t)a.good_row[row] * a.good_stride;
    double * out = a.out + (int64_t)row * a.out_stride;
    if (total == 0) {          // no valid samples: zeros (noise_estimation_utils.py:82-85)
        out[i] = 0.0;
        return;
    }
    // the window of fftconvolve(..., ones(w), mode="same"), clipped to the row
    int64_t lo = max((int64_t)0, i - a.window / 2);
    const int64_t hi = min(a.n, i + (a.window - 1) / 2 + 1);
    const DD * s1 = a.sum1 + (int64_t)row * a.nb1;
    const int32_t * c1 = a.cnt1 + (int64_t)row * a.nb1;
    const DD * s2 = a.sum2 + (int64_t)row * a.nb2;
    const int32_t * c2 = a.cnt2 + (int64_t)row * a.nb2;
    DD s{0.0, 0.0};
    int64_t cnt = 0;
    while (lo < hi) {
        if (lo % kB2 == 0 && lo + kB2 <= hi) {
            dd_add(s, s2[lo / kB2]);
            cnt += c2[lo / kB2];
            lo += kB2;
        } else if (lo % kB1 == 0 && lo + kB1 <= hi) {
            dd_add(s, s1[lo / kB1]);
            cnt += c1[lo / kB1];
            lo += kB1;
        } else {
            if (g[lo] != 0) {
                dd_add(s, x[lo]);
                ++cnt;
            }
            ++lo;
        }
    }
    const double trend = (cnt > 0) ? (s.hi + s.lo) / (double)cnt : 0.0;
    out[i] = x[i] - trend;
}

// ------------------------------------------------------------------------------------ helpers
__global__ __launch_bounds__(kThreads) void k_pair_good(int64_t n, const uint8_t * __restrict__ shared, uint8_t shared_mask,
                                                        const uint8_t * __restrict__ flags, int64_t flag_stride,
                                                        uint8_t det_mask, const int32_t * __restrict__ row1,
                                                        const int32_t * __restrict__ row2, uint8_t * __restrict__ good,
                                                        int64_t good_stride) {
    const int p = (int)blockIdx.y;
    const int r1 = row1[p], r2 = row2[p];
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        uint8_t bad = shared ? (uint8_t)(shared[i] & shared_mask) : (uint8_t)0;
        if (flags) bad |= (uint8_t)((flags[(int64_t)r1 * flag_stride + i] | flags[(int64_t)r2 * flag_stride + i]) & det_mask);
        good[(int64_t)p * good_stride + i] = bad ? 0 : 1;
    }
}

__global__ __launch_bounds__(kThreads) void k_decimate(int64_t n_out, int64_t step, const double * __restrict__ in,
                                                       int64_t in_stride, const uint8_t * __restrict__ good,
                                                       int64_t good_stride, const int32_t * __restrict__ good_row,
                                                       double * __restrict__ out, int64_t out_stride) {
    const int row = (int)blockIdx.y;
    const uint8_t * g = good + (int64_t)good_row[row] * good_stride;
    for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < n_out; k += (int64_t)gridDim.x * kThreads) {
        // flagged samples were set to zero before the decimation (noise_estimation_utils.py:318-320)
        out[(int64_t)row * out_stride + k] = g[k * step] != 0 ? in[(int64_t)row * in_stride + k * step] : 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void k_decimate_good(int64_t n_out, int64_t step, const uint8_t * __restrict__ in,
                                                            int64_t in_stride, uint8_t * __restrict__ out,
                                                            int64_t out_stride) {
    const int row = (int)blockIdx.y;
    for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < n_out; k += (int64_t)gridDim.x * kThreads) {
        out[(int64_t)row * out_stride + k] = in[(int64_t)row * in_stride + k * step];
    }
}

unsigned grid_x(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 1 << 20)); }

hipStream_t pick_stream(void * stream) {
    Manager::get().require_device();
    return stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
}

void check_batch(int64_t n, const char * what) {
    if (n > kMaxGridY) fail_arg(std::string(what) + ": more than 65535 rows in one call");
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- host entries
int toast_hip_fod_autosums(int64_t n, const double * x, const uint8_t * good, int64_t lagmax, double * sums,
                           int64_t * hits, int64_t all_sums) {
    return guarded([&] {
        if (n < 0 || lagmax < 0) fail_arg("fod_autosums: negative size");
        std::vector<double> xgood((size_t)n);
        std::vector<uint8_t> gd((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const bool use = good[i] != 0;
            xgood[(size_t)i] = use ? x[i] : 0.0;
            gd[(size_t)i] = use ? 1 : 0;
        }
        for (int64_t lag = 0; lag < lagmax; ++lag) {
            double lagsum = 0.0;
            int64_t hitsum = 0;
            const int64_t imax = all_sums ? n - lag : n - lagmax;
            for (int64_t i = 0, j = lag; i < imax; ++i, ++j) {
                lagsum += xgood[(size_t)i] * xgood[(size_t)j];
                hitsum += gd[(size_t)i] * gd[(size_t)j];
            }
            sums[lag] += lagsum;
            hits[lag] += hitsum;
        }
    });
}

int toast_hip_fod_crosssums(int64_t n, const double * x, const double * y, const uint8_t * good, int64_t lagmax,
                            double * sums, int64_t * hits, int64_t all_sums, int64_t symmetric) {
    return guarded([&] {
        if (n < 0 || lagmax < 0) fail_arg("fod_crosssums: negative size");
        std::vector<double> xgood((size_t)n), ygood((size_t)n);
        std::vector<uint8_t> gd((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const bool use = good[i] != 0;
            xgood[(size_t)i] = use ? x[i] : 0.0;
            ygood[(size_t)i] = use ? y[i] : 0.0;
            gd[(size_t)i] = use ? 1 : 0;
        }
        for (int64_t lag = 0; lag < lagmax; ++lag) {
            double lagsum = 0.0;
            int64_t hitsum = 0;
            const int64_t imax = all_sums ? n - lag : n - lagmax;
            for (int64_t i = 0, j = lag; i < imax; ++i, ++j) {
                lagsum += xgood[(size_t)i] * ygood[(size_t)j];
                hitsum += gd[(size_t)i] * gd[(size_t)j];
            }
            if (symmetric && lag != 0) {
                for (int64_t i = 0, j = lag; i < imax; ++i, ++j) lagsum += xgood[(size_t)j] * ygood[(size_t)i];
                hitsum *= 2;
            }
            sums[lag] += lagsum;
            hits[lag] += hitsum;
        }
    });
}

int toast_hip_flagged_running_average(int64_t n, const double * signal, const uint8_t * bad, int64_t window,
                                      double * average, int64_t * hits) {
    return guarded([&] {
        if (n < 0 || window < 1) fail_arg("flagged_running_average: the window must be at least one sample");
        // a sliding window sum in extended precision, started afresh every 1024 samples
        long double s = 0.0L;
        int64_t cnt = 0, lo = 0, hi = 0;       // the sum holds [lo, hi)
        for (int64_t i = 0; i < n; ++i) {
            const int64_t want_lo = std::max<int64_t>(0, i - window / 2);
            const int64_t want_hi = std::min(n, i + (window - 1) / 2 + 1);
            if (i % 1024 == 0) {
                s = 0.0L;
                cnt = 0;
                lo = hi = want_lo;
            }
            for (; hi < want_hi; ++hi) {
                if (!bad[hi]) {
                    s += (long double)signal[hi];
                    ++cnt;
                }
            }
            for (; lo < want_lo; ++lo) {
                if (!bad[lo]) {
                    s -= (long double)signal[lo];
                    --cnt;
                }
            }
            average[i] = cnt > 0 ? (double)(s / (long double)cnt) : 0.0;
            if (hits != nullptr) hits[i] = cnt;
        }
    });
}

// ---------------------------------------------------------------------------------- device entries
int toast_hip_fod_sums_dev(int64_t n_pair, const int32_t * row1, const int32_t * row2, const int32_t * good_row,
                           const double * d_data, int64_t n_rows, int64_t stride, const uint8_t * d_good,
                           int64_t n_good_rows, int64_t good_stride, int64_t n_seg, const int64_t * seg_first,
                           const int64_t * seg_last, const int32_t * seg_all_sums, const int32_t * seg_realization,
                           int64_t n_real, int64_t lagmax, int symmetric, double * d_sums, int64_t * d_hits,
                           int64_t max_batch, void * stream) {
    return guarded([&] {
        if (n_pair <= 0 || n_seg <= 0 || lagmax <= 0) return;
        if (!row1 || !row2 || !good_row || !d_data || !d_good || !seg_first || !seg_last || !seg_all_sums ||
            !seg_realization || !d_sums || !d_hits) fail_arg("fod_sums: missing argument");
        if (n_real <= 0) fail_arg("fod_sums: no realization");
        for (int64_t p = 0; p < n_pair; ++p) {
            if (row1[p] < 0 || row1[p] >= n_rows || row2[p] < 0 || row2[p] >= n_rows) fail_arg("fod_sums: a pair names a row outside the data");
            if (good_row[p] < 0 || good_row[p] >= n_good_rows) fail_arg("fod_sums: a pair names a row outside the flags");
        }
        // segments in the order of their realization (stable): the chunks of a realization are contiguous
        std::vector<int> order;
        for (int64_t s = 0; s < n_seg; ++s) {
            if (seg_first[s] < 0 || seg_last[s] < seg_first[s] || seg_last[s] > stride || seg_last[s] > good_stride) {
                fail_arg("fod_sums: a segment lies outside the rows");
            }
            if (seg_realization[s] < 0 || seg_realization[s] >= n_real) fail_arg("fod_sums: a segment names a realization outside the output");
            if (seg_last[s] > seg_first[s]) order.push_back((int)s);
        }
        if (order.empty()) return;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return seg_realization[a] < seg_realization[b]; });
        std::vector<int64_t> s_first, s_len, s_word, c_off;
        std::vector<int32_t> s_all, s_real, c_seg, real_chunk((size_t)n_real + 1, 0);
        int64_t n_word = 0;
        for (int s : order) {
            const int64_t len = seg_last[s] - seg_first[s];
            const int32_t seg = (int32_t)s_first.size();
            s_first.push_back(seg_first[s]);
            s_len.push_back(len);
            s_all.push_back(seg_all_sums[s] ? 1 : 0);
            s_real.push_back(seg_realization[s]);
            s_word.push_back(n_word);
            n_word += (len + 63) / 64;
            for (int64_t c0 = 0; c0 < len; c0 += kSumChunk) {
                c_seg.push_back(seg);
                c_off.push_back(c0);
                real_chunk[(size_t)seg_realization[s] + 1] += 1;
            }
        }
        for (int64_t r = 0; r < n_real; ++r) real_chunk[(size_t)r + 1] += real_chunk[(size_t)r];
        const int64_t n_chunk = (int64_t)c_seg.size();
        const int64_t n_tile = (lagmax + kLagTile - 1) / kLagTile;
        if (n_chunk * n_tile > 0x7fffffff) fail_arg("fod_sums: too many chunks for one launch");

        hipStream_t st = pick_stream(stream);
        // scratch per pair: the chunk sums and the packed flags; a batch is bounded by 1 GB
        const size_t per_pair = (size_t)n_chunk * (size_t)lagmax * sizeof(double) + (size_t)n_word * 2 * sizeof(uint64_t);
        int64_t batch = (int64_t)std::max<size_t>(1, (size_t(1) << 30) / per_pair);
        if (max_batch > 0) batch = std::min(batch, max_batch);
        batch = std::min(std::min(batch, n_pair), kMaxGridY);
        char * scratch = (char *)Manager::get().scratch(Manager::kScratchNoiseEstim, (size_t)batch * per_pair, st);

        ParamBlock pb;
        std::vector<int32_t> v1(row1, row1 + n_pair), v2(row2, row2 + n_pair), vg(good_row, good_row + n_pair);
        const size_t o1 = pb.push_vec(v1), o2 = pb.push_vec(v2), o3 = pb.push_vec(vg);
        const size_t o4 = pb.push_vec(s_first), o5 = pb.push_vec(s_len), o6 = pb.push_vec(s_all), o7 = pb.push_vec(s_real);
        const size_t o8 = pb.push_vec(s_word), o9 = pb.push_vec(c_seg), o10 = pb.push_vec(c_off), o11 = pb.push_vec(real_chunk);
        const char * d = pb.commit(st);
        SumsArgs a;
        a.data = d_data;
        a.stride = stride;
        a.good = d_good;
        a.good_stride = good_stride;
        a.row1 = (const int32_t *)(d + o1);
        a.row2 = (const int32_t *)(d + o2);
        a.good_row = (const int32_t *)(d + o3);
        a.seg_first = (const int64_t *)(d + o4);
        a.seg_len = (const int64_t *)(d + o5);
        a.seg_all = (const int32_t *)(d + o6);
        a.seg_real = (const int32_t *)(d + o7);
        a.seg_word = (const int64_t *)(d + o8);
        a.chunk_seg = (const int32_t *)(d + o9);
        a.chunk_off = (const int64_t *)(d + o10);
        a.real_chunk = (const int32_t *)(d + o11);
        a.lagmax = lagmax;
        a.n_seg = (int)s_first.size();
        a.n_chunk = (int)n_chunk;
        a.n_real = (int)n_real;
        a.n_tile = (int)n_tile;
        a.symmetric = symmetric ? 1 : 0;
        a.n_word = n_word;
        a.partial = (double *)scratch;
        a.bits = (uint64_t *)(scratch + (size_t)batch * (size_t)n_chunk * (size_t)lagmax * sizeof(double));

        PhaseTimer timer(st);
        const unsigned gx_lag = (unsigned)((lagmax + kThreads - 1) / kThreads);
        const unsigned gx_word = (unsigned)((n_word + kThreads - 1) / kThreads);
        for (int64_t p0 = 0; p0 < n_pair; p0 += batch) {
            const unsigned nb = (unsigned)std::min(batch, n_pair - p0);
            hipLaunchKernelGGL(k_fod_partial, dim3((unsigned)(n_chunk * n_tile), nb), dim3(kThreads), 0, st, a, (int)p0);
            hipLaunchKernelGGL(k_fod_pack, dim3(gx_word, nb), dim3(kThreads), 0, st, a, (int)p0);
            hipLaunchKernelGGL(k_fod_hits, dim3(gx_lag, nb), dim3(kThreads), 0, st, a, (int)p0, d_hits);
            timer.stop(1);
            hipLaunchKernelGGL(k_fod_reduce, dim3(gx_lag, nb), dim3(kThreads), 0, st, a, (int)p0, d_sums);
            timer.stop(2);
            TH_HIP(hipGetLastError());
        }
    });
}

int toast_hip_noise_estim_highpass_dev(int64_t n_row, int64_t n, int64_t window, const double * d_in, int64_t n_in_rows,
                                       int64_t in_stride, const int32_t * in_row, const uint8_t * d_good,
                                       int64_t n_good_rows, int64_t good_stride, const int32_t * good_row,
                                       double * d_out, int64_t out_stride, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n <= 0) return;
        if (!d_in || !in_row || !d_good || !good_row || !d_out) fail_arg("noise_estim_highpass: missing argument");
        if (window < 1) fail_arg("noise_estim_highpass: the window must be at least one sample");
        if (n > in_stride || n > good_stride || n > out_stride) fail_arg("noise_estim_highpass: rows are shorter than n");
        check_batch(n_row, "noise_estim_highpass");
        for (int64_t r = 0; r < n_row; ++r) {
            if (in_row[r] < 0 || in_row[r] >= n_in_rows) fail_arg("noise_estim_highpass: a row lies outside the data");
            if (good_row[r] < 0 || good_row[r] >= n_good_rows) fail_arg("noise_estim_highpass: a row lies outside the flags");
        }
        hipStream_t st = pick_stream(stream);
        HpArgs a;
        a.nb1 = (n + kB1 - 1) / kB1;
        a.nb2 = (n + kB2 - 1) / kB2;
        const size_t b1 = (size_t)n_row * (size_t)a.nb1, b2 = (size_t)n_row * (size_t)a.nb2;
        char * scratch = (char *)Manager::get().scratch(Manager::kScratchNoiseEstimHp,
                                                         (b1 + b2) * (sizeof(DD) + sizeof(int32_t)) + 64, st);
        a.sum1 = (DD *)scratch;
        a.sum2 = a.sum1 + b1;
        a.cnt1 = (int32_t *)(a.sum2 + b2);
        a.cnt2 = a.cnt1 + b1;
        ParamBlock pb;
        std::vector<int32_t> vi(in_row, in_row + n_row), vg(good_row, good_row + n_row);
        const size_t o1 = pb.push_vec(vi), o2 = pb.push_vec(vg);
        const char * d = pb.commit(st);
        a.in = d_in;
        a.in_stride = in_stride;
        a.in_row = (const int32_t *)(d + o1);
        a.good = d_good;
        a.good_stride = good_stride;
        a.good_row = (const int32_t *)(d + o2);
        a.n = n;
        a.window = window;
        a.out = d_out;
        a.out_stride = out_stride;
        PhaseTimer timer(st);
        hipLaunchKernelGGL(k_hp_level1, dim3((unsigned)((a.nb1 + kThreads - 1) / kThreads), (unsigned)n_row), dim3(kThreads), 0, st, a);
        hipLaunchKernelGGL(k_hp_level2, dim3((unsigned)((a.nb2 + kThreads - 1) / kThreads), (unsigned)n_row), dim3(kThreads), 0, st, a);
        hipLaunchKernelGGL(k_hp_out, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)n_row), dim3(kThreads), 0, st, a);
        TH_HIP(hipGetLastError());
        timer.stop(0);
    });
}

int toast_hip_noise_estim_pair_good_dev(int64_t n_pair, int64_t n, const uint8_t * d_shared_flags, uint8_t shared_flag_mask,
                                        const uint8_t * d_det_flags, int64_t n_flag_rows, int64_t flag_stride,
                                        uint8_t det_flag_mask, const int32_t * row1, const int32_t * row2,
                                        uint8_t * d_good, int64_t good_stride, void * stream) {
    return guarded([&] {
        if (n_pair <= 0 || n <= 0) return;
        if (!row1 || !row2 || !d_good) fail_arg("noise_estim_pair_good: missing argument");
        if (n > good_stride || (d_det_flags && n > flag_stride)) fail_arg("noise_estim_pair_good: rows are shorter than n");
        check_batch(n_pair, "noise_estim_pair_good");
        if (d_det_flags) {
            for (int64_t p = 0; p < n_pair; ++p) {
                if (row1[p] < 0 || row1[p] >= n_flag_rows || row2[p] < 0 || row2[p] >= n_flag_rows) {
                    fail_arg("noise_estim_pair_good: a pair names a row outside the flags");
                }
            }
        }
        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> v1(row1, row1 + n_pair), v2(row2, row2 + n_pair);
        const size_t o1 = pb.push_vec(v1), o2 = pb.push_vec(v2);
        const char * d = pb.commit(st);
        hipLaunchKernelGGL(k_pair_good, dim3(grid_x(n), (unsigned)n_pair), dim3(kThreads), 0, st, n, d_shared_flags,
                           shared_flag_mask, d_det_flags, flag_stride, det_flag_mask, (const int32_t *)(d + o1),
                           (const int32_t *)(d + o2), d_good, good_stride);
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_noise_estim_decimate_dev(int64_t n_row, int64_t n, int64_t step, const double * d_in, int64_t in_stride,
                                       const int32_t * good_row, const uint8_t * d_good, int64_t n_good_rows,
                                       int64_t good_stride, double * d_out, int64_t out_stride, uint8_t * d_good_out,
                                       int64_t good_out_stride, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n <= 0) return;
        if (!d_in || !good_row || !d_good || !d_out || !d_good_out) fail_arg("noise_estim_decimate: missing argument");
        if (step < 1) fail_arg("noise_estim_decimate: the step must be at least one");
        const int64_t n_out = (n + step - 1) / step;
        if (n > in_stride || n > good_stride || n_out > out_stride || n_out > good_out_stride) {
            fail_arg("noise_estim_decimate: rows are shorter than their samples");
        }
        check_batch(n_row, "noise_estim_decimate");
        check_batch(n_good_rows, "noise_estim_decimate");
        for (int64_t r = 0; r < n_row; ++r) {
            if (good_row[r] < 0 || good_row[r] >= n_good_rows) fail_arg("noise_estim_decimate: a row lies outside the flags");
        }
        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> vg(good_row, good_row + n_row);
        const size_t o1 = pb.push_vec(vg);
        const char * d = pb.commit(st);
        hipLaunchKernelGGL(k_decimate, dim3(grid_x(n_out), (unsigned)n_row), dim3(kThreads), 0, st, n_out, step, d_in,
                           in_stride, d_good, good_stride, (const int32_t *)(d + o1), d_out, out_stride);
        hipLaunchKernelGGL(k_decimate_good, dim3(grid_x(n_out), (unsigned)n_good_rows), dim3(kThreads), 0, st, n_out, step,
                           d_good, good_stride, d_good_out, good_out_stride);
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_noise_estim_fetch(int64_t count, const double * d_sums, double * sums, const int64_t * d_hits,
                                int64_t * hits, void * stream) {
    return guarded([&] {
        if (count <= 0) return;
        if (!d_sums || !sums || !d_hits || !hits) fail_arg("noise_estim_fetch: missing argument");
        hipStream_t st = pick_stream(stream);
        if (g_timing) TH_HIP(hipStreamSynchronize(st));
        const auto t0 = std::chrono::steady_clock::now();
        copy_to_host(sums, d_sums, (size_t)count * sizeof(double), st);
        copy_to_host(hits, d_hits, (size_t)count * sizeof(int64_t), st);
        TH_HIP(hipStreamSynchronize(st));
        if (g_timing) g_phase_ms[3] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    });
}

int toast_hip_noise_estim_fma_ceiling(int64_t n_block, int64_t iterations, double * ms, void * stream) {
    return guarded([&] {
        if (n_block <= 0 || iterations <= 0 || n_block > 0x7fffffff || iterations > 0x7fffffff || ms == nullptr) {
            fail_arg("noise_estim_fma_ceiling: bad argument");
        }
        hipStream_t st = pick_stream(stream);
        double * out = (double *)Manager::get().scratch(Manager::kScratchNoiseEstimHp, (size_t)n_block * sizeof(double), st);
        hipEvent_t e0, e1;
        TH_HIP(hipEventCreate(&e0));
        TH_HIP(hipEventCreate(&e1));
        TH_HIP(hipEventRecord(e0, st));
        hipLaunchKernelGGL(k_fma_ceiling, dim3((unsigned)n_block), dim3(kThreads), 0, st, (int)iterations, 1.0e-3, out);
        TH_HIP(hipEventRecord(e1, st));
        TH_HIP(hipEventSynchronize(e1));
        float t = 0.0f;
        TH_HIP(hipEventElapsedTime(&t, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *ms = (double)t;
    });
}

int toast_hip_noise_estim_timing(int on, double * phase_ms) {
    if (phase_ms != nullptr) {
        for (int ph = 0; ph < 4; ++ph) phase_ms[ph] = g_phase_ms[ph];
    }
    g_timing = on ? 1 : 0;
    for (int ph = 0; ph < 4; ++ph) g_phase_ms[ph] = 0.0;
    return TOAST_HIP_OK;
}

}  // extern "C"
