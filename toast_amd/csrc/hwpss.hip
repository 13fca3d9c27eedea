// hwpss.hip -- the half-wave-plate synchronous signal (HWPSS) model on gfx950.
//
// Counterpart of the per-sample work of the reference's HWPSynchronousModel (src/toast/ops/hwpss_model.py) and of
// src/toast/hwp_utils.py:
//   * hwpss_sincos_buffer + hwpss_compute_coeff_covariance (hwp_utils.py:43-231, without the scaling):
//     toast_hip_hwpss_gram_dev,
//   * _fit_chunk's mean removal and hwpss_compute_coeff's right-hand side (hwpss_model.py:807-818, hwp_utils.py:287-310):
//     toast_hip_hwpss_project_dev,
//   * hwpss_build_model, the subtraction, the flag update and the continuous relative calibration
//     (hwp_utils.py:318-392, hwpss_model.py:325-335, :560-578): toast_hip_hwpss_subtract_dev,
//   * the removal of the mean that is left (hwpss_model.py:334-335): toast_hip_hwpss_remove_mean_dev.
//
// The model of one sample has n_coeff basis values: sin / cos of (h + 1) angle for h < harmonics, in the order
// [sin_1, cos_1, sin_2, ...], or with time_drift [sin_h, t sin_h, cos_h, t cos_h] per harmonic.  No kernel writes them to
// memory: a workgroup forms the values of kSub consecutive samples in LDS (row k, one pad double per row; zero where the
// shared flag byte is not 0) and every detector of its tile reads them from there.
//
// Sums: a chunk [start, end) of the fit is cut into tiles of kTile samples.  A workgroup owns one tile (and one tile of
// detectors), every one of its sums runs over the samples of the tile in order, and a second kernel adds the tiles of a
// chunk in order.  So every sum is a chain of at most kTile + (tiles of the chunk) additions whose order depends on
// nothing but the chunk: no atomics.  The products are explicit FMAs.
//
// The mean of a detector's good samples is a compensated (two-sum) sum, kept as an unevaluated pair hi + lo, and the
// right-hand side is accumulated from (signal - hi) - lo: a DC level of any size in front of the HWPSS costs the
// right-hand side nothing.  That is the second sweep over the chunk; the reference does it by removing the mean twice
// (hwpss_model.py:817-818, hwp_utils.py:291-292).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "runtime.hpp"

using namespace toast_hip;

namespace {

constexpr int kThreads = 256;
constexpr int kSub = 64;                          // samples whose basis is staged at a time
constexpr int kTile = 1024;                       // samples of a chunk per workgroup (toast_hip_hwpss_chunk)
constexpr int kDetTile = 32;                      // detectors per workgroup (toast_hip_hwpss_det_tile)
constexpr int kMaxCoeff = 36;                     // toast_hip_hwpss_max_coeff
constexpr int kKGroup = 8;                        // lanes that share one detector in the projection
constexpr int kPerLane = 5;                       // coefficients per lane: kKGroup * kPerLane >= kMaxCoeff
constexpr int kRows = kKGroup * kPerLane;         // staged rows (rows >= n_coeff are zero; row n_coeff of the Gram: good)
constexpr int kPitch = kSub + 1;
constexpr int kTriPerLane = 3;                    // Gram entries per lane: 36 * 37 / 2 + 1 = 667 <= 3 * 256
constexpr int kSubSamp = 128;                     // samples per step of the subtraction (two lanes per sample)
constexpr int kSubPitch = kSubSamp + 1;
constexpr int kSubDets = kDetTile / 2;            // detectors per lane of the subtraction
constexpr size_t kScratchBudget = size_t(64) << 20;

static_assert(kKGroup * kPerLane >= kMaxCoeff + 1, "a row past the coefficients holds the good-sample indicator");
static_assert(kMaxCoeff * (kMaxCoeff + 1) / 2 + 1 <= kTriPerLane * kThreads, "Gram entries per lane");
static_assert(kThreads % kSub == 0 && kTile % kSub == 0 && kTile % kSubSamp == 0, "tiles are whole steps");
static_assert(kThreads == kDetTile * kKGroup, "one lane per detector and coefficient group");

struct Tile {
    int64_t first;     // first sample
    int32_t count;     // 1 .. kTile
    int32_t chunk;
};

struct Common {
    int64_t n_samp;
    int harmonics;
    int drift;
    int n_coeff;
    const double * angle;
    const double * reltime;
    const uint8_t * shared;        // combined shared flag byte, NULL: nothing flagged
};

struct TwoSum {
    double s, e;
    __device__ __forceinline__ void add(double x) {
        const double t = s + x;
        const double bp = t - s;
        e += (s - (t - bp)) + (x - bp);
        s = t;
    }
    __device__ __forceinline__ void add(const TwoSum & o) {
        add(o.s);
        e += o.e;
    }
};

// rows [0, n_coeff) of bs <- the basis of samples first .. first + count - 1 (zero where flagged or past count); when
// good_row >= 0 that row <- 1.0 at the shared-good samples.  Lanes: sample = t % kSub, harmonics dealt to t / kSub.
template <int PITCH, int NS>
__device__ __forceinline__ void stage_basis(const Common & c, int64_t first, int count, double * bs, int good_row) {
    constexpr int kGroups = kThreads / NS;
    const int s = (int)threadIdx.x % NS;
    const int hg = (int)threadIdx.x / NS;
    const int64_t i = first + s;
    const bool in = s < count;
    const bool good = in && (c.shared == nullptr || c.shared[i] == 0);
    const double ang = good ? c.angle[i] : 0.0;
    const double t = (good && c.drift) ? c.reltime[i] : 0.0;
    for (int h = hg; h < c.harmonics; h += kGroups) {
        double sn = 0.0, cs = 0.0;
        if (good) sincos((double)(h + 1) * ang, &sn, &cs);
        if (c.drift) {
            bs[(4 * h + 0) * PITCH + s] = sn;
            bs[(4 * h + 1) * PITCH + s] = good ? sn * t : 0.0;
            bs[(4 * h + 2) * PITCH + s] = cs;
            bs[(4 * h + 3) * PITCH + s] = good ? cs * t : 0.0;
        } else {
            bs[(2 * h + 0) * PITCH + s] = sn;
            bs[(2 * h + 1) * PITCH + s] = cs;
        }
    }
    if (good_row >= 0 && hg == 0) bs[good_row * PITCH + s] = good ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------------------------------- Gram
// part[tile][e]: entry e < n_tri is element (i, j), i <= j, of the upper triangle in row order; entry n_tri the count
__global__ __launch_bounds__(kThreads) void k_hwpss_gram(Common c, const Tile * __restrict__ tiles, int n_tri,
                                                         double * __restrict__ part) {
    __shared__ double bs[kRows * kPitch];
    const Tile tl = tiles[blockIdx.x];
    int ri[kTriPerLane], rj[kTriPerLane];
    double acc[kTriPerLane];
#pragma unroll
    for (int q = 0; q < kTriPerLane; ++q) {
        const int e = (int)threadIdx.x + q * kThreads;
        acc[q] = 0.0;
        ri[q] = rj[q] = -1;
        if (e < n_tri) {
            int i = 0, rest = e;
            while (rest >= c.n_coeff - i) {
                rest -= c.n_coeff - i;
                ++i;
            }
            ri[q] = i;
            rj[q] = i + rest;
        } else if (e == n_tri) {
            ri[q] = rj[q] = c.n_coeff;
        }
    }
    for (int s0 = 0; s0 < tl.count; s0 += kSub) {
        const int ns = min(kSub, tl.count - s0);
        __syncthreads();
        stage_basis<kPitch, kSub>(c, tl.first + s0, ns, bs, c.n_coeff);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kTriPerLane; ++q) {
            if (ri[q] < 0) continue;
            const double * a = bs + ri[q] * kPitch;
            const double * b = bs + rj[q] * kPitch;
            for (int s = 0; s < ns; ++s) acc[q] = __builtin_fma(a[s], b[s], acc[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < kTriPerLane; ++q) {
        const int e = (int)threadIdx.x + q * kThreads;
        if (e <= n_tri) part[(int64_t)blockIdx.x * (n_tri + 1) + e] = acc[q];
    }
}

__global__ void k_hwpss_gram_finish(int n_chunk, int n_coeff, int n_tri, const int32_t * __restrict__ tile_begin,
                                    const double * __restrict__ part, double * __restrict__ gram,
                                    int64_t * __restrict__ n_good) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)n_chunk * (n_tri + 1)) return;
    const int ch = (int)(id / (n_tri + 1)), e = (int)(id % (n_tri + 1));
    double sum = 0.0;
    for (int t = tile_begin[ch]; t < tile_begin[ch + 1]; ++t) sum += part[(int64_t)t * (n_tri + 1) + e];
    if (e == n_tri) {
        n_good[ch] = (int64_t)sum;        // a sum of ones: exact
        return;
    }
    int i = 0, rest = e;
    while (rest >= n_coeff - i) {
        rest -= n_coeff - i;
        ++i;
    }
    gram[((int64_t)ch * n_coeff + i) * n_coeff + i + rest] = sum;
}

// ---------------------------------------------------------------------------------------------------- mean
struct DetRows {
    const double * signal;         // [row][n_samp]
    const int32_t * signal_index;  // [n_det]
    const uint8_t * det_flags;     // [row][n_samp] or NULL
    const int32_t * flag_index;    // [n_det]
    uint8_t det_flag_mask;
    int n_det;
};

__device__ __forceinline__ bool det_good(const Common & c, const uint8_t * __restrict__ frow, uint8_t mask, int64_t i) {
    if (c.shared != nullptr && c.shared[i] != 0) return false;
    return frow == nullptr || (frow[i] & mask) == 0;
}

// one workgroup per (tile, detector): part3[(det * n_tile + tile) * 3] = (sum hi, sum lo, count) of the good samples
__global__ __launch_bounds__(kThreads) void k_hwpss_sum(Common c, DetRows r, const Tile * __restrict__ tiles, int n_tile,
                                                        double * __restrict__ part3) {
    __shared__ double sh[kThreads], se[kThreads];
    __shared__ int sn[kThreads];
    const Tile tl = tiles[blockIdx.x];
    const int d = (int)blockIdx.y;
    const double * __restrict__ x = r.signal + (int64_t)r.signal_index[d] * c.n_samp;
    const uint8_t * __restrict__ f = r.det_flags ? r.det_flags + (int64_t)r.flag_index[d] * c.n_samp : nullptr;
    TwoSum a{0.0, 0.0};
    int n = 0;
    for (int s = (int)threadIdx.x; s < tl.count; s += kThreads) {
        const int64_t i = tl.first + s;
        if (det_good(c, f, r.det_flag_mask, i)) {
            a.add(x[i]);
            ++n;
        }
    }
    sh[threadIdx.x] = a.s;
    se[threadIdx.x] = a.e;
    sn[threadIdx.x] = n;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            TwoSum m{sh[threadIdx.x], se[threadIdx.x]};
            m.add(TwoSum{sh[threadIdx.x + w], se[threadIdx.x + w]});
            sh[threadIdx.x] = m.s;
            se[threadIdx.x] = m.e;
            sn[threadIdx.x] += sn[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double * o = part3 + ((int64_t)d * n_tile + blockIdx.x) * 3;
        o[0] = sh[0];
        o[1] = se[0];
        o[2] = (double)sn[0];
    }
}

// mean2[(det * n_chunk + chunk) * 2] = (hi, lo): hi + lo is the mean of the good samples far beyond double precision
__global__ void k_hwpss_mean(int n_det, int n_chunk, int n_tile, const int32_t * __restrict__ tile_begin,
                             const double * __restrict__ part3, double * __restrict__ mean2,
                             int64_t * __restrict__ n_good, double * __restrict__ mean, int64_t det0, int64_t ld_chunk) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)n_det * n_chunk) return;
    const int d = (int)(id / n_chunk), ch = (int)(id % n_chunk);
    TwoSum a{0.0, 0.0};
    double cnt = 0.0;
    for (int t = tile_begin[ch]; t < tile_begin[ch + 1]; ++t) {
        const double * p = part3 + ((int64_t)d * n_tile + t) * 3;
        a.add(TwoSum{p[0], p[1]});
        cnt += p[2];
    }
    double hi = 0.0, lo = 0.0;
    if (cnt > 0.0) {
        hi = a.s / cnt;
        lo = (__builtin_fma(-hi, cnt, a.s) + a.e) / cnt;
    }
    mean2[id * 2] = hi;
    mean2[id * 2 + 1] = lo;
    n_good[(det0 + d) * ld_chunk + ch] = (int64_t)cnt;
    mean[(det0 + d) * ld_chunk + ch] = hi + lo;
}

// ---------------------------------------------------------------------------------------------------- projection
// part[(tile * n_det + det) * n_coeff + k] = sum over the tile's good samples of ((signal - hi) - lo) basis_k
__global__ __launch_bounds__(kThreads) void k_hwpss_project(Common c, DetRows r, const Tile * __restrict__ tiles,
                                                            int n_chunk, const double * __restrict__ mean2,
                                                            double * __restrict__ part) {
    __shared__ double bs[kRows * kPitch];
    __shared__ double vs[kDetTile * kPitch];
    const Tile tl = tiles[blockIdx.x];
    const int d0 = (int)blockIdx.y * kDetTile;
    const int dl = (int)threadIdx.x / kKGroup, kg = (int)threadIdx.x % kKGroup;
    // rows n_coeff .. kRows - 1 are read as zeros
    for (int v = (int)threadIdx.x; v < kRows * kPitch; v += kThreads) bs[v] = 0.0;
    double acc[kPerLane];
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) acc[j] = 0.0;
    for (int s0 = 0; s0 < tl.count; s0 += kSub) {
        const int ns = min(kSub, tl.count - s0);
        __syncthreads();
        stage_basis<kPitch, kSub>(c, tl.first + s0, ns, bs, -1);
        for (int v = (int)threadIdx.x; v < kDetTile * kSub; v += kThreads) {
            const int dd = v / kSub, s = v % kSub;
            const int d = d0 + dd;
            double val = 0.0;
            if (d < r.n_det && s < ns) {
                const int64_t i = tl.first + s0 + s;
                const uint8_t * f = r.det_flags ? r.det_flags + (int64_t)r.flag_index[d] * c.n_samp : nullptr;
                if (det_good(c, f, r.det_flag_mask, i)) {
                    const double * m = mean2 + ((int64_t)d * n_chunk + tl.chunk) * 2;
                    val = (r.signal[(int64_t)r.signal_index[d] * c.n_samp + i] - m[0]) - m[1];
                }
            }
            vs[dd * kPitch + s] = val;
        }
        __syncthreads();
        const double * __restrict__ vrow = vs + dl * kPitch;
        for (int s = 0; s < ns; ++s) {
            const double v = vrow[s];
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) acc[j] = __builtin_fma(v, bs[(kg + kKGroup * j) * kPitch + s], acc[j]);
        }
    }
    const int d = d0 + dl;
    if (d < r.n_det) {
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const int k = kg + kKGroup * j;
            if (k < c.n_coeff) part[((int64_t)blockIdx.x * r.n_det + d) * c.n_coeff + k] = acc[j];
        }
    }
}

__global__ void k_hwpss_project_finish(int n_det, int n_chunk, int n_coeff, const int32_t * __restrict__ tile_begin,
                                       const double * __restrict__ part, double * __restrict__ rhs, int64_t det0,
                                       int64_t ld_chunk) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)n_det * n_chunk * n_coeff) return;
    const int k = (int)(id % n_coeff);
    const int ch = (int)((id / n_coeff) % n_chunk);
    const int d = (int)(id / ((int64_t)n_coeff * n_chunk));
    double sum = 0.0;
    for (int t = tile_begin[ch]; t < tile_begin[ch + 1]; ++t) sum += part[((int64_t)t * n_det + d) * n_coeff + k];
    rhs[((det0 + d) * ld_chunk + ch) * n_coeff + k] = sum;
}

// ---------------------------------------------------------------------------------------------------- subtraction
struct SubArgs {
    double * signal;
    const int32_t * signal_index;
    uint8_t * det_flags;
    const int32_t * flag_index;
    const int32_t * active;        // [n_det] 0: only the flags of this detector are updated
    uint8_t det_flag_mask, hwp_flag_mask;
    int n_det;
    int subtract;
    const double * coeff;          // fixed: [n_det][n_coeff]; NULL: splines
    const int64_t * spl_offset;    // [n_det n_coeff + 1] into spl_t / spl_c
    const double * spl_t;
    const double * spl_c;
    float * relcal;                // [row][n_samp] or NULL (splines only)
    const int32_t * relcal_index;
    double cal_center;
    int n_tile;
};

// FITPACK's splev for k = 3, ext = 0 (splev.f, fpbspl.f): the span l is the last one in [3, n - 5] whose knot is <= x
// (the first when there is none), so x outside the knots is evaluated with the end polynomial
__device__ __forceinline__ double splev3(const double * __restrict__ t, const double * __restrict__ cf, int n, double x) {
    int lo = 3, hi = n - 5;              // invariant: the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid] <= x) lo = mid; else hi = mid - 1;
    }
    const int l = lo;
    double h[4], hh[3];
    h[0] = 1.0;
    h[1] = h[2] = h[3] = 0.0;
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            const double tli = t[l + i], tlj = t[l + i - j];
            const double f = hh[i - 1] / (tli - tlj);
            h[i - 1] = h[i - 1] + f * (tli - x);
            h[i] = f * (x - tlj);
        }
    }
    double sp = 0.0;
#pragma unroll
    for (int j = 0; j <= 3; ++j) sp = sp + cf[l - 3 + j] * h[j];
    return sp;
}

// grid (tiles of kTile samples, tiles of kDetTile detectors); lane: sample t % kSubSamp, detectors dd = t / kSubSamp + 2 j.
// part3[(det * n_tile + tile) * 3] = (sum hi, sum lo, count) of the cleaned good samples
__global__ __launch_bounds__(kThreads) void k_hwpss_subtract(Common c, SubArgs a, double * __restrict__ part3) {
    __shared__ double bs[kMaxCoeff * kSubPitch];
    __shared__ double red_s[kThreads / 64][kSubDets], red_e[kThreads / 64][kSubDets];
    __shared__ int red_n[kThreads / 64][kSubDets];
    const int64_t first = (int64_t)blockIdx.x * kTile;
    const int count = (int)min((int64_t)kTile, c.n_samp - first);
    const int d0 = (int)blockIdx.y * kDetTile;
    const int s = (int)threadIdx.x % kSubSamp, half = (int)threadIdx.x / kSubSamp;
    const int lane = (int)threadIdx.x % 64, wave = (int)threadIdx.x / 64;
    if ((int)threadIdx.x < kThreads / 64 * kSubDets) {
        (&red_s[0][0])[threadIdx.x] = 0.0;
        (&red_e[0][0])[threadIdx.x] = 0.0;
        (&red_n[0][0])[threadIdx.x] = 0;
    }
    const int re = c.drift ? 4 : 2, im = c.drift ? 6 : 3;      // the 2f sine and cosine (hwpss_model.py:574-577)
    const bool want_cal = a.relcal != nullptr && a.coeff == nullptr;
    for (int s0 = 0; s0 < count; s0 += kSubSamp) {
        const int ns = min(kSubSamp, count - s0);
        __syncthreads();
        stage_basis<kSubPitch, kSubSamp>(c, first + s0, ns, bs, -1);
        __syncthreads();
        const bool in = s < ns;
        const int64_t i = first + s0 + (in ? s : 0);
        const uint8_t sh = (in && c.shared) ? c.shared[i] : (uint8_t)0;
        const double x = (in && a.coeff == nullptr) ? c.reltime[i] : 0.0;
#pragma unroll 1
        for (int j = 0; j < kSubDets; ++j) {
            const int d = d0 + half + 2 * j;
            if (d0 + 2 * j >= a.n_det) break;              // (uniform: neither half has this detector)
            double v = 0.0;
            int n = 0;
            if (in && d < a.n_det) {
                uint8_t fv = sh;
                if (a.det_flags != nullptr) {
                    uint8_t * f = a.det_flags + (int64_t)a.flag_index[d] * c.n_samp + i;
                    const uint8_t cur = *f;
                    fv = (uint8_t)((cur & a.det_flag_mask) | sh);
                    // hwpss_model.py:325: the uint8 product of the flag VALUE and the mask
                    const uint8_t add = (uint8_t)((unsigned)fv * (unsigned)a.hwp_flag_mask);
                    if ((cur | add) != cur) *f = (uint8_t)(cur | add);
                }
                const bool good = fv == 0;
                if (a.active[d] && !good && want_cal) {
                    // hwpss_model.py:578, :347: the magnitude of a flagged sample is set to one, nothing to evaluate
                    a.relcal[(int64_t)a.relcal_index[d] * c.n_samp + i] = (float)(a.cal_center / 1.0);
                }
                if (a.active[d] && good) {
                    double model = 0.0, c_re = 0.0, c_im = 0.0;
                    for (int k = 0; k < c.n_coeff; ++k) {
                        double ck;
                        if (a.coeff != nullptr) {
                            ck = a.coeff[(int64_t)d * c.n_coeff + k];
                        } else {
                            const int64_t o = a.spl_offset[(int64_t)d * c.n_coeff + k];
                            const int nk = (int)(a.spl_offset[(int64_t)d * c.n_coeff + k + 1] - o);
                            ck = splev3(a.spl_t + o, a.spl_c + o, nk, x);
                            if (k == re) c_re = ck;
                            if (k == im) c_im = ck;
                        }
                        // hwp_utils.py:359-391: model += coeff * basis, one rounded product and one rounded sum per term
                        model = model + ck * bs[k * kSubPitch + s];
                    }
                    if (want_cal) {
                        const double mag = sqrt(c_re * c_re + c_im * c_im);                  // hwpss_model.py:575-577
                        a.relcal[(int64_t)a.relcal_index[d] * c.n_samp + i] = (float)(a.cal_center / mag);
                    }
                    double * p = a.signal + (int64_t)a.signal_index[d] * c.n_samp + i;
                    v = *p;
                    if (a.subtract) {
                        v = v - model;
                        *p = v;
                    }
                    n = 1;
                }
            }
            // the cleaned good samples of this detector and step: the lanes of the wave, then one lane adds them to the
            // wave's running pair
            TwoSum m{v, 0.0};
            for (int w = 32; w > 0; w >>= 1) {
                const TwoSum o{__shfl_down(m.s, w, 64), __shfl_down(m.e, w, 64)};
                m.add(o);
                n += __shfl_down(n, w, 64);
            }
            if (lane == 0) {
                TwoSum r{red_s[wave][j], red_e[wave][j]};
                r.add(m);
                red_s[wave][j] = r.s;
                red_e[wave][j] = r.e;
                red_n[wave][j] += n;
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < kDetTile) {
        const int dd = (int)threadIdx.x, h2 = dd % 2, j = dd / 2;
        const int d = d0 + dd;
        if (d < a.n_det) {
            TwoSum m{red_s[2 * h2][j], red_e[2 * h2][j]};
            m.add(TwoSum{red_s[2 * h2 + 1][j], red_e[2 * h2 + 1][j]});
            double * o = part3 + ((int64_t)d * a.n_tile + blockIdx.x) * 3;
            o[0] = m.s;
            o[1] = m.e;
            o[2] = (double)(red_n[2 * h2][j] + red_n[2 * h2 + 1][j]);
        }
    }
}

__global__ void k_hwpss_subtract_finish(int n_det, int n_tile, const double * __restrict__ part3, double * __restrict__ sum,
                                        int64_t * __restrict__ count) {
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d >= n_det) return;
    TwoSum a{0.0, 0.0};
    double cnt = 0.0;
    for (int t = 0; t < n_tile; ++t) {
        const double * p = part3 + ((int64_t)d * n_tile + t) * 3;
        a.add(TwoSum{p[0], p[1]});
        cnt += p[2];
    }
    sum[d] = a.s + a.e;
    count[d] = (int64_t)cnt;
}

// hwpss_model.py:334-335: signal[good] -= sum / count
__global__ __launch_bounds__(kThreads) void k_hwpss_remove_mean(Common c, SubArgs a, const double * __restrict__ sum,
                                                                const int64_t * __restrict__ count) {
    const int d = (int)blockIdx.y;
    if (!a.active[d] || count[d] <= 0) return;
    const double dc = sum[d] / (double)count[d];
    double * __restrict__ x = a.signal + (int64_t)a.signal_index[d] * c.n_samp;
    const uint8_t * __restrict__ f = a.det_flags ? a.det_flags + (int64_t)a.flag_index[d] * c.n_samp : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < c.n_samp; i += (int64_t)gridDim.x * kThreads) {
        if (det_good(c, f, a.det_flag_mask, i)) x[i] = x[i] - dc;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
hipStream_t pick_stream(void * stream) {
    Manager::get().require_device();
    return stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
}

int check_model(int64_t n_samp, int64_t harmonics, int time_drift, const char * what) {
    if (n_samp < 1 || n_samp > (int64_t(1) << 40)) fail_arg(std::string(what) + ": n_samp out of range");
    const int64_t n_coeff = harmonics * (time_drift ? 4 : 2);
    if (harmonics < 1 || n_coeff > kMaxCoeff) {
        fail_arg(std::string(what) + ": between 1 and toast_hip_hwpss_max_coeff() coefficients per detector");
    }
    return (int)n_coeff;
}

// the tiles of the chunks in chunk order, ends clamped to n_samp like a NumPy slice; begin[c] .. begin[c + 1]: chunk c
void make_tiles(int64_t n_samp, const int64_t * starts, const int64_t * ends, int64_t n_chunk, const char * what,
                std::vector<Tile> & tiles, std::vector<int32_t> & begin) {
    if (n_chunk > 0 && (!starts || !ends)) fail_arg(std::string(what) + ": missing chunk arrays");
    begin.assign(1, 0);
    for (int64_t ch = 0; ch < n_chunk; ++ch) {
        if (starts[ch] < 0) fail_arg(std::string(what) + ": a chunk starts before the first sample");
        const int64_t end = std::min(ends[ch], n_samp);
        for (int64_t f = starts[ch]; f < end; f += kTile) {
            tiles.push_back(Tile{f, (int32_t)std::min<int64_t>(kTile, end - f), (int32_t)ch});
        }
        if (tiles.size() > size_t(1) << 30) fail_arg(std::string(what) + ": too many tiles");
        begin.push_back((int32_t)tiles.size());
    }
}

void check_rows(const int32_t * rows, int64_t n, const char * what) {
    for (int64_t r = 0; r < n; ++r) {
        if (rows[r] < 0) fail_arg(std::string(what) + ": negative row index");
    }
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

}  // namespace

extern "C" {

int toast_hip_hwpss_det_tile(void) { return kDetTile; }
int toast_hip_hwpss_chunk(void) { return kTile; }
int toast_hip_hwpss_max_coeff(void) { return kMaxCoeff; }

int toast_hip_hwpss_gram_dev(int64_t n_samp, int64_t harmonics, int time_drift, const double * d_angle,
                             const double * d_reltime, const uint8_t * d_shared, const int64_t * starts,
                             const int64_t * ends, int64_t n_chunk, double * d_gram, int64_t * d_n_good, void * stream) {
    return guarded([&] {
        const int n_coeff = check_model(n_samp, harmonics, time_drift, "hwpss_gram");
        if (n_chunk <= 0) return;
        if (!d_angle || !d_gram || !d_n_good || (time_drift && !d_reltime)) fail_arg("hwpss_gram: missing argument");
        if (n_chunk > (1 << 24)) fail_arg("hwpss_gram: too many chunks");
        std::vector<Tile> tiles;
        std::vector<int32_t> begin;
        make_tiles(n_samp, starts, ends, n_chunk, "hwpss_gram", tiles, begin);
        hipStream_t st = pick_stream(stream);
        const int n_tri = n_coeff * (n_coeff + 1) / 2;
        TH_HIP(hipMemsetAsync(d_gram, 0, sizeof(double) * (size_t)n_chunk * n_coeff * n_coeff, st));
        ParamBlock pb;
        const size_t o0 = pb.push(tiles.data(), tiles.size() * sizeof(Tile)), o1 = pb.push_vec(begin);
        const char * d = pb.commit(st);
        Common c{n_samp, (int)harmonics, time_drift ? 1 : 0, n_coeff, d_angle, d_reltime, d_shared};
        double * part = static_cast<double *>(Manager::get().scratch(
            Manager::kScratchHwpss, sizeof(double) * std::max<size_t>(1, tiles.size()) * (n_tri + 1), st));
        if (!tiles.empty()) {
            hipLaunchKernelGGL(k_hwpss_gram, dim3((unsigned)tiles.size()), dim3(kThreads), 0, st, c, (const Tile *)(d + o0),
                               n_tri, part);
        }
        hipLaunchKernelGGL(k_hwpss_gram_finish, dim3(blocks_for(n_chunk * (n_tri + 1), kThreads)), dim3(kThreads), 0, st,
                           (int)n_chunk, n_coeff, n_tri, (const int32_t *)(d + o1), (const double *)part, d_gram, d_n_good);
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_hwpss_project_dev(int64_t n_samp, int64_t harmonics, int time_drift, const double * d_angle,
                                const double * d_reltime, const uint8_t * d_shared, const int32_t * signal_index,
                                const double * d_signal, const int32_t * flag_index, const uint8_t * d_det_flags,
                                uint8_t det_flag_mask, int64_t n_det, const int64_t * starts, const int64_t * ends,
                                int64_t n_chunk, int64_t * d_n_good, double * d_mean, double * d_rhs, void * stream) {
    return guarded([&] {
        const int n_coeff = check_model(n_samp, harmonics, time_drift, "hwpss_project");
        if (n_chunk <= 0 || n_det <= 0) return;
        if (!d_angle || !d_signal || !signal_index || !d_n_good || !d_mean || !d_rhs || (time_drift && !d_reltime)) {
            fail_arg("hwpss_project: missing argument");
        }
        if (d_det_flags && !flag_index) fail_arg("hwpss_project: detector flags without their row index");
        if (n_chunk > (1 << 24) || n_det > (1 << 24)) fail_arg("hwpss_project: too many chunks or detectors");
        check_rows(signal_index, n_det, "hwpss_project");
        if (d_det_flags) check_rows(flag_index, n_det, "hwpss_project");
        std::vector<Tile> tiles;
        std::vector<int32_t> begin;
        make_tiles(n_samp, starts, ends, n_chunk, "hwpss_project", tiles, begin);
        hipStream_t st = pick_stream(stream);
        const int64_t n_tile = (int64_t)tiles.size();
        // detectors per pass: the partial sums of a pass stay inside the scratch budget
        const size_t per_det = sizeof(double) * ((size_t)std::max<int64_t>(1, n_tile) * (n_coeff + 3) + 2 * (size_t)n_chunk);
        int64_t batch = std::max<int64_t>(1, (int64_t)(kScratchBudget / per_det)) / kDetTile * kDetTile;
        batch = std::min<int64_t>(std::max<int64_t>(batch, kDetTile), std::min<int64_t>(n_det, 65535));
        char * scratch = static_cast<char *>(Manager::get().scratch(Manager::kScratchHwpss, per_det * (size_t)batch, st));
        double * part3 = reinterpret_cast<double *>(scratch);
        double * mean2 = part3 + (size_t)batch * std::max<int64_t>(1, n_tile) * 3;
        double * part = mean2 + (size_t)batch * n_chunk * 2;
        Common c{n_samp, (int)harmonics, time_drift ? 1 : 0, n_coeff, d_angle, d_reltime, d_shared};
        for (int64_t det0 = 0; det0 < n_det; det0 += batch) {
            const int nb = (int)std::min(batch, n_det - det0);
            ParamBlock pb;
            std::vector<int32_t> si(signal_index + det0, signal_index + det0 + nb), fi;
            if (d_det_flags) fi.assign(flag_index + det0, flag_index + det0 + nb);
            const size_t o0 = pb.push(tiles.data(), tiles.size() * sizeof(Tile)), o1 = pb.push_vec(begin),
                         o2 = pb.push_vec(si), o3 = pb.push_vec(fi);
            const char * d = pb.commit(st);
            DetRows r{d_signal, (const int32_t *)(d + o2), d_det_flags, (const int32_t *)(d + o3), det_flag_mask, nb};
            const Tile * d_tiles = (const Tile *)(d + o0);
            const int32_t * d_begin = (const int32_t *)(d + o1);
            if (n_tile > 0) {
                hipLaunchKernelGGL(k_hwpss_sum, dim3((unsigned)n_tile, (unsigned)nb), dim3(kThreads), 0, st, c, r, d_tiles,
                                   (int)n_tile, part3);
            }
            hipLaunchKernelGGL(k_hwpss_mean, dim3(blocks_for((int64_t)nb * n_chunk, kThreads)), dim3(kThreads), 0, st, nb,
                               (int)n_chunk, (int)n_tile, d_begin, (const double *)part3, mean2, d_n_good, d_mean, det0,
                               n_chunk);
            if (n_tile > 0) {
                hipLaunchKernelGGL(k_hwpss_project, dim3((unsigned)n_tile, blocks_for(nb, kDetTile)), dim3(kThreads), 0, st,
                                   c, r, d_tiles, (int)n_chunk, (const double *)mean2, part);
            }
            hipLaunchKernelGGL(k_hwpss_project_finish, dim3(blocks_for((int64_t)nb * n_chunk * n_coeff, kThreads)),
                               dim3(kThreads), 0, st, nb, (int)n_chunk, n_coeff, d_begin, (const double *)part, d_rhs, det0,
                               n_chunk);
        }
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_hwpss_subtract_dev(int64_t n_samp, int64_t harmonics, int time_drift, const double * d_angle,
                                 const double * d_reltime, const uint8_t * d_shared, const int32_t * signal_index,
                                 double * d_signal, const int32_t * flag_index, uint8_t * d_det_flags,
                                 uint8_t det_flag_mask, uint8_t hwp_flag_mask, int64_t n_det, const int32_t * active,
                                 int subtract, const double * d_coeff, const int64_t * spl_offset, const double * d_spl_t,
                                 const double * d_spl_c, const int32_t * relcal_index, float * d_relcal, double cal_center,
                                 double * d_sum, int64_t * d_count, void * stream) {
    return guarded([&] {
        const int n_coeff = check_model(n_samp, harmonics, time_drift, "hwpss_subtract");
        if (n_det <= 0) return;
        if (!d_angle || !d_signal || !signal_index || !active || !d_sum || !d_count) fail_arg("hwpss_subtract: missing argument");
        const bool spline = d_coeff == nullptr;
        if (spline && (!spl_offset || !d_spl_t || !d_spl_c || !d_reltime)) {
            fail_arg("hwpss_subtract: neither fixed coefficients nor splines");
        }
        if (time_drift && !d_reltime) fail_arg("hwpss_subtract: time drift needs the relative times");
        if (d_det_flags && !flag_index) fail_arg("hwpss_subtract: detector flags without their row index");
        if (d_relcal && (!relcal_index || !spline || n_coeff < 4)) {
            fail_arg("hwpss_subtract: the calibration rows need splines, their row index and a 2f term");
        }
        if (n_det > (1 << 24)) fail_arg("hwpss_subtract: too many detectors");
        check_rows(signal_index, n_det, "hwpss_subtract");
        if (d_det_flags) check_rows(flag_index, n_det, "hwpss_subtract");
        if (d_relcal) check_rows(relcal_index, n_det, "hwpss_subtract");
        std::vector<int64_t> off;
        if (spline) {
            // every active detector's splines are cubic with at least 8 knots, inside the packed arrays
            off.assign(spl_offset, spl_offset + n_det * n_coeff + 1);
            for (int64_t d = 0; d < n_det; ++d) {
                for (int k = 0; k < n_coeff; ++k) {
                    const int64_t a = off[d * n_coeff + k], b = off[d * n_coeff + k + 1];
                    if (a < 0 || b < a || (active[d] && b - a < 8)) fail_arg("hwpss_subtract: a spline has fewer than 8 knots");
                }
            }
        }
        hipStream_t st = pick_stream(stream);
        const int64_t n_tile = (n_samp + kTile - 1) / kTile;
        if (n_tile > 0x7fffffff) fail_arg("hwpss_subtract: too many tiles");
        Common c{n_samp, (int)harmonics, time_drift ? 1 : 0, n_coeff, d_angle, d_reltime, d_shared};
        const size_t per_det = sizeof(double) * 3 * (size_t)n_tile;
        int64_t batch = std::max<int64_t>(kDetTile, (int64_t)(kScratchBudget / per_det) / kDetTile * kDetTile);
        batch = std::min<int64_t>(batch, 65535 / kDetTile * kDetTile);
        double * part3 = static_cast<double *>(
            Manager::get().scratch(Manager::kScratchHwpss, per_det * (size_t)std::min(batch, n_det), st));
        for (int64_t det0 = 0; det0 < n_det; det0 += batch) {
            const int nb = (int)std::min(batch, n_det - det0);
            ParamBlock pb;
            std::vector<int32_t> si(signal_index + det0, signal_index + det0 + nb), fi, ac(active + det0, active + det0 + nb), ri;
            if (d_det_flags) fi.assign(flag_index + det0, flag_index + det0 + nb);
            if (d_relcal) ri.assign(relcal_index + det0, relcal_index + det0 + nb);
            std::vector<int64_t> so;
            if (spline) so.assign(off.begin() + det0 * n_coeff, off.begin() + (det0 + nb) * n_coeff + 1);
            const size_t o0 = pb.push_vec(si), o1 = pb.push_vec(fi), o2 = pb.push_vec(ac), o3 = pb.push_vec(ri),
                         o4 = pb.push_vec(so);
            const char * d = pb.commit(st);
            SubArgs a;
            a.signal = d_signal;
            a.signal_index = (const int32_t *)(d + o0);
            a.det_flags = d_det_flags;
            a.flag_index = (const int32_t *)(d + o1);
            a.active = (const int32_t *)(d + o2);
            a.det_flag_mask = det_flag_mask;
            a.hwp_flag_mask = hwp_flag_mask;
            a.n_det = nb;
            a.subtract = subtract ? 1 : 0;
            a.coeff = spline ? nullptr : d_coeff + det0 * n_coeff;
            a.spl_offset = (const int64_t *)(d + o4);
            a.spl_t = d_spl_t;
            a.spl_c = d_spl_c;
            a.relcal = d_relcal;
            a.relcal_index = (const int32_t *)(d + o3);
            a.cal_center = cal_center;
            a.n_tile = (int)n_tile;
            hipLaunchKernelGGL(k_hwpss_subtract, dim3((unsigned)n_tile, blocks_for(nb, kDetTile)), dim3(kThreads), 0, st, c, a,
                               part3);
            hipLaunchKernelGGL(k_hwpss_subtract_finish, dim3(blocks_for(nb, kThreads)), dim3(kThreads), 0, st, nb, (int)n_tile,
                               (const double *)part3, d_sum + det0, d_count + det0);
        }
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_hwpss_remove_mean_dev(int64_t n_samp, const uint8_t * d_shared, const int32_t * signal_index, double * d_signal,
                                    const int32_t * flag_index, const uint8_t * d_det_flags, uint8_t det_flag_mask,
                                    int64_t n_det, const int32_t * active, const double * d_sum, const int64_t * d_count,
                                    void * stream) {
    return guarded([&] {
        if (n_det <= 0 || n_samp <= 0) return;
        if (!d_signal || !signal_index || !active || !d_sum || !d_count) fail_arg("hwpss_remove_mean: missing argument");
        if (d_det_flags && !flag_index) fail_arg("hwpss_remove_mean: detector flags without their row index");
        check_rows(signal_index, n_det, "hwpss_remove_mean");
        if (d_det_flags) check_rows(flag_index, n_det, "hwpss_remove_mean");
        hipStream_t st = pick_stream(stream);
        Common c{n_samp, 0, 0, 0, nullptr, nullptr, d_shared};
        const unsigned gx = (unsigned)std::min<int64_t>((n_samp + kThreads - 1) / kThreads, 4096);
        for (int64_t det0 = 0; det0 < n_det; det0 += 65535) {
            const int nb = (int)std::min<int64_t>(65535, n_det - det0);
            ParamBlock pb;
            std::vector<int32_t> si(signal_index + det0, signal_index + det0 + nb), fi, ac(active + det0, active + det0 + nb);
            if (d_det_flags) fi.assign(flag_index + det0, flag_index + det0 + nb);
            const size_t o0 = pb.push_vec(si), o1 = pb.push_vec(fi), o2 = pb.push_vec(ac);
            const char * d = pb.commit(st);
            SubArgs a{};
            a.signal = d_signal;
            a.signal_index = (const int32_t *)(d + o0);
            a.det_flags = const_cast<uint8_t *>(d_det_flags);
            a.flag_index = (const int32_t *)(d + o1);
            a.active = (const int32_t *)(d + o2);
            a.det_flag_mask = det_flag_mask;
            a.n_det = nb;
            hipLaunchKernelGGL(k_hwpss_remove_mean, dim3(gx, (unsigned)nb), dim3(kThreads), 0, st, c, a, d_sum + det0,
                               d_count + det0);
        }
        TH_HIP(hipGetLastError());
    });
}

}  // extern "C"
