// sim_noise.hip -- counter-based random streams and PSD noise simulation on gfx950.
//
// Device counterpart of the reference's
//   * rng_dist_uint64 / uniform_01 / uniform_11 / normal and their multi-stream forms
//     (src/libtoast/src/toast_math_rng.cpp:22-219; Threefry2x64-20, one element per counter2 + i),
//   * tod_sim_noise_timestream[_batch] (src/libtoast/src/toast_tod_simnoise.cpp:14-319) as driven by ops.SimNoise
//     (src/toast/ops/sim_tod_noise.py:248-408),
// and the host entries with the same arithmetic (libm, a radix-2 transform in extended precision) that the tests and
// the host path of the operator use.  The arithmetic both sides share is in sim_noise_math.hpp.
//
// Pipeline per batch of B noise streams (B bounded by the two work buffers of 8 fftlen bytes per stream each):
//   k_sim_spectrum   F[b, k] = scale_b(k) (g(c + k) + i g(c + fftlen - k)), 1 <= k < fftlen / 2; F[b, 0] = 0;
//                    F[b, fftlen / 2] real.  One thread draws both Gaussians of its bin and evaluates the interpolated
//                    amplitude once; the binned log grid of the stream sits in LDS.  Neither the Gaussians nor the
//                    interpolated spectrum ever exist as arrays.
//   rocFFT Z2D       batched, the plan cache of fft_filter.hip
//   k_crop_partial   fixed 4096-sample chunks of the middle `samples` of every transform: sums in a fixed order
//   k_crop_dc        the chunk sums of a stream in a fixed order -> DC = sum / samples
//   k_sim_mix        det_data[row] += weight ((1 / fftlen) x - DC) for every (row, weight) of the stream
// No atomics: the result does not depend on the batch size or on the launch shape.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <sstream>
#include <vector>

#include "runtime.hpp"
#include "sim_noise_math.hpp"

using namespace toast_hip;

namespace toast_hip {
void fft_c2r_exec(int64_t length, int64_t count, double2 * d_freq, double * d_time, hipStream_t st);   // fft_filter.hip
}

namespace {

namespace sn = toast_hip::simnoise;

constexpr int kThreads = 256;
constexpr int kBinsPerThread = 4;          // spectrum kernel: bins per thread
constexpr int kCropChunk = 4096;           // samples per partial sum of the DC level: part of the result's definition
constexpr int kLdsBinned = 768;            // binned PSD points held in LDS (3 tables of doubles: 18 KB, 8 workgroups per CU)
constexpr int64_t kMaxGridY = 65535;

size_t g_scratch_held = 0;                 // bytes of FFT scratch toast_hip_sim_noise_dev has asked for so far
int g_timing = 0;                          // toast_hip_sim_noise_timing
double g_phase_ms[3] = {0.0, 0.0, 0.0};    // spectrum, transform, crop + mix of the last timed call

// ------------------------------------------------------------------------------------ random streams
struct RngStreams {
    const uint64_t * key1;
    const uint64_t * key2;
    const uint64_t * counter1;
    const uint64_t * counter2;
    const uint64_t * length;
    const uint64_t * offset;   // first element of the stream in the output
};

template <int KIND>
__global__ __launch_bounds__(kThreads) void k_rng_multi(RngStreams s, int stream0, void * __restrict__ out) {
    const int b = stream0 + blockIdx.y;
    const uint64_t k1 = s.key1[b], k2 = s.key2[b], c1 = s.counter1[b], c2 = s.counter2[b];
    const uint64_t n = s.length[b];
    const uint64_t off = s.offset[b];
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t v = sn::threefry2x64_20(c1, c2 + i, k1, k2);
        if (KIND == sn::kUint64) {
            static_cast<uint64_t *>(out)[off + i] = v;
        } else if (KIND == sn::kUniform01) {
            static_cast<double *>(out)[off + i] = sn::u01(v);
        } else if (KIND == sn::kUniform11) {
            static_cast<double *>(out)[off + i] = sn::uneg11(v);
        } else {
            static_cast<double *>(out)[off + i] = sn::gaussian(v);
        }
    }
}

// ------------------------------------------------------------------------------------ spectrum
struct SpecTables {
    const double * logfreq;    // [n_binned]
    const double * stepinv;    // [n_binned]
    const double * logpsd;     // [n_stream][n_binned]
    const double * psdshift;   // [n_stream]
    const uint64_t * key2;     // [n_stream]
    int n_binned;
    double increment;          // rate / (fftlen - 1); also the frequency shift
};

// the stream's tables: copied behind each other into LDS when they fit, global memory otherwise
struct StreamTables {
    const double * logfreq;
    const double * stepinv;
    const double * logpsd;
};

__device__ __forceinline__ StreamTables load_tables(const SpecTables & t, int b, double * lds) {
    StreamTables r;
    const double * lp = t.logpsd + (int64_t)b * t.n_binned;
    if (t.n_binned <= kLdsBinned) {
        for (int i = threadIdx.x; i < t.n_binned; i += kThreads) {
            lds[i] = t.logfreq[i];
            lds[t.n_binned + i] = t.stepinv[i];
            lds[2 * t.n_binned + i] = lp[i];
        }
        __syncthreads();
        r.logfreq = lds;
        r.stepinv = lds + t.n_binned;
        r.logpsd = lds + 2 * t.n_binned;
    } else {
        r.logfreq = t.logfreq;
        r.stepinv = t.stepinv;
        r.logpsd = lp;
    }
    return r;
}

__device__ __forceinline__ double scale_at(const SpecTables & t, const StreamTables & st, double psdshift, int64_t k) {
    const double x = log10(t.increment * (double)k + t.increment);
    const int ibin = sn::interp_interval(x, st.logfreq, t.n_binned);
    return sn::interp_scale_at(x, ibin, st.logfreq, st.stepinv, st.logpsd, psdshift);
}

// interpolated amplitudes [n_stream][n_psd] (tests, psd_interp users); bin 0 is 0
__global__ __launch_bounds__(kThreads) void k_sim_psd_interp(SpecTables t, int stream0, int64_t n_psd,
                                                            double * __restrict__ out) {
    __shared__ double lds[3 * kLdsBinned];
    const int b = stream0 + blockIdx.y;
    const StreamTables st = load_tables(t, b, lds);
    const double shift = t.psdshift[b];
    double * o = out + (int64_t)b * n_psd;
    const int64_t k0 = (int64_t)blockIdx.x * (kThreads * kBinsPerThread) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kBinsPerThread; ++j) {
        const int64_t k = k0 + (int64_t)j * kThreads;
        if (k < n_psd) o[k] = (k == 0) ? 0.0 : scale_at(t, st, shift, k);
    }
}

// hermitian-interleaved bins of batch row blockIdx.y (stream stream0 + blockIdx.y)
__global__ __launch_bounds__(kThreads) void k_sim_spectrum(SpecTables t, int stream0, uint64_t key1, uint64_t counter2,
                                                          int64_t fftlen, double2 * __restrict__ fdata) {
    __shared__ double lds[3 * kLdsBinned];
    const int b = stream0 + blockIdx.y;
    const StreamTables st = load_tables(t, b, lds);
    const double shift = t.psdshift[b];
    const uint64_t key2 = t.key2[b];
    const int64_t half = fftlen / 2;
    double2 * f = fdata + (int64_t)blockIdx.y * (half + 1);
    const int64_t k0 = (int64_t)blockIdx.x * (kThreads * kBinsPerThread) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kBinsPerThread; ++j) {
        const int64_t k = k0 + (int64_t)j * kThreads;
        if (k > half) continue;
        double2 v = make_double2(0.0, 0.0);
        if (k > 0) {
            const double scale = scale_at(t, st, shift, k);
            v.x = sn::gaussian(sn::threefry2x64_20(0, counter2 + (uint64_t)k, key1, key2)) * scale;
            if (k < half) v.y = sn::gaussian(sn::threefry2x64_20(0, counter2 + (uint64_t)(fftlen - k), key1, key2)) * scale;
        }
        f[k] = v;
    }
}

// ------------------------------------------------------------------------------------ crop, DC, mix
__device__ __forceinline__ double block_sum_fixed(double v, double * lds) {
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
        __syncthreads();
    }
    return lds[0];
}

__global__ __launch_bounds__(kThreads) void k_crop_partial(const double * __restrict__ tdata, int64_t fftlen,
                                                          int64_t offset, int64_t samples, double scale, int n_chunk,
                                                          double * __restrict__ partial) {
    __shared__ double lds[kThreads];
    const double * x = tdata + (int64_t)blockIdx.y * fftlen + offset;
    const int64_t i0 = (int64_t)blockIdx.x * kCropChunk + threadIdx.x;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < kCropChunk / kThreads; ++j) {
        const int64_t i = i0 + (int64_t)j * kThreads;
        if (i < samples) acc += x[i] * scale;
    }
    const double total = block_sum_fixed(acc, lds);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * n_chunk + blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_crop_dc(const double * __restrict__ partial, int n_chunk, int64_t samples,
                                                     double * __restrict__ dc) {
    __shared__ double lds[kThreads];
    const double * p = partial + (int64_t)blockIdx.x * n_chunk;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunk; i += kThreads) acc += p[i];
    const double total = block_sum_fixed(acc, lds);
    if (threadIdx.x == 0) dc[blockIdx.x] = total / (double)samples;
}

struct MixEntries {
    const int32_t * stream;   // row of the batch
    const int64_t * row;      // row of det_data
    const double * weight;
};

__global__ __launch_bounds__(kThreads) void k_sim_mix(const double * __restrict__ tdata, int64_t fftlen, int64_t offset,
                                                     int64_t samples, double scale, const double * __restrict__ dc,
                                                     MixEntries m, int entry0, double * __restrict__ det_data,
                                                     int64_t row_stride) {
    const int e = entry0 + blockIdx.y;
    const int b = m.stream[e];
    const double w = m.weight[e];
    const double level = dc[b];
    const double * x = tdata + (int64_t)b * fftlen + offset;
    double * out = det_data + m.row[e] * row_stride;
    const int64_t i0 = (int64_t)blockIdx.x * (kThreads * 4) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + (int64_t)j * kThreads;
        if (i < samples) out[i] += w * (x[i] * scale - level);
    }
}

// ------------------------------------------------------------------------------------ host side
int64_t sim_fft_length(int64_t samples, int64_t oversample) {
    int64_t fftlen = 2;
    while (fftlen <= oversample * samples) fftlen *= 2;   // "<=": samples = 4096 takes 2^14
    return fftlen;
}

// The binned tables of toast_tod_simnoise.cpp:14-121 with libm, for n_batch PSDs on one frequency grid.
struct BinnedTables {
    int64_t fftlen = 0;
    double increment = 0.0;
    std::vector<double> logfreq, stepinv, logpsd, psdshift;
};

BinnedTables make_tables(double rate, int64_t samples, int64_t oversample, int64_t n_batch, int64_t n_binned,
                         const double * freq, const double * psds) {
    if (samples <= 0 || oversample <= 0) fail_arg("sim_noise: samples and oversample must be positive");
    if (n_binned < 2) fail_arg("sim_noise: a PSD needs at least two frequencies");
    if (n_batch < 0 || freq == nullptr || (n_batch > 0 && psds == nullptr)) fail_arg("sim_noise: missing PSD arrays");
    BinnedTables t;
    t.fftlen = sim_fft_length(samples, oversample);
    const int64_t psdlen = t.fftlen / 2 + 1;
    const double norm = rate * (double)(psdlen - 1);
    t.increment = rate / (double)(t.fftlen - 1);
    if (freq[0] > t.increment) {
        std::ostringstream o;
        o << "input PSDs have lowest frequency " << freq[0] << "Hz, which does not allow interpolation to "
          << t.increment << "Hz";
        fail_arg(o.str());
    }
    const double nyquist = 0.5 * rate;
    if (std::fabs((freq[n_binned - 1] - nyquist) / nyquist) > 0.01) {
        std::ostringstream o;
        o.precision(16);
        o << "last frequency element does not match Nyquist frequency for given sample rate: " << freq[n_binned - 1]
          << " != " << nyquist;
        fail_arg(o.str());
    }
    t.logfreq.resize((size_t)n_binned);
    t.stepinv.assign((size_t)n_binned, 0.0);
    for (int64_t i = 0; i < n_binned; ++i) t.logfreq[(size_t)i] = ::log10(freq[i] + t.increment);
    for (int64_t i = 0; i + 1 < n_binned; ++i) t.stepinv[(size_t)i] = 1 / (t.logfreq[(size_t)i + 1] - t.logfreq[(size_t)i]);
    t.logpsd.resize((size_t)(n_batch * n_binned));
    t.psdshift.resize((size_t)n_batch);
    for (int64_t b = 0; b < n_batch; ++b) {
        const double * p = psds + b * n_binned;
        double psdmin = 1e30;
        for (int64_t i = 0; i < n_binned; ++i) {
            if (p[i] != 0 && p[i] < psdmin) psdmin = p[i];
        }
        if (psdmin < 0) fail_arg("input PSD values should be >= zero");
        const double shift = 0.01 * psdmin;
        t.psdshift[(size_t)b] = shift;
        for (int64_t i = 0; i < n_binned; ++i) t.logpsd[(size_t)(b * n_binned + i)] = ::log10(::sqrt(p[i] * norm) + shift);
    }
    return t;
}

// interpolated amplitudes of PSD b at every bin, by the reference's forward walk over the bins
void host_interp(const BinnedTables & t, int64_t n_binned, int64_t b, double * out) {
    const int64_t psdlen = t.fftlen / 2 + 1;
    const double * lp = t.logpsd.data() + b * n_binned;
    int64_t ibin = 0;
    for (int64_t i = 0; i < psdlen; ++i) {
        const double x = ::log10(t.increment * (double)i + t.increment);
        while (ibin < n_binned - 2 && t.logfreq[(size_t)ibin + 1] < x) ++ibin;
        out[i] = sn::interp_scale_at(x, (int)ibin, t.logfreq.data(), t.stepinv.data(), lp, t.psdshift[(size_t)b]);
    }
    out[0] = 0;
}

template <int KIND, typename T>
void host_rng(size_t n, uint64_t key1, uint64_t key2, uint64_t counter1, uint64_t counter2, T * data) {
    for (size_t i = 0; i < n; ++i) {
        const uint64_t v = sn::threefry2x64_20(counter1, counter2 + i, key1, key2);
        if (KIND == sn::kUint64) {
            data[i] = (T)v;
        } else if (KIND == sn::kUniform01) {
            data[i] = (T)sn::u01(v);
        } else if (KIND == sn::kUniform11) {
            data[i] = (T)sn::uneg11(v);
        } else {
            data[i] = (T)sn::gaussian(v);
        }
    }
}

// Unscaled hc2r of a power-of-two length in extended precision (the host entries are a fidelity path: their transform
// error stays far below that of any double-precision FFT they are compared with).  Radix-2, decimation in time.
void host_hc2r(int64_t n, const double * hc, double * out) {
    typedef std::complex<long double> cld;
    std::vector<cld> a((size_t)n);
    int bits = 0;
    while ((int64_t(1) << bits) < n) ++bits;
    auto rev = [bits](int64_t i) {
        int64_t r = 0;
        for (int j = 0; j < bits; ++j) r |= ((i >> j) & 1) << (bits - 1 - j);
        return r;
    };
    for (int64_t k = 0; k <= n / 2; ++k) {
        const long double im = (k > 0 && 2 * k < n) ? hc[n - k] : 0.0;
        a[(size_t)rev(k)] = cld(hc[k], im);
        if (k > 0 && 2 * k < n) a[(size_t)rev(n - k)] = cld(hc[k], -im);
    }
    std::vector<cld> w((size_t)(n / 2 > 0 ? n / 2 : 1));
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int64_t k = 0; k < n / 2; ++k) {
        const long double ang = two_pi * (long double)k / (long double)n;
        w[(size_t)k] = cld(cosl(ang), sinl(ang));   // e^{+i ...}: the backward transform
    }
    for (int64_t len = 2; len <= n; len <<= 1) {
        const int64_t halfl = len / 2, step = n / len;
        for (int64_t s = 0; s < n; s += len) {
            for (int64_t j = 0; j < halfl; ++j) {
                const cld u = a[(size_t)(s + j)];
                const cld v = a[(size_t)(s + j + halfl)] * w[(size_t)(j * step)];
                a[(size_t)(s + j)] = u + v;
                a[(size_t)(s + j + halfl)] = u - v;
            }
        }
    }
    for (int64_t i = 0; i < n; ++i) out[i] = (double)a[(size_t)i].real();
}

// one timestream of toast_tod_simnoise.cpp:154-228 from the tables of its PSD
void host_timestream(const BinnedTables & t, int64_t n_binned, int64_t b, uint64_t key1, uint64_t key2,
                     int64_t firstsamp, int64_t samples, int64_t oversample, double * noise) {
    const int64_t n = t.fftlen;
    std::vector<double> interp((size_t)(n / 2 + 1)), hc((size_t)n), td((size_t)n);
    host_interp(t, n_binned, b, interp.data());
    host_rng<sn::kNormal>((size_t)n, key1, key2, 0, (uint64_t)(firstsamp * oversample), hc.data());
    hc[0] *= interp[0];
    for (int64_t i = 1; i < n / 2; ++i) {
        hc[(size_t)i] *= interp[(size_t)i];
        hc[(size_t)(n - i)] *= interp[(size_t)i];
    }
    hc[(size_t)(n / 2)] *= interp[(size_t)(n / 2)];
    host_hc2r(n, hc.data(), td.data());
    const double scale = 1.0 / (double)n;
    const int64_t offset = (n - samples) / 2;
    for (int64_t i = 0; i < samples; ++i) noise[i] = td[(size_t)(offset + i)] * scale;
    double dc = 0;
    for (int64_t i = 0; i < samples; ++i) dc += noise[i];
    dc /= (double)samples;
    for (int64_t i = 0; i < samples; ++i) noise[i] -= dc;
}

uint64_t noise_key1(uint64_t realization, uint64_t telescope, uint64_t component) {
    return realization * 4294967296ull + telescope * 65536ull + component;
}

SpecTables push_tables(ParamBlock & pb, const BinnedTables & t, int64_t n_stream, int64_t n_binned,
                       const std::vector<uint64_t> & key2, size_t (&off)[5]) {
    off[0] = pb.push_vec(t.logfreq);
    off[1] = pb.push_vec(t.stepinv);
    off[2] = pb.push_vec(t.logpsd);
    off[3] = pb.push_vec(t.psdshift);
    off[4] = pb.push_vec(key2);
    SpecTables s{};
    s.n_binned = (int)n_binned;
    s.increment = t.increment;
    return s;
}

void bind_tables(SpecTables & s, const char * d, const size_t (&off)[5]) {
    s.logfreq = (const double *)(d + off[0]);
    s.stepinv = (const double *)(d + off[1]);
    s.logpsd = (const double *)(d + off[2]);
    s.psdshift = (const double *)(d + off[3]);
    s.key2 = (const uint64_t *)(d + off[4]);
}

void check_monotone(const double * freq, int64_t n_binned) {
    for (int64_t i = 1; i < n_binned; ++i) {
        if (!(freq[i] >= freq[i - 1])) fail_arg("sim_noise: PSD frequencies must not decrease");
    }
}

template <int KIND>
void rng_multi_dev(int64_t n_stream, const size_t * ndata, const uint64_t * key1, const uint64_t * key2,
                   const uint64_t * counter1, const uint64_t * counter2, const int64_t * offsets, void * d_out,
                   int64_t out_len, void * stream) {
    if (n_stream <= 0) return;
    if (!ndata || !key1 || !key2 || !counter1 || !counter2 || !d_out) fail_arg("rng_dist: missing argument");
    Manager::get().require_device();
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
    std::vector<uint64_t> len((size_t)n_stream), off((size_t)n_stream);
    uint64_t next = 0, longest = 0;
    for (int64_t s = 0; s < n_stream; ++s) {
        len[(size_t)s] = (uint64_t)ndata[s];
        if (offsets != nullptr && offsets[s] < 0) fail_arg("rng_dist: negative output offset");
        off[(size_t)s] = offsets ? (uint64_t)offsets[s] : next;
        next += len[(size_t)s];
        if (off[(size_t)s] + len[(size_t)s] > (uint64_t)out_len) fail_arg("rng_dist: a stream ends beyond the output buffer");
        longest = std::max(longest, len[(size_t)s]);
    }
    if (longest == 0) return;
    ParamBlock pb;
    const size_t o1 = pb.push(key1, sizeof(uint64_t) * n_stream), o2 = pb.push(key2, sizeof(uint64_t) * n_stream);
    const size_t o3 = pb.push(counter1, sizeof(uint64_t) * n_stream), o4 = pb.push(counter2, sizeof(uint64_t) * n_stream);
    const size_t o5 = pb.push_vec(len), o6 = pb.push_vec(off);
    const char * d = pb.commit(st);
    RngStreams rs{(const uint64_t *)(d + o1), (const uint64_t *)(d + o2), (const uint64_t *)(d + o3),
                  (const uint64_t *)(d + o4), (const uint64_t *)(d + o5), (const uint64_t *)(d + o6)};
    const uint64_t gx = std::min<uint64_t>((longest + kThreads - 1) / kThreads, 16384);
    for (int64_t s0 = 0; s0 < n_stream; s0 += kMaxGridY) {
        const int64_t ns = std::min(kMaxGridY, n_stream - s0);
        hipLaunchKernelGGL(k_rng_multi<KIND>, dim3((unsigned)gx, (unsigned)ns), dim3(kThreads), 0, st, rs, (int)s0, d_out);
    }
    TH_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------- host entries
int toast_hip_rng_dist_uint64(size_t n, uint64_t key1, uint64_t key2, uint64_t counter1, uint64_t counter2,
                              uint64_t * data) {
    return guarded([&] { host_rng<sn::kUint64>(n, key1, key2, counter1, counter2, data); });
}
int toast_hip_rng_dist_uniform_01(size_t n, uint64_t key1, uint64_t key2, uint64_t counter1, uint64_t counter2,
                                  double * data) {
    return guarded([&] { host_rng<sn::kUniform01>(n, key1, key2, counter1, counter2, data); });
}
int toast_hip_rng_dist_uniform_11(size_t n, uint64_t key1, uint64_t key2, uint64_t counter1, uint64_t counter2,
                                  double * data) {
    return guarded([&] { host_rng<sn::kUniform11>(n, key1, key2, counter1, counter2, data); });
}
int toast_hip_rng_dist_normal(size_t n, uint64_t key1, uint64_t key2, uint64_t counter1, uint64_t counter2,
                              double * data) {
    return guarded([&] { host_rng<sn::kNormal>(n, key1, key2, counter1, counter2, data); });
}
int toast_hip_rng_multi_dist_uint64(size_t nstream, const size_t * ndata, const uint64_t * key1, const uint64_t * key2,
                                    const uint64_t * counter1, const uint64_t * counter2, uint64_t ** data) {
    return guarded([&] {
        for (size_t s = 0; s < nstream; ++s) host_rng<sn::kUint64>(ndata[s], key1[s], key2[s], counter1[s], counter2[s], data[s]);
    });
}
int toast_hip_rng_multi_dist_uniform_01(size_t nstream, const size_t * ndata, const uint64_t * key1,
                                        const uint64_t * key2, const uint64_t * counter1, const uint64_t * counter2,
                                        double ** data) {
    return guarded([&] {
        for (size_t s = 0; s < nstream; ++s) host_rng<sn::kUniform01>(ndata[s], key1[s], key2[s], counter1[s], counter2[s], data[s]);
    });
}
int toast_hip_rng_multi_dist_uniform_11(size_t nstream, const size_t * ndata, const uint64_t * key1,
                                        const uint64_t * key2, const uint64_t * counter1, const uint64_t * counter2,
                                        double ** data) {
    return guarded([&] {
        for (size_t s = 0; s < nstream; ++s) host_rng<sn::kUniform11>(ndata[s], key1[s], key2[s], counter1[s], counter2[s], data[s]);
    });
}
int toast_hip_rng_multi_dist_normal(size_t nstream, const size_t * ndata, const uint64_t * key1, const uint64_t * key2,
                                    const uint64_t * counter1, const uint64_t * counter2, double ** data) {
    return guarded([&] {
        for (size_t s = 0; s < nstream; ++s) host_rng<sn::kNormal>(ndata[s], key1[s], key2[s], counter1[s], counter2[s], data[s]);
    });
}

int64_t toast_hip_sim_noise_fft_length(int64_t samples, int64_t oversample) {
    if (samples <= 0 || oversample <= 0) return 0;
    return sim_fft_length(samples, oversample);
}

int toast_hip_tod_sim_noise_psd_interp(double rate, int64_t samples, int64_t oversample, int64_t n_batch,
                                       int64_t n_binned, const double * binned_freq, const double * binned_psds,
                                       double * interp_psds) {
    return guarded([&] {
        const BinnedTables t = make_tables(rate, samples, oversample, n_batch, n_binned, binned_freq, binned_psds);
        for (int64_t b = 0; b < n_batch; ++b) host_interp(t, n_binned, b, interp_psds + b * (t.fftlen / 2 + 1));
    });
}

int toast_hip_tod_sim_noise_timestream(uint64_t realization, uint64_t telescope, uint64_t component, uint64_t obsindx,
                                       uint64_t detindx, double rate, int64_t firstsamp, int64_t samples,
                                       int64_t oversample, const double * freq, const double * psd, int64_t psdlen,
                                       double * noise) {
    return guarded([&] {
        const BinnedTables t = make_tables(rate, samples, oversample, 1, psdlen, freq, psd);
        host_timestream(t, psdlen, 0, noise_key1(realization, telescope, component), obsindx * 4294967296ull + detindx,
                        firstsamp, samples, oversample, noise);
    });
}

int toast_hip_tod_sim_noise_timestream_batch(uint64_t realization, uint64_t telescope, uint64_t component,
                                             uint64_t obsindx, double rate, int64_t firstsamp, int64_t samples,
                                             int64_t oversample, int64_t ndet, const uint64_t * detindices,
                                             int64_t psdlen, const double * freq, const double * psds, double * noise) {
    return guarded([&] {
        if (ndet <= 0) return;
        const BinnedTables t = make_tables(rate, samples, oversample, ndet, psdlen, freq, psds);
        for (int64_t d = 0; d < ndet; ++d) {
            host_timestream(t, psdlen, d, noise_key1(realization, telescope, component),
                            obsindx * 4294967296ull + detindices[d], firstsamp, samples, oversample, noise + d * samples);
        }
    });
}

// ---------------------------------------------------------------------------------- device entries
int toast_hip_rng_dist_uint64_dev(int64_t n_stream, const size_t * ndata, const uint64_t * key1, const uint64_t * key2,
                                  const uint64_t * counter1, const uint64_t * counter2, const int64_t * offsets,
                                  uint64_t * d_out, int64_t out_len, void * stream) {
    return guarded([&] { rng_multi_dev<sn::kUint64>(n_stream, ndata, key1, key2, counter1, counter2, offsets, d_out, out_len, stream); });
}
int toast_hip_rng_dist_uniform_01_dev(int64_t n_stream, const size_t * ndata, const uint64_t * key1,
                                      const uint64_t * key2, const uint64_t * counter1, const uint64_t * counter2,
                                      const int64_t * offsets, double * d_out, int64_t out_len, void * stream) {
    return guarded([&] { rng_multi_dev<sn::kUniform01>(n_stream, ndata, key1, key2, counter1, counter2, offsets, d_out, out_len, stream); });
}
int toast_hip_rng_dist_uniform_11_dev(int64_t n_stream, const size_t * ndata, const uint64_t * key1,
                                      const uint64_t * key2, const uint64_t * counter1, const uint64_t * counter2,
                                      const int64_t * offsets, double * d_out, int64_t out_len, void * stream) {
    return guarded([&] { rng_multi_dev<sn::kUniform11>(n_stream, ndata, key1, key2, counter1, counter2, offsets, d_out, out_len, stream); });
}
int toast_hip_rng_dist_normal_dev(int64_t n_stream, const size_t * ndata, const uint64_t * key1, const uint64_t * key2,
                                  const uint64_t * counter1, const uint64_t * counter2, const int64_t * offsets,
                                  double * d_out, int64_t out_len, void * stream) {
    return guarded([&] { rng_multi_dev<sn::kNormal>(n_stream, ndata, key1, key2, counter1, counter2, offsets, d_out, out_len, stream); });
}

int toast_hip_sim_noise_psd_interp_dev(double rate, int64_t samples, int64_t oversample, int64_t n_stream,
                                       int64_t n_binned, const double * freq, const double * psds,
                                       double * d_interp, void * stream) {
    return guarded([&] {
        if (n_stream <= 0) return;
        if (d_interp == nullptr) fail_arg("sim_noise_psd_interp: missing output");
        const BinnedTables t = make_tables(rate, samples, oversample, n_stream, n_binned, freq, psds);
        check_monotone(freq, n_binned);
        Manager::get().require_device();
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
        ParamBlock pb;
        size_t off[5];
        SpecTables tab = push_tables(pb, t, n_stream, n_binned, std::vector<uint64_t>((size_t)n_stream, 0), off);
        bind_tables(tab, pb.commit(st), off);
        const int64_t n_psd = t.fftlen / 2 + 1;
        const int64_t per_block = kThreads * kBinsPerThread;
        const unsigned gx = (unsigned)((n_psd + per_block - 1) / per_block);
        for (int64_t s0 = 0; s0 < n_stream; s0 += kMaxGridY) {
            const int64_t ns = std::min(kMaxGridY, n_stream - s0);
            hipLaunchKernelGGL(k_sim_psd_interp, dim3(gx, (unsigned)ns), dim3(kThreads), 0, st, tab, (int)s0, n_psd, d_interp);
        }
        TH_HIP(hipGetLastError());
    });
}

int toast_hip_sim_noise_dev(uint64_t realization, uint64_t telescope, uint64_t component, uint64_t obsindx, double rate,
                            int64_t firstsamp, int64_t samples, int64_t oversample, int64_t n_stream,
                            const uint64_t * detindices, int64_t n_binned, const double * freq, const double * psds,
                            const int64_t * mix_ptr, const int32_t * mix_row, const double * mix_weight,
                            double * d_det_data, int64_t n_rows, int64_t row_stride, int64_t max_batch, void * stream) {
    return guarded([&] {
        if (n_stream <= 0) return;
        if (detindices == nullptr || d_det_data == nullptr) fail_arg("sim_noise: missing argument");
        if (row_stride < samples) fail_arg("sim_noise: det_data rows are shorter than the simulated samples");
        if ((mix_ptr == nullptr) != (mix_row == nullptr) || (mix_ptr == nullptr) != (mix_weight == nullptr)) {
            fail_arg("sim_noise: the mixing matrix needs all three CSR arrays");
        }
        const BinnedTables t = make_tables(rate, samples, oversample, n_stream, n_binned, freq, psds);
        check_monotone(freq, n_binned);
        // CSR of the mixing matrix by stream; default: stream s -> row s with weight 1
        std::vector<int64_t> ptr((size_t)n_stream + 1);
        std::vector<int64_t> rows;
        std::vector<double> weights;
        if (mix_ptr == nullptr) {
            for (int64_t s = 0; s <= n_stream; ++s) ptr[(size_t)s] = s;
            rows.resize((size_t)n_stream);
            weights.assign((size_t)n_stream, 1.0);
            for (int64_t s = 0; s < n_stream; ++s) rows[(size_t)s] = s;
        } else {
            if (mix_ptr[0] != 0) fail_arg("sim_noise: mix_ptr must start at 0");
            for (int64_t s = 0; s < n_stream; ++s) {
                if (mix_ptr[s + 1] < mix_ptr[s]) fail_arg("sim_noise: mix_ptr must not decrease");
            }
            ptr.assign(mix_ptr, mix_ptr + n_stream + 1);
            rows.assign(mix_row, mix_row + ptr[(size_t)n_stream]);
            weights.assign(mix_weight, mix_weight + ptr[(size_t)n_stream]);
        }
        for (int64_t r : rows) {
            if (r < 0 || r >= n_rows) fail_arg("sim_noise: a mixing matrix row lies outside det_data");
        }
        Manager::get().require_device();
        hipStream_t st = stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
        const int64_t fftlen = t.fftlen, n_psd = fftlen / 2 + 1;
        const int64_t offset = (fftlen - samples) / 2;
        const double scale = 1.0 / (double)fftlen;
        const int n_chunk = (int)((samples + kCropChunk - 1) / kCropChunk);

        int64_t batch = (max_batch > 0) ? max_batch : 64;
        // The two work buffers are grow-only scratch blocks of the arena, which takes further slabs from the driver on
        // demand: they are bounded by 80 % of what the device and the arena's free ranges can still give (plus what an
        // earlier call of this entry already holds), and by 8 GB.  The result does not depend on the batch.
        const size_t per_stream = (size_t)fftlen * 8 + (size_t)n_psd * 16;
        size_t free_bytes = 0, total_bytes = 0;
        if (toast_hip_accel_mem_info(&free_bytes, &total_bytes) != TOAST_HIP_OK) throw Error(TOAST_HIP_ERR_DEVICE, toast_hip_last_error());
        const size_t budget = std::min<size_t>(size_t(8) << 30, (size_t)(0.8 * (double)free_bytes) + g_scratch_held);
        const int64_t cap = (int64_t)(budget / per_stream);
        batch = std::max<int64_t>(1, std::min(std::min(batch, cap), std::min(n_stream, kMaxGridY)));
        g_scratch_held = std::max(g_scratch_held, (size_t)batch * per_stream);

        std::vector<uint64_t> key2((size_t)n_stream);
        for (int64_t s = 0; s < n_stream; ++s) key2[(size_t)s] = obsindx * 4294967296ull + detindices[s];
        const uint64_t key1 = noise_key1(realization, telescope, component);
        const uint64_t counter2 = (uint64_t)(firstsamp * oversample);

        // batch-local stream index of every entry
        std::vector<int32_t> ent_stream(rows.size());
        for (int64_t s = 0; s < n_stream; ++s) {
            for (int64_t e = ptr[(size_t)s]; e < ptr[(size_t)s + 1]; ++e) ent_stream[(size_t)e] = (int32_t)(s % batch);
        }
        ParamBlock pb;
        size_t off[5];
        SpecTables tab = push_tables(pb, t, n_stream, n_binned, key2, off);
        const size_t o_es = pb.push_vec(ent_stream), o_er = pb.push_vec(rows), o_ew = pb.push_vec(weights);
        const char * d = pb.commit(st);
        bind_tables(tab, d, off);
        const MixEntries mix{(const int32_t *)(d + o_es), (const int64_t *)(d + o_er), (const double *)(d + o_ew)};

        double2 * fbuf = (double2 *)Manager::get().scratch(Manager::kScratchFftFreq, (size_t)batch * n_psd * sizeof(double2));
        double * tbuf = (double *)Manager::get().scratch(Manager::kScratchFftTime, (size_t)batch * fftlen * sizeof(double));
        double * red = (double *)Manager::get().scratch(Manager::kScratchSimNoise,
                                                        (size_t)batch * ((size_t)n_chunk + 1) * sizeof(double), st);
        double * d_partial = red;
        double * d_dc = red + (size_t)batch * n_chunk;

        const int64_t per_block = kThreads * kBinsPerThread;
        const unsigned gx_spec = (unsigned)((n_psd + per_block - 1) / per_block);
        const unsigned gx_mix = (unsigned)((samples + kThreads * 4 - 1) / (kThreads * 4));
        std::vector<char> seen((size_t)n_rows);
        std::vector<hipEvent_t> marks;      // timing switch: four events per batch
        auto mark = [&]() {
            if (!g_timing) return;
            hipEvent_t e;
            TH_HIP(hipEventCreate(&e));
            TH_HIP(hipEventRecord(e, st));
            marks.push_back(e);
        };
        for (int64_t s0 = 0; s0 < n_stream; s0 += batch) {
            const int64_t nb = std::min(batch, n_stream - s0);
            mark();
            hipLaunchKernelGGL(k_sim_spectrum, dim3(gx_spec, (unsigned)nb), dim3(kThreads), 0, st, tab, (int)s0, key1,
                               counter2, fftlen, fbuf);
            mark();
            fft_c2r_exec(fftlen, nb, fbuf, tbuf, st);
            mark();
            hipLaunchKernelGGL(k_crop_partial, dim3((unsigned)n_chunk, (unsigned)nb), dim3(kThreads), 0, st, tbuf, fftlen,
                               offset, samples, scale, n_chunk, d_partial);
            hipLaunchKernelGGL(k_crop_dc, dim3((unsigned)nb), dim3(kThreads), 0, st, d_partial, n_chunk, samples, d_dc);
            // Streams that add to the same row are added one after the other in stream order (the reference's loop over
            // keys, sim_tod_noise.py:304-326); rows that one stream alone touches go in one launch.
            const int64_t e0 = ptr[(size_t)s0], e1 = ptr[(size_t)(s0 + nb)];
            bool shared_row = false;
            std::fill(seen.begin(), seen.end(), 0);
            for (int64_t e = e0; e < e1 && !shared_row; ++e) {
                if (seen[(size_t)rows[(size_t)e]]) shared_row = true;
                seen[(size_t)rows[(size_t)e]] = 1;
            }
            auto launch_mix = [&](int64_t a, int64_t b) {
                for (int64_t c = a; c < b; c += kMaxGridY) {
                    const int64_t ne = std::min(kMaxGridY, b - c);
                    hipLaunchKernelGGL(k_sim_mix, dim3(gx_mix, (unsigned)ne), dim3(kThreads), 0, st, tbuf, fftlen, offset,
                                       samples, scale, d_dc, mix, (int)c, d_det_data, row_stride);
                }
            };
            if (!shared_row) {
                launch_mix(e0, e1);
            } else {
                for (int64_t s = s0; s < s0 + nb; ++s) {
                    // one stream names a row once: entries of the same stream with equal rows go one by one
                    bool dup = false;
                    for (int64_t e = ptr[(size_t)s]; e < ptr[(size_t)s + 1] && !dup; ++e) {
                        for (int64_t g = ptr[(size_t)s]; g < e; ++g) dup = dup || rows[(size_t)g] == rows[(size_t)e];
                    }
                    if (!dup) {
                        launch_mix(ptr[(size_t)s], ptr[(size_t)s + 1]);
                    } else {
                        for (int64_t e = ptr[(size_t)s]; e < ptr[(size_t)s + 1]; ++e) launch_mix(e, e + 1);
                    }
                }
            }
            mark();
            TH_HIP(hipGetLastError());
        }
        if (g_timing) {
            TH_HIP(hipStreamSynchronize(st));
            g_phase_ms[0] = g_phase_ms[1] = g_phase_ms[2] = 0.0;
            for (size_t i = 0; i + 3 < marks.size(); i += 4) {
                for (int ph = 0; ph < 3; ++ph) {
                    float ms = 0.0f;
                    TH_HIP(hipEventElapsedTime(&ms, marks[i + ph], marks[i + ph + 1]));
                    g_phase_ms[ph] += (double)ms;
                }
            }
            for (hipEvent_t e : marks) (void)hipEventDestroy(e);
        }
    });
}

int toast_hip_sim_noise_timing(int on, double * phase_ms) {
    g_timing = on ? 1 : 0;
    if (phase_ms != nullptr) {
        for (int ph = 0; ph < 3; ++ph) phase_ms[ph] = g_phase_ms[ph];
    }
    return TOAST_HIP_OK;
}

}  // extern "C"
