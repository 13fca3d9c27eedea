// demod.hip -- half-wave-plate demodulation on gfx950.
//
// Counterpart of the per-sample work of the reference's Demodulate / StokesWeightsDemod operators
// (src/toast/ops/demodulation.py):
//   * Lowpass.__call__ / Bandpass.__call__ (:58-61, :87-89) and the modulation of _demodulate_signal (:726-765):
//     toast_hip_demod_fir_dev, a batched direct-form FIR "same" convolution with optional modulation of the input and
//     decimation of the output,
//   * _demodulate_flag (:700-705): toast_hip_demod_flags_dev,
//   * the constant weights of StokesWeightsDemod._exec (:1060-1114): toast_hip_stokes_weights_demod_dev.
//
// k_demod_fir: out[e][j] = sum_k h[k] y[i_j + c - k], i_j = start + j nskip, c = (W - 1) / 2, y = m x inside the row and
// zero outside.  The taps are split into nskip phases, k = q nskip + t: for one phase the inputs of consecutive outputs
// and consecutive q are consecutive elements of y_t[m] = y[start + c - t + m nskip], i.e. a stride-one convolution
// whatever nskip is.  A workgroup owns an entry and a tile of 2048 outputs.  Per phase and per 512 values of q it stages
// the 2048 + 512 elements of y_t it needs in LDS, reversed (so that the index grows with q) and modulated on the way;
// every lane owns 8 consecutive outputs in registers and slides its window over the staged elements by one 8-byte LDS
// read per 8 FMAs (one pad double per eight: the 64-byte lane stride is free of bank conflicts).  The taps of a phase
// are contiguous in a table built by the host entry; their address is wave-uniform.  An output is the chain
//     for t in phases: for q ascending: acc = fma(h[q nskip + t], y, acc)
// of explicit FMAs: zero taps and zero samples leave acc unchanged, so neither the tile, the staging length, the batch
// nor the order of the entries changes one bit.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "runtime.hpp"

using namespace toast_hip;

namespace {

constexpr int kThreads = 256;
constexpr int kR = 8;                            // outputs per lane
constexpr int kTile = kThreads * kR;             // outputs per workgroup
constexpr int kQ = TOAST_HIP_DEMOD_TAP_CHUNK;    // taps of one phase staged at a time (a multiple of kR)
constexpr int kZLen = kTile + kQ;
constexpr int kZPad = kZLen + kZLen / 8;
constexpr int64_t kMaxGridY = 65535;

static_assert(kQ % kR == 0, "the tap chunk is walked kR taps at a time");

int g_timing = 0;                                // toast_hip_demod_timing
double g_phase_ms[4] = {0.0, 0.0, 0.0, 0.0};     // plain FIR, modulated FIR, flags, weights

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
    }
    ~PhaseTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

struct FirArgs {
    const double * in;            // [row][in_stride]
    int64_t in_stride;
    const int32_t * in_row;       // [n_entry]
    int mode;                     // TOAST_HIP_DEMOD_MOD_*
    const double * mod;           // mode 1: [row][n][nnz] Stokes weights; mode 2: [row][n]
    int64_t mod_stride;           // doubles per row of mod
    const int32_t * mod_row;      // [n_entry]
    const int32_t * mod_comp;     // [n_entry] mode 1: the component that modulates
    int nnz;
    int comp_q;                   // mode 1: Q is component comp_q, U is comp_q + 1
    double * out;                 // [row][out_stride]
    int64_t out_stride;
    const int32_t * out_row;      // [n_entry]
    int64_t n, n_out;
    int64_t nskip, start, c;
    int64_t n_phase;              // min(nskip, W)
    int64_t q_len;                // taps per phase in the table, a multiple of kR
};

__device__ __forceinline__ int zpad(int k) { return k + (k >> 3); }

__global__ __launch_bounds__(kThreads) void k_demod_fir(FirArgs a, const double * __restrict__ taps, int e0) {
    __shared__ double zs[kZPad];
    const int e = e0 + (int)blockIdx.y;
    const int64_t j0 = (int64_t)blockIdx.x * kTile;
    const double * __restrict__ x = a.in + (int64_t)a.in_row[e] * a.in_stride;
    const double * __restrict__ m = a.mode != 0 ? a.mod + (int64_t)a.mod_row[e] * a.mod_stride : nullptr;
    const int comp = a.mode == 1 ? a.mod_comp[e] : 0;
    const int base = (int)threadIdx.x * kR;
    double acc[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = 0.0;
    for (int64_t t = 0; t < a.n_phase; ++t) {
        const double * __restrict__ h = taps + t * a.q_len;
        for (int64_t q0 = 0; q0 < a.q_len; q0 += kQ) {
            const int qn = (int)min((int64_t)kQ, a.q_len - q0);
            const int nz = kTile + qn;
            // staged element v is y[top - v nskip]; nothing to add when the whole span lies outside the row
            const int64_t top = a.start + a.c - t + (j0 + (kTile - 1) - q0) * a.nskip;
            if (top < 0 || top - (int64_t)(nz - 1) * a.nskip >= a.n) continue;
            __syncthreads();
            for (int v = (int)threadIdx.x; v < nz; v += kThreads) {
                const int64_t idx = top - (int64_t)v * a.nskip;
                double y = 0.0;
                if (idx >= 0 && idx < a.n) {
                    y = x[idx];
                    if (a.mode == 1) {
                        // demodulation.py:728-730, :739-740: (signal * 2) * (w_c * (1 / sqrt(w_q^2 + w_u^2)))
                        const double * w = m + idx * a.nnz;
                        const double wq = w[a.comp_q], wu = w[a.comp_q + 1];
                        const double etainv = 1.0 / sqrt(wq * wq + wu * wu);
                        y = (y * 2.0) * ((comp == a.comp_q ? wq : wu) * etainv);
                    } else if (a.mode == 2) {
                        y = y * m[idx];
                    }
                }
                zs[zpad(v)] = y;
            }
            __syncthreads();
            // lane's accumulator r is output j0 + kTile - 1 - (base + r); w[(u + r) % kR] holds staged element
            // i + u + base + r: the window slides without moving a register
            double w[kR];
#pragma unroll
            for (int r = 0; r < kR - 1; ++r) w[r] = zs[zpad(base + r)];
            const double * __restrict__ hq = h + q0;
            for (int i = 0; i < qn; i += kR) {
#pragma unroll
                for (int u = 0; u < kR; ++u) {
                    w[(u + kR - 1) % kR] = zs[zpad(i + u + base + kR - 1)];
                    const double hk = hq[i + u];
#pragma unroll
                    for (int r = 0; r < kR; ++r) acc[r] = __builtin_fma(hk, w[(u + r) % kR], acc[r]);
                }
            }
        }
    }
    double * __restrict__ out = a.out + (int64_t)a.out_row[e] * a.out_stride;
#pragma unroll
    for (int r = 0; r < kR; ++r) {
        const int64_t j = j0 + (kTile - 1) - (base + r);
        if (j < a.n_out) out[j] = acc[r];
    }
}

// demodulation.py:700-705
__global__ __launch_bounds__(kThreads) void k_demod_flags(int64_t n, int64_t n_out, int64_t wkernel, uint8_t mask,
                                                          int64_t nskip, int64_t start, const uint8_t * __restrict__ in,
                                                          int64_t in_stride, const int32_t * __restrict__ in_row,
                                                          uint8_t * __restrict__ out, int64_t out_stride,
                                                          const int32_t * __restrict__ out_row) {
    const int e = (int)blockIdx.y;
    const uint8_t * f = in + (int64_t)in_row[e] * in_stride;
    uint8_t * o = out + (int64_t)out_row[e] * out_stride;
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < n_out; j += (int64_t)gridDim.x * kThreads) {
        const int64_t i = start + j * nskip;
        const bool end = i < wkernel || i >= n - wkernel;
        o[j] = end ? (uint8_t)(f[i] | mask) : f[i];
    }
}

// demodulation.py:1060-1114: every sample of a pseudo-detector has the same weights
template <typename T>
__global__ __launch_bounds__(kThreads) void k_weights_fill(int64_t n_samp, int nnz, const double * __restrict__ values,
                                                           const int32_t * __restrict__ out_row, T * __restrict__ weights) {
    const int e = (int)blockIdx.y;
    const int64_t count = n_samp * nnz;
    T * o = weights + (int64_t)out_row[e] * count;
    const double * v = values + (int64_t)e * nnz;
    for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < count; k += (int64_t)gridDim.x * kThreads) {
        o[k] = (T)v[k % nnz];
    }
}

unsigned grid_x(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 1 << 20)); }

hipStream_t pick_stream(void * stream) {
    Manager::get().require_device();
    return stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
}

void check_rows(const int32_t * rows, int64_t n, int64_t limit, const char * what) {
    for (int64_t r = 0; r < n; ++r) {
        if (rows[r] < 0 || rows[r] >= limit) fail_arg(std::string(what) + ": an entry names a row outside its array");
    }
}

}  // namespace

extern "C" {

int toast_hip_demod_fir_dev(int64_t n_entry, int64_t n, int64_t n_taps, const double * taps, int64_t nskip, int64_t offset,
                            const double * d_in, int64_t n_in_rows, int64_t in_stride, const int32_t * in_row,
                            int mod_mode, const double * d_mod, int64_t n_mod_rows, int64_t mod_stride,
                            const int32_t * mod_row, const int32_t * mod_comp, int64_t nnz, int64_t comp_q,
                            double * d_out, int64_t n_out_rows, int64_t out_stride, const int32_t * out_row,
                            void * stream) {
    return guarded([&] {
        if (n_entry <= 0) return;
        if (n < 1 || n_taps < 1 || nskip < 1 || offset < 0) fail_arg("demod_fir: n, n_taps and nskip must be at least one");
        if (!taps || !d_in || !in_row || !d_out || !out_row) fail_arg("demod_fir: missing argument");
        const int64_t start = offset % nskip;
        const int64_t n_out = start < n ? (n - start + nskip - 1) / nskip : 0;
        if (n_out == 0) return;
        if (n > in_stride || n_out > out_stride) fail_arg("demod_fir: rows are shorter than their samples");
        if (n > (int64_t(1) << 40) || n_taps > (int64_t(1) << 30)) fail_arg("demod_fir: sizes out of range");
        check_rows(in_row, n_entry, n_in_rows, "demod_fir");
        check_rows(out_row, n_entry, n_out_rows, "demod_fir");
        if (mod_mode == TOAST_HIP_DEMOD_MOD_WEIGHTS) {
            if (!d_mod || !mod_row || !mod_comp) fail_arg("demod_fir: modulation by weights needs the weights, rows and components");
            if (nnz < 2 || comp_q < 0 || comp_q + 1 >= nnz) fail_arg("demod_fir: the weights have no Q and U component there");
            if (mod_stride < n * nnz) fail_arg("demod_fir: weight rows are shorter than n x nnz");
            check_rows(mod_row, n_entry, n_mod_rows, "demod_fir");
            for (int64_t e = 0; e < n_entry; ++e) {
                if (mod_comp[e] != comp_q && mod_comp[e] != comp_q + 1) fail_arg("demod_fir: the modulating component is Q or U");
            }
        } else if (mod_mode == TOAST_HIP_DEMOD_MOD_ARRAY) {
            if (!d_mod || !mod_row) fail_arg("demod_fir: modulation by an array needs the array and its rows");
            if (mod_stride < n) fail_arg("demod_fir: modulation rows are shorter than n");
            check_rows(mod_row, n_entry, n_mod_rows, "demod_fir");
        } else if (mod_mode != TOAST_HIP_DEMOD_MOD_NONE) {
            fail_arg("demod_fir: unknown modulation mode");
        }
        const int64_t n_tile = (n_out + kTile - 1) / kTile;
        if (n_tile > 0x7fffffff) fail_arg("demod_fir: too many tiles for one launch");

        // the taps by phase: table[t][q] = h[q nskip + t], zero past the end, rows padded to a multiple of kR
        const int64_t n_phase = std::min(nskip, n_taps);
        const int64_t per_phase = (n_taps + nskip - 1) / nskip;
        const int64_t q_len = (per_phase + kR - 1) / kR * kR;
        std::vector<double> table((size_t)(n_phase * q_len), 0.0);
        for (int64_t k = 0; k < n_taps; ++k) table[(size_t)((k % nskip) * q_len + k / nskip)] = taps[k];

        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> vi(in_row, in_row + n_entry), vo(out_row, out_row + n_entry), vm, vc;
        if (mod_mode != TOAST_HIP_DEMOD_MOD_NONE) vm.assign(mod_row, mod_row + n_entry);
        if (mod_mode == TOAST_HIP_DEMOD_MOD_WEIGHTS) vc.assign(mod_comp, mod_comp + n_entry);
        const size_t o0 = pb.push_vec(table), o1 = pb.push_vec(vi), o2 = pb.push_vec(vo), o3 = pb.push_vec(vm),
                     o4 = pb.push_vec(vc);
        const char * d = pb.commit(st);
        FirArgs a;
        a.in = d_in;
        a.in_stride = in_stride;
        a.in_row = (const int32_t *)(d + o1);
        a.mode = mod_mode;
        a.mod = d_mod;
        a.mod_stride = mod_stride;
        a.mod_row = (const int32_t *)(d + o3);
        a.mod_comp = (const int32_t *)(d + o4);
        a.nnz = (int)nnz;
        a.comp_q = (int)comp_q;
        a.out = d_out;
        a.out_stride = out_stride;
        a.out_row = (const int32_t *)(d + o2);
        a.n = n;
        a.n_out = n_out;
        a.nskip = nskip;
        a.start = start;
        a.c = (n_taps - 1) / 2;
        a.n_phase = n_phase;
        a.q_len = q_len;
        PhaseTimer timer(st);
        for (int64_t e0 = 0; e0 < n_entry; e0 += kMaxGridY) {
            const unsigned nb = (unsigned)std::min(kMaxGridY, n_entry - e0);
            hipLaunchKernelGGL(k_demod_fir, dim3((unsigned)n_tile, nb), dim3(kThreads), 0, st, a, (const double *)(d + o0),
                               (int)e0);
        }
        TH_HIP(hipGetLastError());
        timer.stop(mod_mode == TOAST_HIP_DEMOD_MOD_NONE ? 0 : 1);
    });
}

int toast_hip_demod_flags_dev(int64_t n_entry, int64_t n, int64_t wkernel, uint8_t demod_flag_mask, int64_t nskip,
                              int64_t offset, const uint8_t * d_in, int64_t n_in_rows, int64_t in_stride,
                              const int32_t * in_row, uint8_t * d_out, int64_t n_out_rows, int64_t out_stride,
                              const int32_t * out_row, void * stream) {
    return guarded([&] {
        if (n_entry <= 0) return;
        if (n < 1 || wkernel < 1 || nskip < 1 || offset < 0) fail_arg("demod_flags: n, wkernel and nskip must be at least one");
        if (!d_in || !in_row || !d_out || !out_row) fail_arg("demod_flags: missing argument");
        const int64_t start = offset % nskip;
        const int64_t n_out = start < n ? (n - start + nskip - 1) / nskip : 0;
        if (n_out == 0) return;
        if (n > in_stride || n_out > out_stride) fail_arg("demod_flags: rows are shorter than their samples");
        check_rows(in_row, n_entry, n_in_rows, "demod_flags");
        check_rows(out_row, n_entry, n_out_rows, "demod_flags");
        hipStream_t st = pick_stream(stream);
        PhaseTimer timer(st);
        for (int64_t e0 = 0; e0 < n_entry; e0 += kMaxGridY) {
            const int64_t nb = std::min(kMaxGridY, n_entry - e0);
            ParamBlock pb;
            std::vector<int32_t> vi(in_row + e0, in_row + e0 + nb), vo(out_row + e0, out_row + e0 + nb);
            const size_t o1 = pb.push_vec(vi), o2 = pb.push_vec(vo);
            const char * d = pb.commit(st);
            hipLaunchKernelGGL(k_demod_flags, dim3(grid_x(n_out), (unsigned)nb), dim3(kThreads), 0, st, n, n_out, wkernel,
                               demod_flag_mask, nskip, start, d_in, in_stride, (const int32_t *)(d + o1), d_out, out_stride,
                               (const int32_t *)(d + o2));
        }
        TH_HIP(hipGetLastError());
        timer.stop(2);
    });
}

int toast_hip_stokes_weights_demod_dev(int64_t n_entry, int64_t n_samp, int64_t nnz, const double * values,
                                       const int32_t * out_row, void * d_weights, int64_t n_weight_rows,
                                       int single_precision, void * stream) {
    return guarded([&] {
        if (n_entry <= 0 || n_samp <= 0) return;
        if (nnz < 1 || nnz > 3) fail_arg("stokes_weights_demod: one to three weights per sample");
        if (!values || !out_row || !d_weights) fail_arg("stokes_weights_demod: missing argument");
        check_rows(out_row, n_entry, n_weight_rows, "stokes_weights_demod");
        hipStream_t st = pick_stream(stream);
        PhaseTimer timer(st);
        for (int64_t e0 = 0; e0 < n_entry; e0 += kMaxGridY) {
            const int64_t nb = std::min(kMaxGridY, n_entry - e0);
            ParamBlock pb;
            std::vector<double> vv(values + e0 * nnz, values + (e0 + nb) * nnz);
            std::vector<int32_t> vo(out_row + e0, out_row + e0 + nb);
            const size_t o1 = pb.push_vec(vv), o2 = pb.push_vec(vo);
            const char * d = pb.commit(st);
            const dim3 grid(grid_x(n_samp * nnz), (unsigned)nb);
            if (single_precision) {
                hipLaunchKernelGGL(k_weights_fill<float>, grid, dim3(kThreads), 0, st, n_samp, (int)nnz,
                                   (const double *)(d + o1), (const int32_t *)(d + o2), (float *)d_weights);
            } else {
                hipLaunchKernelGGL(k_weights_fill<double>, grid, dim3(kThreads), 0, st, n_samp, (int)nnz,
                                   (const double *)(d + o1), (const int32_t *)(d + o2), (double *)d_weights);
            }
        }
        TH_HIP(hipGetLastError());
        timer.stop(3);
    });
}

int toast_hip_demod_timing(int on, double * phase_ms) {
    if (phase_ms != nullptr) {
        for (int ph = 0; ph < 4; ++ph) phase_ms[ph] = g_phase_ms[ph];
    }
    g_timing = on ? 1 : 0;
    for (int ph = 0; ph < 4; ++ph) g_phase_ms[ph] = 0.0;
    return TOAST_HIP_OK;
}

}  // extern "C"
