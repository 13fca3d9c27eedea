// sim_dipole.hip -- CMB dipole timestreams straight from the boresight: the per-sample work of the reference's SimDipole
// operator (src/toast/ops/sim_tod_dipole.py:128-217 over src/toast/dipole.py:26-97) in one kernel, behind
// toast_hip_sim_dipole_dev (include/toast_hip.h).
//
// The reference loops over detectors in Python and runs some fifteen NumPy passes over an [n_samp] temporary for each.
// Here a lane owns a sample: it reads the boresight, the flag and the telescope velocity once, composes the unit
// velocity, beta and sqrt(1 - beta^2) once (the relativistic addition of dipole.py:54-68 has two divisions and two
// square roots), and then walks a tile of kDetTile detectors whose focal-plane quaternions and rows are wave-uniform:
//     q = boresight * fp[d]  ->  direction of the z axis under the normalised q  ->  Doppler formula  ->  += into the row.
// Per detector-sample that leaves the 16 bytes of the signal (read + write) and some sixty fp64 operations plus one
// IEEE division in the quaternion's normalisation and one in the freq == 0 formula.  Detector quaternions (32 bytes per
// detector-sample) are never materialised.
//
// Launch shape: that of kernels.hip -- workgroups of 256 threads, blockIdx.x = detector tile (fast: the tiles of one
// chunk run together and share its boresight / velocity lines in L2), blockIdx.y strides over the chunks of <= 1024
// samples that the host cuts from the intervals.  Rows are addressed in 64 bits.
//
// Arithmetic: -ffp-contract=off like the whole library, IEEE sqrt and division.  The composed velocity follows the
// reference's operation order.  The direction does not: the reference normalises q (a square root and four divisions)
// and then forms the products; here the products of the raw q are scaled by 1 / |q|^2 -- one division, no root, the same
// value within two roundings of each component, which enter the signal times beta ~ 1e-3.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_common.hpp"

using namespace toast_hip;

namespace {

constexpr int kDetTile = 16;   // detectors per workgroup: the per-sample work is shared by this many rows
constexpr int kDetGroup = 4;   // rows whose loads are issued together before the arithmetic

enum : int { kModeSolar = 0, kModeOrbital = 1, kModeTotal = 2 };

struct DipoleParams {
    double solar[3];       // km/s
    double solar_speed;    // sqrt(solar . solar)
    double solar_speed2;   // solar_speed^2
    double solar_invgamma; // sqrt(1 - (solar_speed / c)^2)
    double inv_light;      // 1e3 / c: km/s -> beta
    double inv_light2;
    double cmb;            // K
    double fcor;           // quadrupole correction (freq != 0)
    double scale;          // signed
};

// The composed unit velocity v, beta and -- FREQ0 only -- sqrt(1 - beta^2) of one sample [dipole.py:54-77, :87].
template <int MODE, bool FREQ0>
__device__ __forceinline__ void compose_velocity(const DipoleParams & p, const double * __restrict__ vel, int64_t s,
                                                 double (&v)[3], double & beta, double & inv_gamma) {
    if constexpr (MODE == kModeSolar) {
        v[0] = p.solar[0]; v[1] = p.solar[1]; v[2] = p.solar[2];
    } else {
        const double t[3] = {vel[3 * s], vel[3 * s + 1], vel[3 * s + 2]};
        if constexpr (MODE == kModeOrbital) {
            v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
        } else {
            const double dot = t[0] * p.solar[0] + t[1] * p.solar[1] + t[2] * p.solar[2];
            const double along = dot / p.solar_speed2;
            const double vdot = 1.0 / (1.0 + dot * p.inv_light2);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                double vpar = along * p.solar[k];
                double vperp = t[k] - vpar;
                vpar += p.solar[k];
                vperp *= p.solar_invgamma;
                v[k] = vdot * (vpar + vperp);
            }
        }
    }
    const double speed = f_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= speed; v[1] /= speed; v[2] /= speed;
    beta = p.inv_light * speed;
    inv_gamma = FREQ0 ? f_sqrt(1.0 - beta * beta) : 0.0;
}

// scale * dipole of one detector-sample: b the (possibly unnormalised) boresight, f the detector's quaternion.
template <bool FREQ0>
__device__ __forceinline__ double dipole_term(const DipoleParams & p, const double (&b)[4], const double (&f)[4],
                                              const double (&v)[3], double beta, double inv_gamma) {
    double q[4];
    quat_mult(b, f, q);
    const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double r = 1.0 / n2;
    const double xw = q[3] * q[0], yw = q[3] * q[1];
    const double x2 = q[0] * q[0], xz = q[0] * q[2];
    const double y2 = q[1] * q[1], yz = q[1] * q[2];
    const double d0 = 2 * ((yw + xz) * r);
    const double d1 = 2 * ((yz - xw) * r);
    const double d2 = 1.0 - 2 * ((x2 + y2) * r);
    const double along = v[0] * d0 + v[1] * d1 + v[2] * d2;
    double dip;
    if constexpr (FREQ0) {
        const double num = 1.0 - beta * along;
        dip = p.cmb * (inv_gamma / num - 1.0);
    } else {
        const double bt = beta * along;
        dip = p.cmb * (bt + p.fcor * (bt * bt));
    }
    return p.scale * dip;
}

template <int MODE, bool FREQ0>
__global__ __launch_bounds__(kThreads) void k_sim_dipole(const Chunk * __restrict__ chunks, int n_chunks,
                                                         const double * __restrict__ fp,
                                                         const int32_t * __restrict__ row_idx, int n_det,
                                                         const double * __restrict__ bore,
                                                         const uint8_t * __restrict__ flags, uint8_t mask, int use_flags,
                                                         const double * __restrict__ vel, double * __restrict__ det_data,
                                                         int64_t n_samp, DipoleParams p) {
    const int d_first = blockIdx.x * kDetTile;
    const int d_count = (n_det - d_first < kDetTile) ? (n_det - d_first) : kDetTile;
    for (int ci = blockIdx.y; ci < n_chunks; ci += gridDim.y) {
        const Chunk c = chunks[ci];
        for (int i = threadIdx.x; i < c.count; i += kThreads) {
            const int64_t s = c.first + i;
            double b[4] = {0.0, 0.0, 0.0, 1.0};
            if (!(use_flags && (flags[s] & mask))) {
                const Quat bq = load_quat(bore + 4 * s);
                b[0] = bq.x; b[1] = bq.y; b[2] = bq.z; b[3] = bq.w;
            }
            double v[3], beta, inv_gamma;
            compose_velocity<MODE, FREQ0>(p, vel, s, v, beta, inv_gamma);
            for (int g = 0; g < d_count; g += kDetGroup) {
                // d_count, g and the rows are wave-uniform: the group's loads go out together, then the arithmetic
                double * row[kDetGroup];
                double sig[kDetGroup];
#pragma unroll
                for (int e = 0; e < kDetGroup; ++e) {
                    const int d = d_first + ((g + e < d_count) ? g + e : g);
                    row[e] = det_data + (int64_t)row_idx[d] * n_samp + s;
                    sig[e] = *row[e];
                }
#pragma unroll
                for (int e = 0; e < kDetGroup; ++e) {
                    if (g + e < d_count) {
                        const int d = d_first + g + e;
                        const double f[4] = {fp[4 * d], fp[4 * d + 1], fp[4 * d + 2], fp[4 * d + 3]};
                        *row[e] = sig[e] + dipole_term<FREQ0>(p, b, f, v, beta, inv_gamma);
                    }
                }
            }
        }
    }
}

template <int MODE>
void launch_mode(bool freq0, dim3 grid, hipStream_t st, const Chunk * ch, int n_ch, const double * fp, const int32_t * rows,
                 int n_det, const double * bore, const uint8_t * flags, uint8_t mask, int use_flags, const double * vel,
                 double * det_data, int64_t n_samp, const DipoleParams & p) {
    if (freq0) {
        hipLaunchKernelGGL((k_sim_dipole<MODE, true>), grid, dim3(kThreads), 0, st, ch, n_ch, fp, rows, n_det, bore, flags,
                           mask, use_flags, vel, det_data, n_samp, p);
    } else {
        hipLaunchKernelGGL((k_sim_dipole<MODE, false>), grid, dim3(kThreads), 0, st, ch, n_ch, fp, rows, n_det, bore, flags,
                           mask, use_flags, vel, det_data, n_samp, p);
    }
}

}  // namespace

extern "C" {

int toast_hip_sim_dipole_det_tile(void) { return kDetTile; }

int toast_hip_sim_dipole_dev(const double * focalplane, const double * d_boresight, const int32_t * data_index,
                             int64_t n_det, double * d_det_data, int64_t n_data_rows, int64_t n_samp,
                             const toast_hip_interval * intervals, int64_t n_view, const uint8_t * d_shared_flags,
                             int64_t n_flags, uint8_t shared_flag_mask, const double * d_velocity, const double * solar,
                             double cmb_kelvin, double freq_hz, double scale, void * stream) {
    return guarded([&] {
        if (!d_velocity && !solar) fail_arg("sim_dipole: a telescope velocity, a solar velocity or both are required");
        if (n_det <= 0) return;
        if (!focalplane || !d_boresight || !data_index || !d_det_data) fail_arg("sim_dipole: missing argument");
        if (n_view > 0 && !intervals) fail_arg("sim_dipole: missing intervals");
        need_aligned(d_boresight, "boresight");
        for (int64_t d = 0; d < n_det; ++d) {
            if (data_index[d] < 0 || data_index[d] >= n_data_rows) fail_arg("sim_dipole: a row of data_index is outside det_data");
        }
        const auto chunks = make_chunks(intervals, n_view, n_samp);
        if (chunks.empty()) return;
        if (n_det > 0x7fffffff) fail_arg("sim_dipole: too many detectors for one launch");
        const int64_t n_tile = (n_det + kDetTile - 1) / kDetTile;

        DipoleParams p{};
        p.inv_light = 1.0e3 / 299792458.0;
        p.inv_light2 = p.inv_light * p.inv_light;
        if (solar) {
            for (int k = 0; k < 3; ++k) p.solar[k] = solar[k];
            p.solar_speed = std::sqrt(solar[0] * solar[0] + solar[1] * solar[1] + solar[2] * solar[2]);
            p.solar_speed2 = p.solar_speed * p.solar_speed;
            const double bs = p.solar_speed * p.inv_light;
            p.solar_invgamma = std::sqrt(1.0 - bs * bs);
        }
        p.cmb = cmb_kelvin;
        p.scale = scale;
        const bool freq0 = (freq_hz == 0);
        if (!freq0) {
            // scipy.constants.h, .k: exact in the SI of 2019 (CODATA 2018)
            const double h = 6.62607015e-34, k = 1.380649e-23;
            const double fx = h * freq_hz / (k * cmb_kelvin);
            p.fcor = (fx / 2) * (std::exp(fx) + 1) / (std::exp(fx) - 1);
        }

        ParamBlock pb;
        const size_t o_ch = pb.push_vec(chunks);
        const size_t o_fp = pb.push(focalplane, sizeof(double) * 4 * n_det);
        const size_t o_ri = pb.push(data_index, sizeof(int32_t) * n_det);
        hipStream_t st = as_stream(stream);
        const char * d = pb.commit(st);
        const int use_flags = (d_shared_flags && n_flags == n_samp && shared_flag_mask != 0) ? 1 : 0;
        const dim3 grid = chunk_grid(n_tile, chunks.size());
        const Chunk * ch = (const Chunk *)(d + o_ch);
        const double * fp = (const double *)(d + o_fp);
        const int32_t * rows = (const int32_t *)(d + o_ri);
        const int n_ch = (int)chunks.size();
        if (solar && d_velocity) {
            launch_mode<kModeTotal>(freq0, grid, st, ch, n_ch, fp, rows, (int)n_det, d_boresight, d_shared_flags,
                                    shared_flag_mask, use_flags, d_velocity, d_det_data, n_samp, p);
        } else if (solar) {
            launch_mode<kModeSolar>(freq0, grid, st, ch, n_ch, fp, rows, (int)n_det, d_boresight, d_shared_flags,
                                    shared_flag_mask, use_flags, d_velocity, d_det_data, n_samp, p);
        } else {
            launch_mode<kModeOrbital>(freq0, grid, st, ch, n_ch, fp, rows, (int)n_det, d_boresight, d_shared_flags,
                                      shared_flag_mask, use_flags, d_velocity, d_det_data, n_samp, p);
        }
        check_launch();
    });
}

}  // extern "C"
