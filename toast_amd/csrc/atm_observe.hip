// atm_observe.hip -- line-of-sight integration through a simulated atmosphere volume on gfx950.
//
// Counterpart of toast::atm_sim_observe / toast::atm_sim_interp (src/libtoast/src/toast_atm_observe.cpp:28-244, :246-488)
// and of the per-detector chain of ObserveAtmosphere._exec (src/toast/ops/sim_tod_atm_observe.py:238-483):
//   * toast_hip_atm_observe_dev        atm_sim_observe for a batch of rows of (times, az, el), accumulating into tod,
//   * toast_hip_atm_observe_quats_dev  the same integral from detector quaternions (qa_to_angles,
//                                      src/libtoast/src/toast_math_qarray.cpp:1166-1199) into a scratch row,
//   * toast_hip_atm_good_ranges_dev    which samples a detector observes, and the extent of its times, az and el,
//   * toast_hip_atm_flag_failed_dev    sim_tod_atm_observe.py:379-399,
//   * toast_hip_atm_finish_dev         sim_tod_atm_observe.py:424-483,
//   * toast_hip_atm_observe            the host-pointer form of the first (arrays staged for the call).
//
// k_atm_observe: one lane per (row, sample), consecutive lanes on consecutive samples, rows in blockIdx.y.  The radii of
// the steps do not depend on the sample (r starts at 1.5 xstep, grows by repeated r += xstep, ends at r > rmax or
// r sin(elmax) >= zmax), so the host entry walks them once, with the reference's additions, and hands the kernel the
// first radius and the NUMBER of steps: every lane of a wave runs the same trip count and ends early only on a failed
// check.  The trigonometry of a sample is hoisted out of the step loop as in the reference.  A step is eight gathers
// through the compressed index (int32 when nelem < 2^31, else int64), eight gathers of the realization and the seven
// lerps in the reference's association; multiplies and adds are rounded separately (-ffp-contract=off).
//
// Every check of the reference build without NO_ATM_CHECKS is kept, in its order: point outside the box, fractional step
// outside [0, 1], cell index outside the grid, full index outside [0, nn), compressed index outside [0, nelem).  No
// index is dereferenced before it has passed its check, so a malformed volume gives status 1 and never a load outside
// the three arrays.  A failed check discards the partial sum of its sample, which still receives += 0.  The status is a
// device word ORed by one lane per wave that saw a skip or a failure; no atomics touch tod.
//
// The reference's one-cell cache (last_ind / last_nodes) is an option of the launch (cell_cache): registers that keep the
// corner values of the last cell of THIS ray.  It starts empty here; the reference's starts as cell (0, 0, 0) with zero
// values per thread and would return 0 inside that cell until another cell has been read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "runtime.hpp"

using namespace toast_hip;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxGridY = 65535;
constexpr int64_t kMaxSteps = int64_t(1) << 24;   // radii walked on the host per call

// what the kernels need of toast_hip_atm_geometry, with the per-call constants of atm_sim_observe (:293-306) and the
// step sequence (:359-375) worked out once on the host
struct Geom {
    double T0, azmin, azmax, elmin, elmax, tmin;
    double zatm_inv, wx, wy, wz;
    double xstep, ystep, zstep, xstepinv, ystepinv, zstepinv;
    double xstart, ystart, zstart, xend, yend, zend;
    double az0, sinel0, cosel0;
    double r_first;
    int64_t n_step;
    int64_t nn, nx, ny, nz, xstride, ystride, zstride, nelem;
};

struct CellCache {
    int64_t ix = -1, iy = -1, iz = -1;
    double c[8];
};

// atm_sim_interp (:69-243).  false: a check failed.
template <typename IDX, bool CACHE>
__device__ __forceinline__ bool atm_interp(const Geom & g, const IDX * __restrict__ cidx, const double * __restrict__ real,
                                           double x, double y, double z, CellCache & cc, double & out) {
    const int64_t ix = (int64_t)((x - g.xstart) * g.xstepinv);
    const int64_t iy = (int64_t)((y - g.ystart) * g.ystepinv);
    const int64_t iz = (int64_t)((z - g.zstart) * g.zstepinv);
    const double dx = (x - (g.xstart + (double)ix * g.xstep)) * g.xstepinv;
    const double dy = (y - (g.ystart + (double)iy * g.ystep)) * g.ystepinv;
    const double dz = (z - (g.zstart + (double)iz * g.zstep)) * g.zstepinv;
    // (:78) written so that a NaN fails here; the reference lets it through to the cell check, where its INT64_MIN fails
    if (!(dx >= 0 && dx <= 1 && dy >= 0 && dy <= 1 && dz >= 0 && dz <= 1)) return false;
    double c000, c001, c010, c011, c100, c101, c110, c111;
    if (!CACHE || ix != cc.ix || iy != cc.iy || iz != cc.iz) {
        if (ix < 0 || ix > g.nx - 2 || iy < 0 || iy > g.ny - 2 || iz < 0 || iz > g.nz - 2) return false;   // (:98)
        const int64_t offset = ix * g.xstride + iy * g.ystride + iz * g.zstride;
        const int64_t f000 = offset;
        const int64_t f001 = offset + g.zstride;
        const int64_t f010 = offset + g.ystride;
        const int64_t f011 = f010 + g.zstride;
        const int64_t f100 = offset + g.xstride;
        const int64_t f101 = f100 + g.zstride;
        const int64_t f110 = f100 + g.ystride;
        const int64_t f111 = f110 + g.zstride;
        const int64_t fmax = g.nn - 1;
        if (f000 < 0 || f000 > fmax || f001 < 0 || f001 > fmax || f010 < 0 || f010 > fmax || f011 < 0 || f011 > fmax ||
            f100 < 0 || f100 > fmax || f101 < 0 || f101 > fmax || f110 < 0 || f110 > fmax || f111 < 0 || f111 > fmax) {
            return false;   // (:127)
        }
        const int64_t i000 = (int64_t)cidx[f000];
        const int64_t i001 = (int64_t)cidx[f001];
        const int64_t i010 = (int64_t)cidx[f010];
        const int64_t i011 = (int64_t)cidx[f011];
        const int64_t i100 = (int64_t)cidx[f100];
        const int64_t i101 = (int64_t)cidx[f101];
        const int64_t i110 = (int64_t)cidx[f110];
        const int64_t i111 = (int64_t)cidx[f111];
        const int64_t imax = g.nelem - 1;
        if (i000 < 0 || i000 > imax || i001 < 0 || i001 > imax || i010 < 0 || i010 > imax || i011 < 0 || i011 > imax ||
            i100 < 0 || i100 > imax || i101 < 0 || i101 > imax || i110 < 0 || i110 > imax || i111 < 0 || i111 > imax) {
            return false;   // (:165) the normal way a ray leaves the simulated cone
        }
        c000 = real[i000];
        c001 = real[i001];
        c010 = real[i010];
        c011 = real[i011];
        c100 = real[i100];
        c101 = real[i101];
        c110 = real[i110];
        c111 = real[i111];
        if (CACHE) {
            cc.ix = ix;
            cc.iy = iy;
            cc.iz = iz;
            cc.c[0] = c000;
            cc.c[1] = c001;
            cc.c[2] = c010;
            cc.c[3] = c011;
            cc.c[4] = c100;
            cc.c[5] = c101;
            cc.c[6] = c110;
            cc.c[7] = c111;
        }
    } else {
        c000 = cc.c[0];
        c001 = cc.c[1];
        c010 = cc.c[2];
        c011 = cc.c[3];
        c100 = cc.c[4];
        c101 = cc.c[5];
        c110 = cc.c[6];
        c111 = cc.c[7];
    }
    const double c00 = c000 + (c100 - c000) * dx;
    const double c01 = c001 + (c101 - c001) * dx;
    const double c10 = c010 + (c110 - c010) * dx;
    const double c11 = c011 + (c111 - c011) * dx;
    const double c0 = c00 + (c10 - c00) * dy;
    const double c1 = c01 + (c11 - c01) * dy;
    out = c0 + (c1 - c0) * dz;
    return true;
}

// the skip rule of atm_sim_observe (:323-325)
__device__ __forceinline__ bool atm_skipped(const Geom & g, double az, double el) {
    const double azm = az - 2 * M_PI;
    return (!((g.azmin <= az) && (az <= g.azmax)) && !((g.azmin <= azm) && (azm <= g.azmax))) ||
           !((g.elmin <= el) && (el <= g.elmax));
}

// one ray (:345-484): the integral before the factor xstep T0.  false: a check failed (the value is 0 then)
template <typename IDX, bool CACHE>
__device__ __forceinline__ bool atm_ray(const Geom & g, const IDX * __restrict__ cidx, const double * __restrict__ real,
                                        double t, double az, double el, double & val) {
    const double t_now = t - g.tmin;
    const double az_now = az - g.az0;
    const double xtel = g.wx * t_now, ytel = g.wy * t_now, ztel = g.wz * t_now;
    const double sin_el = sin(el), cos_el = cos(el);
    const double sin_az = sin(az_now), cos_az = cos(az_now);
    CellCache cc;
    double r = g.r_first;
    val = 0;
    for (int64_t k = 0; k < g.n_step; ++k) {
        const double zz = r * sin_el;
        const double rproj = r * cos_el;
        const double xx = rproj * cos_az;
        const double yy = rproj * sin_az;
        double x = xx * g.cosel0 + zz * g.sinel0;
        double y = yy;
        double z = -xx * g.sinel0 + zz * g.cosel0;
        x += xtel;
        y += ytel;
        z += ztel;
        if ((x < g.xstart) || (x > g.xend) || (y < g.ystart) || (y > g.yend) || (z < g.zstart) || (z > g.zend)) {   // (:397)
            val = 0;
            return false;
        }
        double c;
        if (!atm_interp<IDX, CACHE>(g, cidx, real, x, y, z, cc, c)) {
            val = 0;
            return false;
        }
        val += c * (1. - z * g.zatm_inv);
        r += g.xstep;
    }
    return true;
}

__device__ __forceinline__ void atm_raise(bool bad, int * status) {
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(status, 1);
}

// atm_sim_observe for rows of az / el: row = blockIdx.y.  time_stride 0: one row of times for all.
template <typename IDX, bool CACHE>
__global__ __launch_bounds__(kThreads) void k_atm_observe(Geom g, const IDX * __restrict__ cidx,
                                                          const double * __restrict__ real, int64_t n_samp, int64_t row0,
                                                          const double * __restrict__ times, int64_t time_stride,
                                                          const double * __restrict__ az, const double * __restrict__ el,
                                                          int64_t angle_stride, double * __restrict__ tod,
                                                          int64_t tod_stride, int * status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = row0 + blockIdx.y;
    bool bad = false;
    if (i < n_samp) {
        const double a = az[row * angle_stride + i], e = el[row * angle_stride + i];
        if (atm_skipped(g, a, e)) {
            bad = true;
        } else {
            double val;
            bad = !atm_ray<IDX, CACHE>(g, cidx, real, times[row * time_stride + i], a, e, val);
            tod[row * tod_stride + i] += val * g.xstep * g.T0;   // (:484)
        }
    }
    atm_raise(bad, status);
}

// qa_to_angles (toast_math_qarray.cpp:1166-1188) and sim_tod_atm_observe.py:287-288
__device__ __forceinline__ void atm_quat_azel(const double * __restrict__ q, double & az, double & el) {
    // qa_normalize_one (:88-99)
    double norm = 0.0;
    for (int k = 0; k < 4; ++k) norm += q[k] * q[k];
    norm = 1.0 / sqrt(norm);
    double qn[4];
    for (int k = 0; k < 4; ++k) qn[k] = q[k] * norm;
    // qa_rotate_one_one (:168-198) of the z axis; it normalises again
    double n2 = 0.0;
    for (int k = 0; k < 4; ++k) n2 += qn[k] * qn[k];
    n2 = 1.0 / sqrt(n2);
    double u[4];
    for (int k = 0; k < 4; ++k) u[k] = qn[k] * n2;
    const double xw = u[3] * u[0], yw = u[3] * u[1];
    const double x2 = -u[0] * u[0], xz = u[0] * u[2], y2 = -u[1] * u[1], yz = u[1] * u[2];
    const double zw = u[3] * u[2], xy = u[0] * u[1], z2 = -u[2] * u[2];
    // v_in = (0, 0, 1), written out as the reference evaluates it: the products with zero decide the sign of a zero sum
    const double d0 = 2 * ((y2 + z2) * 0.0 + (xy - zw) * 0.0 + (yw + xz) * 1.0) + 0.0;
    const double d1 = 2 * ((zw + xy) * 0.0 + (x2 + z2) * 0.0 + (yz - xw) * 1.0) + 0.0;
    const double d2 = 2 * ((xz - yw) * 0.0 + (xw + yz) * 0.0 + (x2 + y2) * 1.0) + 1.0;
    const double theta = M_PI_2 - asin(d2);
    double phi = atan2(d1, d0);
    if (phi < 0.0) phi += 2 * M_PI;
    az = 2 * M_PI - phi;
    el = M_PI / 2 - theta;
}

// which samples of a row a detector observes (sim_tod_atm_observe.py:240-255), and what the operator asks about them
// (:290-294): first and last good sample, extent of el, extent of az unwrapped around the first good sample's.  One
// workgroup per row.  out[row][8] = first, last (as doubles; -1: none), el min, el max, az of the first good sample,
// min and max of wrap(az - az_first) in [-pi, pi), 0.
__global__ __launch_bounds__(kThreads) void k_atm_good_ranges(int64_t n_samp, int64_t stride,
                                                              const int32_t * __restrict__ quat_row,
                                                              const double * __restrict__ quats,
                                                              const int32_t * __restrict__ flag_row,
                                                              const uint8_t * __restrict__ det_flags, uint8_t det_flag_mask,
                                                              const uint8_t * __restrict__ shared_flags,
                                                              uint8_t shared_flag_mask, uint8_t * __restrict__ good,
                                                              double * __restrict__ out) {
    __shared__ double red[4][kThreads];
    __shared__ long long first_s, last_s;
    const int row = (int)blockIdx.x;
    const int tid = (int)threadIdx.x;
    const uint8_t * f = det_flags ? det_flags + (int64_t)flag_row[row] * stride : nullptr;
    const double * q = quats + (int64_t)quat_row[row] * stride * 4;
    uint8_t * gd = good + (int64_t)row * n_samp;
    if (tid == 0) {
        first_s = n_samp;
        last_s = -1;
    }
    __syncthreads();
    long long first = n_samp, last = -1;
    for (int64_t i = tid; i < n_samp; i += kThreads) {
        uint8_t bits = f ? (uint8_t)(f[i] & det_flag_mask) : (uint8_t)0;
        if (shared_flags) bits |= (uint8_t)(shared_flags[i] & shared_flag_mask);
        const bool ok = bits == 0;
        gd[i] = ok ? 1 : 0;
        if (ok) {
            first = min(first, (long long)i);
            last = max(last, (long long)i);
        }
    }
    if (last >= 0) {
        atomicMin(&first_s, first);
        atomicMax(&last_s, last);
    }
    __syncthreads();
    first = first_s;
    last = last_s;
    double * o = out + (int64_t)row * 8;
    if (last < 0) {
        if (tid == 0) {
            o[0] = -1.0;
            o[1] = -1.0;
            for (int k = 2; k < 8; ++k) o[k] = 0.0;
        }
        return;
    }
    double az_first, el_first;
    atm_quat_azel(q + first * 4, az_first, el_first);
    double el_lo = el_first, el_hi = el_first, d_lo = 0.0, d_hi = 0.0;
    for (int64_t i = tid; i < n_samp; i += kThreads) {
        if (!gd[i]) continue;
        double az, el;
        atm_quat_azel(q + i * 4, az, el);
        double d = az - az_first;
        if (d >= M_PI) d -= 2 * M_PI;
        if (d < -M_PI) d += 2 * M_PI;
        el_lo = fmin(el_lo, el);
        el_hi = fmax(el_hi, el);
        d_lo = fmin(d_lo, d);
        d_hi = fmax(d_hi, d);
    }
    red[0][tid] = el_lo;
    red[1][tid] = el_hi;
    red[2][tid] = d_lo;
    red[3][tid] = d_hi;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = fmin(red[0][tid], red[0][tid + s]);
            red[1][tid] = fmax(red[1][tid], red[1][tid + s]);
            red[2][tid] = fmin(red[2][tid], red[2][tid + s]);
            red[3][tid] = fmax(red[3][tid], red[3][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        o[0] = (double)first;
        o[1] = (double)last;
        o[2] = red[0][0];
        o[3] = red[1][0];
        o[4] = az_first;
        o[5] = red[2][0];
        o[6] = red[3][0];
        o[7] = 0.0;
    }
}

// the integral of the good samples of a row of quaternions, added to the scratch row atm (without xstep T0 the sum
// would not be the reference's atmdata: the factor is applied here as at :484)
template <typename IDX, bool CACHE>
__global__ __launch_bounds__(kThreads) void k_atm_observe_quats(Geom g, const IDX * __restrict__ cidx,
                                                                const double * __restrict__ real, int64_t n_samp,
                                                                int64_t stride, int64_t row0,
                                                                const double * __restrict__ times,
                                                                const int32_t * __restrict__ quat_row,
                                                                const double * __restrict__ quats,
                                                                const uint8_t * __restrict__ good,
                                                                double * __restrict__ atm, int * status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = row0 + blockIdx.y;
    bool bad = false;
    if (i < n_samp && good[row * n_samp + i]) {
        double a, e;
        atm_quat_azel(quats + ((int64_t)quat_row[row] * stride + i) * 4, a, e);
        if (atm_skipped(g, a, e)) {
            bad = true;
        } else {
            double val;
            bad = !atm_ray<IDX, CACHE>(g, cidx, real, times[i], a, e, val);
            atm[row * n_samp + i] += val * g.xstep * g.T0;
        }
    }
    atm_raise(bad, status + row);
}

// sim_tod_atm_observe.py:379-399 after a slab that reported a failure
__global__ __launch_bounds__(kThreads) void k_atm_flag_failed(int64_t n_samp, int64_t stride,
                                                              const uint8_t * __restrict__ good,
                                                              const double * __restrict__ atm,
                                                              const int32_t * __restrict__ flag_row,
                                                              const int32_t * __restrict__ enable,
                                                              uint8_t * __restrict__ det_flags, uint8_t det_flag_mask,
                                                              unsigned long long * __restrict__ n_bad) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = blockIdx.y;
    if (!enable[row]) return;   // (:359) only after a slab that failed for this detector
    bool bad = false;
    if (i < n_samp && good[row * n_samp + i] && fabs(atm[row * n_samp + i]) < 1e-30) {
        bad = true;
        det_flags[(int64_t)flag_row[row] * stride + i] |= det_flag_mask;
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0 && (threadIdx.x & 63) == 0) atomicAdd(n_bad + row, (unsigned long long)__popcll(m));
}

// sim_tod_atm_observe.py:424-483 without the fade: per[row] = (gain absorption, loading, use loading)
__global__ __launch_bounds__(kThreads) void k_atm_finish(int64_t n_samp, int64_t stride,
                                                         const uint8_t * __restrict__ good,
                                                         const double * __restrict__ atm, const double * __restrict__ per,
                                                         const int32_t * __restrict__ quat_row,
                                                         const double * __restrict__ quats,
                                                         const int32_t * __restrict__ weight_row,
                                                         const double * __restrict__ weights, int nnz, int comp_i, int comp_q,
                                                         double pfrac, double scale, const int32_t * __restrict__ data_row,
                                                         double * __restrict__ det_data) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = blockIdx.y;
    if (i >= n_samp || !good[row * n_samp + i]) return;
    double v = atm[row * n_samp + i];
    const double * p = per + row * 3;
    v *= p[0];
    double w_i = 1.0, w_q = 0.0;
    if (weights) {
        const double * w = weights + ((int64_t)weight_row[row] * stride + i) * nnz;
        w_i = comp_i >= 0 ? w[comp_i] : 0.0;
        w_q = comp_q >= 0 ? w[comp_q] : 0.0;
    }
    v *= w_i + w_q * pfrac;
    if (p[2] != 0.0) {
        double a, e;
        atm_quat_azel(quats + ((int64_t)quat_row[row] * stride + i) * 4, a, e);
        v += p[1] / sin(e);
    }
    det_data[(int64_t)data_row[row] * stride + i] += scale * v;
}

hipStream_t pick_stream(void * stream) {
    Manager::get().require_device();
    return stream ? static_cast<hipStream_t>(stream) : Manager::get().stream();
}

bool finite_all(std::initializer_list<double> v) {
    for (double x : v) {
        if (!std::isfinite(x)) return false;
    }
    return true;
}

// validate the caller's block and derive the kernels' (atm_sim_observe :293-306, :359-375)
Geom make_geom(const toast_hip_atm_geometry & a) {
    if (!finite_all({a.T0, a.azmin, a.azmax, a.elmin, a.elmax, a.tmin, a.tmax, a.rmin, a.rmax, a.fixed_r, a.zatm, a.zmax,
                     a.wx, a.wy, a.wz, a.xstep, a.ystep, a.zstep, a.xstart, a.delta_x, a.ystart, a.delta_y, a.zstart,
                     a.delta_z})) {
        fail_arg("atm_observe: the geometry holds a value that is not finite");
    }
    if (!(a.xstep > 0 && a.ystep > 0 && a.zstep > 0)) fail_arg("atm_observe: the steps must be positive");
    if (a.zatm == 0) fail_arg("atm_observe: zatm must not be zero");
    if (a.nx < 1 || a.ny < 1 || a.nz < 1 || a.nn < 1 || a.nelem < 1) fail_arg("atm_observe: empty volume");
    const int64_t lim = int64_t(1) << 40;
    if (a.nx > lim || a.ny > lim || a.nz > lim || a.nn > (int64_t(1) << 60) || a.nelem > (int64_t(1) << 60)) {
        fail_arg("atm_observe: volume sizes out of range");
    }
    // the largest offset the kernel can form before its own range check must fit an int64
    const long double reach = (long double)a.nx * fabsl((long double)a.xstride) + (long double)a.ny * fabsl((long double)a.ystride) +
                              (long double)a.nz * fabsl((long double)a.zstride);
    if (reach > 9.0e18L) fail_arg("atm_observe: strides out of range");
    Geom g;
    g.T0 = a.T0;
    g.azmin = a.azmin;
    g.azmax = a.azmax;
    g.elmin = a.elmin;
    g.elmax = a.elmax;
    g.tmin = a.tmin;
    g.zatm_inv = 1.0 / a.zatm;
    g.wx = a.wx;
    g.wy = a.wy;
    g.wz = a.wz;
    g.xstep = a.xstep;
    g.ystep = a.ystep;
    g.zstep = a.zstep;
    g.xstepinv = 1.0 / a.xstep;
    g.ystepinv = 1.0 / a.ystep;
    g.zstepinv = 1.0 / a.zstep;
    g.xstart = a.xstart;
    g.ystart = a.ystart;
    g.zstart = a.zstart;
    g.xend = a.xstart + a.delta_x;
    g.yend = a.ystart + a.delta_y;
    g.zend = a.zstart + a.delta_z;
    const double delta_az = (a.azmax - a.azmin);
    const double delta_el = (a.elmax - a.elmin);
    g.az0 = a.azmin + delta_az / 2;
    const double el0 = a.elmin + delta_el / 2;
    g.sinel0 = sin(el0);
    g.cosel0 = cos(el0);
    // the radii: the same additions as the reference's loop, counted instead of integrated
    const double sin_el_max = sin(a.elmax);
    double r = 1.5 * a.xstep;
    const double rstep = a.xstep;
    int64_t walked = 0;
    while (r < a.rmin) {
        r += rstep;
        if (++walked > kMaxSteps) fail_arg("atm_observe: rmin is more than 2^24 steps away");
    }
    const bool fixed = a.fixed_r > 0;
    if (fixed) r = a.fixed_r;
    g.r_first = r;
    int64_t n = 0;
    while (true) {
        if (r > a.rmax) break;
        if (r * sin_el_max >= a.zmax) break;
        ++n;
        if (n > kMaxSteps) fail_arg("atm_observe: more than 2^24 steps along a ray");
        r += rstep;
        if (fixed) break;
    }
    g.n_step = n;
    g.nn = a.nn;
    g.nx = a.nx;
    g.ny = a.ny;
    g.nz = a.nz;
    g.xstride = a.xstride;
    g.ystride = a.ystride;
    g.zstride = a.zstride;
    g.nelem = a.nelem;
    return g;
}

int * status_word(hipStream_t st) {
    int * d_status = static_cast<int *>(Manager::get().scratch(Manager::kScratchStatus, 64));
    TH_HIP(hipMemsetAsync(d_status, 0, sizeof(int), st));
    return d_status;
}

int read_status(int * d_status, hipStream_t st) {
    int status = 0;
    copy_to_host(&status, d_status, sizeof(int), st);
    return status != 0 ? 1 : 0;
}

void check_rows(const int32_t * rows, int64_t n, int64_t limit, const char * what) {
    for (int64_t r = 0; r < n; ++r) {
        if (rows[r] < 0 || rows[r] >= limit) fail_arg(std::string(what) + ": an entry names a row outside its array");
    }
}

unsigned sample_blocks(int64_t n_samp) {
    const int64_t nb = (n_samp + kThreads - 1) / kThreads;
    if (nb > 0x7fffffff) fail_arg("atm_observe: too many samples for one launch");
    return (unsigned)nb;
}

template <typename IDX, bool CACHE>
void launch_observe(const Geom & g, const void * d_index, const double * d_real, int64_t n_row, int64_t n_samp,
                    const double * d_times, int64_t time_stride, const double * d_az, const double * d_el,
                    int64_t angle_stride, double * d_tod, int64_t tod_stride, int * d_status, hipStream_t st) {
    for (int64_t r0 = 0; r0 < n_row; r0 += kMaxGridY) {
        const unsigned nb = (unsigned)std::min(kMaxGridY, n_row - r0);
        hipLaunchKernelGGL((k_atm_observe<IDX, CACHE>), dim3(sample_blocks(n_samp), nb), dim3(kThreads), 0, st, g,
                           static_cast<const IDX *>(d_index), d_real, n_samp, r0, d_times, time_stride, d_az, d_el,
                           angle_stride, d_tod, tod_stride, d_status);
    }
    TH_HIP(hipGetLastError());
}

template <typename IDX, bool CACHE>
void launch_observe_quats(const Geom & g, const void * d_index, const double * d_real, int64_t n_row, int64_t n_samp,
                          int64_t stride, const double * d_times, const int32_t * d_quat_row, const double * d_quats,
                          const uint8_t * d_good, double * d_atm, int * d_status, hipStream_t st) {
    for (int64_t r0 = 0; r0 < n_row; r0 += kMaxGridY) {
        const unsigned nb = (unsigned)std::min(kMaxGridY, n_row - r0);
        hipLaunchKernelGGL((k_atm_observe_quats<IDX, CACHE>), dim3(sample_blocks(n_samp), nb), dim3(kThreads), 0, st, g,
                           static_cast<const IDX *>(d_index), d_real, n_samp, stride, r0, d_times, d_quat_row, d_quats, d_good,
                           d_atm, d_status);
    }
    TH_HIP(hipGetLastError());
}

void observe_dev(const toast_hip_atm_geometry * geom, const void * d_index, int index32, const double * d_real,
                 int cell_cache, int64_t n_row, int64_t n_samp, const double * d_times, int64_t time_stride,
                 const double * d_az, const double * d_el, int64_t angle_stride, double * d_tod, int64_t tod_stride,
                 int * status, hipStream_t st) {
    if (!geom || !status) fail_arg("atm_observe: missing argument");
    *status = 0;
    const Geom g = make_geom(*geom);
    if (n_row <= 0 || n_samp <= 0) return;
    if (!d_index || !d_real || !d_times || !d_az || !d_el || !d_tod) fail_arg("atm_observe: missing argument");
    if (index32 && geom->nelem >= (int64_t(1) << 31)) fail_arg("atm_observe: an int32 index cannot name 2^31 elements");
    if ((time_stride != 0 && time_stride < n_samp) || angle_stride < n_samp || tod_stride < n_samp) {
        fail_arg("atm_observe: rows are shorter than their samples");
    }
    int * d_status = status_word(st);
    if (index32) {
        if (cell_cache) {
            launch_observe<int32_t, true>(g, d_index, d_real, n_row, n_samp, d_times, time_stride, d_az, d_el, angle_stride,
                                          d_tod, tod_stride, d_status, st);
        } else {
            launch_observe<int32_t, false>(g, d_index, d_real, n_row, n_samp, d_times, time_stride, d_az, d_el, angle_stride,
                                           d_tod, tod_stride, d_status, st);
        }
    } else {
        if (cell_cache) {
            launch_observe<int64_t, true>(g, d_index, d_real, n_row, n_samp, d_times, time_stride, d_az, d_el, angle_stride,
                                          d_tod, tod_stride, d_status, st);
        } else {
            launch_observe<int64_t, false>(g, d_index, d_real, n_row, n_samp, d_times, time_stride, d_az, d_el, angle_stride,
                                           d_tod, tod_stride, d_status, st);
        }
    }
    *status = read_status(d_status, st);
}

}  // namespace

extern "C" {

int toast_hip_atm_observe_dev(const toast_hip_atm_geometry * geom, const void * d_index, int index32,
                              const double * d_realization, int cell_cache, int64_t n_row, int64_t n_samp,
                              const double * d_times, int64_t time_stride, const double * d_az, const double * d_el,
                              int64_t angle_stride, double * d_tod, int64_t tod_stride, int * status, void * stream) {
    return guarded([&] {
        observe_dev(geom, d_index, index32, d_realization, cell_cache, n_row, n_samp, d_times, time_stride, d_az, d_el,
                    angle_stride, d_tod, tod_stride, status, pick_stream(stream));
    });
}

int toast_hip_atm_observe(const toast_hip_atm_geometry * geom, const int64_t * compressed_index, const double * realization,
                          int64_t n_samp, const double * times, const double * az, const double * el, double * tod,
                          int * status) {
    return guarded([&] {
        if (!geom || !status) fail_arg("atm_observe: missing argument");
        *status = 0;
        (void)make_geom(*geom);
        if (n_samp <= 0) return;
        if (!compressed_index || !realization || !times || !az || !el || !tod) fail_arg("atm_observe: missing argument");
        hipStream_t st = pick_stream(nullptr);
        Staging sg(false, st);
        const int64_t * d_index = sg.temp_in(compressed_index, (size_t)geom->nn);
        const double * d_real = sg.temp_in(realization, (size_t)geom->nelem);
        const double * d_t = sg.temp_in(times, (size_t)n_samp);
        const double * d_a = sg.temp_in(az, (size_t)n_samp);
        const double * d_e = sg.temp_in(el, (size_t)n_samp);
        double * d_tod = sg.temp_inout(tod, (size_t)n_samp);
        observe_dev(geom, d_index, 0, d_real, 0, 1, n_samp, d_t, 0, d_a, d_e, n_samp, d_tod, n_samp, status, st);
        sg.finish();
    });
}

int toast_hip_atm_good_ranges_dev(int64_t n_row, int64_t n_samp, int64_t stride, const int32_t * quat_row, const double * d_quats,
                                  int64_t n_quat_rows, const int32_t * flag_row, const uint8_t * d_det_flags,
                                  int64_t n_flag_rows, uint8_t det_flag_mask, const uint8_t * d_shared_flags,
                                  uint8_t shared_flag_mask, uint8_t * d_good, double * ranges, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n_samp <= 0) return;
        if (!quat_row || !d_quats || !d_good || !ranges) fail_arg("atm_good_ranges: missing argument");
        if (stride < n_samp) fail_arg("atm_good_ranges: rows are shorter than their samples");
        if (d_det_flags && !flag_row) fail_arg("atm_good_ranges: detector flags need their rows");
        if (n_row > 0x7fffffff) fail_arg("atm_good_ranges: too many rows for one launch");
        check_rows(quat_row, n_row, n_quat_rows, "atm_good_ranges");
        if (d_det_flags) check_rows(flag_row, n_row, n_flag_rows, "atm_good_ranges");
        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> vq(quat_row, quat_row + n_row), vf;
        if (d_det_flags) vf.assign(flag_row, flag_row + n_row);
        const size_t o1 = pb.push_vec(vq), o2 = pb.push_vec(vf);
        const char * d = pb.commit(st);
        double * d_out = static_cast<double *>(Manager::get().scratch(Manager::kScratchAtm, (size_t)n_row * 8 * sizeof(double), st));
        hipLaunchKernelGGL(k_atm_good_ranges, dim3((unsigned)n_row), dim3(kThreads), 0, st, n_samp, stride,
                           (const int32_t *)(d + o1), d_quats, (const int32_t *)(d + o2), d_det_flags, det_flag_mask, d_shared_flags, shared_flag_mask,
                           d_good, d_out);
        TH_HIP(hipGetLastError());
        copy_to_host(ranges, d_out, (size_t)n_row * 8 * sizeof(double), st);
    });
}

int toast_hip_atm_observe_quats_dev(const toast_hip_atm_geometry * geom, const void * d_index, int index32,
                                    const double * d_realization, int cell_cache, int64_t n_row, int64_t n_samp,
                                    int64_t stride, const double * d_times, const int32_t * quat_row, const double * d_quats,
                                    int64_t n_quat_rows, const uint8_t * d_good, double * d_atm, int * status,
                                    void * stream) {
    return guarded([&] {
        if (!geom || !status) fail_arg("atm_observe_quats: missing argument");
        for (int64_t r = 0; r < n_row; ++r) status[r] = 0;
        const Geom g = make_geom(*geom);
        if (n_row <= 0 || n_samp <= 0) return;
        if (!d_index || !d_realization || !d_times || !quat_row || !d_quats || !d_good || !d_atm) {
            fail_arg("atm_observe_quats: missing argument");
        }
        if (index32 && geom->nelem >= (int64_t(1) << 31)) fail_arg("atm_observe_quats: an int32 index cannot name 2^31 elements");
        if (stride < n_samp) fail_arg("atm_observe_quats: rows are shorter than their samples");
        check_rows(quat_row, n_row, n_quat_rows, "atm_observe_quats");
        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> vq(quat_row, quat_row + n_row);
        const size_t o1 = pb.push_vec(vq);
        const int32_t * d_rows = (const int32_t *)(pb.commit(st) + o1);
        int * d_status = static_cast<int *>(Manager::get().scratch(Manager::kScratchStatus, std::max<size_t>(64, (size_t)n_row * sizeof(int))));
        TH_HIP(hipMemsetAsync(d_status, 0, (size_t)n_row * sizeof(int), st));
        if (index32) {
            if (cell_cache) {
                launch_observe_quats<int32_t, true>(g, d_index, d_realization, n_row, n_samp, stride, d_times, d_rows, d_quats, d_good,
                                                    d_atm, d_status, st);
            } else {
                launch_observe_quats<int32_t, false>(g, d_index, d_realization, n_row, n_samp, stride, d_times, d_rows, d_quats, d_good,
                                                     d_atm, d_status, st);
            }
        } else {
            if (cell_cache) {
                launch_observe_quats<int64_t, true>(g, d_index, d_realization, n_row, n_samp, stride, d_times, d_rows, d_quats, d_good,
                                                    d_atm, d_status, st);
            } else {
                launch_observe_quats<int64_t, false>(g, d_index, d_realization, n_row, n_samp, stride, d_times, d_rows, d_quats, d_good,
                                                     d_atm, d_status, st);
            }
        }
        copy_to_host(status, d_status, (size_t)n_row * sizeof(int), st);
        for (int64_t r = 0; r < n_row; ++r) status[r] = status[r] != 0 ? 1 : 0;
    });
}

int toast_hip_atm_flag_failed_dev(int64_t n_row, int64_t n_samp, int64_t stride, const uint8_t * d_good, const double * d_atm,
                                  const int32_t * flag_row, const int32_t * enable, uint8_t * d_det_flags,
                                  int64_t n_flag_rows, uint8_t det_flag_mask, int64_t * n_bad, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n_samp <= 0) return;
        if (!d_good || !d_atm || !flag_row || !enable || !d_det_flags || !n_bad) fail_arg("atm_flag_failed: missing argument");
        if (n_row > kMaxGridY) fail_arg("atm_flag_failed: too many rows for one launch");
        if (stride < n_samp) fail_arg("atm_flag_failed: rows are shorter than their samples");
        check_rows(flag_row, n_row, n_flag_rows, "atm_flag_failed");
        std::vector<int32_t> sorted(flag_row, flag_row + n_row);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
            fail_arg("atm_flag_failed: two entries name one row of flags");
        }
        hipStream_t st = pick_stream(stream);
        ParamBlock pb;
        std::vector<int32_t> vf(flag_row, flag_row + n_row), ve(enable, enable + n_row);
        const size_t o1 = pb.push_vec(vf), o2 = pb.push_vec(ve);
        const char * d = pb.commit(st);
        unsigned long long * d_bad = static_cast<unsigned long long *>(
            Manager::get().scratch(Manager::kScratchAtm, (size_t)n_row * 8 * sizeof(double), st));
        TH_HIP(hipMemsetAsync(d_bad, 0, (size_t)n_row * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_atm_flag_failed, dim3(sample_blocks(n_samp), (unsigned)n_row), dim3(kThreads), 0, st, n_samp,
                           stride, d_good, d_atm, (const int32_t *)(d + o1), (const int32_t *)(d + o2), d_det_flags,
                           det_flag_mask, d_bad);
        TH_HIP(hipGetLastError());
        copy_to_host(n_bad, d_bad, (size_t)n_row * sizeof(int64_t), st);
    });
}

int toast_hip_atm_finish_dev(int64_t n_row, int64_t n_samp, int64_t stride, const uint8_t * d_good, const double * d_atm,
                             const double * gain_absorption, const double * loading, const int32_t * quat_row,
                             const double * d_quats, int64_t n_quat_rows, const int32_t * weight_row,
                             const double * d_weights, int64_t n_weight_rows, int64_t nnz, int64_t comp_i, int64_t comp_q,
                             double pfrac, double scale, const int32_t * data_row, double * d_det_data,
                             int64_t n_data_rows, void * stream) {
    return guarded([&] {
        if (n_row <= 0 || n_samp <= 0) return;
        if (!d_good || !d_atm || !gain_absorption || !quat_row || !d_quats || !data_row || !d_det_data) {
            fail_arg("atm_finish: missing argument");
        }
        if (n_row > kMaxGridY) fail_arg("atm_finish: too many rows for one launch");
        if (stride < n_samp) fail_arg("atm_finish: rows are shorter than their samples");
        check_rows(quat_row, n_row, n_quat_rows, "atm_finish");
        check_rows(data_row, n_row, n_data_rows, "atm_finish");
        if (d_weights) {
            if (!weight_row) fail_arg("atm_finish: weights need their rows");
            check_rows(weight_row, n_row, n_weight_rows, "atm_finish");
            if (nnz < 1 || comp_i >= nnz || comp_q >= nnz) fail_arg("atm_finish: the weights have no such component");
        }
        hipStream_t st = pick_stream(stream);
        std::vector<double> per((size_t)n_row * 3);
        for (int64_t r = 0; r < n_row; ++r) {
            per[3 * r] = gain_absorption[r];
            per[3 * r + 1] = loading ? loading[r] : 0.0;
            per[3 * r + 2] = loading ? 1.0 : 0.0;
        }
        ParamBlock pb;
        std::vector<int32_t> vq(quat_row, quat_row + n_row), vd(data_row, data_row + n_row), vw;
        if (d_weights) vw.assign(weight_row, weight_row + n_row);
        const size_t o0 = pb.push_vec(per), o1 = pb.push_vec(vq), o2 = pb.push_vec(vw), o3 = pb.push_vec(vd);
        const char * d = pb.commit(st);
        hipLaunchKernelGGL(k_atm_finish, dim3(sample_blocks(n_samp), (unsigned)n_row), dim3(kThreads), 0, st, n_samp, stride,
                           d_good, d_atm, (const double *)(d + o0), (const int32_t *)(d + o1), d_quats, (const int32_t *)(d + o2),
                           d_weights, (int)nnz, (int)comp_i, (int)comp_q, pfrac, scale, (const int32_t *)(d + o3),
                           d_det_data);
        TH_HIP(hipGetLastError());
    });
}

}  // extern "C"
