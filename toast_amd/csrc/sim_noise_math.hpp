// sim_noise_math.hpp -- the arithmetic of the counter-based random streams and of the PSD interpolation, written
// once for the host entries (capi level, libm) and the device kernels (sim_noise.hip).  Every multiply and add is
// rounded on its own (the library is built with -ffp-contract=off), in the operation order of the reference
// [ref: src/libtoast/src/toast_math_rng.cpp:22-131, toast_math_sf.cpp:572-735, toast_tod_simnoise.cpp:14-152].
//
// Threefry2x64 with 20 rounds is written from its published definition: J. K. Salmon, M. A. Moraes, R. O. Dror,
// D. E. Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11 (the Threefish block function of Skein without
// the tweak).  The inverse error function is M. Giles' polynomial approximation, "Approximating the erfinv
// function", GPU Computing Gems Jade edition (2011), double precision variant, in the form the reference evaluates.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TH_HD __host__ __device__ __forceinline__
#else
#define TH_HD inline
#endif

namespace toast_hip {
namespace simnoise {

TH_HD uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// First output word of Threefry2x64-20 for counter (c0, c1) and key (k0, k1).
TH_HD uint64_t threefry2x64_20(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t k1) {
    // key schedule parity constant and the 2x64 rotation schedule of the paper (period 8)
    const uint64_t ks[3] = {k0, k1, 0x1BD11BDAA9FC1A22ull ^ k0 ^ k1};
    const int rot[8] = {16, 42, 12, 31, 16, 32, 24, 21};
    uint64_t x0 = c0 + ks[0];
    uint64_t x1 = c1 + ks[1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 20; ++r) {
        x0 += x1;
        x1 = rotl64(x1, rot[r & 7]);
        x1 ^= x0;
        if ((r & 3) == 3) {
            const int s = (r >> 2) + 1;   // key injection number 1 .. 5
            x0 += ks[s % 3];
            x1 += ks[(s + 1) % 3];
            x1 += (uint64_t)s;
        }
    }
    return x0;
}

// (0, 1]: as dense as a double allows, never 0 [ref: Random123 uniform.hpp u01<double, uint64_t>]
TH_HD double u01(uint64_t v) {
    const double x = (double)v * 0x1p-64;
    return x + 0x1p-65;
}

// [-1, 1], never 0 [ref: Random123 uniform.hpp uneg11<double, uint64_t>]
TH_HD double uneg11(uint64_t v) {
    const double x = (double)(int64_t)v * 0x1p-63;
    return x + 0x1p-64;
}

// Horner steps as two rounded operations each: p *= w; p += c
template <int N>
TH_HD double horner(const double (&c)[N], double w) {
    double p = c[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 1; j < N; ++j) {
        p = p * w;
        p = p + c[j];
    }
    return p;
}

// erfinv(x) by Giles' three-interval polynomials in w = -log((1 - |x|)(1 + |x|)).  The tail polynomial carries the
// coefficient sequence of the reference (toast_math_sf.cpp:690-731), which repeats two pairs of Giles' table: results
// must match the reference's streams, not the published table.
TH_HD double erfinv_giles(double x) {
    const double ab = fabs(x);
    const double arg = (1.0 - ab) * (1.0 + ab);
    double w = -log(arg);
    double p;
    if (w < 6.25) {
        const double c[23] = {-3.6444120640178196996e-21, -1.685059138182016589e-19, 1.2858480715256400167e-18,
                              1.115787767802518096e-17, -1.333171662854620906e-16, 2.0972767875968561637e-17,
                              6.6376381343583238325e-15, -4.0545662729752068639e-14, -8.1519341976054721522e-14,
                              2.6335093153082322977e-12, -1.2975133253453532498e-11, -5.4154120542946279317e-11,
                              1.051212273321532285e-09, -4.1126339803469836976e-09, -2.9070369957882005086e-08,
                              4.2347877827932403518e-07, -1.3654692000834678645e-06, -1.3882523362786468719e-05,
                              0.0001867342080340571352, -0.00074070253416626697512, -0.0060336708714301490533,
                              0.24015818242558961693, 1.6536545626831027356};
        w = w - 3.125;
        p = horner(c, w);
    } else if (w < 16.0) {
        const double c[19] = {2.2137376921775787049e-09, 9.0756561938885390979e-08, -2.7517406297064545428e-07,
                              1.8239629214389227755e-08, 1.5027403968909827627e-06, -4.013867526981545969e-06,
                              2.9234449089955446044e-06, 1.2475304481671778723e-05, -4.7318229009055733981e-05,
                              6.8284851459573175448e-05, 2.4031110387097893999e-05, -0.0003550375203628474796,
                              0.00095328937973738049703, -0.0016882755560235047313, 0.0024914420961078508066,
                              -0.0037512085075692412107, 0.005370914553590063617, 1.0052589676941592334,
                              3.0838856104922207635};
        w = sqrt(w) - 3.25;
        p = horner(c, w);
    } else {
        const double c[21] = {-2.7109920616438573243e-11, -2.5556418169965252055e-10, 1.5076572693500548083e-09,
                              -2.5556418169965252055e-10, 1.5076572693500548083e-09, -3.7894654401267369937e-09,
                              7.6157012080783393804e-09, -1.4960026627149240478e-08, 2.9147953450901080826e-08,
                              -6.7711997758452339498e-08, 2.2900482228026654717e-07, -6.7711997758452339498e-08,
                              2.2900482228026654717e-07, -9.9298272942317002539e-07, 4.5260625972231537039e-06,
                              -1.9681778105531670567e-05, 7.5995277030017761139e-05, -0.00021503011930044477347,
                              -0.00013871931833623122026, 1.0103004648645343977, 4.8499064014085844221};
        w = sqrt(w) - 5.0;
        p = horner(c, w);
    }
    return p * x;
}

// unit-variance Gaussian deviate of one counter: sqrt(2) erfinv(2 u - 1)
TH_HD double gaussian(uint64_t v) {
    const double u = u01(v);
    const double x = 2.0 * u - 1.0;
    return erfinv_giles(x) * 1.4142135623730951;   // ::sqrt(2.0)
}

enum { kUint64 = 0, kUniform01 = 1, kUniform11 = 2, kNormal = 3 };

// Interpolated amplitude sqrt(psd norm) at bin k > 0 of the transform from the binned tables
// (toast_tod_simnoise.cpp:123-144): linear in log10 frequency between log10(sqrt(psd norm) + psdshift).
// `ibin` is the interval: the smallest b <= n_binned - 2 with logfreq[b + 1] >= x.
TH_HD double interp_scale_at(double x, int ibin, const double * logfreq, const double * stepinv,
                             const double * logpsd, double psdshift) {
    const double r = (x - logfreq[ibin]) * stepinv[ibin];
    double v = logpsd[ibin] + r * (logpsd[ibin + 1] - logpsd[ibin]);
    v = pow(10.0, v);
    v -= psdshift;
    return v;
}

// The interval by bisection.  On a non-decreasing logfreq this is where the reference's forward walk over
// increasing bins stands at x (toast_tod_simnoise.cpp:135-138).
TH_HD int interp_interval(double x, const double * logfreq, int n_binned) {
    int lo = 0, hi = n_binned - 2;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (logfreq[mid + 1] < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

}  // namespace simnoise
}  // namespace toast_hip
