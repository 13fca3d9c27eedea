#!/usr/bin/env python3
"""Generate tests/golden/sim_noise.npz from THE REFERENCE'S OWN compiled code.  Build container only.

The reference's toast_math_rng.cpp, toast_math_sf.cpp, toast_tod_simnoise.cpp, toast_math_fft.cpp and the two
toast_sys_* files are compiled where they lie into a temporary directory outside the repository, behind a few lines
of ``extern "C"`` glue written by this script (nothing of the reference is copied into the repository).  Taken from
the reference's code: the four random streams (rng_dist_uint64 / uniform_01 / uniform_11 / normal) and the
interpolated amplitudes of tod_sim_noise_psd_interp.

There is no FFTW in the container, so the reference's plan store throws and tod_sim_noise_timestream itself cannot
run.  Its remaining steps are restated here with NumPy, the same substitution make_golden_fft.py makes: the Gaussians
are multiplied by the interpolated amplitudes into the half-complex array (an element-wise product of doubles, the
same values as the reference's loop), ``numpy.fft.irfft`` stands for ``(1 / len) hc2r``, and the middle ``samples``
are cropped and their mean (a sequential sum, as in the reference) removed.

Next to the data the script stores how far the reference's own results are from a more precise evaluation:
gauss_ref_err and scale_ref_err against ``np.longdouble`` evaluations of the same formulas, ts_ref_err as the
distance between the double ``numpy.fft.irfft`` and ``scipy.fft.irfft`` in long double on the same spectrum.  The
tests' tolerances are multiples of these.

    python tests/golden/make_golden_sim_noise.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import scipy.fft

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/src"

GLUE = r"""
#include <cstdint>
#include <cstring>
#include <toast/sys_utils.hpp>
#include <toast/math_rng.hpp>
void tod_sim_noise_psd_interp(double rate, int64_t samples, int64_t oversample, int64_t n_batch, int64_t n_binned,
                              double const * binned_freq, double const * binned_psds, int64_t & fftlen,
                              toast::AlignedVector <double> & interp_psds);
extern "C" {
void g_uint64(size_t n, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t * o) { toast::rng_dist_uint64(n, a, b, c, d, o); }
void g_uniform_01(size_t n, uint64_t a, uint64_t b, uint64_t c, uint64_t d, double * o) { toast::rng_dist_uniform_01(n, a, b, c, d, o); }
void g_uniform_11(size_t n, uint64_t a, uint64_t b, uint64_t c, uint64_t d, double * o) { toast::rng_dist_uniform_11(n, a, b, c, d, o); }
void g_normal(size_t n, uint64_t a, uint64_t b, uint64_t c, uint64_t d, double * o) { toast::rng_dist_normal(n, a, b, c, d, o); }
int64_t g_interp(double rate, int64_t samples, int64_t oversample, int64_t n_batch, int64_t n_binned, const double * f,
                 const double * p, double * out, int64_t cap) {
    int64_t fftlen = 0;
    toast::AlignedVector <double> v;
    tod_sim_noise_psd_interp(rate, samples, oversample, n_batch, n_binned, f, p, fftlen, v);
    if ((int64_t)v.size() <= cap) std::memcpy(out, v.data(), v.size() * sizeof(double));
    return fftlen;
}
}
"""


def build_reference(tmp):
    glue = os.path.join(tmp, "glue.cpp")
    open(glue, "w").write(GLUE)
    subprocess.check_call(["sh", REF + "/libtoast/generate_version_cpp.sh", "golden"], cwd=tmp, stdout=subprocess.DEVNULL)
    srcs = [REF + "/libtoast/src/" + f for f in ("toast_math_rng.cpp", "toast_math_sf.cpp", "toast_tod_simnoise.cpp",
                                                 "toast_math_fft.cpp", "toast_sys_utils.cpp", "toast_sys_environment.cpp")]
    out = os.path.join(tmp, "libref_simnoise.so")
    # -O2, no -march: no FMA contraction, the numerical ground truth (as oracle/ref_build.sh)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I" + REF + "/libtoast/include",
                           "-I" + REF + "/libtoast/src", glue, os.path.join(tmp, "version.cpp")] + srcs + ["-o", out])
    return C.CDLL(out)


U64 = C.c_uint64


def ref_stream(lib, kind, n, k1, k2, c1, c2):
    out = np.empty(n, dtype=np.uint64 if kind == "uint64" else np.float64)
    getattr(lib, "g_" + kind)(C.c_size_t(n), U64(k1), U64(k2), U64(c1), U64(c2), C.c_void_p(out.ctypes.data))
    return out


def ref_interp(lib, rate, samples, oversample, freq, psds):
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    psds = np.ascontiguousarray(np.atleast_2d(psds), dtype=np.float64)
    fftlen = 2
    while fftlen <= oversample * samples:
        fftlen *= 2
    out = np.empty((psds.shape[0], fftlen // 2 + 1))
    lib.g_interp.restype = C.c_int64
    got = lib.g_interp(C.c_double(rate), C.c_int64(samples), C.c_int64(oversample), C.c_int64(psds.shape[0]),
                       C.c_int64(freq.size), C.c_void_p(freq.ctypes.data), C.c_void_p(psds.ctypes.data),
                       C.c_void_p(out.ctypes.data), C.c_int64(out.size))
    assert got == fftlen, (got, fftlen)
    return out


# ------------------------------------------------------------------------------ long double restatements (error measures)
def gauss_longdouble(u):
    """sqrt(2) erfinv(x) from the reference's uniform deviates, every step after x = 2 u - 1 in long double."""
    L = np.longdouble
    co = {}
    import re
    text = open(REF + "/libtoast/src/toast_math_sf.cpp").read()
    body = text[text.index("void toast::vfast_erfinv"):]
    first = body.index("double w = -lg[i];")
    body = body[first:body.index("double w = -lg[i];", first + 1)]      # the polynomial loop, once
    parts = re.split(r"w = (?:w|::sqrt\(w\)) - ([0-9.]+);", body)
    # parts: [head, shift0, poly0, shift1, poly1, shift2, poly2]
    for j in range(3):
        nums = re.findall(r"p (?:=|\+=)\s+(-?[0-9.]+(?:e[-+][0-9]+)?);", parts[2 + 2 * j])
        co[j] = (L(parts[1 + 2 * j]), [L(x) for x in nums])
    # x = 2 u - 1 is taken as the reference (and the device) round it: a correctly rounded IEEE operation shared by
    # both, whose cancellation near |x| = 1 is part of the definition of the stream, not an error of the evaluation
    x = (2.0 * u - 1.0).astype(L)
    ab = np.abs(x)
    w = -np.log((L(1) - ab) * (L(1) + ab))
    out = np.empty_like(x)
    for j, sel in enumerate((w < L(6.25), (w >= L(6.25)) & (w < L(16)), w >= L(16))):
        shift, c = co[j]
        ww = (w[sel] if j == 0 else np.sqrt(w[sel])) - shift
        p = np.full(ww.shape, c[0], dtype=L)
        for cc in c[1:]:
            p = p * ww + cc
        out[sel] = p * x[sel]
    return out * np.sqrt(L(2))


def interp_longdouble(rate, samples, oversample, freq, psd):
    L = np.longdouble
    fftlen = 2
    while fftlen <= oversample * samples:
        fftlen *= 2
    psdlen = fftlen // 2 + 1
    norm = L(rate) * L(psdlen - 1)
    inc = L(np.float64(rate) / np.float64(fftlen - 1))
    f, p = freq.astype(L), psd.astype(L)
    logfreq = np.log10(f + inc)
    shift = L(np.float64(0.01) * np.min(psd[psd != 0]))
    logpsd = np.log10(np.sqrt(p * norm) + shift)
    x = np.log10(inc * np.arange(psdlen).astype(L) + inc)
    ibin = np.clip(np.searchsorted(logfreq[1:], x, side="left"), 0, f.size - 2)
    r = (x - logfreq[ibin]) / (logfreq[ibin + 1] - logfreq[ibin])
    out = L(10) ** (logpsd[ibin] + r * (logpsd[ibin + 1] - logpsd[ibin])) - shift
    out[0] = 0
    return out


def finish_timestream(gauss, scale, samples):
    """The reference's steps after the Gaussians (toast_tod_simnoise.cpp:200-226) with numpy.fft.irfft for
    (1 / len) hc2r; also the distance of that transform to a long double one, relative to the stream's rms."""
    n = gauss.size
    half = n // 2
    spec = np.zeros(half + 1, dtype=np.complex128)
    spec.real[0] = gauss[0] * scale[0]
    spec.real[1:half] = gauss[1:half] * scale[1:half]
    spec.imag[1:half] = gauss[n - 1:half:-1] * scale[1:half]
    spec.real[half] = gauss[half] * scale[half]
    full = np.fft.irfft(spec, n)
    full_ld = scipy.fft.irfft(spec.astype(np.clongdouble), n)
    assert full_ld.dtype == np.longdouble
    off = (n - samples) // 2
    x = full[off:off + samples].copy()
    dc = 0.0
    for v in x:
        dc += v
    dc /= float(samples)
    out = x - dc
    err = float(np.max(np.abs(full.astype(np.longdouble) - full_ld)) / np.sqrt(np.mean(out**2)))
    return out, err


def main():
    from toast_amd.noise import AnalyticNoise

    tmp = tempfile.mkdtemp(prefix="golden_sim_noise_")
    lib = build_reference(tmp)
    out = {}
    M = (1 << 64) - 1

    # ---- random streams: keys and counters near 0, 2^32 and 2^64 - 1, a wrapping counter2, streams that start inside others
    n = 600
    cases = [
        (0, 0, 0, 0), (1, 2, 3, 4), ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) - 7),
        (M, M - 1, M, 5), (M - 3, 1 << 63, 0, M - 250),            # counter2 wraps after 250 elements
        (1, 2, 3, 4 + 123), (M - 3, 1 << 63, 0, 17),                 # start inside case 1; behind the wrap of case 4
    ]
    out["rng_cases"] = np.array(cases, dtype=np.uint64)
    out["rng_n"] = np.array(n)
    gerr = 0.0
    for i, (k1, k2, c1, c2) in enumerate(cases):
        for kind in ("uint64", "uniform_01", "uniform_11", "normal"):
            out[f"rng_{i}_{kind}"] = ref_stream(lib, kind, n, k1, k2, c1, c2)
        g = out[f"rng_{i}_normal"]
        gl = gauss_longdouble(out[f"rng_{i}_uniform_01"])
        gerr = max(gerr, float(np.max(np.abs(g.astype(np.longdouble) - gl) / np.abs(gl))))
    # a long Gaussian stream for the error measure only (reaches the tail polynomial)
    u = ref_stream(lib, "uniform_01", 4000000, 11, 12, 0, 0)
    g = ref_stream(lib, "normal", 4000000, 11, 12, 0, 0)
    gl = gauss_longdouble(u)
    gerr = max(gerr, float(np.max(np.abs(g.astype(np.longdouble) - gl) / np.abs(gl))))
    tail = np.flatnonzero(-np.log((1 - np.abs(2 * u - 1)) * (1 + np.abs(2 * u - 1))) >= 6.25)[:200]
    out["rng_tail_counter"] = tail.astype(np.uint64)      # counters (key 11, 12) whose deviates use the outer polynomials
    out["rng_tail_normal"] = g[tail]
    out["gauss_ref_err"] = np.array(gerr)

    # ---- PSDs: AnalyticNoise (white; two 1/f slopes) and a tabulated PSD with zero bins
    rate = 37.0
    dets = ["white", "knee1", "knee2"]
    an = AnalyticNoise(detectors=dets, rate={d: rate for d in dets}, fmin={d: 1e-5 for d in dets},
                       fknee={"white": 0.0, "knee1": 0.05, "knee2": 0.3}, alpha={"white": 1.0, "knee1": 1.0, "knee2": 2.3},
                       NET={"white": 1.0, "knee1": 2.5e-3, "knee2": 50e-6})
    freq = np.asarray(an.freq("white"))
    psds = np.array([an.psd(d) for d in dets])
    tab = 1e-4 * (1.0 + (0.1 / np.maximum(freq, 1e-6)) ** 1.5)
    tab[[0, 5, 40, freq.size - 3]] = 0.0
    psds = np.vstack([psds, tab])
    out["psd_rate"] = np.array(rate)
    out["psd_freq"] = freq
    out["psd_psds"] = psds
    serr = 0.0
    for samples, keep in ((3000, None), (12345, 8)):          # fftlen 2^13 (all bins) and 2^15 (a subset of the bins)
        sc = ref_interp(lib, rate, samples, 2, freq, psds)
        assert sc.shape[1] == {3000: 4097, 12345: 16385}[samples]
        for b in range(psds.shape[0]):
            ld = interp_longdouble(rate, samples, 2, freq, psds[b])
            serr = max(serr, float(np.max(np.abs(sc[b].astype(np.longdouble) - ld)) / np.max(sc[b])))
        bins = np.arange(sc.shape[1]) if keep is None else np.unique(
            np.concatenate([np.arange(64), np.arange(0, sc.shape[1], keep), [sc.shape[1] - 1]]))
        out[f"interp_{samples}_bins"] = bins
        out[f"interp_{samples}"] = sc[:, bins]
    out["scale_ref_err"] = np.array(serr)

    # ---- timestreams
    terr = 0.0

    def stream(realization, telescope, component, obsindx, detindx, firstsamp, samples, ipsd):
        nonlocal terr
        sc = ref_interp(lib, rate, samples, 2, freq, psds[ipsd])[0]
        fftlen = 2 * (sc.size - 1)
        key1 = realization * 4294967296 + telescope * 65536 + component
        key2 = obsindx * 4294967296 + detindx
        g = ref_stream(lib, "normal", fftlen, key1, key2, 0, firstsamp * 2)
        ts, err = finish_timestream(g, sc, samples)
        terr = max(terr, err)
        return ts

    # name: (realization, telescope, component, obsindx, firstsamp, samples, [(detindx, psd row)])
    ts_cases = {
        "a": (0, 0, 0, 0, 0, 3000, [(0, 1), (1, 2), (77, 0)]),
        "b": (3, 5, 2, 123456, 1000, 3000, [(4, 3)]),
        "c": (1, 1, 0, 9, 0, 4096, [(2, 1)]),                        # fftlen 2^14
        "d": (2, 40000, 7, 4000000000, 250, 12345, [(4294967295, 2)]),
    }
    for name, (rz, tel, comp, obs, first, samples, strs) in ts_cases.items():
        out[f"ts_{name}_params"] = np.array([rz, tel, comp, obs, first, samples], dtype=np.int64)
        out[f"ts_{name}_detindx"] = np.array([s[0] for s in strs], dtype=np.uint64)
        out[f"ts_{name}_psdrow"] = np.array([s[1] for s in strs], dtype=np.int64)
        out[f"ts_{name}_noise"] = np.array([stream(rz, tel, comp, obs, di, first, samples, ip) for di, ip in strs])
    # mixing: two streams into three detector rows of a det_data that holds 1e-3 linspace(-1, 1) before (the sums of
    # sim_tod_noise.py:392-398)
    rz, tel, comp, obs, first, samples, strs = 1, 2, 3, 4, 0, 3000, [(10, 1), (11, 0)]
    mix = np.array([[1.0, 0.0], [0.5, 0.25], [0.0, -2.0]])           # [row][stream]
    streams = [stream(rz, tel, comp, obs, di, first, samples, ip) for di, ip in strs]
    before = 1e-3 * np.linspace(-1.0, 1.0, 3 * samples).reshape(3, samples)    # below the noise: its rounding stays small
    after = before.copy()
    for s in range(2):
        for r in range(3):
            if mix[r, s] != 0:
                after[r] += mix[r, s] * streams[s]
    out["ts_mix_params"] = np.array([rz, tel, comp, obs, first, samples], dtype=np.int64)
    out["ts_mix_detindx"] = np.array([s[0] for s in strs], dtype=np.uint64)
    out["ts_mix_psdrow"] = np.array([s[1] for s in strs], dtype=np.int64)
    out["ts_mix_matrix"] = mix
    out["ts_mix_after"] = after
    out["ts_ref_err"] = np.array(terr)

    path = os.path.join(HERE, "sim_noise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;",
          {k: float(out[k]) for k in ("gauss_ref_err", "scale_ref_err", "ts_ref_err")})


if __name__ == "__main__":
    main()
