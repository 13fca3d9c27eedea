#!/usr/bin/env python3
"""Generate tests/golden/time_constant.npz and time_constant_long.npz by RUNNING THE REFERENCE'S OWN convolution class
with a kernel function.

As in make_golden_fft.py: `AlgorithmBase` / `AlgorithmNumpy` (src/toast/fft.py:121-350) are compiled from the reference
file's syntax tree where it lies (nothing copied into the repository) and
`AlgorithmNumpy(n_tod, n_samp, rate, None, None, None, None, kernel_func, False).convolve(data)` is run -- the call
`toast.fft.convolve(kernel_func=...)` makes for ops.TimeConstant (src/toast/ops/time_constant.py:208-217).  The kernel
function passed to it is this script's own statement of the single-pole kernel 1 + i 2 pi tau f.

Cases: five detectors with tau = [0, 1, 3, 10, 50] ms, convolution (by 1 / K) and deconvolution (by K), white noise plus
a ramp (one input row per case, shared by the five detectors: only tau differs), each at the smallest shape that reaches
one multiply stage of the device code:

    n_samp  rate    n_fft
    1500     37 Hz   4096   the rocFFT pipeline
    2049    200 Hz   8192   smallest fused length, N1 = 2: only the self-paired rows (DC, Nyquist); odd length
    3000    200 Hz   8192   the same with an even length (aligned pass 1); with impulse extents and flags
    9000    200 Hz  32768   N1 = 8: rows beyond the self-paired ones

Outputs are full-entropy doubles (8 bytes each however they are packed), and 2 x 5 x 15 549 of them do not fit one file
of 1 MiB: the 9000-sample case goes to time_constant_long.npz, the other three to time_constant.npz.

For the 3000-sample case the impulse extents (src/toast/fft.py:838-873 through the same class) are stored, and one
random flag pattern before and after the reference's `extend_flags` (src/toast/utils.py:1055-1113, compiled in place
as well) plus the end flagging of fft.py:938-943.  The extents are integers decided at a 2 % threshold: this script
ASSERTS that the samples on both sides of each boundary are more than 1e-6 (relative) away from the threshold, so that
an implementation which agrees to 1e-12 must find the same integers.

Build container only; the fixtures are committed.

    python tests/golden/make_golden_time_constant.py
"""
import ast
import os

import numpy as np

from make_golden_fft import load_reference_classes

HERE = os.path.dirname(os.path.abspath(__file__))
TAUS = np.array([0.0, 1.0e-3, 3.0e-3, 10.0e-3, 50.0e-3])
CASES = {"n1500": (1500, 37.0), "n2049": (2049, 200.0), "n3000": (3000, 200.0), "n9000": (9000, 200.0)}
LONG = ("n9000",)
# widths of the impulse responses at 200 Hz, measured with the reference on the CPU
EXPECTED_EXTENTS = {False: [2, 17, 24, 16, 44], True: [2, 21, 61, 101, 101]}


def pole_kernel_func(taus, deconvolve):
    def kernel_func(indx, kfreqs):
        kernel = np.zeros(len(kfreqs), dtype=np.complex128)
        kernel.real[:] = 1
        kernel.imag[:] = 2.0 * np.pi * taus[indx] * kfreqs
        if not deconvolve:
            kernel = 1.0 / kernel
        return kernel

    return kernel_func


def load_reference_extend_flags():
    utils = "/root/reference/src/toast/utils.py"
    tree = ast.parse(open(utils).read(), utils)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "extend_flags"]
    mod = ast.Module(body=fn, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, utils, "exec"), ns)
    return ns["extend_flags"]


def impulse_extents(AlgorithmNumpy, n_samp, rate, deconvolve):
    """src/toast/fft.py:838-873 with the threshold margins of every boundary."""
    n_tod = len(TAUS)
    temp = np.zeros((n_tod, n_samp))
    temp[:, n_samp // 2] = 100.0
    AlgorithmNumpy(n_tod, n_samp, rate, None, None, None, None, pole_kernel_func(TAUS, deconvolve), False).convolve(temp)
    extend = np.zeros(n_tod, dtype=np.int32)
    margin = np.inf
    for itod in range(n_tod):
        atemp = np.absolute(temp[itod])
        ipeak = np.argmax(atemp)
        apeak = atemp[ipeak]
        imin = ipeak
        while imin > 0 and atemp[imin] > 0.02 * apeak:
            imin -= 1
        imax = ipeak
        while imax < n_samp and atemp[imax] > 0.02 * apeak:
            imax += 1
        extend[itod] = imax - imin
        assert 0 < imin and imax < n_samp, "the walks ended at the threshold, not at the ends"
        # the peak must be unique too (argmax), and every sample next to a boundary clear of the threshold
        second = np.max(np.delete(atemp, ipeak))
        margin = min(margin, (apeak - second) / apeak)
        for j in (imin, imin + 1, imax - 1, imax):
            margin = min(margin, abs(atemp[j] - 0.02 * apeak) / (0.02 * apeak))
    assert margin > 1.0e-6, margin
    return extend, margin


def main():
    AlgorithmNumpy = load_reference_classes()
    extend_flags = load_reference_extend_flags()
    rng = np.random.default_rng(20261019)
    out = {"taus": TAUS}
    out_long = {"taus": TAUS}
    for name, (n_samp, rate) in CASES.items():
        dst = out_long if name in LONG else out
        data = rng.standard_normal(n_samp) + np.linspace(-1, 2, n_samp)
        dst[f"{name}_rate"] = np.array(rate)
        dst[f"{name}_data"] = data
        for deconvolve in (False, True):
            result = np.tile(data, (len(TAUS), 1))
            alg = AlgorithmNumpy(len(TAUS), n_samp, rate, None, None, None, None, pole_kernel_func(TAUS, deconvolve), False)
            alg.convolve(result)
            dst[f"{name}_out_{'deconvolve' if deconvolve else 'convolve'}"] = result
            dst[f"{name}_n_fft"] = np.array(alg.n_fft)
    n_samp, rate = CASES["n3000"]
    flags_in = (rng.random(n_samp) < 0.002).astype(np.uint8)
    flags_in[7::503] |= 2            # a bit outside the mask
    out["n3000_flags_in"] = flags_in
    for deconvolve in (False, True):
        key = "deconvolve" if deconvolve else "convolve"
        extend, margin = impulse_extents(AlgorithmNumpy, n_samp, rate, deconvolve)
        assert extend.tolist() == EXPECTED_EXTENTS[deconvolve], extend
        print(f"{key}: extents {extend.tolist()}, smallest threshold margin {margin:.2e}")
        out[f"n3000_extents_{key}"] = extend
        flags = np.tile(flags_in, (len(TAUS), 1))
        for itod in range(len(TAUS)):            # fft.py:938-943
            ext = extend[itod]
            extend_flags(flags[itod], 1, ext)
            flags[itod][:ext] |= 1
            flags[itod][-ext:] |= 1
        out[f"n3000_flags_{key}"] = flags
    for fname, d in (("time_constant.npz", out), ("time_constant_long.npz", out_long)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **d)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        print("wrote", fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
