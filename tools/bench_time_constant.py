#!/usr/bin/env python3
"""Time the single-pole (time constant) convolution on the GPU against the tabulated-kernel convolution it sits next to.

Shapes: cfg-3 (1024 detectors x 720 000 samples at 200 Hz) and one GPU's share of the ground configuration (256 x
720 000).  In one process, timed with device events around the C entry points (kernel coefficients prepared once,
outside the timing; every call starts from the same timestreams), the three calls INTERLEAVED call by call:

* toast_hip_fft_convolve_pole_dev: K = 1 / (1 + i 2 pi tau f), one time constant per detector (1 .. 50 ms);
* toast_hip_fft_convolve_dev with one COMPLEX kernel per detector as PCHIP cubics on 77 knots (the baseline: same
  passes, same bytes, plus the interval search, two cubics, sin / cos per bin, the table copy and the table launches);
* toast_hip_fft_convolve_dev with one REAL kernel per detector (NoiseFilter's call).

The measurement is repeated in `--rounds` rounds of `--reps` interleaved calls; the median of each round is printed.
The spread of the baseline against itself is the range of its round medians; the single-pole call passes when its
median over all rounds does not exceed the largest of the baseline's round medians.

Prints one JSON line per shape: the medians in ms, `pipeline_bytes_per_sample`, TB/s and the share of 8 TB/s.

    python tools/bench_time_constant.py [--shapes 1024,256] [--minutes 60] [--rate 200] [--rounds 5] [--reps 7]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TB_S = 8.0


def noise_kernels(freq, n_det, complex_phase):
    """Inverse-PSD kernels of 1/f noise with a knee per detector; with a small frequency-dependent phase when complex."""
    d = np.arange(n_det)[:, None]
    net = 1.0 + 0.1 * (d % 7)
    fknee = 0.05 * (1 + d % 5)
    psd = net ** 2 * (freq[None, :] + fknee) / np.maximum(freq[None, :] + 1e-5, 1e-12)
    kern = net ** 2 / np.maximum(psd, 1e-3 * net ** 2)
    kern[:, 0] = 0
    if complex_phase:
        kern = kern * np.exp(-1j * 0.01 * (1.0 + d / n_det) * freq[None, :])
    return kern


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024,256", help="detector counts, comma separated")
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args(argv)
    import torch

    from toast_amd import accel, capi, fft

    assert accel.accel_enabled(), "no HIP device visible"
    accel.accel_assign_device(1, 0, 1.0, False)
    lib = capi.lib()
    n_samp = int(args.minutes * 60 * args.rate)
    rate = args.rate
    n_fft = fft.fft_length(n_samp)
    apod = fft.apodization(min((n_fft - n_samp) // 2, n_samp))
    freq = np.concatenate([[0.0], np.geomspace(1e-5, rate / 2, 76)])         # 77 knots
    bytes_per_sample = fft.pipeline_bytes_per_sample(n_samp)
    stream = torch.cuda.current_stream().cuda_stream

    for n_det in [int(x) for x in args.shapes.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(n_det)
        orig = torch.randn((n_det, n_samp), dtype=torch.float64, device="cuda", generator=gen)
        work = torch.empty_like(orig)
        idx = np.arange(n_det, dtype=np.int32)
        taus = np.ascontiguousarray(np.geomspace(1e-3, 50e-3, n_det))
        tabs = {}
        for name, cplx in (("pchip_complex", True), ("pchip_real", False)):
            mag_c, ang_c = fft.kernel_coefficients(freq, noise_kernels(freq, n_det, cplx))
            assert (ang_c is not None) == cplx
            tabs[name] = (mag_c, ang_c)

        def call_pole():
            capi._check(lib.toast_hip_fft_convolve_pole_dev(
                C.c_void_p(work.data_ptr()), fft._p(idx), C.c_int64(n_det), C.c_int64(n_samp), C.c_double(rate),
                fft._p(taus), C.c_int(1), fft._p(apod), C.c_int64(apod.size), C.c_int64(0), C.c_void_p(stream)))

        def call_tab(name):
            mag_c, ang_c = tabs[name]
            capi._check(lib.toast_hip_fft_convolve_dev(
                C.c_void_p(work.data_ptr()), fft._p(idx), C.c_int64(n_det), C.c_int64(n_samp), C.c_double(rate),
                fft._p(freq), C.c_int64(freq.size), fft._p(mag_c), fft._p(ang_c), C.c_int64(n_det), C.c_int(0),
                fft._p(apod), C.c_int64(apod.size), C.c_int64(0), C.c_void_p(stream)))

        calls = {"pole": call_pole, "pchip_complex": lambda: call_tab("pchip_complex"),
                 "pchip_real": lambda: call_tab("pchip_real")}

        def timed(fn):
            work.copy_(orig)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        for fn in calls.values():        # plans, tables, scratch
            timed(fn)
            timed(fn)
        rounds = {k: [] for k in calls}
        samples = {k: [] for k in calls}
        for _ in range(args.rounds):
            this = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, fn in calls.items():
                    this[k].append(timed(fn))
            for k in calls:
                rounds[k].append(float(np.median(this[k])))
                samples[k] += this[k]
        total_bytes = bytes_per_sample * n_det * n_samp
        out = {"bench": "time_constant", "n_det": n_det, "n_samp": n_samp, "rate": rate, "n_fft": n_fft,
               "implementation": fft.implementation(n_samp), "rounds": args.rounds, "reps": args.reps, "n_knot": int(freq.size),
               "pipeline_bytes_per_sample": round(bytes_per_sample, 2)}
        for k in calls:
            med = float(np.median(samples[k]))
            out[k] = {"median_ms": round(med, 4), "round_medians_ms": [round(x, 4) for x in rounds[k]],
                      "min_ms": round(min(samples[k]), 4), "tb_s": round(total_bytes / med / 1e9, 3),
                      "share_of_peak": round(total_bytes / med / 1e9 / PEAK_TB_S, 3)}
        base = rounds["pchip_complex"]
        out["baseline_spread_ms"] = [round(min(base), 4), round(max(base), 4)]
        out["pole_not_slower_than_baseline"] = bool(out["pole"]["median_ms"] <= max(base))
        print(json.dumps(out), flush=True)
        del orig, work


if __name__ == "__main__":
    main()
