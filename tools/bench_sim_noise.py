#!/usr/bin/env python3
"""Noise simulation on the device against the host way of filling ``det_data``.

One JSON line: Gaussian deviates per second of the random-stream kernel alone; seconds of ``toast_hip_sim_noise_dev``
for --ndet x --samples (default cfg-3: 1024 x 720 000 at 200 Hz, fftlen 2^21) into a resident buffer, first call and
warmed up, and split into spectrum, transform and crop / mix by events on the stream; and, for comparison,
``np.random.default_rng().standard_normal`` of the same shape plus its upload on the same machine.

    python tools/bench_sim_noise.py [--ndet 1024] [--samples 720000] [--rate 200] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=720000)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--no-host", action="store_true", help="skip the host white noise + upload comparison")
    args = ap.parse_args(argv)
    from toast_amd import capi, rng
    from toast_amd.accel import (accel_assign_device, accel_data_create, accel_data_delete, accel_data_update_device,
                                 accel_device_ptr)
    from toast_amd.noise import AnalyticNoise

    accel_assign_device(1, 0, 8.0 * args.ndet * args.samples / 2**30 + 6.0, False)
    buf = np.zeros((args.ndet, args.samples))
    accel_data_create(buf, "bench_sim_noise")
    ptr = accel_device_ptr(buf)
    out = {"ndet": args.ndet, "samples": args.samples, "rate": args.rate,
           "fftlen": capi.sim_noise_fft_length(args.samples, 2)}

    # the Gaussian kernel alone: one stream per row of the buffer
    lengths, keys, counters = [args.samples] * args.ndet, [(1, d) for d in range(args.ndet)], [(0, 0)] * args.ndet

    def timed(fn):
        t = time.perf_counter()
        fn()
        return time.perf_counter() - t

    def gauss():
        rng.random_multi_device(lengths, keys, counters, ptr, buf.size)
        capi.synchronize()

    gauss()
    out["gaussian_deviates_per_s"] = buf.size / min(timed(gauss) for _ in range(5))

    dets = ["d"]
    an = AnalyticNoise(detectors=dets, rate={"d": args.rate}, fmin={"d": 1e-5}, fknee={"d": 0.05}, alpha={"d": 1.0},
                       NET={"d": 50e-6})
    freq, psds = np.asarray(an.freq("d")), np.tile(np.asarray(an.psd("d")), (args.ndet, 1))
    idx = np.arange(args.ndet, dtype=np.uint64)

    def sim():
        capi.dev.sim_noise(0, 1, 0, 2, args.rate, 0, args.samples, 2, idx, freq, psds, ptr, args.ndet)
        capi.synchronize()

    out["sim_noise_first_call_s"] = timed(sim)
    out["sim_noise_s"] = min(timed(sim) for _ in range(3))
    # the same call with events around the three phases of every batch (toast_hip_sim_noise_timing)
    capi.dev.sim_noise_timing(True)
    sim()
    spectrum, transform, crop = capi.dev.sim_noise_timing(False)
    out["sim_noise_spectrum_s"], out["sim_noise_transform_s"], out["sim_noise_crop_mix_s"] = (
        spectrum / 1e3, transform / 1e3, crop / 1e3)
    if not args.no_host:
        t = time.perf_counter()
        buf[:] = np.random.default_rng(1).standard_normal(buf.shape)
        out["host_standard_normal_s"] = time.perf_counter() - t
        t = time.perf_counter()
        accel_data_update_device(buf, "bench_sim_noise")
        capi.synchronize()
        out["host_upload_s"] = time.perf_counter() - t
    accel_data_delete(buf, "bench_sim_noise")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
