#!/usr/bin/env python3
"""Time the PolyFilter / CommonModeFilter kernels on the GPU against the read-modify-write stream of the same arrays.

Shape: 256 detectors x 720 000 samples at 200 Hz (one GPU's share of BASELINE configs[4]), the `throw` intervals of an
ops.SimGround constant-elevation scan, 10 % of the samples flagged.  Timed with device events, in one process:

* toast_hip_filter_polynomial_dev, single-pass and two-pass path forced in turn, order 1, 3 and 5;
* toast_hip_common_mode_subtract_dev;
* toast_hip_noise_weight_dev over the same rows: 16 B per detector-sample read and written, the ceiling of a
  read-modify-write sweep over these arrays.

Prints one JSON line: ms, algorithmic bytes, TB/s and the ratio of each time to that ceiling.

    python tools/bench_filters.py [--ndet 256] [--minutes 60] [--rate 200] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def throw_intervals(minutes, rate):
    from toast_amd.ops.sim_ground import create_ground_data_from_schedule
    from toast_amd.schedule import make_ces_schedule

    schedule = make_ces_schedule(1, scan_seconds=minutes * 60.0, az_min=40.0, az_max=70.0, el=50.0)
    data = create_ground_data_from_schedule(schedule, n_det=2, rate=rate, fov_deg=8.0, scan_rate_az=1.0, scan_accel_az=1.0,
                                            fix_rate_on_sky=False)
    ob = data.obs[0]
    ivl = ob.intervals["throw"]
    return ob.n_local_samples, np.array([iv.first for iv in ivl], dtype=np.int64), np.array([iv.last for iv in ivl],
                                                                                             dtype=np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    import torch

    from toast_amd import accel, capi
    from toast_amd.capi import interval_dtype

    assert accel.accel_enabled(), "no HIP device visible"
    accel.accel_assign_device(1, 0, 1.0, False)
    D = capi.dev
    n_samp, starts, stops = throw_intervals(args.minutes, args.rate)
    n_det = args.ndet
    cap = D.filter_polynomial_stage_cap()
    longest = int(np.max(stops - starts))
    assert longest <= cap, f"throw of {longest} samples exceeds the single-pass cap {cap}"
    covered = int(np.sum(stops - starts))
    gen = torch.Generator(device="cuda").manual_seed(1)
    sig = 1.0e3 + torch.randn((n_det, n_samp), dtype=torch.float64, device="cuda", generator=gen)
    dflags = (torch.rand((n_det, n_samp), device="cuda", generator=gen) < 0.08).to(torch.uint8)
    sflags = (torch.rand(n_samp, device="cuda", generator=gen) < 0.02).to(torch.uint8)
    idx = np.arange(n_det, dtype=np.int32)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))

    out = {"bench": "filters", "n_det": n_det, "n_samp": n_samp, "rate": args.rate, "n_interval": int(starts.size),
           "longest_interval": longest, "samples_in_intervals": covered, "stage_cap": cap, "reps": args.reps}
    # the ceiling: 16 B read-modify-write over the same rows and the same intervals
    ivl = np.zeros(starts.size, dtype=interval_dtype)
    ivl["first"], ivl["last"] = starts, stops
    ones = np.ones(n_det)
    ms = timed(lambda: D.noise_weight(sig.data_ptr(), n_samp, idx, ivl, ones))
    ceiling_bytes = 16 * n_det * covered
    ceiling_rate = ceiling_bytes / ms          # bytes per ms
    out["noise_weight"] = {"ms": round(ms, 4), "bytes": ceiling_bytes, "tb_s": round(ceiling_bytes / ms / 1e9, 3)}

    def entry(ms, nbytes):
        return {"ms": round(ms, 4), "bytes": nbytes, "tb_s": round(nbytes / ms / 1e9, 3),
                "time_vs_ceiling": round(ms / out["noise_weight"]["ms"], 3),
                "byte_ratio": round(nbytes / ceiling_bytes, 3), "rate_vs_ceiling": round(nbytes / ms / ceiling_rate, 3)}

    for order in (1, 3, 5):
        coeff = torch.zeros((n_det, starts.size, order + 1), dtype=torch.float64, device="cuda")
        status = torch.zeros((n_det, starts.size), dtype=torch.int32, device="cuda")
        for name, path, per_sample in (("single", D.POLY_PATH_SINGLE, 17), ("two_pass", D.POLY_PATH_TWO_PASS, 25)):
            ms = timed(lambda: D.filter_polynomial(order, n_samp, idx, sig.data_ptr(), idx, dflags.data_ptr(), 1,
                                                   sflags.data_ptr(), 1, starts, stops, coeff.data_ptr(), status.data_ptr(),
                                                   path=path))
            # signal read + write (+ a second read), detector flags per detector-sample; the shared flags per sample
            nbytes = per_sample * n_det * covered + covered
            out[f"filter_polynomial_order{order}_{name}"] = entry(ms, nbytes)
        assert int(status.max()) == 0
    ms = timed(lambda: D.common_mode_subtract(n_samp, idx, sig.data_ptr(), idx, dflags.data_ptr(), 1, sflags.data_ptr(), 1))
    out["common_mode_subtract"] = entry(ms, 25 * n_det * n_samp + n_samp)
    out["common_mode_subtract"]["note"] = "whole observation; ceiling scaled by samples"
    scale = n_samp / covered
    out["common_mode_subtract"]["time_vs_ceiling"] = round(ms / (out["noise_weight"]["ms"] * scale), 3)
    out["common_mode_subtract"]["byte_ratio"] = round((25 * n_det * n_samp + n_samp) / (ceiling_bytes * scale), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
