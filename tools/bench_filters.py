#!/usr/bin/env python3
"""Time the PolyFilter / CommonModeFilter kernels on the GPU against the read-modify-write stream of the same arrays.

Shape: 256 detectors x 720 000 samples at 200 Hz (one GPU's share of BASELINE configs[4]), the `throw` intervals of an
ops.SimGround constant-elevation scan, 10 % of the samples flagged.  Timed with device events, in one process:

* toast_hip_filter_polynomial_dev, single-pass and two-pass path forced in turn, order 1, 3 and 5;
* toast_hip_common_mode_subtract_dev;
* toast_hip_filter_poly2d_dev, order 1, 2 and 3, over the whole observation with all detectors in one group and in four
  groups: total ms, ms per phase (moments / solve / subtraction, device events inside the launcher), the solve's share,
  and -- with --poly2d-host-samples N -- the host path (``ops.poly_filter.poly2d_host``: lstsq per system) on the first
  N samples, scaled to the observation;
* toast_hip_noise_weight_dev over the same rows: 16 B per detector-sample read and written, the ceiling of a
  read-modify-write sweep over these arrays.

Prints one JSON line: ms, algorithmic bytes, TB/s and the ratio of each time to that ceiling.

    python tools/bench_filters.py [--ndet 256] [--minutes 60] [--rate 200] [--reps 5] [--poly2d-host-samples 0]
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
    # the single throws, left-right and right-left in turn (the `throw` list itself is their union: one interval)
    ivl = sorted(list(ob.intervals["throw_leftright"]) + list(ob.intervals["throw_rightleft"]), key=lambda iv: iv.first)
    return ob.n_local_samples, np.array([iv.first for iv in ivl], dtype=np.int64), np.array([iv.last for iv in ivl],
                                                                                             dtype=np.int64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poly2d-host-samples", type=int, default=0)
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
    poly2d_entries(out, args, D, entry, timed, sig, dflags, sflags, n_det, n_samp)
    print(json.dumps(out))


def poly2d_entries(out, args, D, entry, timed, sig, dflags, sflags, n_det, n_samp):
    """PolyFilter2D over the whole observation (its default view).  Bytes: the signal read twice and written once, the
    detector flags read twice (18 B per detector-sample), the shared flags once per sample and group."""
    import time

    from toast_amd.data import detector_direction
    from toast_amd.ops.poly_filter import poly2d_host, poly2d_templates
    from toast_amd.synth import hex_focalplane

    quats, _ = hex_focalplane(n_det, fov_deg=8.0)
    positions = [np.arcsin(detector_direction(q)[:2]) for q in quats]
    idx = np.arange(n_det, dtype=np.int32)
    starts, stops = np.array([0], dtype=np.int64), np.array([n_samp], dtype=np.int64)
    reps = min(args.reps, 3)
    for n_group in (1, 4):
        det_group = ((np.arange(n_det) // 2) % n_group).astype(np.int32)
        members = [list(np.flatnonzero(det_group == g)) for g in range(n_group)]
        for order in (1, 2, 3):
            templates = poly2d_templates(positions, members, order)

            def call():
                D.filter_poly2d(order, n_samp, idx, sig.data_ptr(), idx, dflags.data_ptr(), 1, sflags.data_ptr(), 1, 0,
                                det_group, n_group, templates, starts, stops)

            saved = args.reps
            args.reps = reps
            ms = timed(call)
            args.reps = saved
            D.filter_poly2d_profile(True)
            call()
            phases = D.filter_poly2d_profile(False)
            e = entry(ms, 18 * n_det * n_samp + n_group * n_samp)
            scale = n_samp / out["samples_in_intervals"]       # the ceiling was timed over the intervals only
            e["time_vs_ceiling"] = round(ms / (out["noise_weight"]["ms"] * scale), 3)
            e["byte_ratio"] = round(e["bytes"] / (16 * n_det * n_samp), 3)
            e["phase_ms"] = {k: round(float(v), 4) for k, v in zip(("moments", "solve", "subtract"), phases)}
            e["solve_share"] = round(float(phases[1] / max(phases.sum(), 1e-30)), 3)
            if args.poly2d_host_samples > 0:
                n_host = min(args.poly2d_host_samples, n_samp)
                hs = sig[:, :n_host].cpu().numpy()
                hf = dflags[:, :n_host].cpu().numpy()
                hsf = sflags[:n_host].cpu().numpy()
                t0 = time.perf_counter()
                poly2d_host(templates, det_group, n_group, hs, idx, hf, idx, 1, hsf, 1, 0, [0], [n_host])
                dt = time.perf_counter() - t0
                e["host_path_ms_scaled"] = round(dt * 1e3 * n_samp / n_host, 1)
                e["host_path_samples"] = n_host
            out[f"filter_poly2d_order{order}_groups{n_group}"] = e


if __name__ == "__main__":
    main()
