#!/usr/bin/env python3
"""Time ops.FilterBin's regression on the GPU, phase by phase, next to the stream ceiling of the same arrays and next to
PolyFilter followed by GroundFilter on the same shape.

Shape: 256 detectors x 720 000 samples at 200 Hz (one GPU's share of BASELINE configs[4]) from an ops.SimGround
constant-elevation scan with an HWP angle; the single left-right / right-left throws (~120) are the polynomial view;
white noise plus an offset per detector, 1 % of the samples flagged per detector.  Filter: hwp_filter_order 4,
ground_filter_order 5 split by scan direction, poly_filter_order 1 (Nd = 8 + 8 dense templates, K = 2).

Reported (one JSON line), all measured in this run unless marked otherwise:

* ``phase_ms``: template build, dense fit (toast_hip_filterbin_good_counts_dev + toast_hip_template_fit_dev), interval
  accumulate (toast_hip_filterbin_accumulate_dev), host algebra (everything of ``regress`` that is not a device call,
  the scratch transfers included), subtract (toast_hip_filterbin_subtract_dev): wall time around device
  synchronisations (``report_timing``) of the SECOND call on resident data -- the first pays uploads and module load;
* ``host_algebra_share`` of the sum of the phases, and how many detectors took the block-elimination route;
* the two sweeps against the ceiling: toast_hip_noise_weight_dev over the same rows (16 B per detector-sample read and
  written, device events), and the algorithmic bytes of the accumulation (9 B: signal + flag, inside the intervals) and
  of the subtraction (16 B) at that rate -- ``rate_vs_ceiling`` is bytes / ms over the ceiling's bytes / ms.  The
  algorithmic bytes are counted, not measured: no counter run is part of this tool;
* ``poly_then_ground_ms``: ops.PolyFilter(order 1) then ops.GroundFilter(filter_order 5, split, no trend) on the same
  resident arrays in the same process, second call, wall time.

    python tools/bench_filterbin.py [--ndet 256] [--minutes 60] [--rate 200] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VIEW = "subscans"


def build(n_det, minutes, rate):
    from toast_amd.data import IntervalList, defaults
    from toast_amd.ops.sim_ground import create_ground_data_from_schedule
    from toast_amd.schedule import make_ces_schedule

    schedule = make_ces_schedule(1, scan_seconds=minutes * 60.0, az_min=40.0, az_max=70.0, el=50.0)
    data = create_ground_data_from_schedule(schedule, n_det=n_det, rate=rate, fov_deg=8.0, scan_rate_az=1.0,
                                            scan_accel_az=1.0, fix_rate_on_sky=False, hwp_angle=defaults.hwp_angle,
                                            hwp_rpm=120.0)
    data.lazy_host = True
    ob = data.obs[0]
    # the `throw` list is the union of the two directions, i.e. one interval: the single throws are the view
    single = sorted([(int(iv.first), int(iv.last)) for name in (defaults.throw_leftright_interval,
                                                                 defaults.throw_rightleft_interval)
                     for iv in ob.intervals[name]])
    ob.intervals[VIEW] = IntervalList(ob.shared[defaults.times].data, samplespans=single)
    rng = np.random.default_rng(1)
    sig = ob.detdata[defaults.det_data].data
    for d in range(sig.shape[0]):
        sig[d] = 10.0 * rng.standard_normal() + rng.standard_normal(sig.shape[1])
    fl = ob.detdata[defaults.det_flags].data
    fl[rng.random(fl.shape) < 0.01] = defaults.det_mask_invalid
    return data


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    import torch

    from toast_amd import accel, capi, ops
    from toast_amd.capi import interval_dtype
    from toast_amd.data import defaults

    assert accel.accel_enabled(), "no HIP device visible"
    accel.accel_assign_device(1, 0, 1.0, False)
    D = capi.dev
    data = build(args.ndet, args.minutes, args.rate)
    ob = data.obs[0]
    n_det, n_samp = args.ndet, ob.n_local_samples
    spans = [(int(iv.first), int(iv.last)) for iv in ob.intervals[VIEW]]
    covered = sum(b - a for a, b in spans)
    mask = defaults.det_mask_invalid
    fb = ops.FilterBin(name="filterbin", hwp_filter_order=4, ground_filter_order=5, split_ground_template=True,
                       poly_filter_order=1, poly_filter_view=VIEW, det_flag_mask=mask, shared_flag_mask=mask,
                       filter_flag_mask=mask, report_timing=True)
    fb._filter_observation(data, ob, None)          # uploads, module load
    fb.seconds = {}
    fb._filter_observation(data, ob, None)
    phases = {k: round(1e3 * fb.seconds[k], 3) for k in ("template_build", "dense_fit", "interval_accumulate", "host_algebra",
                                                        "subtract")}
    routes = list(fb.routes[ob.name].values())
    n_templates = len(next(a for a in fb.amplitudes[ob.name].values() if a is not None))
    out = {"bench": "filterbin", "n_det": n_det, "n_samp": n_samp, "rate": args.rate, "n_interval": len(spans),
           "samples_in_intervals": covered, "templates_per_detector": n_templates, "phase_ms": phases,
           "total_ms": round(sum(phases.values()), 3),
           "host_algebra_share": round(phases["host_algebra"] / max(sum(phases.values()), 1e-30), 3),
           "routes": {"inv": routes.count(0), "pinv": routes.count(1), "rejected": routes.count(2), "no_fit": routes.count(3)}}
    # ---- the ceiling: 16 B read-modify-write over the same rows (device events)
    dd = ob.detdata[defaults.det_data]
    sig_ptr = accel.accel_device_ptr(dd.buffer)
    idx = np.arange(n_det, dtype=np.int32)
    ivl = np.zeros(1, dtype=interval_dtype)
    ivl["first"], ivl["last"] = 0, n_samp
    ones = np.ones(n_det)

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

    ms = timed(lambda: D.noise_weight(sig_ptr, n_samp, idx, ivl, ones))
    ceiling_rate = 16 * n_det * n_samp / ms
    out["noise_weight"] = {"ms": round(ms, 4), "bytes_per_det_sample": 16, "tb_s": round(ceiling_rate / 1e9, 3)}
    for key, per_sample, samples in (("interval_accumulate", 9, covered), ("subtract", 16, n_samp)):
        nbytes = per_sample * n_det * samples
        out[f"{key}_sweep"] = {"bytes_per_det_sample": per_sample, "bytes": nbytes,
                               "tb_s": round(nbytes / max(phases[key], 1e-9) / 1e9, 3),
                               "rate_vs_ceiling": round(nbytes / max(phases[key], 1e-9) / ceiling_rate, 3),
                               "note": "bytes counted from the algorithm; ms is wall time around a synchronisation and "
                                       "includes the scratch transfers of the call"}
    # ---- the separate filters on the same arrays, for scale
    pf = ops.PolyFilter(order=1, view=VIEW, det_flag_mask=mask, shared_flag_mask=mask, name="polyfilter")
    gf = ops.GroundFilter(trend_order=None, filter_order=5, split_template=True, det_flag_mask=mask, shared_flag_mask=mask,
                          name="groundfilter")

    def both():
        pf.apply(data)
        gf.apply(data)
        accel.native().accel_synchronize()

    both()
    t0 = time.perf_counter()
    both()
    out["poly_then_ground_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
