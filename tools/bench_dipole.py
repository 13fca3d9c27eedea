#!/usr/bin/env python3
"""Time the dipole kernel (csrc/sim_dipole.hip, toast_hip_sim_dipole_dev) on the GPU against the 16-byte stream ceiling.

Shapes: cfg-3 (1024 detectors x 720 000 samples) and one GPU's share of the ground configuration (256 x 720 000).  In one
process, timed with device events around the C entry points, the calls INTERLEAVED call by call:

* toast_hip_sim_dipole_dev, mode total (telescope and solar velocity, the relativistic addition) at freq 0 and at
  150 GHz, one launch over the whole observation and all detectors, flags with mask 1 on two per cent of the samples;
* toast_hip_noise_weight_dev over the same rows: 16 B per detector-sample read and written, the ceiling of a
  read-modify-write sweep over these arrays (the ceiling of tools/bench_filters.py);
* toast_hip_pointing_detector_dev on the same shape, for scale: the kernel that a chain PointingDetectorSimple -> host
  math would start with writes 32 B of quaternions per detector-sample.

Prints one JSON line per shape: median ms, detector-samples per second, ``16 B x detector-samples / time`` in TB/s and
that rate as a share of the ceiling's.

    python tools/bench_dipole.py [--shapes 1024,256] [--minutes 60] [--rate 200] [--rounds 3] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024,256", help="detector counts, comma separated")
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    import torch

    from toast_amd import accel, capi, dipole, synth

    assert accel.accel_enabled(), "no HIP device visible"
    accel.accel_assign_device(1, 0, 1.0, False)
    D = capi.dev
    n_samp = int(args.minutes * 60 * args.rate)
    times = np.arange(n_samp) / args.rate
    bore = torch.from_numpy(synth.satellite_boresight(n_samp, args.rate)).cuda()
    vel = torch.from_numpy(np.ascontiguousarray(synth.orbital_velocity(times, period_s=86400.0))).cuda()
    flags = torch.from_numpy(synth.shared_flags_block(n_samp, frac=0.02)).cuda()
    solar = dipole.solar_velocity("E")
    ivl = synth.make_intervals(n_samp, 1)

    for n_det in [int(x) for x in args.shapes.split(",")]:
        fp, _ = synth.hex_focalplane(n_det)
        idx = np.arange(n_det, dtype=np.int32)
        gen = torch.Generator(device="cuda").manual_seed(n_det)
        sig = torch.randn((n_det, n_samp), dtype=torch.float64, device="cuda", generator=gen)
        quats = torch.empty((n_det, n_samp, 4), dtype=torch.float64, device="cuda")
        ones = np.ones(n_det)

        def call_dipole(freq):
            D.sim_dipole(fp, bore.data_ptr(), idx, sig.data_ptr(), n_det, n_samp, ivl, flags.data_ptr(), n_samp, 1,
                         vel.data_ptr(), solar, dipole.t_cmb, freq, 1.0)

        calls = {
            "sim_dipole_total_f0": lambda: call_dipole(0.0),
            "sim_dipole_total_f150": lambda: call_dipole(150.0e9),
            "noise_weight": lambda: D.noise_weight(sig.data_ptr(), n_samp, idx, ivl, ones),
            "pointing_detector": lambda: D.pointing_detector(fp, bore.data_ptr(), idx, quats.data_ptr(), n_samp, ivl,
                                                             flags.data_ptr(), n_samp, 1),
        }

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        for fn in calls.values():        # parameter blocks, first touch
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
        assert bool(torch.isfinite(sig).all())
        det_samples = n_det * n_samp
        ceiling = float(np.median(samples["noise_weight"]))
        out = {"bench": "sim_dipole", "n_det": n_det, "n_samp": n_samp, "rounds": args.rounds, "reps": args.reps,
               "det_tile": D.sim_dipole_det_tile()}
        for k in calls:
            med = float(np.median(samples[k]))
            nbytes = (32 if k == "pointing_detector" else 16) * det_samples
            out[k] = {"median_ms": round(med, 4), "round_medians_ms": [round(x, 4) for x in rounds[k]],
                      "min_ms": round(min(samples[k]), 4), "det_samples_per_s": float(f"{det_samples / med * 1e3:.4g}"),
                      "bytes_per_det_sample": nbytes // det_samples, "tb_s": round(nbytes / med / 1e9, 3)}
            if k.startswith("sim_dipole"):
                out[k]["share_of_16B_ceiling"] = round(ceiling / med, 3)
        print(json.dumps(out), flush=True)
        del sig, quats


if __name__ == "__main__":
    main()
