#!/usr/bin/env python3
"""Time the noise-estimation kernels (csrc/noise_estim.hip): one JSON line per shape.

* cfg-3 (1024 detectors x 720 000 samples at 200 Hz, lagmax 10 000; ``--ndet`` pairs are run and the time is also scaled to
  1024) and a ground-like shape (about 100 views of a few thousand samples);
* phases by ``toast_hip_noise_estim_timing``: high-pass, sums (with hits), reduction, download [ms];
* FMA/s of the sums kernel next to the FMA/s of a register-only FP64 FMA loop in the same launch shape
  (``toast_hip_noise_estim_fma_ceiling``): the ceiling this tool measures itself;
* the host entry on one detector of the same shape (left out with ``--no-host``) and the host tail after the sums.

    python tools/bench_noise_estim.py [--ndet 16] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from toast_amd import capi  # noqa: E402
from toast_amd.accel import accel_data_create, accel_data_delete, accel_data_update_device, accel_device_ptr  # noqa: E402
from toast_amd.ops.noise_estimation_utils import psds_from_sums  # noqa: E402


def run_shape(name, n_det, n, lagmax, segments, rate, host):
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n_det, n))
    good = (rng.random((n_det, n)) > 0.01).astype(np.uint8)
    hp = np.empty((n_det, n))
    sums, hits = np.zeros((n_det, 1, lagmax)), np.zeros((n_det, 1, lagmax), dtype=np.int64)
    dev = [rows, good, hp, sums, hits]
    for a in dev:
        accel_data_create(a, "bench_noise_estim")
    for a in (rows, good, sums, hits):
        accel_data_update_device(a, "bench_noise_estim")
    p_rows, p_good, p_hp, p_sums, p_hits = (accel_device_ptr(a) for a in dev)
    idx = list(range(n_det))
    first, last = [s[0] for s in segments], [s[1] for s in segments]
    all_sums, real = [1] * len(segments), [0] * len(segments)

    def once():
        capi.dev.noise_estim_highpass(n, lagmax, p_rows, n_det, n, idx, p_good, n_det, n, idx, p_hp, n)
        capi.dev.fod_sums(idx, idx, idx, p_hp, n_det, n, p_good, n_det, n, first, last, all_sums, real, 1, lagmax, 0,
                          p_sums, p_hits)
        capi.dev.noise_estim_fetch(p_sums, sums, p_hits, hits)

    once()                                        # warm-up: scratch, parameter blocks
    capi.dev.noise_estim_timing(True)
    t0 = time.perf_counter()
    once()
    wall = time.perf_counter() - t0
    phases = capi.dev.noise_estim_timing(False)
    # products actually wanted (the kernel also multiplies its zero padding)
    fma = float(sum((b - a) * min(lagmax, b - a) - min(lagmax, b - a) * (min(lagmax, b - a) - 1) / 2 for a, b in segments)) * n_det
    n_block = max(1, int(fma / (256 * 8 * 1024)))
    ceiling_ms = capi.dev.noise_estim_fma_ceiling(n_block, 1024)
    t0 = time.perf_counter()
    psds_from_sums(hits[:, 0].copy(), sums[:, 0].copy(), lagmax, lagmax, rate)
    tail = time.perf_counter() - t0
    out = dict(shape=name, pairs=n_det, samples=n, lagmax=lagmax, segments=len(segments), wall_s=round(wall, 4),
               highpass_ms=round(phases[0], 3), sums_ms=round(phases[1], 3), reduce_ms=round(phases[2], 3),
               download_ms=round(phases[3], 3), sums_gfma_per_s=round(fma / phases[1] / 1e6, 1) if phases[1] else None,
               ceiling_gfma_per_s=round(n_block * 256 * 8 * 1024 / ceiling_ms / 1e6, 1), host_tail_s=round(tail, 4))
    if host:
        s1, h1 = np.zeros(lagmax), np.zeros(lagmax, dtype=np.int64)
        t0 = time.perf_counter()
        for a, b in segments:
            capi.fod_autosums(np.ascontiguousarray(rows[0, a:b]), np.ascontiguousarray(good[0, a:b]), lagmax, s1, h1, 1)
        out["host_one_detector_s"] = round(time.perf_counter() - t0, 3)
    for a in dev:
        accel_data_delete(a, "bench_noise_estim")
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=16, help="pairs run at cfg-3 length (1024 in the configuration)")
    ap.add_argument("--no-host", action="store_true", help="leave out the host entry on one detector (tens of seconds)")
    args = ap.parse_args()
    run_shape("cfg-3", args.ndet, 720000, 10000, [(0, 720000)], 200.0, not args.no_host)
    views = [(i * 3600, i * 3600 + 3000) for i in range(100)]
    run_shape("ground-like", max(args.ndet, 64), 360000, 1000, views, 100.0, not args.no_host)


if __name__ == "__main__":
    main()
