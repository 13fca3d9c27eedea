#!/usr/bin/env python3
"""Time the atmosphere-observation kernel (csrc/atm_observe.hip: toast_hip_atm_observe_dev): one JSON line per shape
and kernel option.

* the workflow's shape (``--ndet`` 256 detectors x 720 000 samples through the stand-in slab of
  workflows/ground_filter_mapmaker.py --atmosphere: 20 m cells, rays to 2 km) and one short shape (64 x 6000);
* per option -- compressed index as int32 or int64, with and without the one-cell register cache -- the best and the
  median of ``--reps`` timed launches after one warm-up launch, alternating the options inside every repetition;
* ``ms`` is a host clock around one launch that ends with the read-back of the status word (a device synchronise);
  ``ray_steps_per_s`` = rows x samples x steps / time; ``gather_bytes_per_s`` = what the gathers of that many steps ask
  for (8 index entries of 4 or 8 bytes + 8 realization values of 8 bytes per step; a count of requested bytes, not of
  HBM traffic: neighbouring lanes and steps share cache lines);
* the outputs of all options are compared bit for bit at the sizes timed.

    python tools/bench_atm_observe.py [--ndet 256] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from toast_amd import capi  # noqa: E402
from toast_amd.accel import (accel_data_create, accel_data_delete, accel_data_update_device,  # noqa: E402
                             accel_data_update_host, accel_device_ptr, ensure_assigned)
from toast_amd.atm import ray_steps, standin_slab  # noqa: E402


def dev(arr):
    accel_data_create(arr, "bench_atm")
    accel_data_update_device(arr, "bench_atm")
    return accel_device_ptr(arr)


def run_shape(name, n_det, n_samp, reps):
    rate = 200.0
    t = np.arange(n_samp) / rate
    az_lo, az_hi, el0 = np.radians(40.0), np.radians(110.0), np.radians(50.0)
    pad = np.radians(6.0)
    sim = standin_slab(az_lo - pad, az_hi + pad, el0 - pad, el0 + pad, t[0] - 1.0, t[-1] + 1.0)
    # a one-degree-per-second sweep; detector k is offset inside the padding
    sweep = (az_hi - az_lo) * (0.5 - 0.5 * np.cos(np.pi * t * np.radians(1.0) / (az_hi - az_lo)))
    off = np.linspace(-0.8, 0.8, n_det)[:, None] * pad
    az = np.ascontiguousarray(az_lo + sweep[None, :] + off)
    el = np.ascontiguousarray(np.full((n_det, n_samp), el0) + off[::-1])
    geom = sim.geometry()
    _, n_step = ray_steps(sim._xstep, sim._rmin, sim._rmax, -1.0, sim._elmax, sim._zmax)
    idx64 = sim._compressed_index
    idx32 = np.where((idx64 >= 0) & (idx64 < sim._nelem), idx64, -1).astype(np.int32)
    tod = np.zeros((n_det, n_samp))
    arrays = [t, az, el, tod, idx64, idx32, sim._realization]
    p_t, p_az, p_el, p_tod, p_i64, p_i32, p_re = (dev(a) for a in arrays)
    options = [("int32", True, False), ("int64", False, False), ("int32+cache", True, True), ("int64+cache", False, True)]
    times = {o[0]: [] for o in options}
    outputs = {}

    def launch(index32, cache):
        t0 = time.perf_counter()
        st = capi.dev.atm_observe(geom, p_i32 if index32 else p_i64, index32, p_re, n_det, n_samp, p_t, 0, p_az, p_el,
                                  n_samp, p_tod, n_samp, cell_cache=cache)
        return (time.perf_counter() - t0) * 1e3, st

    for label, index32, cache in options:           # warm-up of every variant; its output is the one compared
        capi.dev.memset(p_tod, 0, tod.nbytes)
        _, status = launch(index32, cache)
        accel_data_update_host(tod, "bench_atm")
        outputs[label] = (tod[:: max(1, n_det // 8), ::97].copy(), status)
    for _ in range(reps):
        for label, index32, cache in options:
            ms, _ = launch(index32, cache)
            times[label].append(ms)
    same = all(np.array_equal(outputs[o[0]][0].view(np.uint64), outputs["int32"][0].view(np.uint64)) and
               outputs[o[0]][1] == outputs["int32"][1] for o in options)
    steps = float(n_det) * n_samp * n_step
    for label, index32, cache in options:
        best, med = min(times[label]), float(np.median(times[label]))
        per_step = 8 * (4 if index32 else 8) + 8 * 8
        print(json.dumps(dict(shape=name, option=label, detectors=n_det, samples=n_samp, steps_per_ray=n_step,
                              volume_cells=int(idx64.size), volume_elements=int(sim._nelem), status=outputs[label][1],
                              ms_best=round(best, 3), ms_median=round(med, 3),
                              ray_steps_per_s=round(steps / best * 1e3, 1),
                              gather_bytes_per_s=round(steps * per_step / best * 1e3, 1),
                              same_bits_as_int32=bool(same), nonzero_fraction=round(float(np.mean(outputs[label][0] != 0)), 4))),
              flush=True)
    for a in arrays:
        accel_data_delete(a, "bench_atm")
    sim.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=256, help="detectors at the workflow's length")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    ensure_assigned()
    if not capi.accel_enabled():
        raise RuntimeError("bench_atm_observe needs a gfx950 device")
    run_shape("workflow", args.ndet, 720000, args.reps)
    run_shape("short", 64, 6000, args.reps)


if __name__ == "__main__":
    main()
