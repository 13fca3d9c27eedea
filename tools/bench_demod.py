#!/usr/bin/env python3
"""Time HWP demodulation (csrc/demod.hip, ops.Demodulate): one JSON line per shape.

* cfg-3 length (720 000 samples at 200 Hz with a 2 Hz HWP: 2047 / 511 taps; ``--ndet`` detectors are run and the
  kernel time is also scaled to 1024) and a short-observation shape (6000 samples at 100 Hz: 1023 / 255 taps);
* phases: Stokes weights (here an upload of ready weights stands in for the pointing operator), band-pass and
  low-pass (``toast_hip_demod_timing``: plain FIR = demod0 + band-pass, modulated FIR = the Q / U low-pass), flags, and
  the host bookkeeping (everything of the operator's wall time that is not one of those);
* FMA/s of the FIR kernel next to the FMA/s of a register-only FP64 FMA loop in the same launch shape (256 lanes, 8
  accumulators per lane: ``toast_hip_noise_estim_fma_ceiling``), the ceiling this tool measures itself;
* the host path (``fftconvolve``) on one detector.

    python tools/bench_demod.py [--ndet 16] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from toast_amd import capi, ops  # noqa: E402
from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults  # noqa: E402
from toast_amd.traits import Unicode  # noqa: E402


class ReadyWeights(ops.Operator):
    """Hands out precomputed Stokes weights (the pointing operators are timed elsewhere)."""

    weights = Unicode("weights", help="Observation detdata key for output weights")
    view = Unicode(None, allow_none=True, help="unused")
    mode = Unicode("IQU", help="The Stokes weights to generate")
    hwp_angle = Unicode("hwp_angle", allow_none=True, help="Observation shared key for HWP angle")
    seconds = 0.0

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        t0 = time.perf_counter()
        for ob in data.obs:
            dets = ob.select_local_detectors(detectors)
            ob.detdata.ensure(self.weights, sample_shape=(3,), dtype=np.float64, detectors=dets)
            wd = ob.detdata[self.weights]
            ang = 4 * ob.shared[self.hwp_angle].data
            for i, d in enumerate(dets):
                wd[d] = np.stack([np.ones_like(ang), 0.9 * np.cos(ang + i), 0.9 * np.sin(ang + i)], axis=1)
            if use_accel:
                if not wd.accel_exists():
                    wd.accel_create(self.weights)
                wd.accel_update_device()
                capi.synchronize()
        type(self).seconds += time.perf_counter() - t0

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        return {}

    def _provides(self):
        return {"detdata": [self.weights]}


def make(n_det, n, rate, hwp_hz):
    dets = [f"D{i:04d}" for i in range(n_det)]
    fp = Focalplane(dets, np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n_det, 1)), sample_rate=rate)
    ob = Observation(None, Telescope("bench", fp), n, name="bench")
    t = np.arange(n) / rate
    ob.set_times(t)
    ob.shared.create(defaults.hwp_angle, np.mod(2 * np.pi * hwp_hz * t, 2 * np.pi))
    ob.shared.create(defaults.shared_flags, np.zeros(n, dtype=np.uint8))
    ob.detdata.create(defaults.det_data, dtype=np.float64, units="K")
    ob.detdata.create(defaults.det_flags, dtype=np.uint8)
    ob.detdata[defaults.det_data].data[:] = 100.0 + np.random.default_rng(2).standard_normal((n_det, n))
    data = Data()
    data.obs.append(ob)
    return data


def run_shape(name, n_det, n, rate, hwp_hz, host):
    def once(use_accel):
        data = make(n_det if use_accel else 1, n, rate, hwp_hz)
        if use_accel:
            for key in (defaults.det_data, defaults.det_flags):
                data.obs[0].detdata[key].accel_create(key)
                data.obs[0].detdata[key].accel_update_device()
            capi.synchronize()
        ReadyWeights.seconds = 0.0
        op = ops.Demodulate(stokes_weights=ReadyWeights(), noise_model=None)
        t0 = time.perf_counter()
        out = op.apply(data, use_accel=use_accel)
        if use_accel:
            capi.synchronize()
        wall = time.perf_counter() - t0
        taps = (int(2 ** np.ceil(np.log2(rate / (0.95 * hwp_hz) * 10))) - 1, int(2 ** np.ceil(np.log2(rate / (3.05 * hwp_hz) * 10))) - 1)
        del out
        return wall, ReadyWeights.seconds, taps

    once(True)                                    # warm-up: arena, parameter blocks
    capi.dev.demod_timing(True)
    wall, weights_s, (w_lp, w_bp) = once(True)
    plain, modulated, flags, _ = capi.dev.demod_timing(False)
    n_out = len(range(0, n, 3))
    fma = float(n_det) * (n_out * w_lp + n * w_bp + 2 * n_out * w_lp)          # demod0, band-pass, Q and U
    # long enough to be a ceiling whatever the shape: at least 65 536 workgroups of 8 x 4096 FMAs per lane
    n_iter = 4096
    n_block = max(65536, int(fma / (256 * 8 * n_iter)))
    ceiling_ms = capi.dev.noise_estim_fma_ceiling(n_block, n_iter)
    kernel_ms = plain + modulated
    out = dict(shape=name, detectors=n_det, samples=n, taps_lowpass=w_lp, taps_bandpass=w_bp, wall_s=round(wall, 4),
               weights_ms=round(weights_s * 1e3, 3), plain_fir_ms=round(plain, 3), modulated_fir_ms=round(modulated, 3),
               flags_ms=round(flags, 3), host_bookkeeping_ms=round(wall * 1e3 - weights_s * 1e3 - kernel_ms - flags, 3),
               fir_gfma_per_s=round(fma / kernel_ms / 1e6, 1) if kernel_ms else None,
               ceiling_gfma_per_s=round(n_block * 256 * 8 * n_iter / ceiling_ms / 1e6, 1),
               fir_ms_scaled_to_1024_detectors=round(kernel_ms * 1024 / n_det, 1))
    if host:
        wall_h, weights_h, _ = once(False)
        out["host_one_detector_s"] = round(wall_h - weights_h, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=16, help="detectors run at cfg-3 length (1024 in the configuration)")
    ap.add_argument("--no-host", action="store_true", help="leave out the host path on one detector")
    args = ap.parse_args()
    run_shape("cfg-3", args.ndet, 720000, 200.0, 2.0, not args.no_host)
    run_shape("short", max(args.ndet, 64), 6000, 100.0, 2.0, not args.no_host)


if __name__ == "__main__":
    main()
