#!/usr/bin/env python3
"""Time the HWPSS model (csrc/hwpss.hip, ops.HWPSynchronousModel's device path) on the GPU, phase by phase, next to the
stream ceiling of the same arrays.

Shapes: 1024 x 720 000 and 256 x 720 000 samples at 200 Hz with a 2 Hz HWP.  Cases: one chunk and 60 s chunks (overlapping,
as ``chunk_time=60`` cuts them); 9 harmonics without and with ``time_drift`` (18 / 36 coefficients).  Signal: an offset,
harmonics 1, 2 and 4 and white noise per detector, made on the device; 1 % of the samples flagged per detector.

Reported, one JSON line per shape and case, all measured in this run:

* ``phase_ms``: gram (toast_hip_hwpss_gram_dev), project (toast_hip_hwpss_project_dev: both sweeps), host solve
  (eigvalsh, lu_factor and one lu_solve per detector and chunk: ops.hwpss_model.solve_chunk), host splrep (one
  scipy.interpolate.splrep per detector and coefficient; chunked cases), subtract (toast_hip_hwpss_subtract_dev with the
  flag update + toast_hip_hwpss_remove_mean_dev).  Device phases: device events, median of ``--reps`` after a first call;
  host phases: wall time, once;
* the stream rate of the probe the other tools use (toast_hip_probe_stream: one read + write pass over the signal), and
  from it the ceilings of a 9-byte stream per detector-sample (signal + flag byte: one sweep of the projection) and of a
  17-byte stream (signal read and written + flag byte: the subtraction).  The projection sweeps twice (mean, then
  right-hand side): ``project_vs_18B`` is the 18-byte ceiling's ms over the measured ms.  The subtract phase is the 17-byte
  sweep plus the 16-byte removal of the mean: ``subtract_vs_33B`` likewise.  The bytes are counted from the algorithm,
  not measured.

    python tools/bench_hwpss.py [--ndet 1024 256] [--minutes 60] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE = 200.0
HWP_HZ = 2.0


def chunking(n_samp, chunk_time):
    """(starts, ends, times) as ops.HWPSynchronousModel._compute_chunking cuts them."""
    reltime_end = (n_samp - 1) / RATE
    if chunk_time is None:
        return np.array([0]), np.array([n_samp]), np.array([(n_samp // 2) / RATE])
    non_overlap = int(reltime_end / chunk_time)
    chunk_samples = int(reltime_end / non_overlap * RATE + 0.5)
    half = chunk_samples // 2
    starts, ends, times = [], [], []
    for ch in range(non_overlap):
        a = ch * chunk_samples
        starts.append(a), ends.append(a + chunk_samples), times.append((a + half) / RATE)
        if ch != non_overlap - 1:
            starts.append(a + half), ends.append(a + half + chunk_samples), times.append((a + chunk_samples) / RATE)
    return np.array(starts), np.array(ends), np.array(times)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, nargs="+", default=[1024, 256])
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-time", type=float, default=60.0)
    args = ap.parse_args(argv)
    import scipy.interpolate
    import torch

    from toast_amd import accel, capi
    from toast_amd.ops import hwpss_model as HM

    assert accel.accel_enabled(), "no HIP device visible"
    accel.accel_assign_device(1, 0, 1.0, False)
    D = capi.dev
    n_samp = int(args.minutes * 60 * RATE)
    t = torch.arange(n_samp, dtype=torch.float64, device="cuda") / RATE
    angle = torch.remainder(2 * np.pi * HWP_HZ * t, 2 * np.pi)
    shared = torch.zeros(n_samp, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

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

    for n_det in args.ndet:
        signal = torch.randn((n_det, n_samp), dtype=torch.float64, device="cuda", generator=gen)
        for d0 in range(0, n_det, 64):          # in slices: no second array of the full size
            rows = slice(d0, min(d0 + 64, n_det))
            k = rows.stop - rows.start
            amp = 1.0 + 0.03 * torch.randn((k, 1), dtype=torch.float64, device="cuda", generator=gen)
            signal[rows] += 10.0 * torch.randn((k, 1), dtype=torch.float64, device="cuda", generator=gen)
            for h, a in ((1, 40.0), (2, 100.0), (4, 25.0)):
                signal[rows] += a * amp * torch.sin(h * angle[None, :] + 0.1 * h)
        flags = (torch.rand((n_det, n_samp), device="cuda", generator=gen) < 0.01).to(torch.uint8)
        rows = np.arange(n_det, dtype=np.int32)
        probe_ms = capi.probe_stream(signal.data_ptr(), signal.numel() * 8)
        probe_ms = min(probe_ms, capi.probe_stream(signal.data_ptr(), signal.numel() * 8))
        rate = 2 * signal.numel() * 8 / probe_ms          # bytes per ms
        for chunk_time in (None, args.chunk_time):
            starts, ends, ch_times = chunking(n_samp, chunk_time)
            n_chunk = len(starts)
            for drift in (False, True):
                harmonics = 9
                n_coeff = HM.n_coefficients(harmonics, drift)
                common = (n_samp, harmonics, drift, angle.data_ptr(), t.data_ptr(), shared.data_ptr())
                gram = torch.zeros((n_chunk, n_coeff, n_coeff), dtype=torch.float64, device="cuda")
                ngs = torch.zeros(n_chunk, dtype=torch.int64, device="cuda")
                ng = torch.zeros((n_det, n_chunk), dtype=torch.int64, device="cuda")
                mean = torch.zeros((n_det, n_chunk), dtype=torch.float64, device="cuda")
                rhs = torch.zeros((n_det, n_chunk, n_coeff), dtype=torch.float64, device="cuda")
                phases = {}
                phases["gram"] = timed(lambda: D.hwpss_gram(*common, starts, ends, gram.data_ptr(), ngs.data_ptr()))
                phases["project"] = timed(lambda: D.hwpss_project(
                    *common, rows, signal.data_ptr(), rows, flags.data_ptr(), 1, starts, ends, ng.data_ptr(), mean.data_ptr(),
                    rhs.data_ptr()))
                h_gram, h_ngs, h_rhs, h_ng = gram.cpu().numpy(), ngs.cpu().numpy(), rhs.cpu().numpy(), ng.cpu().numpy()
                t0 = time.perf_counter()
                coeff = np.zeros((n_det, n_coeff, n_chunk))
                flagged = 0
                for c in range(n_chunk):
                    sol = HM.solve_chunk(h_gram[c], h_ngs[c], min(ends[c], n_samp) - starts[c], h_rhs[:, c], h_ng[:, c], n_coeff)
                    if sol is None:
                        flagged += 1
                    else:
                        coeff[:, :, c] = sol
                phases["host_solve"] = 1e3 * (time.perf_counter() - t0)
                sums = torch.zeros(n_det, dtype=torch.float64, device="cuda")
                counts = torch.zeros(n_det, dtype=torch.int64, device="cuda")
                active = np.ones(n_det, dtype=np.int32)
                work = signal.clone()                 # every case fits the same signal
                wflags = flags.clone()
                if n_chunk == 1:
                    phases["host_splrep"] = 0.0
                    d_coeff = torch.from_numpy(np.ascontiguousarray(coeff[:, :, 0])).cuda()
                    kw = dict(d_coeff=d_coeff.data_ptr())
                else:
                    good = np.array([bool(np.any(coeff[0, :, c])) for c in range(n_chunk)])
                    if np.count_nonzero(good) < 4:
                        print(json.dumps({"bench": "hwpss", "n_det": n_det, "n_chunk": n_chunk, "time_drift": drift,
                                          "chunks_flagged": flagged, "skipped": "fewer than four good chunks"}), flush=True)
                        continue
                    t0 = time.perf_counter()
                    splines = [[scipy.interpolate.splrep(ch_times[good], coeff[d, k, good], s=max(n_chunk // 16, 4))
                                for k in range(n_coeff)] for d in range(n_det)]
                    phases["host_splrep"] = 1e3 * (time.perf_counter() - t0)
                    offsets, st, sc = HM.pack_splines(splines, n_coeff)
                    d_st, d_sc = torch.from_numpy(st).cuda(), torch.from_numpy(sc).cuda()
                    kw = dict(spl_offset=offsets, d_spl_t=d_st.data_ptr(), d_spl_c=d_sc.data_ptr())

                def subtract():
                    D.hwpss_subtract(*common, rows, work.data_ptr(), rows, wflags.data_ptr(), 1, 1, active, True,
                                     sums.data_ptr(), counts.data_ptr(), **kw)
                    D.hwpss_remove_mean(n_samp, shared.data_ptr(), rows, work.data_ptr(), rows, wflags.data_ptr(), 1, active,
                                        sums.data_ptr(), counts.data_ptr())

                phases["subtract"] = timed(subtract)
                samples = float(np.sum(np.minimum(ends, n_samp) - starts))
                ceil_project = 18 * n_det * samples / rate
                ceil_subtract = 17 * n_det * n_samp / rate
                ceil_remove = 16 * n_det * n_samp / rate
                out = {"bench": "hwpss", "n_det": n_det, "n_samp": n_samp, "n_chunk": n_chunk, "chunks_flagged": flagged,
                       "harmonics": harmonics, "time_drift": drift, "n_coeff": n_coeff,
                       "phase_ms": {k: round(v, 3) for k, v in phases.items()},
                       "probe_stream_tb_s": round(rate / 1e9, 3),
                       "ceiling_9B_ms": round(9 * n_det * samples / rate, 3),
                       "ceiling_17B_ms": round(ceil_subtract, 3),
                       "project_ceiling_18B_ms": round(ceil_project, 3),
                       "project_vs_18B": round(ceil_project / phases["project"], 3),
                       "subtract_ceiling_33B_ms": round(ceil_subtract + ceil_remove, 3),
                       "subtract_vs_33B": round((ceil_subtract + ceil_remove) / phases["subtract"], 3),
                       "note": "project = two 9 B sweeps over the chunks' samples (18 B); subtract = the 17 B sweep + the "
                               "16 B mean removal (33 B); each ratio is that ceiling's ms over the measured ms"}
                print(json.dumps(out), flush=True)
                del work, wflags
        del signal, flags
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
