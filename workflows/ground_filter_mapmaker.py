#!/usr/bin/env python3
"""The structure of BASELINE configs[4] on one GPU's share of the detectors: constant-elevation
scans (sweeps as intervals, flagged turnarounds), a ground-synchronous signal injected into the
timestreams, `GroundFilter` (ground-template subtraction), then `MapMaker` at Nside 2048 with
baseline offsets, everything through the reference's Operator names.  `--atmosphere` observes one or
two STAND-IN atmosphere slabs into the signal with `ObserveAtmosphere` before the filters; generating
the atmosphere as configs[4] does (GenerateAtmosphere, CHOLMOD) is not part of this path.

    python workflows/ground_filter_mapmaker.py [--ndet 256] [--minutes 60] [--rate 200] [--nside 2048]
                                               [--iter 10] [--split] [--filter-order 5] [--trend-order 5]
                                               [--polyfilter ORDER] [--polyfilter2d ORDER [--polyfilter2d-key COLUMN]]
                                               [--common-mode] [--save-map FILE]
                                               [--subharmonic ORDER] [--periodic-az BINS] [--fourier2d ORDER]
                                               [--time-constant MS [--time-constant-sigma S]]
                                               [--atmosphere {1,2}]
                                               [--filterbin [--hwp-filter-order N] [--ground-filter-order N]
                                                            [--poly-filter-order N]]

`--filterbin` replaces the separate filters and MapMaker by `FilterBin`: HWP-synchronous harmonics, ground polynomials and
per-subscan polynomials regressed in one fit per detector, then the binned map.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from toast_amd import ops  # noqa: E402
from toast_amd.accel import native  # noqa: E402
from toast_amd.data import defaults  # noqa: E402
from toast_amd.sim import create_ground_data  # noqa: E402
from toast_amd.templates import Fourier2D, Offset, Periodic, SubHarmonic  # noqa: E402


def observe_standin_atmosphere(data, n_slab):
    """Detector az / el quaternions from the boresight's azimuth and elevation (PointingDetectorSimple on the device),
    ``n_slab`` stand-in slabs along the line of sight (toast_amd.atm.standin_slab) for one wind interval that spans the
    observation, then ObserveAtmosphere into the signal."""
    from toast_amd.atm import azel_to_quat, standin_slab

    edges = np.linspace(0.0, 2000.0, n_slab + 1)
    sims = {}
    for ob in data.obs:
        az, el = ob.shared[defaults.azimuth].data, ob.shared[defaults.elevation].data
        times = ob.shared[defaults.times].data
        ob.shared.create(defaults.boresight_azel, azel_to_quat(az, el))
        ob.intervals.create("wind", [(0, ob.n_local_samples)])
        half = 0.55 * ob.telescope.focalplane.field_of_view
        el_lo, el_hi = max(float(el.min()) - half, 0.0), min(float(el.max()) + half, np.pi / 2)
        az_pad = half / np.cos(el_hi) + 0.01
        sims[ob.session.name] = [[
            standin_slab(float(az.min()) - az_pad, float(az.max()) + az_pad, el_lo, el_hi, float(times[0]) - 1.0,
                         float(times[-1]) + 1.0, rmin=edges[k], rmax=edges[k + 1], seed=100 + k)
            for k in range(n_slab)]]
        ob["atm_absorption"] = {d: 1.0 for d in ob.local_detectors}
    data["atm_sim"] = sims
    ops.PointingDetectorSimple(boresight=defaults.boresight_azel, quats=defaults.quats_azel, hwp_angle=None,
                               shared_flags=None, name="pointing_azel").apply(data, use_accel=True)
    ops.ObserveAtmosphere(absorption="atm_absorption", name="observe_atmosphere").apply(data, use_accel=True)
    for slabs in sims.values():
        for sim in slabs[0]:
            sim.close()
    for ob in data.obs:
        del ob.detdata[defaults.quats_azel]
        if ob.shared[defaults.boresight_azel].accel_exists():
            ob.shared[defaults.boresight_azel].accel_delete()
        del ob.shared[defaults.boresight_azel]


def filter_and_bin(data, args, lap, rms_before):
    """--filterbin: ops.FilterBin instead of the separate filters and MapMaker.  The polynomial view is the list of single
    throws (the `throw` list of SimGround is the union of both directions: one interval); observations of the synthetic
    generator get their scan range from the azimuth and, with --hwp-filter-order, a 2 Hz HWP angle."""
    from toast_amd.data import IntervalList

    for o in data.obs:
        single = sorted((int(iv.first), int(iv.last)) for name in (defaults.throw_leftright_interval,
                                                                    defaults.throw_rightleft_interval)
                        for iv in o.intervals[name])
        o.intervals["subscans"] = IntervalList(o.shared[defaults.times].data, samplespans=single)
        if "scan_min_az" not in o:
            az = o.shared[defaults.azimuth].data
            o["scan_min_az"], o["scan_max_az"] = float(az.min()), float(az.max())
        if args.hwp_filter_order is not None and not np.any(o.shared[defaults.hwp_angle].data):
            times = o.shared[defaults.times].data
            o.shared[defaults.hwp_angle].data[:] = 2 * np.pi * (((times - times[0]) * 2.0) % 1.0)
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=args.nside, nest=True, view=defaults.scanning_interval)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU", view=defaults.scanning_interval)
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=weights)
    fb = ops.FilterBin(name="filterbin", binning=binner, hwp_filter_order=args.hwp_filter_order,
                       ground_filter_order=args.ground_filter_order, split_ground_template=args.split,
                       poly_filter_order=args.poly_filter_order, poly_filter_view="subscans", keep_final_products=True,
                       report_timing=True)
    fb.apply(data)
    lap("FilterBin (regression + cov + bin)")
    ob = data.obs[0]
    good = (ob.shared[defaults.shared_flags].data & fb.shared_flag_mask) == 0
    good &= (ob.detdata[defaults.det_flags].data[0] & fb.det_flag_mask) == 0
    rms_after = float(np.std(ob.detdata[defaults.det_data].data[0][good]))
    routes = [r for per_obs in fb.routes.values() for r in per_obs.values()]
    fitted = [a for per_obs in fb.amplitudes.values() for a in per_obs.values() if a is not None]
    print(f"detectors {args.ndet}  samples/det {ob.n_local_samples}  subscans {len(ob.intervals['subscans'])}  nside "
          f"{args.nside}  templates {len(fitted[0]) if fitted else 0}  routes inv {routes.count(0)} pinv {routes.count(1)} "
          f"rejected {routes.count(2)} not fitted {routes.count(3)}")
    print(f"ground signal: rms of detector 0 over good samples {rms_before:.2f} -> {rms_after:.3f} (white noise rms 1)")
    print("FilterBin phases [ms]: " + "  ".join(f"{k} {1e3 * v:.1f}" for k, v in fb.seconds.items()))
    fmap = np.asarray(data["filterbin_filtered_map"].data)
    hit = np.asarray(data["filterbin_filtered_hits"].data).reshape(-1) > 0
    print(f"hit pixels {int(np.count_nonzero(hit))}  rms of the filtered map (I, hit pixels) "
          f"{float(np.std(fmap.reshape(hit.size, -1)[hit, 0])):.4f}")
    if args.save_map is not None:
        np.save(args.save_map, fmap)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=256)
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--rate", type=float, default=200.0)
    ap.add_argument("--nside", type=int, default=2048)
    ap.add_argument("--iter", type=int, default=10)
    ap.add_argument("--step-time", type=float, default=1.0)
    ap.add_argument("--trend-order", type=int, default=5)
    ap.add_argument("--filter-order", type=int, default=5)
    ap.add_argument("--split", action="store_true", help="separate templates for left- and right-going sweeps")
    ap.add_argument("--scheduled", type=int, default=0, metavar="N",
                    help="build the observations with ops.SimGround from a schedule of N constant-elevation scans of "
                         "--minutes each (finite-acceleration turnarounds, one observation per scan) instead of "
                         "the synthetic single-observation generator")
    ap.add_argument("--elnods", action="store_true",
                    help="with --scheduled: an el-nod (+1, -1, 0 degrees) before and after every scan and elevation steps of "
                         "0.05 degrees after every scan pair (ops.SimGround elnod_start / elnod_end / el_mod_step); the "
                         "el-nod samples carry the `irregular` flag bit and stay out of the maps")
    ap.add_argument("--polyfilter", type=int, default=None, metavar="ORDER",
                    help="run ops.PolyFilter(order=ORDER, view='throw') before GroundFilter (off by default)")
    ap.add_argument("--polyfilter2d", type=int, default=None, metavar="ORDER",
                    help="run ops.PolyFilter2D(order=ORDER) -- a 2-D polynomial across the focal plane at every time stamp -- "
                         "before CommonModeFilter and GroundFilter (off by default)")
    ap.add_argument("--polyfilter2d-key", default=None, metavar="COLUMN",
                    help="with --polyfilter2d: fit one polynomial per value of this focalplane column (focalplane_key)")
    ap.add_argument("--common-mode", action="store_true", help="run ops.CommonModeFilter() before GroundFilter (off by default)")
    ap.add_argument("--subharmonic", type=int, default=None, metavar="ORDER",
                    help="solve for Legendre polynomials up to ORDER per detector and sweep next to the baselines "
                         "(templates.SubHarmonic; off by default)")
    ap.add_argument("--periodic-az", type=int, default=None, metavar="BINS",
                    help="solve for a ground template of BINS azimuth bins per detector and observation next to the "
                         "baselines (templates.Periodic, key = azimuth; off by default)")
    ap.add_argument("--fourier2d", type=int, default=None, metavar="ORDER",
                    help="solve for 2-D Fourier modes up to ORDER across the focal plane, shared by all detectors, with a "
                         "correlation prior in time, next to the baselines (templates.Fourier2D; off by default)")
    ap.add_argument("--sim-noise", action="store_true",
                    help="draw the detector noise on the device with ops.SimNoise from the observation's AnalyticNoise "
                         "instead of host white noise (off by default)")
    ap.add_argument("--time-constant", type=float, default=None, metavar="MS",
                    help="give every detector a single-pole time constant around MS milliseconds (focalplane column `tau`), "
                         "convolve the simulated signal with it (ops.TimeConstant) and deconvolve it again with "
                         "ops.TimeConstant(deconvolve=True) before the filters; prints the residual (off by default)")
    ap.add_argument("--time-constant-sigma", type=float, default=0.0, metavar="S",
                    help="with --time-constant: relative Gaussian spread of the time constants across the focal plane")
    ap.add_argument("--atmosphere", type=int, default=0, choices=(0, 1, 2), metavar="SLABS",
                    help="observe SLABS (1 or 2) atmosphere slabs into the signal with ops.ObserveAtmosphere before the "
                         "filters.  The slabs are a STAND-IN, not the reference's generator: a box around the scan cone, "
                         "cells kept by a cone predicate, a smooth random field from a filtered FFT (off by default)")
    ap.add_argument("--filterbin", action="store_true",
                    help="replace the separate filters and the MapMaker call by ops.FilterBin: one joint regression of "
                         "HWP-synchronous harmonics, ground polynomials (split with --split) and per-subscan polynomials, "
                         "then the binned map; prints the rms of the filtered map and the phase times")
    ap.add_argument("--hwp-filter-order", type=int, default=None, metavar="ORDER", help="with --filterbin: hwp_filter_order")
    ap.add_argument("--ground-filter-order", type=int, default=5, metavar="ORDER",
                    help="with --filterbin: ground_filter_order")
    ap.add_argument("--poly-filter-order", type=int, default=1, metavar="ORDER", help="with --filterbin: poly_filter_order")
    ap.add_argument("--save-map", default=None, metavar="FILE", help="save the binned map as a .npy file")
    args = ap.parse_args(argv)
    n_samp = int(args.minutes * 60 * args.rate)
    t = time.time()

    def lap(name):
        nonlocal t
        native().accel_synchronize()
        now = time.time()
        print(f"  {name:40s} {now - t:8.2f} s", flush=True)
        t = now

    if args.scheduled > 0:
        from toast_amd.ops.sim_ground import create_ground_data_from_schedule
        from toast_amd.schedule import make_ces_schedule

        schedule = make_ces_schedule(args.scheduled, scan_seconds=args.minutes * 60.0, az_min=40.0, az_max=110.0, el=50.0)
        el_motion = dict(elnod_start=True, elnod_end=True, elnods=[1.0, -1.0, 0.0], scan_rate_el=1.0, scan_accel_el=1.0,
                         el_mod_step=0.05) if args.elnods else {}
        if args.filterbin and args.hwp_filter_order is not None:
            el_motion.update(hwp_angle=defaults.hwp_angle, hwp_rpm=120.0)
        data = create_ground_data_from_schedule(schedule, n_det=args.ndet, rate=args.rate, fov_deg=8.0,
                                                scan_rate_az=1.0, scan_accel_az=1.0, fix_rate_on_sky=False, **el_motion)
        for ob in data.obs:     # the map-maker skips samples with any non-science bit: raise "invalid" too
            ob.shared[defaults.shared_flags].data[ob.shared[defaults.shared_flags].data != 0] |= defaults.shared_mask_invalid
    else:
        data = create_ground_data(n_det=args.ndet, n_samp=n_samp, rate=args.rate, az_min_deg=40.0, az_max_deg=110.0,
                                  scan_rate_deg_s=1.0, fov_deg=8.0)
    data.lazy_host = True
    rng = np.random.default_rng(1)
    for ob in data.obs:
        az = ob.shared[defaults.azimuth].data
        phase = (az - az.min()) / (az.max() - az.min()) * 2 - 1
        ground = 20.0 * (np.sin(3 * phase) + 0.5 * phase ** 2)
        sig = ob.detdata[defaults.det_data].data
        for d in range(sig.shape[0]):
            white = 0.0 if args.sim_noise else rng.standard_normal(sig.shape[1])
            sig[d] = white + ground * (1.0 + 0.1 * rng.standard_normal())
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data].data
    n_samp = ob.n_local_samples
    lap("simulate (host)")
    if args.sim_noise:
        ops.SimNoise(noise_model=defaults.noise_model).apply(data, use_accel=True)
        lap("SimNoise")
        sig = ob.detdata[defaults.det_data].data
    if args.atmosphere:
        observe_standin_atmosphere(data, args.atmosphere)
        lap(f"ObserveAtmosphere ({args.atmosphere} stand-in slab{'s' * (args.atmosphere > 1)}; upload)")
        sig = ob.detdata[defaults.det_data].data
        print(f"atmosphere: rms of detector 0 after observing {float(np.std(sig[0])):.2f}")
    if args.time_constant is not None:
        n_keep = min(8, sig.shape[0])
        untouched = np.array(sig[:n_keep])
        tau_rng = np.random.default_rng(2)
        for o in data.obs:
            fp = o.telescope.focalplane
            for d in fp.detectors:
                fp[d]["tau"] = 1.0e-3 * args.time_constant * (1.0 + args.time_constant_sigma * tau_rng.standard_normal())
        # the detectors' response: no flags are involved in making the signal
        ops.TimeConstant(tau_name="tau", det_flags=None, name="timeconstant_sim").apply(data)
        lap("TimeConstant (convolve; first call: upload)")
        ops.TimeConstant(tau_name="tau", deconvolve=True, name="timeconstant").apply(data)
        lap("TimeConstant (deconvolve)")
        sig = ob.detdata[defaults.det_data].data
        dflags = ob.detdata[defaults.det_flags].data
        diffs = []
        for d in range(n_keep):
            ok = (dflags[d] & defaults.det_mask_invalid) == 0
            diffs.append((sig[d] - untouched[d])[ok])
        # both calls remove the mean of the padded series: the difference is an offset per detector plus the residual
        offsets = [float(np.mean(x)) for x in diffs]
        resid = float(np.sqrt(np.mean(np.concatenate([x - m for x, m in zip(diffs, offsets)]) ** 2)))
        taus = [ob.telescope.focalplane[d]["tau"] for d in ob.local_detectors]
        print(f"time constants {1e3 * min(taus):.3f} .. {1e3 * max(taus):.3f} ms: convolved and deconvolved, rms residual "
              f"against the untouched signal {resid:.3e} (first {n_keep} detectors, unflagged samples, mean offset "
              f"{np.mean(offsets):.3f} removed; signal rms {float(np.std(untouched)):.2f})")
        del untouched, diffs
    good = (ob.shared[defaults.shared_flags].data & 1) == 0
    rms_before = float(np.std(sig[0][good]))
    if args.filterbin:
        filter_and_bin(data, args, lap, rms_before)
        return data
    if args.polyfilter is not None:
        for o in data.obs:
            if "throw" not in o.intervals:      # the synthetic generator names the sweeps `scanning` only
                o.intervals.create("throw", [(int(iv.first), int(iv.last)) for iv in o.intervals[defaults.scanning_interval]])
        ops.PolyFilter(order=args.polyfilter, view="throw", name="polyfilter").apply(data)
        lap("PolyFilter")
    if args.polyfilter2d is not None:
        ops.PolyFilter2D(order=args.polyfilter2d, focalplane_key=args.polyfilter2d_key, name="polyfilter2d").apply(data)
        lap("PolyFilter2D")
    if args.common_mode:
        ops.CommonModeFilter(name="commonmode").apply(data)
        lap("CommonModeFilter")
    gf = ops.GroundFilter(trend_order=args.trend_order, filter_order=args.filter_order, split_template=args.split,
                          name="groundfilter")
    gf.apply(data)
    lap("GroundFilter (first call: upload + JIT)")
    rms_after = float(np.std(ob.detdata[defaults.det_data].data[0][good]))
    t = time.time()
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=args.nside, nest=True,
                               view=defaults.scanning_interval)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU", view=defaults.scanning_interval)
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=weights, full_pointing=True)
    templates = [Offset(step_time=args.step_time, noise_model=defaults.noise_model, name="baselines")]
    if args.subharmonic is not None:
        templates.append(SubHarmonic(order=args.subharmonic, noise_model=defaults.noise_model, name="subharmonic"))
    if args.periodic_az is not None:
        templates.append(Periodic(key=defaults.azimuth, bins=args.periodic_az, name="ground"))
    if args.fourier2d is not None:
        templates.append(Fourier2D(order=args.fourier2d, noise_model=defaults.noise_model, name="fourier2d"))
    tmatrix = ops.TemplateMatrix(templates=templates, view=defaults.scanning_interval)
    mapper = ops.MapMaker(name="mapmaker", det_data=defaults.det_data, binning=binner, template_matrix=tmatrix,
                          iter_min=args.iter, iter_max=args.iter, convergence=1e-30, keep_solver_products=True)
    mapper.apply(data)
    lap("MapMaker (cov + RHS + PCG + bin)")
    nds = args.ndet * sum(o.n_local_samples for o in data.obs)
    n_views = len(ob.intervals[defaults.scanning_interval])
    print(f"detectors {args.ndet}  samples/det {n_samp}  sweeps {n_views}  nside {args.nside}  templates "
          f"{len(next(iter(gf.coefficients.values())))}  rcond mean {gf.rcondsum / max(gf.ngood + gf.nsingular, 1):.2e}")
    print(f"ground signal: rms of detector 0 over good samples {rms_before:.2f} -> {rms_after:.3f} (white noise rms 1)")
    its = getattr(mapper, "iteration_seconds", None)
    if its:
        med = float(np.median(its))
        print(f"PCG iteration (median wall time): {1e3 * med:.1f} ms  = {nds / med / 1e9:.1f} G det-samples/s")
    hits = data["mapmaker_hits"]
    print(f"hit pixels {int(np.count_nonzero(hits.data))}  relative residual {mapper.history[-1]:.2e}")
    if args.save_map is not None:
        np.save(args.save_map, np.asarray(data["mapmaker_map"].data))
    return data


if __name__ == "__main__":
    main()
