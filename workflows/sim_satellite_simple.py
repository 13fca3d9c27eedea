#!/usr/bin/env python3
"""Simulated satellite scan -> binned map, with the reference's operator names.

Counterpart of the reference's ``workflows/toast_sim_satellite_simple.py`` restated with its
current API (PixelsHealpix + StokesWeights + BinMap) -- BASELINE.json
configs[0] (4 detectors x 10 min @ 100 Hz, Nside 64) by default, configs[1] with
``--ndet 64 --minutes 60 --nside 512``.  Everything numerical runs on the MI355X.

    python workflows/sim_satellite_simple.py [--ndet 4] [--minutes 10] [--rate 100] [--nside 64]
                                             [--destripe] [--sim-noise] [--estimate-noise] [--out map.npz]
                                             [--demodulate [--nskip N] [--hwp-rpm R]]

``--demodulate``: the HWP spins at ``--hwp-rpm`` (default 120, i.e. 2 Hz), a piecewise-constant input sky is scanned into
the signal, and after the usual (modulated) map the data goes through Demodulate -> StokesWeightsDemod -> the same
binning / ``--destripe`` map-maker; the residual of both maps against the input sky is printed.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from toast_amd import ops  # noqa: E402
from toast_amd.data import defaults  # noqa: E402
from toast_amd.sim import create_satellite_data  # noqa: E402
from toast_amd.templates import Offset  # noqa: E402


def input_sky(nside):
    """[12 nside^2][I, Q, U], NESTED: constant over the pixels of Nside 4, so that it varies slowly along the scan."""
    npix = 12 * nside * nside
    coarse = np.arange(npix) // max(1, (nside // 4) ** 2)
    return np.stack([1.0 + 0.1 * np.sin(0.7 * coarse), 0.05 * np.cos(0.4 * coarse), 0.03 * np.sin(0.9 * coarse + 1.0)], axis=1)


def scan_input_sky(data, nside):
    """Add the input sky to the signal through the pointing the map-maker will use; returns the sky."""
    from toast_amd.accel import ensure_assigned

    ensure_assigned()                   # the host-level pointing calls below are staged through the device
    sky = input_sky(nside)
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=nside, nest=True)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU", hwp_angle=defaults.hwp_angle)
    pixels.apply(data)
    weights.apply(data)
    for ob in data.obs:
        pix, w = ob.detdata[pixels.pixels].data, ob.detdata[weights.weights].data
        seen = pix >= 0
        ob.detdata[defaults.det_data].data[seen] += np.sum(w[seen] * sky[pix[seen]], axis=1)
    ops.Delete(detdata=[pixels.pixels, weights.weights, det_pointing.quats]).apply(data)
    return sky


def residual(m, good, sky, dist):
    """rms of map - input sky over the solved pixels; the map holds the local submaps of ``dist``."""
    n_sub = m.shape[1]
    pix = (np.asarray(dist.local_submaps)[:, None] * n_sub + np.arange(n_sub)[None, :]).reshape(-1)
    flat = m.reshape(-1, m.shape[-1])
    ok = good.reshape(-1) & np.any(flat != 0, axis=1) & (pix < sky.shape[0])
    return "map - input sky rms  I %.4g  Q %.4g  U %.4g  over %d pixels" % (
        *np.sqrt(np.mean((flat[ok] - sky[pix[ok]]) ** 2, axis=0)), int(np.count_nonzero(ok)))


def demodulate_and_map(data, args, sky):
    """Demodulate -> StokesWeightsDemod -> the same map-maker on the pseudo-detectors."""
    from toast_amd.accel import accel_enabled

    t0 = time.time()
    weights = ops.StokesWeights(detector_pointing=ops.PointingDetectorSimple(), mode="IQU", hwp_angle=defaults.hwp_angle)
    demod = ops.Demodulate(stokes_weights=weights, nskip=args.nskip)
    demod_data = demod.apply(data, use_accel=accel_enabled())
    pixels = ops.PixelsHealpix(detector_pointing=ops.PointingDetectorSimple(), nside=args.nside, nest=True)
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=ops.StokesWeightsDemod(mode="IQU"),
                        full_pointing=args.full_pointing)
    templates = None
    if args.destripe:
        templates = ops.TemplateMatrix(templates=[Offset(step_time=60.0, noise_model=defaults.noise_model,
                                                         name="baselines")])
    mapper = ops.MapMaker(name="mapmaker", det_data=defaults.det_data, binning=binner, template_matrix=templates,
                          iter_max=50, convergence=1e-12)
    mapper.apply(demod_data)
    hits = demod_data["mapmaker_hits"].data
    m = demod_data["mapmaker_map"].data
    good = hits[:, :, 0] > 0
    n_pseudo = sum(len(ob.local_detectors) for ob in demod_data.obs)
    print(f"demodulated run: {n_pseudo} pseudo-detectors x {demod_data.obs[0].n_local_samples} samples (nskip {args.nskip})  "
          f"hit pixels {np.count_nonzero(good)}  wall {time.time() - t0:.2f} s")
    print("demodulated run: " + residual(m, good, sky, demod_data["pixel_dist"]))
    return demod_data


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndet", type=int, default=4)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rate", type=float, default=100.0)
    ap.add_argument("--nside", type=int, default=64)
    ap.add_argument("--destripe", action="store_true", help="solve for baseline offsets (MapMaker PCG)")
    ap.add_argument("--full-pointing", action="store_true", help="cache pixels / weights instead of recomputing")
    ap.add_argument("--sim-noise", action="store_true",
                    help="draw the detector noise on the device with ops.SimNoise from the observation's AnalyticNoise "
                         "(1/f included) instead of host white noise")
    ap.add_argument("--estimate-noise", action="store_true",
                    help="measure the noise PSDs from the timestreams with ops.NoiseEstim; the measured model replaces "
                         "the analytic one for what follows (detector weights)")
    ap.add_argument("--demodulate", action="store_true",
                    help="scan an input sky, then also demodulate (ops.Demodulate, ops.StokesWeightsDemod) and map the "
                         "pseudo-detectors; prints both maps' residual against the input sky")
    ap.add_argument("--nskip", type=int, default=3, help="decimation factor of --demodulate")
    ap.add_argument("--hwp-rpm", type=float, default=None, help="HWP rotation rate (9, or 120 with --demodulate)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    n_samp = int(args.minutes * 60 * args.rate)
    t0 = time.time()
    data = create_satellite_data(n_det=args.ndet, n_samp=n_samp, rate=args.rate, spin_period_s=600.0,
                                 spin_angle_deg=30.0, prec_period_s=3000.0, prec_angle_deg=65.0, net=1.0,
                                 hwp_rpm=args.hwp_rpm if args.hwp_rpm is not None else (120.0 if args.demodulate else 9.0))
    rng = np.random.default_rng(1)
    for ob in data.obs:
        sig = ob.detdata[defaults.det_data].data
        sig[:] = 0.0 if args.sim_noise else rng.standard_normal(sig.shape)
        if args.destripe:
            sig += (rng.standard_normal((sig.shape[0], 1)) * 5.0)  # one offset per detector
    sky = None
    if args.demodulate:
        sky = scan_input_sky(data, args.nside)
    if args.sim_noise:
        from toast_amd.accel import accel_enabled

        ops.SimNoise(noise_model=defaults.noise_model).apply(data, use_accel=accel_enabled())
    if args.estimate_noise:
        ops.NoiseEstim(out_model="measured_noise", lagmax=min(10000, n_samp // 4)).apply(data)
        for ob in data.obs:
            truth, measured = ob[defaults.noise_model], ob["measured_noise"]
            ratios = {}
            for det in measured.keys:
                f, p = measured.freq(det), measured.psd(det)
                band = f > args.rate / 4                      # the upper half of the band
                ratios.setdefault(truth.NET(det), []).append(
                    float(np.mean(p[band] / np.interp(f[band], truth.freq(det), truth.psd(det)))))
            for net, r in sorted(ratios.items()):
                print(f"NoiseEstim, {len(r)} detectors with NET {net:g}: estimated / input PSD over the upper half band "
                      f"{np.mean(r):.4f} (min {np.min(r):.4f}, max {np.max(r):.4f})")
            ob[defaults.noise_model] = measured
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=args.nside, nest=True)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU", hwp_angle=defaults.hwp_angle)
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=weights,
                        full_pointing=args.full_pointing)
    templates = None
    if args.destripe:
        templates = ops.TemplateMatrix(templates=[Offset(step_time=60.0, noise_model=defaults.noise_model,
                                                         name="baselines")])
    mapper = ops.MapMaker(name="mapmaker", det_data=defaults.det_data, binning=binner, template_matrix=templates,
                          iter_max=50, convergence=1e-12)
    mapper.apply(data)
    dt = time.time() - t0
    hits = data["mapmaker_hits"].data
    m = data["mapmaker_map"].data
    good = hits[:, :, 0] > 0
    print(f"detectors {args.ndet}  samples/det {n_samp}  nside {args.nside}  "
          f"local submaps {data['pixel_dist'].n_local_submap}  hit pixels {np.count_nonzero(good)}  "
          f"total hits {int(hits.sum())}  PCG iterations {len(mapper.history)}  wall {dt:.2f} s")
    print("map rms  I %.6g  Q %.6g  U %.6g" % tuple(np.sqrt(np.mean(m[good] ** 2, axis=0))))
    if args.demodulate:
        print("modulated run:   " + residual(m, good, sky, data["pixel_dist"]))
        demodulate_and_map(data, args, sky)
    if args.out:
        np.savez_compressed(args.out, map=m, hits=hits, submaps=data["pixel_dist"].local_submaps,
                            rcond=data["mapmaker_rcond"].data)
    return data


if __name__ == "__main__":
    main()
