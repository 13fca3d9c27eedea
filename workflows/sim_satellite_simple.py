#!/usr/bin/env python3
"""Simulated satellite scan -> binned map, with the reference's operator names.

Counterpart of the reference's ``workflows/toast_sim_satellite_simple.py`` restated with its
current API (PixelsHealpix + StokesWeights + BinMap) -- BASELINE.json
configs[0] (4 detectors x 10 min @ 100 Hz, Nside 64) by default, configs[1] with
``--ndet 64 --minutes 60 --nside 512``.  Everything numerical runs on the MI355X.

    python workflows/sim_satellite_simple.py [--ndet 4] [--minutes 10] [--rate 100] [--nside 64]
                                             [--destripe] [--sim-noise] [--estimate-noise] [--out map.npz]
                                             [--demodulate [--nskip N] [--hwp-rpm R] [--hwpss AMP]]
                                             [--gain-drift ORDER [--noise-free]]
                                             [--dipole {solar,orbital,total}]

``--demodulate``: the HWP spins at ``--hwp-rpm`` (default 120, i.e. 2 Hz), a piecewise-constant input sky is scanned into
the signal, and after the usual (modulated) map the data goes through Demodulate -> StokesWeightsDemod -> the same
binning / ``--destripe`` map-maker; the residual of both maps against the input sky is printed.

``--hwpss AMP`` (with ``--demodulate``): an HWP-synchronous signal -- harmonics 1, 2 and 4 of the HWP angle, the 2f line
``AMP`` times the rms of the scanned signal, a few per cent of scatter between detectors -- is added to the signal.  The
data is demodulated and mapped once as it is (residual printed), then ops.HWPSynchronousModel subtracts its model and the
usual modulated and demodulated runs follow.

``--gain-drift ORDER``: the input sky is scanned into a detdata key of its own, the *signal estimate*; the signal is
``estimate * (1 + L a_injected)`` -- a Legendre series of that order per detector, a few per cent -- plus the usual noise
(none with ``--noise-free``), and the map-maker solves for [Offset, GainTemplate].  Injected and recovered amplitudes are
printed.  The mean of the order-0 terms over the detectors is degenerate with the map -- a common gain is a brighter sky
-- so order 0 is reported relative to that mean.  A drift can only be told from the sky where pixels are seen again at
another time: this run spins once a minute instead of once in ten.

``--dipole MODE``: a STAND-IN telescope velocity (``synth.orbital_velocity``: a circular orbit in the ecliptic plane) is
stored under ``ob.shared["velocity"]`` and ops.SimDipole adds the CMB dipole -- solar, orbital or both -- to the signal
before map-making; the rms and the peak of what it added are printed.  With ``--gain-drift`` the dipole goes into the
signal estimate, ahead of the drift: the signal is ``(sky + dipole) * (1 + drift)`` and the gain is calibrated on sky
plus dipole, as a satellite's is.
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
from toast_amd.templates import GainTemplate, Offset  # noqa: E402

GAIN_ESTIMATE = "gain_estimate"


def input_sky(nside):
    """[12 nside^2][I, Q, U], NESTED: constant over the pixels of Nside 4, so that it varies slowly along the scan."""
    npix = 12 * nside * nside
    coarse = np.arange(npix) // max(1, (nside // 4) ** 2)
    return np.stack([1.0 + 0.1 * np.sin(0.7 * coarse), 0.05 * np.cos(0.4 * coarse), 0.03 * np.sin(0.9 * coarse + 1.0)], axis=1)


def scan_input_sky(data, nside, det_data=defaults.det_data):
    """Add the input sky to ``det_data`` through the pointing the map-maker will use; returns the sky."""
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
        ob.detdata[det_data].data[seen] += np.sum(w[seen] * sky[pix[seen]], axis=1)
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


def add_dipole(data, args, det_data):
    """Store the stand-in velocity, run SimDipole into ``det_data`` and print what it added."""
    from toast_amd import synth
    from toast_amd.accel import accel_enabled

    before = []
    for ob in data.obs:
        if defaults.velocity not in ob.shared:
            ob.shared.create(defaults.velocity, synth.orbital_velocity(ob.shared[defaults.times].data))
        if ob.detdata[det_data].units is None:
            ob.detdata[det_data].update_units(defaults.det_data_units)
        before.append(ob.detdata[det_data].data.copy())
    ops.SimDipole(det_data=det_data, mode=args.dipole, coord="E").apply(data, use_accel=accel_enabled())
    added = np.concatenate([(ob.detdata[det_data].data - b).reshape(-1) for ob, b in zip(data.obs, before)])
    print(f"dipole ({args.dipole}, STAND-IN orbit) added to '{det_data}': rms {np.sqrt(np.mean(added ** 2)):.6e} K  "
          f"peak {np.max(np.abs(added)):.6e} K")


def inject_gain_drift(data, args):
    """Scan the input sky into the estimate, add ``estimate * (1 + drift)`` to the signal; returns the injected amplitudes
    [n_det][order + 1] (one observation)."""
    from toast_amd.templates.subharmonic import legendre_basis

    for ob in data.obs:
        ob.detdata.create(GAIN_ESTIMATE, dtype=np.float64)
    scan_input_sky(data, args.nside, det_data=GAIN_ESTIMATE)
    if args.dipole:
        add_dipole(data, args, GAIN_ESTIMATE)
    rng = np.random.default_rng(2)
    injected = 0.03 * rng.standard_normal((args.ndet, args.gain_drift + 1))
    for ob in data.obs:
        basis = legendre_basis(args.gain_drift + 1, ob.n_local_samples)
        ob.detdata[defaults.det_data].data[:] += ob.detdata[GAIN_ESTIMATE].data * (1.0 + injected @ basis)
    return injected


def report_gain_drift(data, mapper, injected):
    """Print injected against recovered amplitudes; order 0 relative to its mean over the detectors."""
    recovered = data["mapmaker_solve_amplitudes"]["gain"].local.reshape(injected.shape).copy()
    data["gain_drift_injected"], data["gain_drift_recovered"] = injected, recovered
    data["gain_drift_history"] = np.array(mapper.history)
    diff = recovered - injected
    print(f"gain drift: mean over the detectors of recovered - injected order 0 = {diff[:, 0].mean():+.6f} (degenerate with "
          f"the map: a common gain is a brighter sky; order 0 below is relative to that mean)")
    diff[:, 0] -= diff[:, 0].mean()
    for d in range(injected.shape[0]):
        print(f"gain drift, detector {d}: injected " + " ".join(f"{x:+.6f}" for x in injected[d]) + "   recovered " +
              " ".join(f"{x:+.6f}" for x in injected[d] + diff[d]))
    print(f"gain drift: largest error {np.abs(diff).max():.3e}, rms of the injected amplitudes "
          f"{np.sqrt(np.mean(injected ** 2)):.3e}")


def add_hwpss(data, amp, det_data):
    """Add an HWP-synchronous signal to every detector: harmonics 1, 2 and 4 of the HWP angle, ``amp`` times the rms of the
    scanned signal at 2f (0.4 and 0.25 of that at 1f and 4f), with a few per cent of scatter between the detectors."""
    rng = np.random.default_rng(7)
    for ob in data.obs:
        sig = ob.detdata[det_data].data
        angle = ob.shared[defaults.hwp_angle].data
        level = amp * float(np.sqrt(np.mean((sig - sig.mean(axis=1, keepdims=True)) ** 2)))
        for d in range(sig.shape[0]):
            for h, rel in ((1, 0.4), (2, 1.0), (4, 0.25)):
                sig[d] += level * rel * (1 + 0.03 * rng.standard_normal()) * np.sin(h * angle + rng.uniform(0, 2 * np.pi))
    print(f"HWPSS added to '{det_data}': 2f amplitude {level:.4g} = {amp:g} x the rms of the scanned signal")


def demodulate_and_map(data, args, sky, label="demodulated run"):
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
    print(f"{label}: {n_pseudo} pseudo-detectors x {demod_data.obs[0].n_local_samples} samples (nskip {args.nskip})  "
          f"hit pixels {np.count_nonzero(good)}  wall {time.time() - t0:.2f} s")
    print(f"{label}: " + residual(m, good, sky, demod_data["pixel_dist"]))
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
    ap.add_argument("--hwpss", type=float, default=None, metavar="AMP",
                    help="with --demodulate: add an HWP-synchronous signal of AMP times the sky rms per detector, demodulate "
                         "and map it once as it is, then remove it with ops.HWPSynchronousModel before everything else")
    ap.add_argument("--gain-drift", type=int, default=None, metavar="ORDER",
                    help="inject a Legendre gain drift of this order per detector on a scanned input sky and solve for "
                         "[Offset, GainTemplate]; prints injected against recovered amplitudes")
    ap.add_argument("--noise-free", action="store_true", help="with --gain-drift: no detector noise")
    ap.add_argument("--dipole", choices=("solar", "orbital", "total"), default=None,
                    help="add the CMB dipole with ops.SimDipole from a stand-in orbital velocity before map-making; with "
                         "--gain-drift it is part of the signal estimate")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    gain = args.gain_drift is not None
    if gain and (args.demodulate or args.gain_drift < 0):
        ap.error("--gain-drift takes an order >= 0 and does not combine with --demodulate")
    if args.noise_free and not gain:
        ap.error("--noise-free belongs to --gain-drift")
    if args.hwpss is not None and not args.demodulate:
        ap.error("--hwpss belongs to --demodulate")

    n_samp = int(args.minutes * 60 * args.rate)
    t0 = time.time()
    data = create_satellite_data(n_det=args.ndet, n_samp=n_samp, rate=args.rate, spin_period_s=60.0 if gain else 600.0,
                                 spin_angle_deg=30.0, prec_period_s=3000.0, prec_angle_deg=65.0, net=1.0,
                                 hwp_rpm=args.hwp_rpm if args.hwp_rpm is not None else (120.0 if args.demodulate else 9.0))
    rng = np.random.default_rng(1)
    for ob in data.obs:
        sig = ob.detdata[defaults.det_data].data
        sig[:] = 0.0 if (args.sim_noise or args.noise_free) else rng.standard_normal(sig.shape)
        if args.destripe:
            sig += (rng.standard_normal((sig.shape[0], 1)) * 5.0)  # one offset per detector
    sky = None
    if args.demodulate:
        sky = scan_input_sky(data, args.nside)
    if gain:
        injected = inject_gain_drift(data, args)
    elif args.dipole:
        add_dipole(data, args, defaults.det_data)
    if args.sim_noise:
        from toast_amd.accel import accel_enabled

        ops.SimNoise(noise_model=defaults.noise_model).apply(data, use_accel=accel_enabled())
    if args.hwpss is not None:
        from toast_amd.accel import accel_enabled

        add_hwpss(data, args.hwpss, defaults.det_data)
        demodulate_and_map(data, args, sky, label="demodulated run, HWPSS left in")
        for key in ("pixel_dist", "mapmaker_hits", "mapmaker_map"):
            if key in data:
                del data[key]
        # Every sample is modelled and cleaned (no flags): the operator subtracts from good samples only, a flagged sample
        # would keep its HWPSS (the reference fills such gaps with noise, fill_gaps) and Demodulate's filters spread it.
        # The operator also removes each detector's mean; the level the detector had before (the HWPSS adds next to
        # nothing to it over whole turns) is put back so that the I map can be compared.
        level = [ob.detdata[defaults.det_data].data.mean(axis=1, keepdims=True) for ob in data.obs]
        ops.HWPSynchronousModel(subtract_model=True, det_flags=None, shared_flags=None).apply(data, use_accel=accel_enabled())
        for ob, dc in zip(data.obs, level):
            ob.detdata[defaults.det_data].data[:] += dc
        print("HWPSynchronousModel: one chunk, 9 harmonics, model subtracted from every sample, detector levels restored")
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
    solver = dict(iter_max=50, convergence=1e-12)
    if gain:
        templates = ops.TemplateMatrix(templates=[
            Offset(step_time=60.0, noise_model=defaults.noise_model, name="baselines"),
            GainTemplate(order=args.gain_drift, template_name=GAIN_ESTIMATE, noise_model=defaults.noise_model, name="gain")])
        # (the amplitudes are compared with what was injected: solved to rounding, no stall test on the way, and kept)
        solver = dict(iter_min=100, iter_max=300, convergence=1e-24, keep_solver_products=True)
    mapper = ops.MapMaker(name="mapmaker", det_data=defaults.det_data, binning=binner, template_matrix=templates, **solver)
    mapper.apply(data)
    dt = time.time() - t0
    hits = data["mapmaker_hits"].data
    m = data["mapmaker_map"].data
    good = hits[:, :, 0] > 0
    print(f"detectors {args.ndet}  samples/det {n_samp}  nside {args.nside}  "
          f"local submaps {data['pixel_dist'].n_local_submap}  hit pixels {np.count_nonzero(good)}  "
          f"total hits {int(hits.sum())}  PCG iterations {len(mapper.history)}  wall {dt:.2f} s")
    print("map rms  I %.6g  Q %.6g  U %.6g" % tuple(np.sqrt(np.mean(m[good] ** 2, axis=0))))
    if gain:
        report_gain_drift(data, mapper, injected)
    if args.demodulate:
        print("modulated run:   " + residual(m, good, sky, data["pixel_dist"]))
        demodulate_and_map(data, args, sky)
    if args.out:
        np.savez_compressed(args.out, map=m, hits=hits, submaps=data["pixel_dist"].local_submaps,
                            rcond=data["mapmaker_rcond"].data)
    return data


if __name__ == "__main__":
    main()
