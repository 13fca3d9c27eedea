"""Host: the lagged-sum entries, the running average, autocov_psd / crosscov_psd and the host path of ops.NoiseEstim
against tests/golden/noise_estim.npz -- the reference's own compiled sums and Python functions
(tests/golden/make_golden_noise_estim.py).

* fod_autosums / fod_crosssums: sums bit-identical, hits equal (the same sequential loops, no contraction).
* running average: <= 4 x trend_ref_err of the row's rms (one rounded chain); the same hit / no-hit decision.
* PSDs: <= 10 x psd_ref_err of the row's largest |PSD| (an FFT sits in the chain).  The case with remove_common_mode
  is asserted in test_gpu_noise_estim.py, with the sums on the host as well: CommonModeFilter has no host path.

Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import noise_estim_case as nc  # noqa: E402

G = nc.gold()
TREND_BOUND = 4.0 * float(G["trend_ref_err"])
PSD_BOUND = 10.0 * float(G["psd_ref_err"])


@pytest.mark.parametrize("binding", ["capi", "pybind"])
def test_host_sums_bit_identical(binding):
    if binding == "capi":
        from toast_amd import capi as mod
    else:
        from toast_amd import _libtoast_hip as mod
    differing = 0
    for name, n, lagmax, fk, kind, all_sums, sym, seed in nc.sums_cases():
        x, y, good = nc.sums_inputs(n, lagmax, fk, kind, seed)
        sums, hits = np.full(lagmax, 0.25), np.full(lagmax, 3, dtype=np.int64)
        if kind == "auto":
            mod.fod_autosums(x, good, lagmax, sums, hits, all_sums)
        else:
            mod.fod_crosssums(x, y, good, lagmax, sums, hits, all_sums, sym)
        differing += int(np.count_nonzero(sums != G[f"sums_{name}"]))
        assert np.array_equal(hits, G[f"hits_{name}"]), name
        assert np.array_equal(sums, G[f"sums_{name}"]), name
    print(f"{binding}: {len(nc.sums_cases())} cases, {differing} sums differ from the fixture")


def test_binding_size_checks():
    from toast_amd import _libtoast_hip as lt
    from toast_amd import capi

    x, g = np.zeros(10), np.ones(10, dtype=np.uint8)
    s, h = np.zeros(4), np.zeros(4, dtype=np.int64)
    for mod in (lt, capi):
        with pytest.raises(RuntimeError, match="not consistent"):
            mod.fod_autosums(x, g[:9], 4, s, h, 1)
        with pytest.raises(RuntimeError, match="not consistent"):
            mod.fod_autosums(x, g, 5, s, h, 1)
        with pytest.raises(RuntimeError, match="not consistent"):
            mod.fod_crosssums(x, x[:9], g, 4, s, h, 1, 0)
        with pytest.raises(RuntimeError, match="not consistent"):
            mod.fod_crosssums(x, x, g, 4, s, h[:3], 1, 0)
        with pytest.raises(RuntimeError):
            mod.fod_autosums(x.astype(np.float32), g, 4, s, h, 1)
    # lagmax > n is legal and contributes nothing past the row
    s, h = np.zeros(20), np.zeros(20, dtype=np.int64)
    capi.fod_autosums(np.ones(10), g, 20, s, h, 1)
    assert np.array_equal(h, np.concatenate([np.arange(10, 0, -1), np.zeros(10, dtype=np.int64)]))
    capi.fod_autosums(np.ones(10), g, 20, s, h, 0)
    assert h[0] == 10


def test_host_running_average():
    from toast_amd.ops.noise_estimation_utils import flagged_running_average, highpass_flagged_signal

    for name, n, w, fk, off in nc.TREND_ROWS:
        x, good = nc.trend_inputs(name, n, w, fk, off)
        trend, flags = flagged_running_average(x, good == 0, w, return_flags=True)
        dist = float(np.max(np.abs(trend - G[f"trend_{name}"]))) / nc.row_rms(x)
        ld, cnt = nc.trend_longdouble(x, good, w)
        dist_ld = float(np.max(np.abs(trend.astype(nc.L) - ld))) / nc.row_rms(x)
        print(f"running average {name} (n {n}, window {w}, flags {fk}, offset {off:g}): {dist:.3e} of the rms from the "
              f"fixture, {dist_ld:.3e} from long double; bound {TREND_BOUND:.3e}")
        assert np.array_equal(flags == 0, G[f"trend_hit_{name}"]), name
        assert dist <= TREND_BOUND and dist_ld <= TREND_BOUND, name
        hp = highpass_flagged_signal(x, good, w)
        assert np.array_equal(hp, x - trend)
    x, good = nc.trend_inputs("all", 500, 10, "all", 0.0)
    assert np.all(highpass_flagged_signal(x, good, 10) == 0)
    with pytest.raises(Exception, match="lengths"):
        flagged_running_average(x, good[:-1], 10)


def test_covariance_psd_functions():
    """autocov_psd / crosscov_psd with the reference's signatures: the operator's host path calls the same pieces, so
    the fixture's "views" case is reproduced by hand for its first key."""
    from toast_amd.data import defaults
    from toast_amd.ops import noise_estimation_utils as u

    case = nc.OP_CASES["views"]["op"]
    ob = nc.make_obs("views").obs[0]
    times = np.array(ob.shared[defaults.times].data)
    flags = ((ob.shared[defaults.shared_flags].data & defaults.shared_mask_nonscience) != 0) | \
        ((ob.detdata[defaults.det_flags]["D00"] & defaults.det_mask_invalid) != 0)
    ivals = [(iv.start, iv.stop) for iv in ob.intervals["scan"]]
    sig = u.highpass_flagged_signal(np.array(ob.detdata[defaults.det_data]["D00"]), flags == 0, case["lagmax"])
    psds, cov = u.autocov_psd(times, times, ivals, sig, flags, case["lagmax"], case["lagmax"],
                              float(case["stationary_period"]), nc.RATE, return_cov=True)
    assert len(psds) == len(cov) == 3 and np.all(sig[flags] == 0)
    mean = np.mean([p[3] for p in psds], axis=0)
    want = G["op_views_psd_0"]
    dist = float(np.max(np.abs(mean[1:] - want)) / np.max(np.abs(want)))
    print(f"autocov_psd, three periods and three views: {dist:.3e} of max |PSD|; bound {PSD_BOUND:.3e}")
    assert dist <= PSD_BOUND
    with pytest.raises(NotImplementedError):
        u.crosscov_psd(times, times, ivals, sig, sig, flags, 10, 10, 50.0, nc.RATE, comm=object())
    hits, smooth = u.smooth_with_hits(np.array([2, 0, 2, 2]), np.array([1.0, 5.0, 3.0, 4.0]), 3)
    assert np.array_equal(hits, [2, 4, 4, 4]) and np.allclose(smooth, [1.0, 2.0, 3.5, 3.5])


@pytest.mark.parametrize("name", sorted(set(nc.OP_CASES) - set(nc.DEVICE_ONLY_CASES)))
def test_operator_host_path(name):
    data, model = nc.estimate(name, use_accel=False)
    dist = nc.psd_distance(model, G, name)
    print(f"NoiseEstim host path, case {name} ({nc.OP_CASES[name]['op']}): {dist:.3e} of max |PSD|; bound {PSD_BOUND:.3e}")
    assert dist <= PSD_BOUND


def test_operator_refusals_and_model():
    from toast_amd import ops
    from toast_amd.noise import Noise

    data = nc.make_obs("auto")
    with pytest.raises(NotImplementedError):
        ops.NoiseEstim(mapfile="map.fits").apply(data)
    with pytest.raises(NotImplementedError):
        ops.NoiseEstim(maskfile="mask.fits").apply(data)
    with pytest.raises(RuntimeError, match="subsets of detectors"):
        ops.NoiseEstim().apply(data, detectors=["D00"])
    with pytest.raises(RuntimeError, match="not compatible"):
        ops.NoiseEstim(focalplane_key="wafer", pairs=[["D00", "D01"]]).apply(data)
    _, model = nc.estimate("pairs_cut", use_accel=False, save_cov=True)
    assert isinstance(model, Noise) and sorted(model.keys) == ["D00 x D02", "D01", "D02"]
    assert model.freq("D01").size == 3 and np.all(model.psd("D01") == 0)        # the cut detector: four points less one
    from toast_amd.noise import name_UID

    assert model.index("D00 x D02") == name_UID("D00")          # the first detector's uid
    assert model.detector_weight("D02") > 0 and model.detector_weight("D01") == 0


def test_white_noise_recovery_host():
    """SimNoise white noise through NoiseEstim: the mean PSD over the upper half band against NET^2 within
    5 * 2 / sqrt(n) (n / 4 independent modes, 5 sigma)."""
    import sim_noise_case as sc
    from toast_amd import ops

    n = 1 << 14
    data = sc.make_data(n_det=4, n_samp=n, rate=100.0, fknee=0.0, net=1.0)
    ops.SimNoise().apply(data)
    ops.NoiseEstim(out_model="measured", lagmax=512, nbin_psd=64, det_flags=None, shared_flags=None).apply(data)
    model, truth = data.obs[0]["measured"], data.obs[0]["noise_model"]
    bound = 5.0 * 2.0 / np.sqrt(n)
    for det in model.keys:
        f, p = model.freq(det), model.psd(det)
        ratio = float(np.mean(p[f > 25.0]) / truth.NET(det) ** 2)
        print(f"{det}: estimated / input PSD over the upper half band {ratio:.4f}; bound 1 +- {bound:.4f}")
        assert abs(ratio - 1.0) <= bound
