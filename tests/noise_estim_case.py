"""Shared by test_noise_estim_host.py, test_gpu_noise_estim.py and tests/golden/make_golden_noise_estim.py: the inputs
of the fixture tests/golden/noise_estim.npz, regenerated from ``toast_amd.rng`` streams (pinned bit for bit by the
sim-noise fixture), long-double evaluations of the lagged sums and of the running average, and small observations."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "noise_estim.npz")
L = np.longdouble

FLAG_KINDS = ("none", "random", "gap", "all")


def gold():
    return np.load(GOLD_PATH, allow_pickle=False)


def signal(seed, n, offset=0.0):
    from toast_amd import rng

    return rng.random(n, key=(int(seed), 77), counter=(0, 0), sampler="gaussian") + offset


def good_mask(kind, seed, n, lagmax):
    """uint8, non-zero = use: none flagged, 10 % random, one gap longer than lagmax, all flagged."""
    from toast_amd import rng

    good = np.ones(n, dtype=np.uint8)
    if kind == "random":
        good[rng.random(n, key=(int(seed), 78), counter=(0, 0), sampler="uniform_01") < 0.1] = 0
    elif kind == "gap":
        a = n // 3
        good[a:min(n, a + lagmax + 5)] = 0
    elif kind == "all":
        good[:] = 0
    return good


# ---------------------------------------------------------------------------------------------- lagged sums
#: (n, lagmax) of the fixture's sums cases; each with every flag kind and four variants
SUMS_SHAPES = ((1000, 37), (300, 257), (65, 100), (4099, 64))
SUMS_VARIANTS = (("auto", 1, 0), ("auto", 0, 0), ("cross", 1, 0), ("cross", 0, 1))      # (kind, all_sums, symmetric)


def sums_cases():
    """[(name, n, lagmax, flag kind, kind, all_sums, symmetric, seed)]"""
    out, seed = [], 100
    for n, lagmax in SUMS_SHAPES:
        for fk in FLAG_KINDS:
            for kind, all_sums, sym in SUMS_VARIANTS:
                out.append((f"s{len(out):02d}", n, lagmax, fk, kind, all_sums, sym, seed))
                seed += 1
    return out


def sums_inputs(n, lagmax, fk, kind, seed):
    x = signal(seed, n)
    y = signal(seed + 5000, n) * 0.5 + 0.5 * x if kind == "cross" else None
    return x, y, good_mask(fk, seed, n, lagmax)


def sums_longdouble(x, y, good, lagmax, all_sums, symmetric, lags=None):
    """(sums in long double, sum of |products| in double, hits) of toast_fod_psd.cpp:12-93 at ``lags`` (all)."""
    n = x.size
    g = good != 0
    xg = np.where(g, x, 0.0).astype(L)
    yg = xg if y is None else np.where(g, y, 0.0).astype(L)
    gi = g.astype(np.int64)
    lags = np.arange(lagmax) if lags is None else np.asarray(lags)
    sums, norm, hits = np.zeros(lags.size, dtype=L), np.zeros(lags.size), np.zeros(lags.size, dtype=np.int64)
    for k, lag in enumerate(lags):
        imax = n - lag if all_sums else n - lagmax
        if imax <= 0:
            continue
        p = xg[:imax] * yg[lag:lag + imax]
        h = int(np.sum(gi[:imax] * gi[lag:lag + imax]))
        a = np.sum(np.abs(p))
        s = np.sum(p)
        if y is not None and symmetric and lag != 0:
            q = xg[lag:lag + imax] * yg[:imax]
            s += np.sum(q)
            a += np.sum(np.abs(q))
            h *= 2
        sums[k], norm[k], hits[k] = s, float(a), h
    return sums, norm, hits


def sums_distance(got, want_ld, norm):
    """max |got - long double| / sum |products| over the lags that have any product."""
    ok = norm > 0
    if not np.any(ok):
        return 0.0
    return float(np.max(np.abs(got.astype(L)[ok] - want_ld[ok]) / norm[ok].astype(L)))


# ---------------------------------------------------------------------------------------------- running average
#: (name, n, window, flag kind, offset) of the trend rows stored in the fixture
TREND_ROWS = (("t0", 1000, 2, "random", 0.0), ("t1", 1000, 101, "random", 0.0), ("t2", 1000, 101, "gap", 0.0),
              ("t3", 1000, 3000, "random", 0.0), ("t4", 1000, 100, "none", 0.0), ("t5", 4099, 100, "random", 1.0e6))
#: every combination that enters trend_ref_err
TREND_WINDOWS = (1, 2, 100, 101, 3000)


def trend_inputs(name_or_seed, n, window, fk, offset):
    seed = 900 + sum(ord(c) for c in str(name_or_seed))
    return signal(seed, n, offset), good_mask(fk, seed, n, min(window, n // 4))


def trend_longdouble(x, good, window):
    """(trend in long double, count): the flagged running average over [i - w // 2, i + (w - 1) // 2]."""
    n = x.size
    g = good != 0
    c = np.concatenate([[L(0)], np.cumsum(np.where(g, x, 0.0).astype(L))])
    k = np.concatenate([[0], np.cumsum(g.astype(np.int64))])
    i = np.arange(n)
    lo = np.clip(i - window // 2, 0, n)
    hi = np.clip(i + (window - 1) // 2 + 1, 0, n)
    cnt = k[hi] - k[lo]
    s = c[hi] - c[lo]
    return np.where(cnt > 0, s / np.maximum(cnt, 1).astype(L), L(0)), cnt


def row_rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, dtype=np.float64) ** 2)))


# ---------------------------------------------------------------------------------------------- observations
RATE = 50.0
OP_CASES = {
    "auto": dict(op=dict(lagmax=200, nbin_psd=30)),
    "cross_flags": dict(flags=True, op=dict(lagmax=150, nbin_psd=30, nocross=False, symmetric=True)),
    "views": dict(flags=True, views=[(100, 1500), (1500, 2600), (3000, 5900)],
                  op=dict(lagmax=120, nbin_psd=None, view="scan", stationary_period=50)),
    "nsum": dict(flags=True, op=dict(lagmax=300, nbin_psd=40, nsum=4, naverage=5)),
    "pairs_cut": dict(cut=["D01"], op=dict(lagmax=200, nbin_psd=25,
                                           pairs=[["D00", "D02"], ["D01", "D01"], ["D02", "D02"], ["D00", "nope"]])),
    "outliers": dict(op=dict(lagmax=100, nbin_psd=12, stationary_period=10)),
    "common": dict(n_det=4, flags=True, op=dict(lagmax=150, nbin_psd=20, focalplane_key="wafer", nocross=False)),
    "common_rm": dict(n_det=4, flags=True, op=dict(lagmax=150, nbin_psd=20, focalplane_key="wafer", nocross=False,
                                                   remove_common_mode=True)),
}


#: cases whose pre-processing (CommonModeFilter) runs on the device only
DEVICE_ONLY_CASES = ("common_rm",)


def make_obs(name, n=6000):
    """Data with one observation for an operator case: white noise plus a common component and an offset per
    detector, uint8 detector and shared flags, the intervals "scan"."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults

    case = OP_CASES[name]
    n_det = case.get("n_det", 3)
    dets = [f"D{i:02d}" for i in range(n_det)]
    quats = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n_det, 1))
    fp = Focalplane(dets, quats, sample_rate=RATE, columns={"wafer": [f"w{i // 2}" for i in range(n_det)]})
    ob = Observation(None, Telescope("ne_tele", fp), n, name="obs_" + name)
    ob.set_times(1000.0 + np.arange(n) / RATE)
    seed = 2000 + 10 * sorted(OP_CASES).index(name)
    common = signal(seed + 9, n)
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=defaults.det_data_units)
    ob.detdata.create(defaults.det_flags, dtype=np.uint8)
    shared = np.zeros(n, dtype=np.uint8)
    for i, d in enumerate(dets):
        ob.detdata[defaults.det_data][d] = (1.0 + 0.2 * i) * signal(seed + i, n) + 0.4 * common + 3.0 * i
        if case.get("flags"):
            ob.detdata[defaults.det_flags][d] = (good_mask("random", seed + i, n, 0) == 0).astype(np.uint8)
    if case.get("flags"):
        shared[n // 2:n // 2 + 40] = 1
        shared[7::501] = 16          # outside the shared mask
    ob.shared.create(defaults.shared_flags, shared)
    ob.intervals.create("scan", case.get("views", [(0, n)]))
    ob.update_local_detector_flags({d: 1 for d in case.get("cut", [])})
    data = Data()
    data.obs.append(ob)
    return data


def estimate(name, use_accel=None, resident=False, **extra):
    """(data, noise model) of NoiseEstim on an operator case."""
    from toast_amd import ops
    from toast_amd.data import defaults

    data = make_obs(name)
    if resident:
        dd = data.obs[0].detdata[defaults.det_data]
        dd.accel_create(defaults.det_data)
        dd.accel_update_device()
    op = ops.NoiseEstim(out_model="measured", **OP_CASES[name]["op"])
    for k, v in extra.items():
        setattr(op, k, v)
    op.apply(data, use_accel=use_accel)
    return data, data.obs[0]["measured"]


def psd_distance(model, G, name):
    """Largest |PSD - fixture| / max |fixture PSD| over the keys of an operator case; the keys must match."""
    keys = [str(k) for k in G[f"op_{name}_keys"]]
    assert sorted(model.keys) == sorted(keys), (model.keys, keys)
    worst = 0.0
    for i, k in enumerate(keys):
        want_f, want_p = G[f"op_{name}_freq_{i}"], G[f"op_{name}_psd_{i}"]
        assert np.array_equal(model.freq(k), want_f), (name, k)
        scale = np.max(np.abs(want_p))
        if scale == 0:
            assert np.all(model.psd(k) == 0)
            continue
        worst = max(worst, float(np.max(np.abs(model.psd(k) - want_p)) / scale))
    return worst
