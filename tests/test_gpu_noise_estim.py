"""GPU: the noise-estimation kernels (csrc/noise_estim.hip) and the device path of ops.NoiseEstim.

* Lagged sums: hits exact; |device - long double| / sum |products| <= 4 x sums_ref_err (the device is to be no further
  from the truth than four times the reference is).  The long double sums are evaluated here with NumPy
  (noise_estim_case.sums_longdouble, the evaluation the fixture's sums_ref_err was measured against).
* Invariance: batch size, repetition and the order of the pairs do not change one bit.
* High-pass: <= 4 x trend_ref_err of the row's rms against a long double window sum; zero rows where all is flagged.
* Operator on resident data: <= 10 x psd_ref_err of max |PSD| against the fixture; det_data and the flags unchanged.
* Recovery of a simulated white spectrum within 5 * 2 / sqrt(n).

Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import noise_estim_case as nc  # noqa: E402

pytestmark = pytest.mark.gpu

G = nc.gold()
SUMS_BOUND = 4.0 * float(G["sums_ref_err"])
TREND_BOUND = 4.0 * float(G["trend_ref_err"])
PSD_BOUND = 10.0 * float(G["psd_ref_err"])


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)
        accel_data_create(self.a, "test_noise_estim")
        accel_data_update_device(self.a, "test_noise_estim")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_noise_estim")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_noise_estim")


def device_sums(rows, good, pairs, segments, n_real, lagmax, symmetric, start=None, max_batch=0):
    """toast_hip_fod_sums_dev on ``rows`` [r][n] / ``good`` [g][n]; pairs = [(row1, row2, good row)]; segments =
    [(first, last, all_sums, realization)].  Returns (sums, hits) [pair][n_real][lagmax]."""
    from toast_amd import capi

    d_rows, d_good = Dev(rows), Dev(good)
    shape = (len(pairs), n_real, lagmax)
    d_sums = Dev(np.zeros(shape) if start is None else start[0])
    d_hits = Dev(np.zeros(shape, dtype=np.int64) if start is None else start[1])
    first, last, all_sums, real = (list(x) for x in zip(*segments))
    try:
        capi.dev.fod_sums([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], d_rows.ptr, rows.shape[0],
                          rows.shape[1], d_good.ptr, good.shape[0], good.shape[1], first, last, all_sums, real, n_real,
                          lagmax, symmetric, d_sums.ptr, d_hits.ptr, max_batch=max_batch)
        capi.synchronize()
        return d_sums.get(), d_hits.get()
    finally:
        for d in (d_rows, d_good, d_sums, d_hits):
            d.free()


def check_single(n, lagmax, fk, kind, all_sums, sym, seed, lags=None):
    x, y, good = nc.sums_inputs(n, lagmax, fk, kind, seed)
    rows = np.vstack([x, x if y is None else y])
    pair = (0, 0, 0) if y is None else (0, 1, 0)
    sums, hits = device_sums(rows, good[None, :], [pair], [(0, n, all_sums, 0)], 1, lagmax, sym)
    ld, norm, want_hits = nc.sums_longdouble(x, y, good, lagmax, all_sums, sym, lags)
    sel = slice(None) if lags is None else lags
    assert np.array_equal(hits[0, 0][sel], want_hits), (n, lagmax, fk, kind, all_sums, sym)
    return nc.sums_distance(sums[0, 0][sel], ld, norm)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4099])
def test_device_sums_grid(n):
    worst = 0.0
    for lagmax in (1, 2, 37, 256, 257, 700):
        for i, fk in enumerate(nc.FLAG_KINDS):
            # auto with and without all_sums, cross with and without symmetry, turning over the flag kinds
            for kind, all_sums, sym in (("auto", (i + 1) % 2, 0), ("cross", i % 2, 0), ("cross", (i + 1) % 2, 1)):
                d = check_single(n, lagmax, fk, kind, all_sums, sym, seed=7000 + n + lagmax)
                worst = max(worst, d)
    print(f"n {n}: lagmax 1 .. 700, four flag kinds, auto / cross / symmetric: worst distance {worst:.3e}; "
          f"bound {SUMS_BOUND:.3e}")
    assert worst <= SUMS_BOUND


def test_device_sums_fixture_cases():
    """The fixture's cases against its stored long double sums and the reference's hits; accumulation into the
    fixture's non-zero start values adds exactly the sums of a run from zero."""
    worst = 0.0
    for name, n, lagmax, fk, kind, all_sums, sym, seed in nc.sums_cases():
        x, y, good = nc.sums_inputs(n, lagmax, fk, kind, seed)
        rows = np.vstack([x, x if y is None else y])
        pair = [(0, 0, 0) if y is None else (0, 1, 0)]
        fresh, _ = device_sums(rows, good[None, :], pair, [(0, n, all_sums, 0)], 1, lagmax, sym)
        start = (np.full((1, 1, lagmax), 0.25), np.full((1, 1, lagmax), 3, dtype=np.int64))
        sums, hits = device_sums(rows, good[None, :], pair, [(0, n, all_sums, 0)], 1, lagmax, sym, start=start)
        assert np.array_equal(hits[0, 0], G[f"hits_{name}"]), name
        assert np.array_equal(sums, 0.25 + fresh), name
        ld = G[f"ld_{name}"][0].astype(nc.L) + G[f"ld_{name}"][1].astype(nc.L)
        _, norm, _ = nc.sums_longdouble(x, y, good, lagmax, all_sums, sym)
        worst = max(worst, nc.sums_distance(fresh[0, 0], ld, norm))
    print(f"{len(nc.sums_cases())} fixture cases: worst distance {worst:.3e}; bound {SUMS_BOUND:.3e}")
    assert worst <= SUMS_BOUND


def test_device_sums_segments_and_realizations():
    n, lagmax = 3000, 300
    x, y, good = nc.sums_inputs(n, lagmax, "random", "cross", 8100)
    rows = np.vstack([x, y])
    # two segments into realization 0 (the second without all_sums), one that starts and ends inside a tile into 1,
    # one into 2; realization 3 stays empty
    segments = [(0, 1100, 1, 0), (1100, 2000, 0, 0), (2040, 2100, 1, 1), (2100, 3000, 1, 2)]
    sums, hits = device_sums(rows, good[None, :], [(0, 1, 0), (1, 1, 0)], segments, 4, lagmax, 1)
    worst = 0.0
    for p, (a, b) in enumerate(((x, y), (y, None))):
        want = np.zeros((4, lagmax), dtype=nc.L)
        norm = np.zeros((4, lagmax))
        want_hits = np.zeros((4, lagmax), dtype=np.int64)
        for first, last, all_sums, real in segments:
            s, m, h = nc.sums_longdouble(a[first:last], None if b is None else b[first:last], good[first:last], lagmax,
                                         all_sums, 1)
            want[real] += s
            norm[real] += m
            want_hits[real] += h
        assert np.array_equal(hits[p], want_hits), p
        assert np.all(sums[p, 3] == 0)
        for r in range(3):
            worst = max(worst, nc.sums_distance(sums[p, r], want[r], norm[r]))
    print(f"four segments into three realizations, cross (symmetric) and auto: worst distance {worst:.3e}; bound {SUMS_BOUND:.3e}")
    assert worst <= SUMS_BOUND


def test_device_sums_mid_size_and_invariance():
    n, lagmax = 20000, 1500
    rows = np.vstack([nc.signal(8200 + i, n) for i in range(3)])
    good = np.vstack([nc.good_mask("random", 8200, n, lagmax), nc.good_mask("gap", 8201, n, lagmax)])
    pairs = [(0, 0, 0), (0, 1, 1), (2, 1, 0)]
    segments = [(0, n, 1, 0)]
    sums, hits = device_sums(rows, good, pairs, segments, 1, lagmax, 0)
    # several sample chunks meet in one lag tile: long double at chosen lags and every 41st
    lags = np.unique(np.concatenate([np.arange(0, lagmax, 41), [1, 2, 7, 8, 1023, 1024, 1025, lagmax - 1]]))
    worst = 0.0
    for p, (r1, r2, g) in enumerate(pairs):
        ld, norm, want_hits = nc.sums_longdouble(rows[r1], None if r1 == r2 else rows[r2], good[g], lagmax, 1, 0, lags)
        assert np.array_equal(hits[p, 0][lags], want_hits), p
        worst = max(worst, nc.sums_distance(sums[p, 0][lags], ld, norm))
    print(f"n {n}, lagmax {lagmax}, three pairs: worst distance {worst:.3e} at {lags.size} lags; bound {SUMS_BOUND:.3e}")
    assert worst <= SUMS_BOUND
    # the same bits: again, in batches of 1 and 2, and with the pairs in another order
    for kw in (dict(), dict(max_batch=1), dict(max_batch=2)):
        again = device_sums(rows, good, pairs, segments, 1, lagmax, 0, **kw)
        assert np.array_equal(again[0], sums) and np.array_equal(again[1], hits), kw
    order = [2, 0, 1]
    shuffled = device_sums(rows, good, [pairs[i] for i in order], segments, 1, lagmax, 0, max_batch=2)
    assert np.array_equal(shuffled[0], sums[order]) and np.array_equal(shuffled[1], hits[order])


def test_device_sums_several_lag_tiles():
    """lagmax 4500 = three lag tiles of 2048 over three 8192-sample chunks: an auto pair, a symmetric cross pair, a
    segment without all_sums; long double at lags on both sides of 2048 and 4096, at the ends and every 97th."""
    n, lagmax = 20000, 4500
    rows = np.vstack([nc.signal(8300 + i, n) for i in range(3)])
    good = np.vstack([nc.good_mask("random", 8300, n, lagmax), nc.good_mask("gap", 8301, n, lagmax)])
    pairs = [(0, 0, 0), (0, 1, 1), (2, 1, 0)]
    segments = [(0, 9000, 0, 0), (9000, n, 1, 0)]
    sums, hits = device_sums(rows, good, pairs, segments, 1, lagmax, 1)
    lags = np.unique(np.concatenate([np.arange(0, lagmax, 97), [1, 7, 8, 2039, 2040, 2046, 2047, 2048, 2049, 2055, 2056,
                                                                  4094, 4095, 4096, 4097, 4103, 4104, lagmax - 2,
                                                                  lagmax - 1]]))
    worst = 0.0
    for p, (r1, r2, g) in enumerate(pairs):
        want, norm, want_hits = np.zeros(lags.size, dtype=nc.L), np.zeros(lags.size), np.zeros(lags.size, dtype=np.int64)
        for first, last, all_sums, _ in segments:
            s, m, h = nc.sums_longdouble(rows[r1][first:last], None if r1 == r2 else rows[r2][first:last],
                                         good[g][first:last], lagmax, all_sums, 1, lags)
            want += s
            norm += m
            want_hits += h
        assert np.array_equal(hits[p, 0][lags], want_hits), p
        worst = max(worst, nc.sums_distance(sums[p, 0][lags], want, norm))
    # lags in the last tile past lagmax do not exist; the first segment (all_sums = 0, 9000 - 4500 samples) and the
    # second give every lag hits
    assert np.all(hits[:, 0, :] > 0)
    print(f"n {n}, lagmax {lagmax} (three lag tiles), three pairs, symmetric: worst distance {worst:.3e} at {lags.size} "
          f"lags; bound {SUMS_BOUND:.3e}")
    assert worst <= SUMS_BOUND
    for kw in (dict(), dict(max_batch=1), dict(max_batch=2)):
        again = device_sums(rows, good, pairs, segments, 1, lagmax, 1, **kw)
        assert np.array_equal(again[0], sums) and np.array_equal(again[1], hits), kw
    order = [2, 0, 1]
    shuffled = device_sums(rows, good, [pairs[i] for i in order], segments, 1, lagmax, 1, max_batch=2)
    assert np.array_equal(shuffled[0], sums[order]) and np.array_equal(shuffled[1], hits[order])


def test_device_sums_argument_checks():
    rows, good = np.zeros((2, 100)), np.ones((1, 100), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="outside the data"):
        device_sums(rows, good, [(0, 2, 0)], [(0, 100, 1, 0)], 1, 10, 0)
    with pytest.raises(RuntimeError, match="outside the flags"):
        device_sums(rows, good, [(0, 1, 1)], [(0, 100, 1, 0)], 1, 10, 0)
    with pytest.raises(RuntimeError, match="outside the rows"):
        device_sums(rows, good, [(0, 1, 0)], [(0, 101, 1, 0)], 1, 10, 0)
    with pytest.raises(RuntimeError, match="realization"):
        device_sums(rows, good, [(0, 1, 0)], [(0, 100, 1, 1)], 1, 10, 0)


def device_highpass(x, good, window):
    from toast_amd import capi

    d_x, d_g, d_out = Dev(np.atleast_2d(x)), Dev(np.atleast_2d(good)), Dev(np.full((1, x.size), np.nan))
    capi.dev.noise_estim_highpass(x.size, window, d_x.ptr, 1, x.size, [0], d_g.ptr, 1, x.size, [0], d_out.ptr, x.size)
    capi.synchronize()
    out, after = d_out.get()[0], d_x.get()[0]
    for d in (d_x, d_g, d_out):
        d.free()
    assert np.array_equal(after, x)          # the input row is not modified
    return out


def test_device_highpass():
    worst = 0.0
    cases = [(1000, w, fk, 0.0) for w in (1, 2, 100, 101, 3000) for fk in nc.FLAG_KINDS]
    cases += [(4099, 100, "random", 1.0e6), (9000, 101, "random", 1.0e6), (9000, 8999, "gap", 0.0)]
    # a long row with a large offset: a global prefix sum in double reaches 2.6e11 here and misses the bound
    cases += [(262144, 10001, "random", 1.0e6)]
    for n, w, fk, off in cases:
        x, good = nc.trend_inputs(f"{n}_{w}_{fk}", n, w, fk, off)
        got = device_highpass(x, good, w)
        if fk == "all":
            assert np.all(got == 0), (n, w)
            continue
        ld, _ = nc.trend_longdouble(x, good, w)
        dist = float(np.max(np.abs(got.astype(nc.L) - (x.astype(nc.L) - ld)))) / nc.row_rms(x)
        worst = max(worst, dist)
        if off or w > n:
            print(f"high-pass n {n}, window {w}, flags {fk}, offset {off:g}: {dist:.3e} of the rms; bound {TREND_BOUND:.3e}")
    print(f"high-pass, {len(cases)} rows: worst distance {worst:.3e} of the rms; bound {TREND_BOUND:.3e}")
    assert worst <= TREND_BOUND


@pytest.mark.parametrize("name", sorted(nc.OP_CASES))
def test_operator_on_resident_data(name):
    from toast_amd.data import defaults

    before = nc.make_obs(name).obs[0]
    data, model = nc.estimate(name, resident=True, max_batch=2)
    ob = data.obs[0]
    assert ob.detdata[defaults.det_data].accel_in_use()          # the path followed the data
    dist = nc.psd_distance(model, G, name)
    print(f"NoiseEstim on resident data, case {name}: {dist:.3e} of max |PSD|; bound {PSD_BOUND:.3e}")
    assert dist <= PSD_BOUND
    assert np.array_equal(ob.detdata[defaults.det_flags].data, before.detdata[defaults.det_flags].data)
    assert np.array_equal(ob.shared[defaults.shared_flags].data, before.shared[defaults.shared_flags].data)
    if not nc.OP_CASES[name]["op"].get("remove_common_mode"):
        # (removing the common mode rewrites det_data, as in the reference, and leaves the flags resident)
        assert np.array_equal(ob.detdata[defaults.det_data].data, before.detdata[defaults.det_data].data)
        assert not ob.detdata[defaults.det_flags].accel_exists()      # the temporary upload of the flags is gone


@pytest.mark.parametrize("name", nc.DEVICE_ONLY_CASES)
def test_operator_host_sums_after_device_preprocessing(name):
    """The cases the host tests cannot run (CommonModeFilter works on the device only), with high-pass and sums on the
    host entries."""
    _, model = nc.estimate(name, use_accel=False)
    dist = nc.psd_distance(model, G, name)
    print(f"NoiseEstim host sums, case {name}: {dist:.3e} of max |PSD|; bound {PSD_BOUND:.3e}")
    assert dist <= PSD_BOUND


def test_common_mode_removal_on_device():
    """focalplane_key with remove_common_mode goes through Copy / CommonModeFilter / Combine: the estimate equals the one
    on data from which the same operators removed the common mode beforehand."""
    from toast_amd import ops
    from toast_amd.data import defaults

    kw = dict(nc.OP_CASES["common"]["op"])
    data = nc.make_obs("common")
    ops.NoiseEstim(out_model="a", remove_common_mode=True, **kw).apply(data, use_accel=True)
    other = nc.make_obs("common")
    ops.Copy(detdata=[(defaults.det_data, "temp_signal")]).apply(other)
    other.obs[0].detdata["temp_signal"].update_units(other.obs[0].detdata[defaults.det_data].units)
    ops.CommonModeFilter(det_data="temp_signal", det_mask=1, det_flags=defaults.det_flags, det_flag_mask=1,
                         focalplane_key="wafer").apply(other)
    ops.Combine(op="subtract", first=defaults.det_data, second="temp_signal", result=defaults.det_data).apply(other)
    ops.NoiseEstim(out_model="b", **kw).apply(other, use_accel=True)
    a, b = data.obs[0]["a"], other.obs[0]["b"]
    assert a.keys == b.keys and "temp_signal" not in data.obs[0].detdata
    for k in a.keys:
        assert np.array_equal(a.psd(k), b.psd(k)), k
    plain = nc.estimate("common", use_accel=True)[1]
    assert any(not np.array_equal(a.psd(k), plain.psd(k)) for k in a.keys)


def test_white_noise_recovery():
    """SimNoise white noise, 8 detectors x 2^16 samples, through NoiseEstim on the device: the mean PSD over the upper
    half band against NET^2 within 5 * 2 / sqrt(n) (n / 4 independent modes at 5 sigma, 3.9 %).  A 1/f case is printed."""
    import sim_noise_case as sc
    from toast_amd import ops

    n = 1 << 16
    bound = 5.0 * 2.0 / np.sqrt(n)
    for fknee in (0.0, 1.0):
        data = sc.make_data(n_det=8, n_samp=n, rate=100.0, fknee=fknee, net=1.0)
        ops.SimNoise().apply(data, use_accel=True)
        ops.NoiseEstim(out_model="measured", lagmax=1024, nbin_psd=64, det_flags=None, shared_flags=None).apply(data)
        model, truth = data.obs[0]["measured"], data.obs[0]["noise_model"]
        for det in model.keys:
            f, p = model.freq(det), model.psd(det)
            want = np.interp(f, truth.freq(det), truth.psd(det))
            ratio = float(np.mean(p[f > 25.0] / want[f > 25.0]))
            print(f"fknee {fknee:g} {det}: estimated / input PSD over the upper half band {ratio:.4f}; bound 1 +- {bound:.4f}")
            if fknee == 0.0:
                assert abs(ratio - 1.0) <= bound, det
