"""GPU: the polynomial and common-mode filter kernels (csrc/poly_filter.hip) and ops.PolyFilter /
ops.CommonModeFilter against the reference's own kernel outputs (tests/golden/poly_filter.npz), the host restatement
of the compiled kernel (tests/poly_filter_host.py) and the reference's operator tests
(src/toast/tests/ops_polyfilter.py).

Tolerance of the polynomial filter: 1e-12 * max|input signal| for orders <= 8 -- a plain fp64 normal-equations
solve in the Legendre basis agrees with the reference's SVD solve to 3e-14 on scans with at least half of their
samples good (measured on the host), times 30 for a different summation order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import poly_filter_host as H
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.sim import create_ground_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
SINGLE, TWO_PASS = 1, 2


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(gu.GOLDEN, "poly_filter.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_poly(order, signal, sig_index, det_flags, flag_index, det_mask, shared, shared_mask, starts, stops, path=0):
    """filter_polynomial_dev on host arrays; returns (filtered buffer, coeff, status)."""
    import torch

    from toast_amd import capi

    d_s = dev(signal)
    d_f = dev(det_flags) if det_flags is not None else None
    d_sh = dev(shared) if shared is not None else None
    n_det, n_iv = len(sig_index), len(starts)
    coeff = torch.full((n_det, n_iv, order + 1), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((n_det, n_iv), -1, dtype=torch.int32, device="cuda")
    capi.dev.filter_polynomial(order, signal.shape[1], sig_index, d_s.data_ptr(), flag_index,
                               d_f.data_ptr() if d_f is not None else 0, det_mask,
                               d_sh.data_ptr() if d_sh is not None else 0, shared_mask, starts, stops, coeff.data_ptr(),
                               status.data_ptr(), path=path)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), coeff.cpu().numpy(), status.cpu().numpy()


def host_poly(order, signal, sig_index, det_flags, flag_index, det_mask, shared, shared_mask, starts, stops):
    want = signal.copy()
    coeff = np.zeros((len(sig_index), len(starts), order + 1))
    status = np.zeros((len(sig_index), len(starts)), dtype=np.int32)
    for k, row in enumerate(sig_index):
        fl = H.combined_flags(shared, shared_mask, det_flags[flag_index[k]] if det_flags is not None else None, det_mask) \
            if (shared is not None or det_flags is not None) else np.zeros(signal.shape[1], dtype=np.uint8)
        coeff[k], status[k] = H.filter_polynomial(order, fl, want[row], starts, stops)
    return want, coeff, status


@pytest.mark.parametrize("path", [SINGLE, TWO_PASS])
def test_filter_polynomial_vs_reference_fixture(golden, path):
    g = golden
    for i in range(int(g["n_poly_cases"])):
        order, n_det, n_samp = int(g[f"p{i}_order"]), int(g[f"p{i}_n_det"]), int(g[f"p{i}_n_samp"])
        starts, stops, flags, want = g[f"p{i}_starts"], g[f"p{i}_stops"], g[f"p{i}_flags"], g[f"p{i}_out"]
        signals = H.poly_case_signals(int(g[f"p{i}_seed"]), n_det, n_samp)
        # rows permuted inside larger buffers; the flags split into shared bits (common to all rows) and detector bits
        n_rows = n_det + 3
        rows = np.random.default_rng(i).permutation(n_rows)[:n_det].astype(np.int32)
        frows = np.array([(n_det - 1 - k) for k in range(n_det)], dtype=np.int32)
        buf = np.full((n_rows, n_samp), 7.25)
        buf[rows] = signals
        common = np.all(flags != 0, axis=0)
        shared = np.where(common, 16, 0).astype(np.uint8) | 2          # bit 2 is outside the mask
        fbuf = np.zeros((n_det, n_samp), dtype=np.uint8)
        fbuf[frows] = np.where(common[None, :], 0, flags) | 64          # bit 64 is outside the mask
        got, coeff, status = run_poly(order, buf, rows, fbuf, frows, 7, shared, 16, starts, stops, path=path)
        scale = np.max(np.abs(signals))
        err = np.max(np.abs(got[rows] - want)) / scale
        print(f"order {order} path {path}: max |device - reference| = {err:.2e} of max|signal|")
        assert err < TOL
        # untouched samples are bit-identical: outside the intervals, the all-flagged interval, the rows not listed
        outside = np.ones(n_samp, dtype=bool)
        for a, b in zip(starts, stops):
            outside[a:b] = False
        assert np.array_equal(got[rows][:, outside], signals[:, outside])
        dead = int(g[f"p{i}_dead"])
        assert np.array_equal(got[rows][:, starts[dead]:stops[dead]], signals[:, starts[dead]:stops[dead]])
        others = np.setdiff1d(np.arange(n_rows), rows)
        assert np.all(got[others] == 7.25)
        want_status = np.zeros((n_det, len(starts)), dtype=np.int32)
        want_status[:, dead] = H.NO_GOOD
        assert np.array_equal(status, want_status)
        ref_coeff = g[f"p{i}_coeff"]
        assert np.max(np.abs(coeff - ref_coeff)) < 1e-9 * scale
        assert np.all(coeff[:, dead] == 0)


def compare_with_host(order, signal, sig_index, det_flags, flag_index, det_mask, shared, shared_mask, starts, stops, path=0):
    got, coeff, status = run_poly(order, signal, sig_index, det_flags, flag_index, det_mask, shared, shared_mask, starts,
                                  stops, path=path)
    want, wcoeff, wstatus = host_poly(order, signal, sig_index, det_flags, flag_index, det_mask, shared, shared_mask, starts,
                                      stops)
    err = np.max(np.abs(got - want)) / np.max(np.abs(signal))
    print(f"order {order} path {path}: max |device - host restatement| = {err:.2e} of max|signal|")
    assert err < TOL
    assert np.array_equal(status, wstatus)
    return got, coeff, status


def flags_half_good(rng, shape, frac=0.1):
    return (rng.random(shape) < frac).astype(np.uint8)


def test_lengths_the_reference_arange_cannot_hold():
    def arange_fails(length):
        return np.arange(start=1.0 / length - 1.0, stop=1.0 / length + 1.0, step=2.0 / length).size != length

    lengths = [n for n in range(50, 4000) if arange_fails(n)][:40]
    assert len(lengths) == 40
    rng = np.random.default_rng(3)
    starts = np.cumsum([5] + [n + 3 for n in lengths[:-1]]).astype(np.int64)
    stops = starts + np.array(lengths)
    n_samp = int(stops[-1]) + 9
    sig = 2.0e3 + rng.standard_normal((3, n_samp))
    fl = flags_half_good(rng, (3, n_samp))
    sh = flags_half_good(rng, n_samp, 0.05)
    for path in (SINGLE, TWO_PASS):
        compare_with_host(3, sig, [0, 1, 2], fl, [0, 1, 2], 1, sh, 1, starts, stops, path=path)


def test_long_interval_takes_the_two_pass_path_by_the_rule():
    from toast_amd import capi

    rng = np.random.default_rng(4)
    n_samp = 100000 + 77
    assert 100000 > capi.dev.filter_polynomial_stage_cap()
    sig = 1.5e3 + rng.standard_normal((2, n_samp)) + 3.0 * np.linspace(-1, 1, n_samp) ** 3
    fl = flags_half_good(rng, (2, n_samp))
    sh = flags_half_good(rng, n_samp, 0.05)
    # one long interval (two passes) next to a short one (single pass), both in one call, path by the rule
    starts, stops = np.array([31, 100040], dtype=np.int64), np.array([100031, 100070], dtype=np.int64)
    got, _, _ = compare_with_host(5, sig, [1, 0], fl, [0, 1], 1, sh, 1, starts, stops, path=0)
    forced, _, _ = run_poly(5, sig, [1, 0], fl, [0, 1], 1, sh, 1, starts, stops, path=TWO_PASS)
    assert np.array_equal(got[:, 31:100031], forced[:, 31:100031])
    # forcing the single pass on an interval that cannot be staged is an error, not a silently wrong result
    with pytest.raises(RuntimeError, match="single-pass"):
        run_poly(5, sig, [1, 0], fl, [0, 1], 1, sh, 1, starts, stops, path=SINGLE)


def test_more_workgroups_than_cus_odd_starts_and_null_flags():
    rng = np.random.default_rng(5)
    n_iv, n_det = 300, 64
    lengths = rng.integers(40, 200, n_iv)
    gaps = rng.integers(0, 4, n_iv)
    starts = (np.cumsum(lengths + gaps) - lengths - gaps + 1).astype(np.int64)     # odd and even starts
    stops = starts + lengths
    assert np.any(starts % 2 == 1) and np.any(starts % 2 == 0) and np.any(starts % 16 != 0)
    n_samp = int(stops[-1]) + 5           # odd row length: rows alternate between 16-byte alignments
    if n_samp % 2 == 0:
        n_samp += 1
    sig = 3.0e3 + rng.standard_normal((n_det, n_samp))
    fl = flags_half_good(rng, (n_det, n_samp))
    sh = flags_half_good(rng, n_samp, 0.05)
    idx = rng.permutation(n_det).astype(np.int32)
    for path in (SINGLE, TWO_PASS):
        compare_with_host(3, sig, idx, fl, idx[::-1].copy(), 1, sh, 1, starts, stops, path=path)
    compare_with_host(1, sig, idx, None, None, 1, sh, 1, starts, stops)            # NULL detector flags
    compare_with_host(5, sig, idx, fl, idx, 1, None, 1, starts, stops)             # NULL shared flags
    compare_with_host(2, sig, idx, None, None, 1, None, 1, starts, stops)          # no flags at all


def test_order_limits():
    rng = np.random.default_rng(6)
    sig = 1.0e3 + rng.standard_normal((2, 3000))
    starts, stops = np.array([0, 1500], dtype=np.int64), np.array([1400, 3000], dtype=np.int64)
    # 16 terms are supported.  The bound: normal equations against the SVD solve agree to 2e-11 at order 12 and 2e-12 at
    # order 16 on such scans (measured on the host); the larger figure times the same factor 30 as for the low orders.
    got, _, status = run_poly(15, sig, [0, 1], None, None, 0, None, 0, starts, stops)
    want, _, _ = host_poly(15, sig, [0, 1], None, None, 0, None, 0, starts, stops)
    assert np.max(np.abs(got - want)) < 6e-10 * np.max(np.abs(sig)) and np.all(status == 0)
    with pytest.raises(RuntimeError, match="at most 16"):
        run_poly(16, sig, [0, 1], None, None, 0, None, 0, starts, stops)
    same, _, _ = run_poly(-1, sig, [0, 1], None, None, 0, None, 0, starts, stops)      # order < 0: no-op
    assert np.array_equal(same, sig)


@pytest.mark.parametrize("path", [SINGLE, TWO_PASS])
@pytest.mark.parametrize("ngood", [1, 2, 3])
def test_degenerate_intervals_lower_the_order(path, ngood):
    rng = np.random.default_rng(10 + ngood)
    n, order = 400, 5
    sig = 50.0 + 10.0 * rng.standard_normal((1, n))
    fl = np.ones((1, n), dtype=np.uint8)
    good = np.sort(rng.choice(np.arange(20, 380), ngood, replace=False))
    fl[0, good] = 0
    starts, stops = np.array([10], dtype=np.int64), np.array([390], dtype=np.int64)
    got, coeff, status = run_poly(order, sig, [0], fl, [0], 1, None, 0, starts, stops, path=path)
    scale = np.max(np.abs(sig))
    assert status[0, 0] == (H.REDUCED)
    assert np.max(np.abs(got[0, good])) < 1e-9 * scale
    assert np.all(coeff[0, 0, ngood:] == 0) and np.all(coeff[0, 0, :ngood] != 0)
    # flagged samples: the signal minus the degree ngood - 1 interpolant of the good ones
    x = (0.5 * (2.0 / 380) - 1) + np.arange(380) * (2.0 / 380)
    poly = np.polyfit(x[good - 10], sig[0, good], ngood - 1)
    want = sig[0, 10:390] - np.polyval(poly, x)
    assert np.max(np.abs(got[0, 10:390] - want)) < 1e-9 * scale
    assert np.array_equal(got[0, :10], sig[0, :10]) and np.array_equal(got[0, 390:], sig[0, 390:])


@pytest.mark.parametrize("path", [SINGLE, TWO_PASS])
def test_two_runs_are_bit_identical(path):
    import torch

    from toast_amd import capi

    rng = np.random.default_rng(8)
    n_det, n_samp = 48, 60000
    sig = 2.0e3 + rng.standard_normal((n_det, n_samp))
    fl = flags_half_good(rng, (n_det, n_samp))
    starts = np.arange(0, n_samp - 3000, 3000, dtype=np.int64) + 7
    stops = starts + 2950
    idx = np.arange(n_det, dtype=np.int32)
    d_f = dev(fl)
    outs = []
    for _ in range(2):
        d_s = dev(sig)
        coeff = torch.zeros((n_det, starts.size, 6), dtype=torch.float64, device="cuda")
        status = torch.zeros((n_det, starts.size), dtype=torch.int32, device="cuda")
        capi.dev.filter_polynomial(5, n_samp, idx, d_s.data_ptr(), idx, d_f.data_ptr(), 1, 0, 0, starts, stops,
                                   coeff.data_ptr(), status.data_ptr(), path=path)
        torch.cuda.synchronize()
        outs.append((d_s, coeff))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def cm_inputs(g):
    n_rows, n_samp = int(g["cm_n_rows"]), g["cm_shared"].size
    return H.common_mode_signals(int(g["cm_seed"]), n_rows, n_samp), n_samp


def test_common_mode_kernels_bit_identical_to_the_reference(golden):
    import torch

    from toast_amd import capi

    g = golden
    signals, n = cm_inputs(g)
    di, fi = g["cm_det_index"], g["cm_flag_index"]
    smask, dmask = int(g["cm_shared_mask"]), int(g["cm_det_mask"])
    want = signals.copy()
    want[di] -= g["cm_mean"][None, :]
    d_f, d_sh = dev(g["cm_det_flags"]), dev(g["cm_shared"])
    # the separate pair
    d_s = dev(signals)
    total = torch.zeros(n, dtype=torch.float64, device="cuda")
    hits = torch.zeros(n, dtype=torch.int64, device="cuda")
    capi.dev.sum_detectors(n, di, d_s.data_ptr(), fi, d_f.data_ptr(), dmask, d_sh.data_ptr(), smask, total.data_ptr(),
                           hits.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(total.cpu().numpy(), g["cm_sum"]) and np.array_equal(hits.cpu().numpy(), g["cm_hits"])
    assert np.array_equal(d_s.cpu().numpy(), signals)
    capi.dev.subtract_mean(n, di, d_s.data_ptr(), total.data_ptr(), hits.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(total.cpu().numpy(), g["cm_mean"])
    assert np.array_equal(d_s.cpu().numpy(), want)
    assert int(hits[int(g["cm_nobody"])]) == 0
    # the fused form, with and without the optional outputs
    d_s = dev(signals)
    mean = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hits2 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    capi.dev.common_mode_subtract(n, di, d_s.data_ptr(), fi, d_f.data_ptr(), dmask, d_sh.data_ptr(), smask, mean.data_ptr(),
                                  hits2.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(mean.cpu().numpy(), g["cm_mean"]) and np.array_equal(hits2.cpu().numpy(), g["cm_hits"])
    assert np.array_equal(d_s.cpu().numpy(), want)
    d_s = dev(signals)
    capi.dev.common_mode_subtract(n, di, d_s.data_ptr(), fi, d_f.data_ptr(), dmask, d_sh.data_ptr(), smask)
    torch.cuda.synchronize()
    assert np.array_equal(d_s.cpu().numpy(), want)


def test_host_signature_entries(golden):
    """_libtoast_hip.filter_polynomial / sum_detectors / subtract_mean with the reference's arguments."""
    from toast_amd import _libtoast_hip as lt

    g = golden
    signals, n = cm_inputs(g)
    total, hits = np.zeros(n), np.zeros(n, dtype=np.int64)
    work = signals.copy()
    lt.sum_detectors(g["cm_det_index"], g["cm_flag_index"], g["cm_shared"], int(g["cm_shared_mask"]), work, g["cm_det_flags"],
                     int(g["cm_det_mask"]), total, hits)
    assert np.array_equal(total, g["cm_sum"]) and np.array_equal(hits, g["cm_hits"])
    lt.subtract_mean(g["cm_det_index"], work, total, hits)
    want = signals.copy()
    want[g["cm_det_index"]] -= g["cm_mean"][None, :]
    assert np.array_equal(total, g["cm_mean"]) and np.array_equal(work, want)
    i = 2
    n_det, n_samp = int(g[f"p{i}_n_det"]), int(g[f"p{i}_n_samp"])
    sig = H.poly_case_signals(int(g[f"p{i}_seed"]), n_det, n_samp)
    flags = g[f"p{i}_flags"]
    # two signals sharing detector 0's flags, like the reference's grouping
    rows = [sig[0].copy(), sig[0].copy() * 2.0]
    lt.filter_polynomial(int(g[f"p{i}_order"]), flags[0], rows, g[f"p{i}_starts"], g[f"p{i}_stops"], False)
    scale = np.max(np.abs(sig[0]))
    assert np.max(np.abs(rows[0] - g[f"p{i}_out"][0])) < TOL * scale
    assert np.max(np.abs(rows[1] - 2.0 * g[f"p{i}_out"][0])) < 2 * TOL * scale
    # use_accel=True: the signals are looked up in the memory manager and filtered where they are resident
    from toast_amd.accel import accel_data_create, accel_data_delete, accel_data_update_device, accel_data_update_host

    res = [sig[0].copy(), sig[0].copy() * 2.0]
    for k, arr in enumerate(res):
        accel_data_create(arr, f"sig{k}")
        accel_data_update_device(arr, f"sig{k}")
    lt.filter_polynomial(int(g[f"p{i}_order"]), flags[0], res, g[f"p{i}_starts"], g[f"p{i}_stops"], True)
    assert np.array_equal(res[0], sig[0])            # the host copies are untouched until they are fetched
    for k, arr in enumerate(res):
        accel_data_update_host(arr, f"sig{k}")
        accel_data_delete(arr, f"sig{k}")
    assert np.array_equal(res[0], rows[0]) and np.array_equal(res[1], rows[1])


def ground_data(n_det=6, n_samp=24000, n_obs=2, seed=0):
    data = create_ground_data(n_det=n_det, n_samp=n_samp, rate=20.0, n_obs=n_obs, seed=seed)
    for ob in data.obs:
        spans = [(int(iv.first), int(iv.last)) for iv in ob.intervals[defaults.scanning_interval]]
        ob.intervals.create("throw", spans)
    return data


def test_polyfilter_operator_vs_host_restatement():
    rng = np.random.default_rng(21)
    data = ground_data()
    for ob in data.obs:
        sig = ob.detdata[defaults.det_data].data
        sig[:] = 100.0 + rng.standard_normal(sig.shape)
        ob.detdata[defaults.det_flags].data[:, ::7] |= defaults.det_mask_processing
        ob.shared[defaults.shared_flags].data[100:140] |= defaults.shared_mask_irregular
    cut = data.obs[0].local_detectors[2]
    data.obs[0].update_local_detector_flags({cut: defaults.det_mask_invalid})
    before = {ob.name: ob.detdata[defaults.det_data].data.copy() for ob in data.obs}
    sflags = {ob.name: ob.shared[defaults.shared_flags].data.copy() for ob in data.obs}
    pf = ops.PolyFilter(order=3, pattern="D000.*", name="polyfilter")
    pf.apply(data)
    for ob in data.obs:
        starts = np.array([iv.first for iv in ob.intervals["throw"]])
        stops = np.array([iv.last for iv in ob.intervals["throw"]])
        dets = [d for d in ob.local_detectors if d.startswith("D000") and not (ob.name == data.obs[0].name and d == cut)]
        assert pf.filtered_detectors[ob.name] == dets
        want = before[ob.name].copy()
        for i, det in enumerate(ob.local_detectors):
            if det not in dets:
                continue
            fl = H.combined_flags(sflags[ob.name], pf.shared_flag_mask, ob.detdata[defaults.det_flags].data[i],
                                  pf.det_flag_mask)
            c, s = H.filter_polynomial(3, fl, want[i], starts, stops)
            k = dets.index(det)
            assert np.array_equal(pf.status[ob.name][k], s)
            assert np.max(np.abs(pf.coefficients[ob.name][k] - c)) < 1e-9 * 100.0
        got = ob.detdata[defaults.det_data].data
        assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(before[ob.name]))
        # samples outside the view carry poly_flag_mask, the others keep their flags
        outside = np.ones(ob.n_local_samples, dtype=bool)
        for a, b in zip(starts, stops):
            outside[a:b] = False
        now = ob.shared[defaults.shared_flags].data
        assert np.all(now[outside] & pf.poly_flag_mask) and np.array_equal(now[~outside], sflags[ob.name][~outside])
    with pytest.raises(RuntimeError, match="is not defined for observation"):
        ops.PolyFilter(view="nonexistent").apply(data)
    data.obs[0].detdata.create("single", dtype=np.float32)
    with pytest.raises(RuntimeError, match="float64"):
        ops.PolyFilter(det_data="single").apply(data)


def test_polyfilter_whole_observation_and_resident_data():
    """view=None is one interval (two-pass path by the rule); resident timestreams stay resident and the device copy of
    the shared flags follows the host."""
    rng = np.random.default_rng(22)
    data = ground_data(n_det=3, n_samp=30000, n_obs=1)
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data]
    sig.data[:] = 10.0 + rng.standard_normal(sig.data.shape)
    before = sig.data.copy()
    sig.accel_create(defaults.det_data)
    sig.accel_update_device()
    sf = ob.shared[defaults.shared_flags]
    sf.accel_create(defaults.shared_flags)
    sf.accel_update_device()
    shared_before = sf.data.copy()
    pf = ops.PolyFilter(order=2, view=None, name="polyfilter")
    pf.apply(data)
    assert sig.accel_in_use() and pf.status[ob.name].shape == (3, 1)
    want = before.copy()
    for i in range(3):
        fl = H.combined_flags(shared_before, pf.shared_flag_mask, ob.detdata[defaults.det_flags].data[i], pf.det_flag_mask)
        H.filter_polynomial(2, fl, want[i], [0], [ob.n_local_samples])
    assert np.max(np.abs(sig.data - want)) < TOL * np.max(np.abs(before))
    assert np.array_equal(sf.data, shared_before)       # nothing lies outside the whole observation
    pf2 = ops.PolyFilter(order=0, name="polyfilter2")   # the throw view: turnarounds get poly_flag_mask on both sides
    pf2.apply(data)
    host = sf.data.copy()
    from toast_amd.accel import accel_data_update_host

    probe = sf.data.copy()
    sf.data[:] = 0
    accel_data_update_host(sf.data, defaults.shared_flags)
    assert np.array_equal(sf.data, probe) and np.array_equal(host, probe)


def test_polyfilter_reference_operator_tests():
    """src/toast/tests/ops_polyfilter.py: test_polyfilter (:134) and test_polyfilter_trend (:233-239)."""
    rng = np.random.default_rng(23)
    data = ground_data(n_det=4, n_samp=24000, n_obs=1)
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data].data
    # a large per-scan linear trend, nothing else: the rms over the good samples falls by 1e-6
    for iv in ob.intervals["throw"]:
        n = iv.last - iv.first
        sig[:, iv.first:iv.last] = rng.uniform(-1e3, 1e3) + rng.uniform(0.5, 2.0) * 1e3 * np.linspace(-1, 1, n)[None, :]
    old = sig.copy()
    pf = ops.PolyFilter(order=1, name="polyfilter")
    pf.apply(data)
    new = ob.detdata[defaults.det_data].data
    sflags = ob.shared[defaults.shared_flags].data
    for i in range(4):
        good = ((sflags & pf.shared_flag_mask) == 0) & ((ob.detdata[defaults.det_flags].data[i] & pf.det_flag_mask) == 0)
        assert np.std(new[i][good]) / np.std(old[i][good]) < 1e-6
    # test_polyfilter_trend: noise plus a strong gradient, one interval; the rms falls below 1e-1 and the differenced
    # signal is the original's to 1e-3, across the flagged regions too
    data = ground_data(n_det=4, n_samp=24000, n_obs=1)
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data].data
    orig = rng.standard_normal(sig.shape)
    sig[:] = orig + ob.shared[defaults.times].data[None, :]
    old = sig.copy()
    ops.PolyFilter(order=1, det_flag_mask=defaults.det_mask_invalid, shared_flag_mask=defaults.shared_mask_invalid,
                   poly_flag_mask=1, view=None, name="polyfilter").apply(data)
    new = ob.detdata[defaults.det_data].data
    sflags = ob.shared[defaults.shared_flags].data
    for i in range(4):
        good = ((sflags & defaults.shared_mask_invalid) == 0) & \
            ((ob.detdata[defaults.det_flags].data[i] & defaults.det_mask_invalid) == 0)
        assert np.std(new[i][good]) / np.std(old[i][good]) < 1e-1
        assert np.std(np.diff(new[i]) - np.diff(orig[i])) / np.std(np.diff(orig[i])) < 1e-3


def cm_data(seed=0, n_det=8, n_samp=9000):
    rng = np.random.default_rng(seed)
    data = create_ground_data(n_det=n_det, n_samp=n_samp, rate=20.0, n_obs=1, seed=seed)
    ob = data.obs[0]
    fp = ob.telescope.focalplane
    for i, d in enumerate(ob.local_detectors):
        fp[d]["wafer"] = "W%d" % (i % 3)
    sig = ob.detdata[defaults.det_data].data
    sig[:] = rng.standard_normal(sig.shape) + 5.0 * np.sin(np.arange(n_samp) * 0.01)[None, :]
    ob.detdata[defaults.det_flags].data[:, 200:230] = defaults.det_mask_invalid      # samples nobody hits
    ob.update_local_detector_flags({ob.local_detectors[1]: defaults.det_mask_invalid})
    return data, ob


@pytest.mark.parametrize("key", [None, "wafer"])
def test_common_mode_operator_subtract(key):
    data, ob = cm_data(31)
    before = ob.detdata[defaults.det_data].data.copy()
    cm = ops.CommonModeFilter(focalplane_key=key, name="commonmode")
    cm.apply(data)
    want = before.copy()
    fp = ob.telescope.focalplane
    values = [None] if key is None else sorted({fp[d][key] for d in ob.local_detectors})
    dflags, sflags = ob.detdata[defaults.det_flags].data, ob.shared[defaults.shared_flags].data
    for value in values:
        rows = [i for i, d in enumerate(ob.local_detectors)
                if not (ob.local_detector_flags[d] & cm.det_mask) and (value is None or fp[d][key] == value)]
        total, hits = np.zeros(ob.n_local_samples), np.zeros(ob.n_local_samples, dtype=np.int64)
        H.sum_detectors(rows, rows, sflags, cm.shared_flag_mask, want, dflags, cm.det_flag_mask, total, hits)
        H.subtract_mean(rows, want, total, hits)
    got = ob.detdata[defaults.det_data].data
    assert np.array_equal(got, want)                      # the fixture-pinned summation order: bit-identical
    assert np.array_equal(got[1], before[1])              # the cut detector is not touched
    with pytest.raises(RuntimeError, match="batch mode"):
        cm.apply(data, detectors=ob.local_detectors[:2])
    for bad in ({"redistribute": True}, {"plot": True}):
        with pytest.raises(NotImplementedError):
            ops.CommonModeFilter(**bad).apply(data)


def test_common_mode_operator_regress_and_singular():
    data, ob = cm_data(32)
    before = ob.detdata[defaults.det_data].data.copy()
    cm = ops.CommonModeFilter(regress=True, name="commonmode")
    cm.apply(data)
    # NumPy transcription of polyfilter.py:943-970
    dflags, sflags = ob.detdata[defaults.det_flags].data, ob.shared[defaults.shared_flags].data
    rows = [i for i, d in enumerate(ob.local_detectors) if not (ob.local_detector_flags[d] & cm.det_mask)]
    template, hits = np.zeros(ob.n_local_samples), np.zeros(ob.n_local_samples, dtype=np.int64)
    want = before.copy()
    H.sum_detectors(rows, rows, sflags, cm.shared_flag_mask, want, dflags, cm.det_flag_mask, template, hits)
    good = hits != 0
    mean_template = template.copy()
    mean_template[good] /= hits[good]
    templates = np.vstack([np.ones(np.sum(good)), mean_template[good]])
    cov = np.linalg.inv(np.dot(templates, templates.T))
    for idet in rows:
        sig = want[idet]
        sig_copy = sig[good].copy()
        sig_copy[dflags[idet][good] & cm.det_flag_mask != 0] = 0
        coeff = np.dot(cov, np.dot(templates, sig_copy))
        sig -= coeff[0] + coeff[1] * mean_template
    got = ob.detdata[defaults.det_data].data
    assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(before))
    assert np.array_equal(got[1], before[1])
    # singular: every sample flagged -> no hits -> the 2 x 2 matrix is zero -> the group's detectors are flagged
    data, ob = cm_data(33, n_det=4, n_samp=3000)
    ob.shared[defaults.shared_flags].data[:] = defaults.shared_mask_invalid
    before = ob.detdata[defaults.det_data].data.copy()
    ops.CommonModeFilter(regress=True, name="commonmode").apply(data)
    assert np.array_equal(ob.detdata[defaults.det_data].data, before)
    for i, d in enumerate(ob.local_detectors):
        assert ob.local_detector_flags[d] == defaults.det_mask_invalid


def test_common_mode_reference_operator_test():
    """src/toast/tests/ops_polyfilter.py:469-540: a common signal injected into all detectors is gone afterwards."""
    rng = np.random.default_rng(34)
    data = create_ground_data(n_det=16, n_samp=12000, rate=20.0, n_obs=1, flag_samples=False)
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data].data
    sig[:] = 0.0
    common = 10.0 * rng.standard_normal(ob.n_local_samples)
    sig += common[None, :]
    old_rms = np.std(sig, axis=1)
    ops.CommonModeFilter(name="commonmode").apply(data)
    new = ob.detdata[defaults.det_data].data
    good = (ob.shared[defaults.shared_flags].data & defaults.shared_mask_invalid) == 0
    for i in range(16):
        assert np.std(new[i][good]) < 1e-3 * old_rms[i]


def test_workflow_with_both_filters(tmp_path):
    """The ground workflow with --polyfilter 3 --common-mode at a reduced size, each run a fresh child process with a
    time limit of its own; the map differs from the run without the options."""
    script = os.path.join(ROOT, "workflows", "ground_filter_mapmaker.py")
    base = [sys.executable, script, "--ndet", "8", "--minutes", "2", "--rate", "50", "--nside", "64", "--iter", "3"]
    maps = []
    for extra in ([], ["--polyfilter", "3", "--common-mode"]):
        out = str(tmp_path / ("map_%d.npy" % len(maps)))
        r = subprocess.run(base + extra + ["--save-map", out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("PolyFilter" in r.stdout) == bool(extra) and ("CommonModeFilter" in r.stdout) == bool(extra)
        maps.append(np.load(out))
    assert maps[0].shape == maps[1].shape and np.all(np.isfinite(maps[1]))
    assert np.max(np.abs(maps[0] - maps[1])) > 1e-3 * np.max(np.abs(maps[0]))
