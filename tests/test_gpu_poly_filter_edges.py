"""GPU: the polynomial filter where the templates are ill conditioned on the good samples, and every term count,
length edge, clip and common-mode row count of csrc/poly_filter.hip.

Conditioning (tests/golden/poly_filter_edges.npz, made by tests/golden/make_golden_poly_filter_edges.py): the good
samples of an interval form a contiguous stretch, as real flags do (a detector cut for most of a scan).  The truth is
a 120-digit least-squares solve on the double-precision templates; `ref_err_*` is how far the reference's own kernel
(double SVD) lands from it.  The device may be no further from the truth than max(1e-12, 4 x ref_err): 1e-12 is the
suite's bound for the filter, 4 x the project's convention for "no worse than four times the reference".  Cases whose
templates are rank deficient in double (cond >= 1e12) have no usable reference; there the bound is derived: a
least-squares fit of any order >= 0 leaves no more rms on the good samples than removing their mean does.

Everything else compares with the host restatement tests/poly_filter_host.py at the suite's bounds (1e-12 of
max|signal| up to order 8, 6e-10 for orders 9-15, as in test_gpu_poly_filter.py::test_order_limits)."""
import os

import numpy as np
import pytest

import golden_util as gu
import poly_filter_host as H
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.sim import create_ground_data

pytestmark = pytest.mark.gpu

TOL = 1e-12
TOL_HIGH = 6e-10          # orders 9-15
RULE, SINGLE, TWO_PASS = 0, 1, 2
GOOD, ALL, RANK = 1, 2, 4


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture(scope="module")
def edges():
    z = np.load(os.path.join(gu.GOLDEN, "poly_filter_edges.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def stage_cap():
    from toast_amd import capi

    cap = capi.dev.filter_polynomial_stage_cap()
    assert cap == 7424
    return cap


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


def random_flags(seed, shape, frac=0.1):
    return (H.hashed_uniform(seed, int(np.prod(shape))).reshape(shape) < frac).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("path", [RULE, SINGLE, TWO_PASS])
def test_contiguous_good_stretches_against_the_high_precision_truth(edges, stage_cap, path):
    g = edges
    smask, dmask = int(g["shared_mask"]), int(g["det_mask"])
    failures, n_run = [], 0
    for i in range(int(g["n_cases"])):
        c = {k[len(f"c{i}_"):]: g[k] for k in g if k.startswith(f"c{i}_")}
        order, cls, a, b, row = int(c["order"]), int(c["cls"]), int(c["start"]), int(c["stop"]), int(c["row"])
        if path == SINGLE and b - a > stage_cap:
            continue
        n_run += 1
        n_samp = int(c["n_samp"])
        buf = H.poly_case_signals(int(c["seed"]), 3, n_samp)
        fbuf = np.stack([np.full(n_samp, 7, dtype=np.uint8), c["det"]])      # row 0 is not the listed one
        args = (order, buf, [row], fbuf, [1], dmask, c["shared"], smask, np.array([a]), np.array([b]))
        got, coeff, status = run_poly(*args, path=path)
        again, coeff2, status2 = run_poly(*args, path=path)
        ok = H.combined_flags(c["shared"], smask, c["det"], dmask)[a:b] == 0
        scale = np.max(np.abs(buf[row, a:b]))
        tag = f"case {i} order {order} mask {int(c['mask'])} cond {float(c['cond']):.1e} path {path}"
        fin = np.isfinite(got[row, a:b])
        err = np.where(fin, np.abs(got[row, a:b] - c["truth"]), np.inf) / scale
        bound_good = max(TOL, 4 * float(c["ref_err_good"]))
        bound_all = max(TOL, 4 * float(c["ref_err_all"]))
        print(f"{tag}: status {int(status[0, 0])}, |device - truth| good {np.max(err[ok]):.1e} (bound {bound_good:.1e}, "
              f"reference {float(c['ref_err_good']):.1e}), all {np.max(err):.1e} (bound {bound_all:.1e}, reference "
              f"{float(c['ref_err_all']):.1e}), class {cls}")
        # every case
        if int(status[0, 0]) not in (H.FITTED, H.REDUCED):
            failures.append(f"{tag}: status {int(status[0, 0])}")
        others = [r for r in range(3) if r != row]
        if not (np.array_equal(got[row, :a], buf[row, :a]) and np.array_equal(got[row, b:], buf[row, b:])
                and np.array_equal(got[others], buf[others])):
            failures.append(f"{tag}: samples outside the interval or rows not listed changed")
        if not (np.array_equal(got, again, equal_nan=True) and np.array_equal(coeff, coeff2, equal_nan=True)
                and np.array_equal(status, status2)):
            failures.append(f"{tag}: two runs differ")
        if cls & GOOD and not np.max(err[ok]) <= bound_good:
            failures.append(f"{tag}: good samples {np.max(err[ok]):.1e} > {bound_good:.1e}")
        if cls & ALL and not np.max(err) <= bound_all:
            failures.append(f"{tag}: all samples {np.max(err):.1e} > {bound_all:.1e}")
        if cls & RANK:
            resid = got[row, a:b][ok]
            rms, rms_mean = np.sqrt(np.mean(resid ** 2)), np.std(buf[row, a:b][ok])
            print(f"{tag}: rms of the good-sample residual {rms:.4f}, about their own mean {rms_mean:.4f}")
            if not np.all(fin):
                failures.append(f"{tag}: output not finite")
            elif not rms <= (1 + 1e-9) * rms_mean:
                failures.append(f"{tag}: residual rms {rms:.3e} > {rms_mean:.3e} of mean removal")
    assert n_run >= int(g["n_cases"]) - 1
    print(f"path {path}: {len(failures)} failures in {n_run} cases")
    assert not failures, "\n".join(failures)


def test_polyfilter_operator_with_a_detector_cut_for_most_of_every_throw(edges):
    """ops.PolyFilter on resident data, order 5: one detector has only the first 10 % of each throw good.  Bound on its
    good samples: max(1e-12, 4 x e), e the distance of the host restatement -- the comparison target -- from the
    120-digit truth on exactly these inputs (`op_host_err_good` of the fixture)."""
    g = edges
    data = create_ground_data(**H.EDGE_OPERATOR_SIM)
    ob = data.obs[0]
    starts = np.array([iv.first for iv in ob.intervals["scanning"]], dtype=np.int64)
    stops = np.array([iv.last for iv in ob.intervals["scanning"]], dtype=np.int64)
    assert np.array_equal(starts, g["op_starts"]) and np.array_equal(stops, g["op_stops"])
    signal, det_flags = H.edge_operator_inputs(starts, stops, ob.n_local_samples)
    sig = ob.detdata[defaults.det_data]
    sig.data[:] = signal
    ob.detdata[defaults.det_flags].data[:] = det_flags
    shared = np.array(ob.shared[defaults.shared_flags].data)
    sig.accel_create(defaults.det_data)
    sig.accel_update_device()
    smask, dmask = H.EDGE_OPERATOR_MASKS
    pf = ops.PolyFilter(order=H.EDGE_OPERATOR_ORDER, view="scanning", shared_flag_mask=smask, det_flag_mask=dmask,
                        name="polyfilter")
    pf.apply(data)
    assert sig.accel_in_use()
    sig.accel_update_host()
    got = np.array(sig.data)
    sig.accel_delete()
    want = signal.copy()
    bound = max(TOL, 4 * float(g["op_host_err_good"]))
    for d in range(3):
        fl = H.combined_flags(shared, smask, det_flags[d], dmask)
        _, status = H.filter_polynomial(H.EDGE_OPERATOR_ORDER, fl, want[d], starts, stops)
        ok = np.zeros(ob.n_local_samples, dtype=bool)
        for a, b in zip(starts, stops):
            ok[a:b] = fl[a:b] == 0
        err = np.max(np.abs(got[d] - want[d])[ok]) / np.max(np.abs(signal[d]))
        this = bound if d == H.EDGE_OPERATOR_DET else TOL
        print(f"detector {d}: status {pf.status[ob.name][d].tolist()}, max |operator - host| on the good samples "
              f"{err:.2e} of max|signal| (bound {this:.1e})")
        assert np.all(pf.status[ob.name][d] == 0) and np.all(status == 0)
        assert err <= this
    assert np.all(np.isfinite(got))


# ------------------------------------------------------------------------------------------------ every term count
ORDER_N_SAMP = 10 + 700 + 13 + 5000 + 7 + 120 + 9
ORDER_STARTS = np.array([10, 723, 5730], dtype=np.int64)
ORDER_STOPS = np.array([710, 5723, 5850], dtype=np.int64)
_order_cache = {}


def order_inputs(order, flagged):
    """3 detectors, intervals of 700, 5000 and 120 samples.  Flagged: 10 % at random in the detector flags, 5 % in
    the shared ones; detector 0 keeps only (order + 1) // 2 evenly spread good samples in the last interval."""
    key = (order, flagged)
    if key not in _order_cache:
        sig = H.poly_case_signals(400 + order, 3, ORDER_N_SAMP)
        fl = sh = None
        if flagged:
            fl = random_flags(500 + order, (3, ORDER_N_SAMP)) * np.uint8(2)
            sh = random_flags(600 + order, (ORDER_N_SAMP,), 0.05)
            keep = (order + 1) // 2
            if keep > 0:
                fl[0, 5730:5850] = 2
                fl[0, np.linspace(5735, 5845, keep).astype(np.int64)] = 0
                sh[5730:5850] = 0
        host = host_poly(order, sig, [2, 0, 1], fl, [1, 2, 0] if flagged else None, 2, sh, 1, ORDER_STARTS, ORDER_STOPS)
        _order_cache[key] = (sig, fl, sh, host)
    return _order_cache[key]


@pytest.mark.parametrize("path", [SINGLE, TWO_PASS])
@pytest.mark.parametrize("order", range(16))
def test_every_order_on_both_paths(order, path):
    """Each instantiation (2, 4, 6, 9, 16 terms) with terms == N and terms < N, with flags and without."""
    tol = TOL if order <= 8 else TOL_HIGH
    for flagged in (True, False):
        sig, fl, sh, (want, wcoeff, wstatus) = order_inputs(order, flagged)
        rows, frows = [2, 0, 1], ([1, 2, 0] if flagged else None)
        got, coeff, status = run_poly(order, sig, rows, fl, frows, 2, sh, 1, ORDER_STARTS, ORDER_STOPS, path=path)
        scale = np.max(np.abs(sig))
        reduced = flagged and (order + 1) // 2 > 0
        cmp = np.ones(sig.shape, dtype=bool)
        if reduced:
            # detector 0's flags belong to signal row 1 (flag_index 0 is third in the list)
            cmp[1, 5730:5850] = False
        err = np.max(np.abs(got - want)[cmp]) / scale
        print(f"order {order} path {path} flagged {flagged}: max |device - host| = {err:.2e} of max|signal|")
        assert err < tol
        assert np.array_equal(status, wstatus)
        well = np.ones(status.shape, dtype=bool)
        if reduced:
            keep = (order + 1) // 2
            good = np.linspace(5735, 5845, keep).astype(np.int64)
            assert status[2, 2] == H.REDUCED and np.all(coeff[2, 2, keep:] == 0)
            assert np.max(np.abs(got[1, good])) < 1e-9 * scale
            well[2, 2] = False
        assert np.all(status[well] == H.FITTED)
        cerr = np.max(np.abs(coeff - wcoeff)[well]) / scale
        print(f"order {order} path {path} flagged {flagged}: max coefficient difference {cerr:.2e} of max|signal|")
        assert cerr < 1e-9
        assert np.all(np.isfinite(coeff)) and coeff.shape[2] == order + 1


def test_order_zero_to_fifteen_leave_nothing_beyond_the_fitted_order():
    """Fewer good samples than terms at every order: the coefficients beyond the fitted order are exactly zero."""
    n = 300
    sig = H.poly_case_signals(450, 1, n)
    for order in range(1, 16):
        for ngood in sorted({1, (order + 1) // 2, order}):
            fl = np.ones((1, n), dtype=np.uint8)
            good = np.linspace(20, 280, ngood).astype(np.int64)
            fl[0, good] = 0
            for path in (SINGLE, TWO_PASS):
                got, coeff, status = run_poly(order, sig, [0], fl, [0], 1, None, 0, np.array([5]), np.array([295]), path=path)
                assert status[0, 0] == H.REDUCED
                assert np.all(coeff[0, 0, ngood:] == 0) and np.all(np.isfinite(coeff))
                assert np.max(np.abs(got[0, good])) < 1e-9 * np.max(np.abs(sig))


# ------------------------------------------------------------------------------------------------ lengths
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 7423, 7424, 7425, 8191, 8192, 8193, 12289]


def length_layout(lengths):
    gaps = [3 + (k % 4) for k in range(len(lengths))]                 # odd and even starts
    starts = np.cumsum([2] + [n + gp for n, gp in zip(lengths[:-1], gaps[:-1])]).astype(np.int64)
    stops = starts + np.array(lengths)
    return starts, stops, int(stops[-1]) + 11


@pytest.mark.parametrize("flagged", [True, False])
def test_length_edges_at_order_three(stage_cap, flagged):
    """All the intervals of one path in a single call: every interval carries its own row of status and coefficients."""
    starts, stops, n_samp = length_layout(LENGTHS)
    sig = H.poly_case_signals(470, 2, n_samp)
    fl = random_flags(471, (2, n_samp)) if flagged else None
    sh = random_flags(472, (n_samp,), 0.05) if flagged else None
    fidx = [1, 0] if flagged else None
    want, wcoeff, wstatus = host_poly(3, sig, [0, 1], fl, fidx, 1, sh, 1, starts, stops)
    scale = np.max(np.abs(sig))
    if not flagged:
        assert np.all(wstatus[:, :3] == H.REDUCED) and np.all(wstatus[:, 3:] == H.FITTED)
    short = np.array(LENGTHS) <= stage_cap
    assert LENGTHS[int(np.count_nonzero(short)) - 1] == stage_cap and LENGTHS[int(np.count_nonzero(short))] == stage_cap + 1
    outs = {}
    for path, sel in ((SINGLE, short), (TWO_PASS, np.ones(len(LENGTHS), dtype=bool)), (RULE, np.ones(len(LENGTHS), dtype=bool))):
        got, coeff, status = run_poly(3, sig, [0, 1], fl, fidx, 1, sh, 1, starts[sel], stops[sel], path=path)
        outs[path] = got
        touched = np.zeros(n_samp, dtype=bool)
        for a, b in zip(starts[sel], stops[sel]):
            touched[a:b] = True
        err = np.max(np.abs(got - want)[:, touched]) / scale
        print(f"path {path} flagged {flagged}: {int(np.count_nonzero(sel))} lengths, max |device - host| = {err:.2e}")
        assert err < TOL
        assert np.array_equal(got[:, ~touched], sig[:, ~touched])
        assert np.array_equal(status, wstatus[:, sel])
        fitted = status == H.FITTED
        assert np.max(np.abs(coeff - wcoeff[:, sel])[fitted]) < 1e-9 * scale
        assert np.all(coeff[status == H.NO_GOOD] == 0)
    # the rule: up to the stage cap the single pass, beyond it the two passes
    for k, (a, b) in enumerate(zip(starts, stops)):
        chosen = SINGLE if LENGTHS[k] <= stage_cap else TWO_PASS
        assert np.array_equal(outs[RULE][:, a:b], outs[chosen][:, a:b]), LENGTHS[k]
    with pytest.raises(RuntimeError, match="single-pass"):
        run_poly(3, sig, [0, 1], fl, fidx, 1, sh, 1, starts[~short][:1], stops[~short][:1], path=SINGLE)


def test_chunk_bookkeeping_between_single_pass_jobs():
    """Two-pass jobs of 2-5 chunks interleaved with single-pass jobs in one call by the rule: the same bits as the
    intervals filtered one call each."""
    lengths = [9000, 300, 20000, 7424, 8193]
    starts, stops, n_samp = length_layout(lengths)
    n_det = 5
    sig = H.poly_case_signals(480, n_det, n_samp)
    fl = random_flags(481, (n_det, n_samp))
    sh = random_flags(482, (n_samp,), 0.05)
    rows = [3, 0, 4, 1, 2]
    frows = [0, 1, 2, 3, 4]
    got, coeff, status = run_poly(5, sig, rows, fl, frows, 1, sh, 1, starts, stops)
    want, _, wstatus = host_poly(5, sig, rows, fl, frows, 1, sh, 1, starts, stops)
    err = np.max(np.abs(got - want)) / np.max(np.abs(sig))
    print(f"interleaved call: max |device - host| = {err:.2e} of max|signal|")
    assert err < TOL and np.array_equal(status, wstatus) and np.all(status == H.FITTED)
    for k in range(len(lengths)):
        one, c1, s1 = run_poly(5, sig, rows, fl, frows, 1, sh, 1, starts[k:k + 1], stops[k:k + 1])
        assert np.array_equal(one[:, starts[k]:stops[k]], got[:, starts[k]:stops[k]]), lengths[k]
        assert np.array_equal(c1[:, 0], coeff[:, k]) and np.array_equal(s1[:, 0], status[:, k])


def test_robust_two_pass_jobs_on_more_workgroups_than_run_at_once():
    """An interval of three chunks with only its first tenth good, the same data in 1200 rows: 3600 workgroups in the
    subtraction, more than the GPU holds at once, so those of one interval start at different times.  Rows are
    independent and the arithmetic is fixed: every row must come out like the first, bit for bit, and like the
    interval filtered alone.  The comparison with the host restatement is loose on purpose (1e-9 of max|signal|: the
    accuracy is the fixture test's business); a fit subtracted twice would be off by the offset itself."""
    n_det, length, order = 1200, 8200, 5
    n_samp = length + 9
    row = H.poly_case_signals(485, 1, n_samp)
    sig = np.repeat(row, n_det, axis=0)
    shared = np.zeros(n_samp, dtype=np.uint8)
    shared[4 + length // 10:] = 1
    starts, stops = np.array([4]), np.array([4 + length])
    idx = np.arange(n_det, dtype=np.int32)
    got, coeff, status = run_poly(order, sig, idx, None, None, 0, shared, 1, starts, stops, path=TWO_PASS)
    assert np.all(status == H.FITTED)
    assert np.all(got == got[0][None, :]) and np.all(coeff == coeff[0][None])
    alone, c1, _ = run_poly(order, row, [0], None, None, 0, shared, 1, starts, stops, path=TWO_PASS)
    assert np.array_equal(alone[0], got[0]) and np.array_equal(c1[0], coeff[0])
    assert np.array_equal(got[0, :4], row[0, :4]) and np.array_equal(got[0, 4 + length:], row[0, 4 + length:])
    want = row.copy()
    H.filter_polynomial(order, shared, want[0], starts, stops)
    err = np.max(np.abs(got[0] - want[0])[4:4 + length // 10]) / np.max(np.abs(row))
    print(f"robust two-pass job: max |device - host| on the good samples = {err:.2e} of max|signal|")
    assert err < 1e-9


@pytest.mark.parametrize("path", [RULE, SINGLE, TWO_PASS])
def test_interval_clipping(path):
    n = 1000
    sig = H.poly_case_signals(490, 2, n)
    fl = random_flags(491, (2, n))
    starts = np.array([-7, 300, 500, n + 10, 900, n], dtype=np.int64)
    stops = np.array([200, 300, 450, n + 50, n + 40, n + 5], dtype=np.int64)
    got, coeff, status = run_poly(2, sig, [1, 0], fl, [0, 1], 1, None, 0, starts, stops, path=path)
    want, wcoeff, wstatus = host_poly(2, sig, [1, 0], fl, [0, 1], 1, None, 0, starts, stops)
    assert wstatus.tolist() == [[0, 1, 1, 1, 0, 1]] * 2
    assert np.array_equal(status, wstatus)
    assert np.max(np.abs(got - want)) < TOL * np.max(np.abs(sig))
    assert np.array_equal(got[:, 200:900], sig[:, 200:900])               # the empty intervals touched nothing
    assert np.all(coeff[:, [1, 2, 3, 5]] == 0)
    assert np.max(np.abs(coeff - wcoeff)) < 1e-9 * np.max(np.abs(sig))
    # [-7, 200) is [0, 200) and [900, n + 40) is [900, n): the same bits as the clipped intervals given directly
    direct, dcoeff, _ = run_poly(2, sig, [1, 0], fl, [0, 1], 1, None, 0, np.array([0, 900]), np.array([200, n]), path=path)
    assert np.array_equal(direct, got) and np.array_equal(dcoeff, coeff[:, [0, 4]])


# ------------------------------------------------------------------------------------------------ common mode
@pytest.mark.parametrize("n_det", [1, 8, 9, 17])
def test_common_mode_row_counts_and_null_flags(n_det):
    """On either side of the load-ahead of 8 rows; NULL detector flags, NULL shared flags, both; the separate pair and
    the fused kernel.  The kernels keep the reference's summation order: bit-identical to the host restatement."""
    import torch

    from toast_amd import capi

    n, n_rows = 1031, n_det + 2
    signals = H.common_mode_signals(700 + n_det, n_rows, n)
    rows = np.array([(3 * k + 1) % n_rows for k in range(n_rows)][:n_det], dtype=np.int32)
    assert len(set(rows.tolist())) == n_det
    frows = np.arange(n_det, dtype=np.int32)[::-1].copy()
    det_flags = random_flags(710 + n_det, (n_det, n), 0.3) * np.uint8(2) | np.uint8(8)      # 8 is outside the mask
    shared = random_flags(720 + n_det, (n,), 0.1) | np.uint8(4)
    det_flags[:, 500] = 2                                                                  # a sample nobody hits
    shared[500] = 4
    for use_det, use_shared in ((True, True), (False, True), (True, False), (False, False)):
        h_det = det_flags if use_det else np.zeros_like(det_flags)
        h_shared = shared if use_shared else np.zeros_like(shared)
        want = signals.copy()
        total, hits = np.zeros(n), np.zeros(n, dtype=np.int64)
        H.sum_detectors(rows, frows, h_shared, 1, want, h_det, 2, total, hits)
        summed = total.copy()
        H.subtract_mean(rows, want, total, hits)
        assert hits.max() <= n_det and (hits[500] == 0) == use_det
        t_f, t_sh = dev(det_flags), dev(shared)              # kept alive while their addresses are in use
        d_f = t_f.data_ptr() if use_det else 0
        d_sh = t_sh.data_ptr() if use_shared else 0
        fi = frows if use_det else None
        # the separate pair
        d_s = dev(signals)
        d_total = torch.zeros(n, dtype=torch.float64, device="cuda")
        d_hits = torch.zeros(n, dtype=torch.int64, device="cuda")
        capi.dev.sum_detectors(n, rows, d_s.data_ptr(), fi, d_f, 2, d_sh, 1, d_total.data_ptr(), d_hits.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_total.cpu().numpy(), summed) and np.array_equal(d_hits.cpu().numpy(), hits)
        capi.dev.subtract_mean(n, rows, d_s.data_ptr(), d_total.data_ptr(), d_hits.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_total.cpu().numpy(), total) and np.array_equal(d_s.cpu().numpy(), want)
        # the fused form
        d_s = dev(signals)
        mean = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        hits2 = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        capi.dev.common_mode_subtract(n, rows, d_s.data_ptr(), fi, d_f, 2, d_sh, 1, mean.data_ptr(), hits2.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(mean.cpu().numpy(), total) and np.array_equal(hits2.cpu().numpy(), hits)
        assert np.array_equal(d_s.cpu().numpy(), want)
