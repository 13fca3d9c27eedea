"""GPU: the HWPSS kernels (csrc/hwpss.hip) through the C ABI, and ops.HWPSynchronousModel on device-resident data against
the reference's own run (tests/golden/hwpss.npz).

Sums (Gram matrices, right-hand sides) are compared with long-double evaluations of the same formulas
(hwpss_case.fit_ld) in units of eps * sum |terms|.  The kernel's bound follows its summation order: one lane adds the
samples of a tile of toast_hip_hwpss_chunk() samples in order, with one FMA per term, and a second kernel adds the tiles
of the chunk in order: a chain of at most  min(n, tile) + ceil(n / tile)  roundings for a chunk of n samples (RUN).  HIP's
documentation of the error of double sin / cos is not on this machine; the project's other tests (test_gpu_filterbin.py)
use the documented 2 ulp, and so does this one.  The allowances on top of RUN are those of hwpss_case.check_case with the
reference's stored error set to zero where the comparison is with the long-double value directly.

The means are compensated sums: hi + lo is exact far beyond double, so the double that is returned is within one rounding
of the exact mean (asserted: 1 eps |mean| against rational arithmetic), also under a DC level of 1e6.

Splines: the kernel repeats FITPACK's fpbspl / splev operation by operation in double, without contraction; each of the
four basis values goes through at most 3 levels of (one division, two differences, one product, one sum) and the value
is a sum of four products: 3 * 5 + 4 + 1 = 20 roundings at most, asserted as 20 eps sum_j |c_j h_j| against
scipy.interpolate.splev (the printed figure of a run on an MI355X is in profiles/hwpss_parity.txt).

Every test prints its measured deviations before it asserts."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.interpolate

import hwpss_case as hc
from toast_amd.data import defaults
from toast_amd.ops import hwpss_model as HM

pytestmark = pytest.mark.gpu

EPS = hc.EPS
TRIG_ULP = 2


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture(scope="module")
def G():
    return hc.gold()


@pytest.fixture(scope="module")
def D():
    from toast_amd import capi

    return capi.dev


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_length(D):
    tile = D.hwpss_chunk()
    return lambda n: min(n, tile) + -(-n // tile)


def test_launch_constants(D):
    assert D.hwpss_max_coeff() >= 36
    assert D.hwpss_det_tile() >= 1 and D.hwpss_chunk() >= 64
    assert hc.N % D.hwpss_chunk() != 0 and hc.N > 2 * D.hwpss_chunk()       # the fixture's length straddles tiles


def kernel_inputs(n_det, seed, dc=None):
    """Signals with Inf in the shared-flagged samples, flags with the values 0 .. 7, shared byte with flagged spans."""
    rng = np.random.default_rng(seed)
    n = hc.N
    t = np.arange(n) / hc.RATE
    angle = np.mod(2 * np.pi * hc.HWP_HZ * t, 2 * np.pi)
    rows = n_det + 2                                            # two rows nobody names
    signal = rng.standard_normal((rows, n)) * 0.1 + np.sin(2 * angle + 0.3)[None, :]
    if dc is not None:
        signal[0] += dc
    flags = np.where(rng.random((rows, n)) < 0.1, rng.integers(1, 8, (rows, n)), 0).astype(np.uint8)
    shared = np.zeros(n, dtype=np.uint8)
    shared[700:760] = 1
    shared[1020:1030] = 4
    signal[:, shared != 0] = np.inf
    return t, angle, signal, flags, shared


# chunks: overlapping, boundaries inside the tiles, one shorter than a 64-sample step, one of a single sample, the last
# one ending past n_samp, one empty
STARTS = np.array([0, 500, 1000, 1030, 2047, 2500, 2900, 40], dtype=np.int64)
ENDS = np.array([1500, 1524, 1010, 1090, 2048, 3001, 3500, 40], dtype=np.int64)


@pytest.mark.parametrize("harmonics,drift", [(2, False), (9, False), (1, True), (9, True)])
def test_gram_kernel(D, harmonics, drift):
    import torch

    t, angle, _, _, shared = kernel_inputs(1, 5)
    n_coeff = HM.n_coefficients(harmonics, drift)
    assert n_coeff <= D.hwpss_max_coeff()
    gram = torch.full((len(STARTS), n_coeff, n_coeff), -7.0, dtype=torch.float64, device="cuda")
    n_good = torch.full((len(STARTS),), -7, dtype=torch.int64, device="cuda")
    d_angle, d_t, d_sh = dev(angle), dev(t), dev(shared)
    D.hwpss_gram(hc.N, harmonics, drift, d_angle.data_ptr(), d_t.data_ptr(), d_sh.data_ptr(), STARTS, ENDS,
                 gram.data_ptr(), n_good.data_ptr())
    torch.cuda.synchronize()
    d_gram, d_n_good = gram, n_good
    gram, n_good = gram.cpu().numpy(), n_good.cpu().numpy()
    basis = hc.basis_ld(angle, t, shared, harmonics, drift)
    fit = hc.fit_ld(basis, shared, np.zeros((0, hc.N)), np.zeros((0, hc.N)), STARTS, ENDS)
    assert np.array_equal(n_good, fit["n_good_shared"])
    rl = run_length(D)
    worst = 0.0
    for c in range(len(STARTS)):
        assert not np.any(np.tril(gram[c], -1))
        allow = rl(max(hc.chunk_length(STARTS[c], ENDS[c]), 1)) + 2 * (TRIG_ULP + 1) + 2
        u = hc.units(np.triu(gram[c]) - np.triu(fit["gram"][c]), np.triu(fit["gram_scale"][c]))
        worst = max(worst, u / allow)
        print(f"gram H={harmonics} drift={drift} chunk {c}: {u:.2f} of {allow} eps scale")
        assert u <= allow
    # without shared flags and without times (no drift): NULL pointers flag nothing
    if not drift:
        D.hwpss_gram(hc.N, harmonics, drift, d_angle.data_ptr(), 0, 0, STARTS[:1], ENDS[:1], d_gram.data_ptr(),
                     d_n_good.data_ptr())
        torch.cuda.synchronize()
        assert int(d_n_good[0]) == hc.chunk_length(STARTS[0], ENDS[0])


@pytest.mark.parametrize("n_det_kind", ["one", "tile", "tile_plus_one"])
@pytest.mark.parametrize("harmonics,drift", [(2, False), (9, True)])
def test_project_kernel(D, n_det_kind, harmonics, drift):
    import torch

    tile = D.hwpss_det_tile()
    n_det = {"one": 1, "tile": tile, "tile_plus_one": tile + 1}[n_det_kind]
    t, angle, signal, flags, shared = kernel_inputs(n_det, 11, dc=1.0e6)
    n_coeff = HM.n_coefficients(harmonics, drift)
    rng = np.random.default_rng(3)
    sig_rows = rng.permutation(n_det + 2)[:n_det].astype(np.int32)          # non-identity row indices
    flag_rows = rng.permutation(n_det + 2)[:n_det].astype(np.int32)
    mask = 3
    for d in range(n_det):                                                  # NaN where the detector's own flag row flags
        signal[sig_rows[d], (flags[flag_rows[d]] & mask) != 0] = np.nan
    for with_flags in (True, False):
        n_chunk = len(STARTS)
        n_good = torch.full((n_det, n_chunk), -7, dtype=torch.int64, device="cuda")
        mean = torch.full((n_det, n_chunk), -7.0, dtype=torch.float64, device="cuda")
        rhs = torch.full((n_det, n_chunk, n_coeff), -7.0, dtype=torch.float64, device="cuda")
        sig = signal if with_flags else np.nan_to_num(signal, nan=0.5, posinf=0.25)
        d_sig, d_fl, d_sh, d_angle, d_t = dev(sig), dev(flags), dev(shared), dev(angle), dev(t)
        D.hwpss_project(hc.N, harmonics, drift, d_angle.data_ptr(), d_t.data_ptr(), d_sh.data_ptr() if with_flags else 0,
                        sig_rows, d_sig.data_ptr(), flag_rows if with_flags else None, d_fl.data_ptr() if with_flags else 0,
                        mask, STARTS, ENDS, n_good.data_ptr(), mean.data_ptr(), rhs.data_ptr())
        torch.cuda.synchronize()
        n_good, mean, rhs = n_good.cpu().numpy(), mean.cpu().numpy(), rhs.cpu().numpy()
        sh = shared if with_flags else np.zeros_like(shared)
        fv = hc.flag_values(flags[flag_rows] if with_flags else None, mask, sh, n_det)
        basis = hc.basis_ld(angle, t, sh, harmonics, drift)
        fit = hc.fit_ld(basis, sh, fv, sig[sig_rows], STARTS, ENDS)
        assert np.array_equal(n_good, fit["n_good"])
        assert np.all(np.isfinite(rhs)) and np.all(np.isfinite(mean))
        # the mean against exact rational arithmetic: extended precision cannot resolve one rounding of a sum that nearly
        # cancels (its own error, ~ sqrt(n) 5e-20 |x|, reaches eps |mean| for a mean of 1e-3)
        u_mean = 0.0
        for d in range(n_det):
            for c in range(n_chunk):
                span = slice(int(STARTS[c]), min(int(ENDS[c]), hc.N))
                xs = sig[sig_rows[d], span][fv[d][span] == 0]
                if xs.size == 0:
                    assert mean[d, c] == 0.0
                    continue
                exact = sum(map(Fraction, xs.tolist()), Fraction(0)) / xs.size
                if exact != 0:
                    u_mean = max(u_mean, float(abs(Fraction(float(mean[d, c])) - exact) / (Fraction(EPS) * abs(exact))))
        print(f"project n_det={n_det} H={harmonics} flags={with_flags}: mean {u_mean:.2f} eps |mean|")
        assert u_mean <= 1.0
        rl = run_length(D)
        for c in range(n_chunk):
            allow = rl(max(hc.chunk_length(STARTS[c], ENDS[c]), 1)) + (TRIG_ULP + 1) + 3
            u = max(hc.units(rhs[d, c] - fit["rhs"][d, c], fit["rhs_scale"][d, c]) for d in range(n_det))
            print(f"  chunk {c}: rhs {u:.2f} of {allow} eps scale")
            assert u <= allow, (c, u, allow)


def fpbspl_scale(tck, x):
    """sum_j |c_j h_j| of splev's own evaluation at x (fpbspl.f in double)."""
    t, c, k = tck
    n = len(t)
    out = np.zeros(len(x))
    for m, arg in enumerate(x):
        l = k                                  # noqa: E741
        while arg >= t[l + 1] and l != n - k - 2:
            l += 1                             # noqa: E741
        h = np.zeros(k + 1)
        h[0] = 1.0
        for j in range(1, k + 1):
            hh = h[:j].copy()
            h[0] = 0.0
            for i in range(1, j + 1):
                f = hh[i - 1] / (t[l + i] - t[l + i - j])
                h[i - 1] += f * (t[l + i] - arg)
                h[i] = f * (arg - t[l + i - j])
        out[m] = np.sum(np.abs(c[l - k:l + 1] * h))
    return out


def test_subtract_kernel_splines_flags_and_calibration(D):
    """Spline evaluation against splev (no interior knots, several, interpolating; times inside, at and outside the knots),
    the uint8 flag product, the float32 calibration rows and the sums, through toast_hip_hwpss_subtract_dev with two
    harmonics at angle 0: the basis is (0, 1, 0, 1) exactly, so the model is spline_1(t) + spline_3(t)."""
    import torch

    rng = np.random.default_rng(17)
    n = 700
    x = np.linspace(1.0, 9.0, 12)
    y = np.sin(x) + 0.3 * x
    tcks = [scipy.interpolate.splrep(x, y, s=1e6),                                  # one polynomial: 8 knots
            scipy.interpolate.splrep(x, y + 0.05 * rng.standard_normal(12), s=0.02),   # several interior knots
            scipy.interpolate.splrep(x, y, s=0)]                                    # interpolating
    assert len(tcks[0][0]) == 8 and 8 < len(tcks[1][0]) < 16 and len(tcks[2][0]) == 16
    reltime = np.sort(np.concatenate([np.linspace(-2.0, 12.0, n - len(tcks[1][0]) - 16), tcks[1][0], tcks[2][0]]))
    assert reltime[0] < x[0] and reltime[-1] > x[-1] and len(reltime) == n
    n_det, n_coeff = len(tcks), 4
    zero = (np.array([0.0] * 4 + [1.0] * 4), np.zeros(8), 3)
    second = scipy.interpolate.splrep(x, 2.0 + np.cos(x), s=0)
    splines = [[zero, tck, zero, second] for tck in tcks]
    offsets, st, sc = HM.pack_splines(splines, n_coeff)
    signal = rng.standard_normal((n_det, n))
    flags = rng.integers(0, 8, (n_det, n)).astype(np.uint8)
    flags[:, ::3] = 0
    shared = np.zeros(n, dtype=np.uint8)
    shared[100:110] = 1
    det_mask, hwp_mask, cal_center = 3, 2, 1.75
    d_sig, d_fl = dev(signal), dev(flags)
    relcal = torch.full((n_det, n), -7.0, dtype=torch.float32, device="cuda")
    sums = torch.zeros(n_det, dtype=torch.float64, device="cuda")
    counts = torch.zeros(n_det, dtype=torch.int64, device="cuda")
    rows = np.arange(n_det, dtype=np.int32)[::-1]
    d_angle, d_t, d_sh, d_st, d_sc = dev(np.zeros(n)), dev(reltime), dev(shared), dev(st), dev(sc)
    D.hwpss_subtract(n, 2, False, d_angle.data_ptr(), d_t.data_ptr(), d_sh.data_ptr(), rows,
                     d_sig.data_ptr(), rows, d_fl.data_ptr(), det_mask, hwp_mask, np.ones(n_det, dtype=np.int32), True,
                     sums.data_ptr(), counts.data_ptr(), spl_offset=offsets, d_spl_t=d_st.data_ptr(),
                     d_spl_c=d_sc.data_ptr(), relcal_index=rows, d_relcal=relcal.data_ptr(), cal_center=cal_center)
    torch.cuda.synchronize()
    got, got_flags, relcal = d_sig.cpu().numpy(), d_fl.cpu().numpy(), relcal.cpu().numpy()
    fv = (flags & det_mask) | shared[None, :]
    assert np.array_equal(got_flags, flags | (fv * np.uint8(hwp_mask)).astype(np.uint8))
    for k, row in enumerate(rows):
        good = fv[row] == 0
        s1 = scipy.interpolate.splev(reltime, splines[k][1], ext=0)
        s3 = scipy.interpolate.splev(reltime, splines[k][3], ext=0)
        model = s1 + s3
        scale = fpbspl_scale(splines[k][1], reltime) + fpbspl_scale(splines[k][3], reltime)
        # the shared-flagged samples have a zero basis: nothing but zeros is added there (and they are not good)
        delta = np.abs(got[row][good] - (signal[row][good] - model[good]))
        allowed = 20 * EPS * scale[good] + EPS * (np.abs(signal[row][good]) + np.abs(model[good]))
        print(f"spline {k} ({len(splines[k][1][0])} knots): {float(np.max(delta / allowed)):.3f} of the allowance, "
              f"{int(np.count_nonzero(delta))} samples differ from splev at all")
        assert np.all(delta <= allowed)
        assert np.array_equal(got[row][~good], signal[row][~good])
        mag = np.where(good, np.sqrt(0.0 * 0.0 + s3 * s3), 1.0)
        want = (cal_center / mag).astype(np.float32)
        assert np.all(np.abs(relcal[row] - want) <= 2 * np.spacing(np.abs(want)))
        assert int(counts[k]) == int(np.count_nonzero(good))
        total = float(np.sum(got[row][good].astype(hc.L)))
        assert abs(float(sums[k]) - total) <= 2 * EPS * abs(total) + 1e-300
    # inactive detectors: flags only
    d_sig2, d_fl2 = dev(signal), dev(flags)
    D.hwpss_subtract(n, 2, False, d_angle.data_ptr(), d_t.data_ptr(), d_sh.data_ptr(), rows,
                     d_sig2.data_ptr(), rows, d_fl2.data_ptr(), det_mask, hwp_mask, np.zeros(n_det, dtype=np.int32), True,
                     sums.data_ptr(), counts.data_ptr(), spl_offset=offsets, d_spl_t=d_st.data_ptr(),
                     d_spl_c=d_sc.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d_sig2.cpu().numpy(), signal)
    assert np.array_equal(d_fl2.cpu().numpy(), got_flags)


@pytest.mark.parametrize("case", list(hc.CASES))
def test_resident_operator_matches_the_reference(G, D, case):
    op, data = hc.run_case(case, resident=True)
    seen = hc.check_case(case, op, data, G, run_length=run_length(D), trig_ulp=TRIG_ULP)
    print(case, {k: f"{v:.3g}" for k, v in seen.items()}, "(fractions of the allowances)")


@pytest.mark.parametrize("kind", ["one", "tile", "tile_plus_one"])
def test_operator_detector_tiles_and_row_indices(G, D, kind):
    """n_det 1, det_tile and det_tile + 1 (detector i a copy of detector i % 3 of the case), rows in reverse order, host
    data with use_accel=True."""
    n_det = {"one": 1, "tile": D.hwpss_det_tile(), "tile_plus_one": D.hwpss_det_tile() + 1}[kind]
    op, data = hc.run_case("one", use_accel=True, n_det=n_det, reverse_rows=True)
    seen = hc.check_case("one", op, data, G, run_length=run_length(D), trig_ulp=TRIG_ULP, n_det=n_det)
    print(kind, {k: f"{v:.3g}" for k, v in seen.items()})


def test_more_coefficients_than_the_kernels_take_use_the_host_path(D):
    data = hc.make_data("h2")
    dd = data.obs[0].detdata[defaults.det_data]
    dd.accel_create(defaults.det_data)
    dd.accel_update_device()
    from toast_amd import ops

    harmonics = D.hwpss_max_coeff() // 2 + 1
    op = ops.HWPSynchronousModel(harmonics=harmonics, subtract_model=True)
    op.apply(data)
    ref = hc.make_data("h2")
    ops.HWPSynchronousModel(harmonics=harmonics, subtract_model=True).apply(ref)
    assert np.array_equal(data.obs[0].detdata[defaults.det_data].data, ref.obs[0].detdata[defaults.det_data].data,
                          equal_nan=True)
