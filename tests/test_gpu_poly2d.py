"""GPU: the PolyFilter2D kernels (csrc/poly2d_filter.hip), the `filter_poly2D` binding and ops.PolyFilter2D against the
coefficients of the reference's own kernel (tests/golden/poly2d.npz) and the host restatements of tests/poly2d_host.py.

Bounds: per case and stored in the fixture -- 4 x max |reference - host emulation of the device algorithm| over the
compared systems (tests/golden/make_golden_poly2d.py); the factor covers the device's own rounding of divisions and
square roots.  Systems with an eigenvalue ratio next to the 1e-6 threshold are left out of the VALUE comparison only."""
import numpy as np
import pytest

import poly2d_host as P
from toast_amd import ops
from toast_amd.data import defaults

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


def paths():
    from toast_amd import capi

    return capi.dev.POLY2D_PATHS


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_device(case, path=0, with_flags=True, with_outputs=True):
    """toast_hip_filter_poly2d_dev on the case's buffers -> (signal, det_flags, coeff, status)."""
    import torch

    from toast_amd import capi

    d_s = dev(case["signal"])
    d_f = dev(case["det_flags"])
    d_sh = dev(case["shared"])
    n = case["n_samp"]
    coeff = torch.zeros((n, case["n_group"], case["n_mode"]), dtype=torch.float64, device="cuda")
    status = torch.full((n, case["n_group"]), -1, dtype=torch.int32, device="cuda")
    capi.dev.filter_poly2d(case["order"], n, case["sig_rows"], d_s.data_ptr(), case["flag_rows"] if with_flags else None,
                           d_f.data_ptr() if with_flags else 0, P.DET_MASK, d_sh.data_ptr(), P.SHARED_MASK, P.POLY_MASK,
                           case["det_group"], case["n_group"], case["templates"], case["starts"], case["stops"],
                           d_coeff=coeff.data_ptr() if with_outputs else 0,
                           d_status=status.data_ptr() if with_outputs else 0, path=path)
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_f.cpu().numpy(), coeff.cpu().numpy(), status.cpu().numpy()


_runs = {}


def cached_run(fixture, name, path):
    """One device run per (case, path), shared by the tests below and never modified."""
    if (name, path) not in _runs:
        case = P.fixture_case(fixture, name)[0]
        _runs[(name, path)] = run_device(case, path=path)
    return _runs[(name, path)]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", list(P.CASES))
def test_kernels_against_reference_fixture(fixture, name, path):
    assert path in paths()
    case, ref_coeff, excluded, bounds = P.fixture_case(fixture, name)
    sig, flags, coeff, status = cached_run(fixture, name, path)
    P.check_result(case, ref_coeff, excluded, bounds, sig, flags, coeff, label=f"device {name} path {path}")
    samples = P.view_samples(case)
    assert np.all(status[samples] >= 0) and np.all(status[samples] <= 3)
    outside = np.ones(case["n_samp"], dtype=bool)
    outside[samples] = False
    assert np.all(status[outside] == -1)
    _, _, _, emu_status, _ = P.emulate(case)
    assert np.array_equal(status[samples][~excluded], emu_status[samples][~excluded])


@pytest.mark.parametrize("name", list(P.CASES))
def test_runs_and_variants_are_bitwise_equal(fixture, name):
    case = P.fixture_case(fixture, name)[0]
    first = cached_run(fixture, name, 0)
    again = run_device(case, path=0)
    other = cached_run(fixture, name, 1)
    for got in (again, other):
        assert np.array_equal(got[0].view(np.uint64), first[0].view(np.uint64))
        assert np.array_equal(got[1], first[1])
        assert np.array_equal(got[2].view(np.uint64), first[2].view(np.uint64))
        assert np.array_equal(got[3], first[3])
    # the optional outputs change nothing
    bare = run_device(case, path=0, with_outputs=False)
    assert np.array_equal(bare[0].view(np.uint64), first[0].view(np.uint64)) and np.array_equal(bare[1], first[1])


@pytest.mark.parametrize("name", ["o1_d19_g2", "o3_d37"])
def test_null_flag_pointer(fixture, name):
    """No detector flags: every detector is good where the shared flag is clear, and no flag is written."""
    case, _, _, bounds = P.fixture_case(fixture, name)
    clean = dict(case)
    clean["signal"] = np.nan_to_num(case["signal"], nan=1.25)       # the NaN was under a flag that is not looked at now
    sig, flags, coeff, status = run_device(clean, with_flags=False)
    assert np.array_equal(flags, case["det_flags"])
    emu_sig, _, emu_coeff, emu_status, _ = P.emulate(clean, with_flags=False)
    # the same algorithm in the same order: a quarter of the stored bound is the distance reference <-> emulation
    good = ((case["shared"] & P.SHARED_MASK) == 0)
    assert np.max(np.abs(sig - emu_sig)) <= bounds["filtered"]
    assert np.max(np.abs(coeff - emu_coeff)) <= bounds["coeff"]
    assert np.array_equal(status[P.view_samples(case)], emu_status[P.view_samples(case)])
    assert np.array_equal(sig[:, ~good].view(np.uint64), clean["signal"][:, ~good].view(np.uint64))


def test_nan_in_a_good_sample(fixture):
    from toast_amd import capi

    case = P.build_nan_case()
    s, d = P.NAN_CASE["sample"], P.NAN_CASE["det"]
    bounds = dict(zip(("filtered", "fit", "coeff"), fixture["nan_bounds"]))
    for path in paths():
        sig, flags, coeff, status = run_device(case, path=path)
        assert status[s, 0] == capi.dev.POLY2D_NOT_FINITE and np.all(coeff[s] == 0) and np.all(flags[:, s] & P.POLY_MASK)
        assert np.array_equal(sig[:, s].view(np.uint64), case["signal"][:, s].view(np.uint64)) and np.isnan(sig[d, s])
        P.check_result(case, fixture["nan_coeff"], np.zeros((case["n_samp"], 1), dtype=bool), bounds, sig, flags, coeff,
                       label=f"device nan path {path}")


def test_arguments_are_checked(fixture):
    from toast_amd import capi

    case = P.build_nan_case()
    bad = dict(case)
    bad["order"], bad["n_mode"] = 4, 25
    bad["templates"] = P.case_templates(case["n_det"], 1, 4)[0]
    with pytest.raises(Exception, match="order"):
        run_device(bad)
    with pytest.raises(Exception, match="path"):
        run_device(case, path=2)
    wrong = dict(case)
    wrong["templates"] = case["templates"] + 0.01          # no longer theta^i phi^j
    with pytest.raises(Exception, match="theta"):
        run_device(wrong)
    group = dict(case)
    group["det_group"] = np.full(case["n_det"], 1, dtype=np.int32)
    with pytest.raises(Exception, match="group"):
        run_device(group)
    assert capi.dev.filter_poly2d_max_order() == 3


@pytest.mark.parametrize("name", ["o1_d19_g2", "o3_d37"])
def test_binding_with_the_reference_layouts(fixture, name):
    """_libtoast_hip.filter_poly2D(det_groups, templates, signals, masks, coeff): the reference's arguments and layouts."""
    from toast_amd import _libtoast_hip as lt

    case, ref_coeff, excluded, bounds = P.fixture_case(fixture, name)
    first, last = int(case["starts"][0]), int(case["stops"][0])
    signals, masks = P.reference_inputs(case, first, last)
    keep_s, keep_m = signals.copy(), masks.copy()
    coeff = np.full((last - first, case["n_group"], case["n_mode"]), np.nan)
    lt.filter_poly2D(case["det_group"], case["templates"], signals, masks, coeff)
    assert np.array_equal(signals, keep_s) and np.array_equal(masks, keep_m)
    diff = np.abs(coeff - ref_coeff[first:last])[~excluded[:last - first]]
    assert np.max(diff) <= bounds["coeff"]
    device_coeff = cached_run(fixture, name, 0)[2][first:last]
    assert np.array_equal(coeff.view(np.uint64), device_coeff.view(np.uint64))


@pytest.mark.parametrize("name", ["o2_d37_g2", "o3_d64_g2"])
def test_operator_on_a_resident_observation(fixture, name):
    from toast_amd.accel import accel_data_update_host

    case, ref_coeff, excluded, bounds = P.fixture_case(fixture, name)
    host = P.build_observation(case)
    ops.PolyFilter2D(name="poly2d", **P.operator_traits(case)).apply(host, use_accel=False)
    data = P.build_observation(case)
    assert data.lazy_host
    ob = data.obs[0]
    sig, flg = ob.detdata[defaults.det_data], ob.detdata[defaults.det_flags]
    sig.accel_create(defaults.det_data)
    sig.accel_update_device()
    op = ops.PolyFilter2D(name="poly2d", **P.operator_traits(case))
    op.apply(data)
    # the timestreams stay resident, the flags became resident and were updated on the device copy
    assert sig.accel_in_use() and flg.accel_exists() and flg.accel_in_use()
    probe = np.zeros_like(flg.buffer)
    probe[:] = flg.buffer
    flg.buffer[:] = 0
    accel_data_update_host(flg.buffer, defaults.det_flags)
    device_flags = flg.buffer.copy()
    flg.buffer[:] = probe
    want_flags = host.obs[0].detdata[defaults.det_flags].data
    assert np.array_equal(device_flags, want_flags) and np.array_equal(flg.data, want_flags)
    got = np.array(sig.data)
    want = host.obs[0].detdata[defaults.det_data].data
    cmp = P.compared(case, excluded)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)[cmp]) <= bounds["filtered"]
    full = case["signal"].copy()
    full[case["sig_rows"]] = got
    flags = case["det_flags"].copy()
    flags[case["flag_rows"]] = want_flags
    P.check_result(case, ref_coeff, excluded, bounds, full, flags, op.coefficients[ob.name], label=f"operator {name}")
    zero = np.all(op.coefficients[ob.name][P.view_samples(case)] == 0, axis=2)
    assert np.array_equal(op.flagged_samples[ob.name], np.count_nonzero(zero, axis=0))
    # data.lazy_host = False: timestreams the operator made resident itself go back to the host and are released
    eager = P.build_observation(case)
    eager.lazy_host = False
    ops.PolyFilter2D(name="poly2d", **P.operator_traits(case)).apply(eager)
    esig = eager.obs[0].detdata[defaults.det_data]
    assert not esig.accel_exists() and not esig.accel_in_use()
    assert np.array_equal(esig.data.view(np.uint64), got.view(np.uint64))
    lazy = P.build_observation(case)
    ops.PolyFilter2D(name="poly2d", **P.operator_traits(case)).apply(lazy)
    lsig = lazy.obs[0].detdata[defaults.det_data]
    assert lsig.accel_exists() and lsig.accel_in_use()
    assert np.array_equal(lsig.data.view(np.uint64), got.view(np.uint64))


def test_order_four_takes_the_host_path():
    case = P.build_nan_case()
    case["signal"][P.NAN_CASE["det"], P.NAN_CASE["sample"]] = 1.5
    case["order"], case["n_mode"] = 4, 25
    case["templates"], _, _ = P.case_templates(case["n_det"], 1, 4)
    data = P.build_observation(case)
    ops.PolyFilter2D(name="poly2d", **P.operator_traits(case)).apply(data)
    got = data.obs[0].detdata[defaults.det_data].data
    t = case["templates"]
    for s in P.view_samples(case):
        good = (case["det_flags"][:, s] & P.DET_MASK) == 0
        c = np.linalg.lstsq(t[good].T @ t[good], t[good].T @ case["signal"][good, s], rcond=1e-6)[0]
        want = case["signal"][:, s].copy()
        want[good] -= t[good] @ c
        assert np.max(np.abs(got[:, s] - want)) < 1e-11
