"""Host: the PolyFilter2D fixture (tests/golden/poly2d.npz: coefficients of the reference's own `filter_poly2D_numpy`), the
NumPy emulation of the device algorithm (tests/poly2d_host.py) and the host path of ``ops.PolyFilter2D``.

Bounds: per case and stored in the fixture, 4 x max |reference - emulation| over the compared systems, measured by
tests/golden/make_golden_poly2d.py.  For the operator's host path (lstsq per system, the reference's own solve) the same
bounds hold with room: it differs from the reference by the summation order of A and b only."""
import numpy as np
import pytest

import poly2d_host as P
from toast_amd import ops
from toast_amd.data import defaults


@pytest.fixture(scope="module")
def fixture():
    return P.load_fixture()


check_result = P.check_result


@pytest.mark.parametrize("name", list(P.CASES))
def test_emulation_against_reference_fixture(fixture, name):
    case, ref_coeff, excluded, bounds = P.fixture_case(fixture, name)
    assert np.max(np.abs(case["templates"] - fixture[f"{name}_templates"])) <= 1e-15
    # the exclusion share, recomputed from the spectra of A
    again = P.excluded_systems(case)
    assert np.mean(again) <= P.MAX_EXCLUDED and np.mean(excluded) <= P.MAX_EXCLUDED
    sig, flags, coeff, status, sweeps = P.emulate(case)
    assert sweeps <= 12
    # a quarter of the stored bound: the bound is four times what this very comparison measured
    check_result(case, ref_coeff, excluded, {k: v / 4 * (1 + 1e-12) for k, v in bounds.items()}, sig, flags, coeff,
                 label=f"emulation {name}")
    # the engineered samples
    for s in (P.S_GROUP_FLAGGED, P.S_SHARED, P.S_ZERO):
        assert np.all(coeff[s, 0] == 0) and status[s, 0] == (0 if s == P.S_ZERO else 1)
    g0 = np.flatnonzero(case["det_group"] == 0)
    for s in (P.S_GROUP_FLAGGED, P.S_SHARED, P.S_ZERO):
        assert np.all(flags[case["flag_rows"][g0], s] & P.POLY_MASK)
    assert np.any(coeff[P.S_ONE_GOOD, 0] != 0)
    if case["n_mode"] > 1:
        assert status[P.S_ONE_GOOD, 0] == 2 and status[P.S_FEW_GOOD, 0] == 2       # truncated
    assert np.isnan(sig[case["sig_rows"][g0[1]], P.S_NAN_FLAGGED])
    assert np.all(np.isfinite(coeff[P.S_NAN_FLAGGED]))


def test_emulation_nan_in_a_good_sample(fixture):
    case = P.build_nan_case()
    s, d = P.NAN_CASE["sample"], P.NAN_CASE["det"]
    ref_coeff = fixture["nan_coeff"]
    bounds = dict(zip(("filtered", "fit", "coeff"), fixture["nan_bounds"]))
    sig, flags, coeff, status, _ = P.emulate(case)
    assert status[s, 0] == 3 and np.all(coeff[s] == 0) and np.all(flags[:, s] & P.POLY_MASK)
    assert np.array_equal(sig[:, s].view(np.uint64), case["signal"][:, s].view(np.uint64)) and np.isnan(sig[d, s])
    check_result(case, ref_coeff, np.zeros((case["n_samp"], 1), dtype=bool), bounds, sig, flags, coeff, label="emulation nan")


@pytest.mark.parametrize("name", list(P.CASES) + ["nan"])
def test_operator_host_path(fixture, name):
    if name == "nan":
        case = P.build_nan_case()
        ref_coeff, excluded = fixture["nan_coeff"], np.zeros((case["n_samp"], 1), dtype=bool)
        bounds = dict(zip(("filtered", "fit", "coeff"), fixture["nan_bounds"]))
        templates = case["templates"]
    else:
        case, ref_coeff, excluded, bounds = P.fixture_case(fixture, name)
        templates = fixture[f"{name}_templates"]
    data = P.build_observation(case)
    ob = data.obs[0]
    op = ops.PolyFilter2D(name="poly2d", **P.operator_traits(case))
    dets, det_group, keys, op_templates = op._setup(ob, __import__("re").compile(".*"))
    assert dets == ob.local_detectors and np.array_equal(det_group, case["det_group"])
    assert keys == ([None] if case["n_group"] == 1 else [f"w{g}" for g in range(case["n_group"])])
    assert np.max(np.abs(op_templates - templates)) <= 1e-15
    op.apply(data, use_accel=False)
    # back into the case's buffers
    sig = case["signal"].copy()
    sig[case["sig_rows"]] = ob.detdata[defaults.det_data].data
    flags = case["det_flags"].copy()
    flags[case["flag_rows"]] = ob.detdata[defaults.det_flags].data
    coeff = op.coefficients[ob.name]
    check_result(case, ref_coeff, excluded, bounds, sig, flags, coeff, label=f"host path {name}")
    zero = np.all(ref_coeff[P.view_samples(case)] == 0, axis=2)
    assert np.array_equal(op.flagged_samples[ob.name], np.count_nonzero(zero, axis=0))
    assert np.array_equal(ob.shared[defaults.shared_flags].data, case["shared"])


def test_operator_raises():
    case = P.build_nan_case()
    data = P.build_observation(case)
    traits = P.operator_traits(case)
    with pytest.raises(RuntimeError, match="subsets of detectors"):
        ops.PolyFilter2D(**traits).apply(data, detectors=["D000"], use_accel=False)
    with pytest.raises(RuntimeError, match="not defined in the focalplane"):
        ops.PolyFilter2D(**dict(traits, focalplane_key="nonexistent")).apply(data, use_accel=False)
    data.obs[0].detdata.create("single", dtype=np.float32)
    with pytest.raises(RuntimeError, match="float64"):
        ops.PolyFilter2D(**dict(traits, det_data="single")).apply(data, use_accel=False)
    with pytest.raises(RuntimeError, match="is not defined for observation"):
        ops.PolyFilter2D(**dict(traits, view="nonexistent")).apply(data, use_accel=False)
    op = ops.PolyFilter2D(**traits)
    assert op.requires()["intervals"] == [P.VIEW] and op.provides()["detdata"] == []


def test_operator_order_above_device_limit_matches_lstsq():
    """Order 4 (25 modes) is beyond the device kernels: the host path, checked against lstsq written out here."""
    case = P.build_nan_case()
    case["signal"][P.NAN_CASE["det"], P.NAN_CASE["sample"]] = 1.5
    case["order"], case["n_mode"] = 4, 25
    case["templates"], _, _ = P.case_templates(case["n_det"], 1, 4)
    data = P.build_observation(case)
    op = ops.PolyFilter2D(name="poly2d", **P.operator_traits(case))
    op.apply(data)
    got = data.obs[0].detdata[defaults.det_data].data
    t = case["templates"]
    for s in P.view_samples(case):
        good = (case["det_flags"][:, s] & P.DET_MASK) == 0
        c = np.linalg.lstsq(t[good].T @ t[good], t[good].T @ case["signal"][good, s], rcond=1e-6)[0]
        want = case["signal"][:, s].copy()
        want[good] -= t[good] @ c
        assert np.max(np.abs(got[:, s] - want)) < 1e-11
