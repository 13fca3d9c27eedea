"""CPU: ops.HWPSynchronousModel on host data (its NumPy path) against the reference's own run (tests/golden/hwpss.npz,
made by tests/golden/make_golden_hwpss.py from the reference's Python), the conditions the fixture recorded about
itself, and the operator's checks.

The comparison and its allowances are hwpss_case.check_case.  For this path a sum over n samples may be formed in any
order (BLAS): the bound of n additions covers every order.  NumPy's double sin / cos are taken as 1 ulp (glibc documents
less)."""
import numpy as np
import pytest

import hwpss_case as hc
from toast_amd import ops
from toast_amd.data import defaults


@pytest.fixture(scope="module")
def G():
    return hc.gold()


def test_fixture_conditions(G):
    """What keeps the comparison honest (recorded by the generator): no chunk's rcond near the 1e-8 decision, every
    spline in the one-polynomial regime (8 knots) or interpolating, no good-sample count at n_coeff or n_coeff - 1
    outside the case built for it, the sigma cut removes exactly the sixth detector."""
    for case, spec in hc.CASES.items():
        P = case + "_"
        rcond, ngs = G[P + "rcond"], G[P + "n_good_shared"]
        for c in range(len(rcond)):
            assert ngs[c] == 0 or rcond[c] >= 1e-6 or rcond[c] <= 1e-10, (case, c)
            assert bool(G[P + "coeff_flags"][c]) == (ngs[c] == 0 or rcond[c] < 1e-8)
        assert G[P + "min_count_distance"] > 0
        n_good_chunks = int(np.count_nonzero(G[P + "coeff_flags"] == 0))
        assert all(k in (8, n_good_chunks + 4, n_good_chunks + 3) for k in G[P + "knots"]), (case, set(G[P + "knots"]))
    assert len(G["chunks_starts"]) == 9 and list(np.flatnonzero(G["chunks_coeff_flags"])) == [3, 6]
    assert not bool(G["chunks_last_end_past_n_samp"])       # so the C-ABI tests pass explicit chunks that end past n_samp
    n_coeff = 18
    assert 0 < G["chunks_n_good"][1, 0] < n_coeff
    assert len(G["view_starts"]) == len(hc.VIEW) - 1
    assert list(G["cut_detector_flags"]) == [0, 0, 0, 0, 0, 1]
    assert list(G["chunks_bad_detector_flags"]) == [0, 0, 1]


@pytest.mark.parametrize("case", list(hc.CASES))
def test_host_path_matches_the_reference(G, case):
    op, data = hc.run_case(case)
    seen = hc.check_case(case, op, data, G, run_length=lambda n: n, trig_ulp=1)
    print(case, {k: f"{v:.3g}" for k, v in seen.items()})


def test_rows_through_index_arrays(G):
    op, data = hc.run_case("h2", reverse_rows=True)
    hc.check_case("h2", op, data, G, run_length=lambda n: n, trig_ulp=1)


def test_option_checks():
    data = hc.make_data("h2")
    with pytest.raises(RuntimeError, match="Only one of continuous and fixed"):
        ops.HWPSynchronousModel(relcal_fixed="a", relcal_continuous="b").apply(data)
    with pytest.raises(RuntimeError, match="Only one of chunk_view and chunk_time"):
        ops.HWPSynchronousModel(subtract_model=True, chunk_view="chunks", chunk_time=3.0).apply(data)
    with pytest.raises(RuntimeError, match="Nothing to do"):
        ops.HWPSynchronousModel().apply(data)
    with pytest.raises(NotImplementedError):
        ops.HWPSynchronousModel(subtract_model=True, fill_gaps=True)
    with pytest.raises(NotImplementedError):
        ops.HWPSynchronousModel(subtract_model=True, debug="plots")
    op = ops.HWPSynchronousModel()
    assert op.chunk_time is None and op.harmonics == 9 and op.relcal_cut_sigma == 5.0 and op.debug is None


def test_observation_without_hwp_angle_is_skipped():
    for traits in (dict(relcal_fixed="relcal"), dict(relcal_continuous="relcal_ts")):
        data = hc.make_data("h2")
        ob = data.obs[0]
        del ob.shared[defaults.hwp_angle]
        before = np.array(ob.detdata[defaults.det_data].data)
        ops.HWPSynchronousModel(subtract_model=True, **traits).apply(data)
        assert np.array_equal(ob.detdata[defaults.det_data].data, before)
        if "relcal_fixed" in traits:
            assert ob["relcal"] == {d: 1.0 for d in ob.local_detectors}
        else:
            rd = ob.detdata["relcal_ts"]
            assert rd.dtype == np.float32 and np.all(rd.data == 1.0)


def test_too_few_chunks_for_the_spline():
    """smoothing = max(n_chunk // 16, 4) >= n_chunk is the reference's own error; fewer than four good chunks would fail
    inside FITPACK (m > k must hold) and is reported with the detector's name instead."""
    data = hc.make_data("h2")
    with pytest.raises(RuntimeError, match="Only 3 chunks for interpolation"):
        ops.HWPSynchronousModel(harmonics=2, subtract_model=True, chunk_time=7.5).apply(data)
    data = hc.make_data("h2")
    ob = data.obs[0]
    ob.shared[defaults.shared_flags].data[0:1500] |= 1          # chunks 0 .. 3 of nine lose every sample, 4 half
    ob.shared[defaults.shared_flags].data[2100:] |= 1           # ... and 7, 8: three good chunks are left
    with pytest.raises(RuntimeError, match=r"obs_h2\[D0\].*good chunks"):
        ops.HWPSynchronousModel(harmonics=2, subtract_model=True, chunk_time=3.0).apply(data)
