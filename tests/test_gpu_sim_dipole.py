"""GPU: the dipole kernel (csrc/sim_dipole.hip) through ``capi.dev.sim_dipole`` and ``ops.SimDipole`` on
device-resident data, against the reference's own outputs (tests/golden/sim_dipole.npz).

Values: within ten times the reference's own stored deviation from the long-double evaluation, in units eps * scale
(scale = cmb for freq 0, cmb * max(beta) otherwise; times the unit scale of the call), plus eps * |signal before| where
the signal starts non-zero (the rule of tests/test_gpu_templates.py and tests/test_gpu_atm_observe.py).  Exact: samples
outside the views and rows that the call does not name keep their bits; one launch of three detectors gives the bits
of three launches of one; abutting views give the bits of one view; mask 0 gives the bits of a NULL flag pointer.
Every figure is printed before it is asserted.

Measured on an MI355X (largest deviation from the reference's doubles, eps * scale; allowance in brackets).  At
n = 257, three detectors: solar_f0 1.000 (8.99), orbital_f0 0.000 (10.02), total_f0 0.000 (9.38), solar_f150 2.903
(34.26), orbital_f150 1.743 (24.08), total_f150 2.732 (35.56); shorter runs are heads of these (n = 1: 0 / 0 / 0 / 0.581 /
0.871 / 0.546; n = 63, 64, 65: 1.000 / 0 / 0 / 1.760 / 1.743 / 1.639).  17 detectors: total_f0 1.000, total_f150 3.278.
Accumulation into a signal of order 1 with scale -2.5 and permuted rows, less the rounding of the sum: 0.942 / 0.000 /
0.613 at freq 0, 0.970 / 0.055 / 0.913 at 150 GHz.  Mask 0: as with mask 1.  Views 0.000 (orbital_f0), 0.967
(total_f150).  The sample with |q| = 1.001: 0.000 / 1.639.  Operator on resident data: solar_f0 1.000, orbital_f150 1.664,
total_f0 0.001, total_f150 2.829; on host data 0.983 (its host path 0.000: bit-identical to the reference).  All exact
comparisons held; the module takes 3.5 s."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sim_dipole_case as sc  # noqa: E402

pytestmark = pytest.mark.gpu

INP = sc.inputs()
WHOLE = "whole"


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)
        accel_data_create(self.a, "test_dipole")
        accel_data_update_device(self.a, "test_dipole")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_dipole")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_dipole")


def intervals(spans):
    from toast_amd.capi import interval_dtype

    iv = np.zeros(len(spans), dtype=interval_dtype)
    for k, (first, last) in enumerate(spans):
        iv[k]["first"], iv[k]["last"] = first, last
    return iv


def abi(case, n=sc.N, dets=(0, 1, 2), rows=None, n_rows=None, before=None, scale=1.0, mask=1, use_flags=True,
        views=WHOLE, launches=None):
    """``capi.dev.sim_dipole`` on the head ``n`` of the case's inputs; returns the signal [n_rows, n] afterwards.
    ``launches``: groups of positions in ``dets``, one call each (default: one call for all)."""
    from toast_amd import capi

    mode, freq = sc.case_parts(case)
    dets = list(dets)
    rows = list(range(len(dets))) if rows is None else list(rows)
    n_rows = len(dets) if n_rows is None else n_rows
    start = np.zeros((n_rows, n)) if before is None else np.ascontiguousarray(before[:n_rows, :n])
    vel, solar = sc.velocities(INP, mode)
    spans = [(0, n)] if views is WHOLE else views
    bufs = dict(bore=Dev(INP["bore"][:n]), flags=Dev(INP["flags"][:n]), vel=Dev(INP["vel"][:n]), sig=Dev(start))
    try:
        for group in (launches or [list(range(len(dets)))]):
            capi.dev.sim_dipole(INP["fp"][[dets[k] for k in group]], bufs["bore"].ptr, [rows[k] for k in group],
                                bufs["sig"].ptr, n_rows, n, intervals(spans),
                                bufs["flags"].ptr if use_flags else 0, n if use_flags else 0, mask,
                                0 if vel is None else bufs["vel"].ptr, solar, INP["cmb"], freq, scale)
        return bufs["sig"].get()
    finally:
        for b in bufs.values():
            b.free()


def check(label, got, case, dets, n, mask=1, factor=1.0, before=None):
    want = sc.accumulated(0.0 if before is None else before, sc.expected(case, mask)[list(dets), :n], factor)
    dev, ok = sc.deviation(got, want, case, INP, factor=factor, before=before)
    print(f"{label}: deviation {dev:.3f} eps*scale, allowed {10 * float(sc.gold()['err_' + case]):.2f}"
          f"{'' if before is None else ' + eps*|before|'}")
    assert ok, label
    return dev


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_detector_tile_is_what_the_fixture_straddles():
    from toast_amd import capi

    assert capi.dev.sim_dipole_det_tile() + 1 == sc.N_DET


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("case", sc.CASES)
def test_values_at_every_length(case, n):
    got = abi(case, n=n)
    assert np.all(got != 0)
    check(f"{case} n={n}", got, case, (0, 1, 2), n)


@pytest.mark.parametrize("n_det", [1, 3, sc.N_DET])
@pytest.mark.parametrize("case", ["total_f0", "total_f150"])
def test_values_at_every_detector_count(case, n_det):
    dets = tuple(range(n_det))
    check(f"{case} n_det={n_det}", abi(case, dets=dets), case, dets, sc.N)


@pytest.mark.parametrize("case", sc.CASES)
def test_accumulation_negative_scale_and_permuted_rows(case):
    """A signal of order 1, scale -2.5, detectors (2, 0, 3, 1) into rows (4, 1, 0, 3) of a six-row buffer: rows 2 and 5
    keep their bits."""
    dets, rows, n_rows = (2, 0, 3, 1), (4, 1, 0, 3), 6
    before = INP["noise"][:n_rows]
    got = abi(case, dets=dets, rows=rows, n_rows=n_rows, before=before, scale=-2.5)
    check(f"{case} accumulate", got[list(rows)], case, dets, sc.N, factor=-2.5, before=before[list(rows)])
    assert same_bits(got[[2, 5]], before[[2, 5]])
    assert np.all(got[list(rows)] != before[list(rows)])


@pytest.mark.parametrize("case", ["solar_f0", "orbital_f150", "total_f0", "total_f150"])
def test_flag_mask(case):
    """Bit 1 lies on a third of the samples (every other test runs with mask 1): mask 0 ignores it, as a NULL flag
    pointer does; mask 2 differs from both."""
    masked = abi(case)
    open_ = abi(case, mask=0)
    check(f"{case} mask 0", open_, case, (0, 1, 2), sc.N, mask=0)
    assert same_bits(open_, abi(case, use_flags=False))
    hit = (INP["flags"] & 1) != 0
    assert np.all(masked[:, hit] != open_[:, hit]) and same_bits(masked[:, ~hit], open_[:, ~hit])
    two = abi(case, mask=2)
    hit2 = (INP["flags"] & 2) != 0
    assert same_bits(two[:, ~hit2], open_[:, ~hit2]) and np.all(two[:, hit2] != open_[:, hit2])
    # a flagged sample sees the detector alone: the same value wherever the boresight points
    if case.startswith("solar"):
        flagged = np.flatnonzero(hit)
        assert same_bits(masked[:, flagged], np.repeat(masked[:, flagged[:1]], flagged.size, axis=1))


@pytest.mark.parametrize("case", ["orbital_f0", "total_f150"])
def test_views(case):
    before = INP["noise"][:3]
    whole = abi(case, before=before)
    spans = [(5, 70), (90, 90), (131, 250)]
    got = abi(case, before=before, views=spans)
    inside = np.zeros(sc.N, dtype=bool)
    for first, last in spans:
        inside[first:last] = True
    assert same_bits(got[:, ~inside], before[:, ~inside])
    assert same_bits(got[:, inside], whole[:, inside])
    want = sc.accumulated(before, sc.expected(case)[:3])[:, inside]
    dev, ok = sc.deviation(got[:, inside], want, case, INP, before=before[:, inside])
    print(f"{case} views: deviation {dev:.3f} eps*scale")
    assert ok
    assert same_bits(abi(case, before=before, views=[(0, 64), (64, sc.N)]), whole)
    assert same_bits(abi(case, before=before, views=[]), before)
    assert same_bits(abi(case, before=before, views=[(17, 17)]), before)


@pytest.mark.parametrize("case", ["solar_f150", "total_f0"])
def test_one_launch_of_three_detectors_is_three_launches_of_one(case):
    before = INP["noise"][:3]
    assert same_bits(abi(case, before=before), abi(case, before=before, launches=[[0], [1], [2]]))


@pytest.mark.parametrize("case", ["total_f0", "total_f150"])
def test_scaled_boresight_is_normalised(case):
    """Sample 102 holds 1.001 times a unit quaternion: the direction is that of the unit quaternion (an unnormalised
    rotation would be off by 2e-3 of the signal, 1e13 eps)."""
    s = sc.SCALED_SAMPLE
    assert INP["flags"][s] == 0
    got = abi(case, n=s + 1)
    want = sc.accumulated(0.0, sc.expected(case)[:3, s:s + 1])
    dev, ok = sc.deviation(got[:, s:], want, case, INP)
    print(f"{case} sample {s} (|q| = 1.001): deviation {dev:.3f} eps*scale")
    assert ok


def test_no_velocity_is_an_error_and_nothing_is_launched():
    from toast_amd import capi

    before = INP["noise"][:3]
    sig, bore = Dev(before), Dev(INP["bore"])
    try:
        with pytest.raises(RuntimeError, match="velocity"):
            capi.dev.sim_dipole(INP["fp"][:3], bore.ptr, [0, 1, 2], sig.ptr, 3, sc.N, intervals([(0, sc.N)]))
        assert b"velocity" in capi.lib().toast_hip_last_error()
        assert same_bits(sig.get(), before)
        with pytest.raises(RuntimeError, match="outside det_data"):
            capi.dev.sim_dipole(INP["fp"][:3], bore.ptr, [0, 1, 3], sig.ptr, 3, sc.N, intervals([(0, sc.N)]),
                                solar=INP["solar"])
        with pytest.raises(RuntimeError, match="outside"):
            capi.dev.sim_dipole(INP["fp"][:3], bore.ptr, [0, 1, 2], sig.ptr, 3, sc.N, intervals([(0, sc.N + 1)]),
                                solar=INP["solar"])
        assert same_bits(sig.get(), before)
    finally:
        sig.free()
        bore.free()


# ---------------------------------------------------------------------------------------------- the operator
VIEWS = [(3, 40), (40, 41), (90, 90), (120, 200)]
DETS = ["D0", "D1", "D2"]


def operator_data(units="K"):
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults

    fp = Focalplane(DETS, INP["fp"][:3], sample_rate=1.0)
    ob = Observation(None, Telescope("dipole_tele", fp), sc.N, name="obs_dipole")
    ob.set_times(np.arange(sc.N, dtype=np.float64))
    ob.shared.create(defaults.boresight_radec, INP["bore"].copy())
    ob.shared.create(defaults.shared_flags, INP["flags"].copy())
    ob.shared.create(defaults.velocity, INP["vel"].copy())
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=units)
    ob.detdata[defaults.det_data].data[:] = INP["noise"][:3]
    ob.intervals.create("some", VIEWS)
    data = Data()
    data.obs.append(ob)
    return data, ob


@pytest.mark.parametrize("case", ["solar_f0", "orbital_f150", "total_f0", "total_f150"])
def test_operator_on_resident_data(case):
    from toast_amd.data import defaults
    from toast_amd.ops import SimDipole

    mode, freq = sc.case_parts(case)
    data, ob = operator_data(units="mK")
    sig = ob.detdata[defaults.det_data]
    sig.accel_create(defaults.det_data)
    sig.accel_update_device()
    SimDipole(coord="G", view="some", mode=mode, freq=freq, subtract=True).apply(data, use_accel=True)
    # resident data stays resident: the device copy is the current one until somebody asks for the host's
    assert sig.accel_in_use()
    for key in (defaults.boresight_radec, defaults.shared_flags, defaults.velocity):
        assert not ob.shared[key].accel_in_use() and not ob.shared[key].accel_exists(), key
    assert np.array_equal(ob.shared[defaults.boresight_radec].data, INP["bore"])
    assert np.array_equal(ob.shared[defaults.shared_flags].data, INP["flags"])
    assert np.array_equal(ob.shared[defaults.velocity].data, INP["vel"])
    got = sig.data.copy()
    if sig.accel_exists():
        sig.accel_delete()
    before = INP["noise"][:3]
    inside = np.zeros(sc.N, dtype=bool)
    for first, last in VIEWS:
        inside[first:last] = True
    assert same_bits(got[:, ~inside], before[:, ~inside])
    want = sc.accumulated(before, sc.expected(case)[:3], -1.0e3)[:, inside]
    dev, ok = sc.deviation(got[:, inside], want, case, INP, factor=-1.0e3, before=before[:, inside])
    print(f"operator {case}: deviation {dev:.3f} eps*scale")
    assert ok
    # the same bits as the C ABI call with the operator's arguments
    assert same_bits(got, abi(case, before=before, scale=-1.0e3, views=VIEWS))


def test_operator_on_host_data_eager_and_lazy():
    """Data that is not resident is uploaded; with eager coherence (``data.lazy_host`` False) the signal is written back
    and released, otherwise it stays current on the device and the host copy follows on access.  shared_flags=None is
    a NULL flag pointer; the host path's result is within the same allowance."""
    from toast_amd.data import defaults
    from toast_amd.ops import SimDipole

    case = "total_f0"
    results = {}
    for use_accel, lazy in ((False, False), (True, False), (True, True)):
        data, ob = operator_data()
        data.lazy_host = lazy
        SimDipole(coord="G", shared_flags=None).apply(data, use_accel=use_accel)
        sig = ob.detdata[defaults.det_data]
        assert sig.accel_in_use() == lazy and sig.accel_exists() == lazy
        results[use_accel, lazy] = sig.data.copy()
        if sig.accel_exists():
            sig.accel_delete()
        for key in (defaults.boresight_radec, defaults.velocity):
            assert not ob.shared[key].accel_in_use() and not ob.shared[key].accel_exists(), key
    assert same_bits(results[True, True], results[True, False])
    results = {False: results[False, False], True: results[True, False]}
    before = INP["noise"][:3]
    assert same_bits(results[True], abi(case, before=before, use_flags=False))
    dev, ok = sc.deviation(results[True], sc.accumulated(before, sc.expected(case, 0)[:3]), case, INP, before=before)
    dev_h, ok_h = sc.deviation(results[False], sc.accumulated(before, sc.expected(case, 0)[:3]), case, INP, before=before)
    print(f"operator, eager: device {dev:.3f}, host path {dev_h:.3f} eps*scale")
    assert ok and ok_h
