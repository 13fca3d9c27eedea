"""toast_amd.dipole and ops.SimDipole without a GPU: ``dipole.dipole`` against the reference's own outputs
(tests/golden/sim_dipole.npz, written by tests/golden/make_golden_sim_dipole.py from the reference's ``dipole``), the
coordinate rotations of ``solar_velocity`` against the IAU numbers, and the operator's host path.

Values: within ten times the reference's own stored deviation from the long-double evaluation, in the same units
eps * scale (the rule of tests/test_gpu_templates.py and tests/test_gpu_atm_observe.py).  Measured here: the NumPy path
reproduces the reference's timestreams bit for bit in all six cases, flagged and unflagged."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sim_dipole_case as sc  # noqa: E402
from toast_amd import dipole as dp  # noqa: E402
from toast_amd import synth  # noqa: E402
from toast_amd.traits import TraitError  # noqa: E402

INP = sc.inputs()


def test_fixture_pins_the_inputs():
    g = sc.gold()
    for key in ("bore", "fp", "vel", "solar", "flags", "noise"):
        assert np.array_equal(g[key], INP[key]), key
    assert float(g["cmb"]) == dp.t_cmb == 2.72548
    assert np.all(INP["vel"] != 0) and np.all(INP["solar"] != 0)
    assert abs(np.sum(INP["bore"][sc.SCALED_SAMPLE] ** 2) - 1.001 ** 2) < 1e-12
    assert 80 <= np.count_nonzero(INP["flags"] & 1) <= 95 and np.any(INP["flags"] == 2)
    # the detectors are one to five degrees off axis
    off = np.degrees(np.arccos(dp.rotate_zaxis(INP["fp"])[:, 2]))
    assert off.min() > 0.5 and off.max() < 5.0
    for case in sc.CASES:
        err = float(g["err_" + case])
        assert (0.5 < err < 1.5) if case.endswith("f0") else (1.0 < err < 5.0), (case, err)


@pytest.mark.parametrize("case", sc.CASES)
def test_dipole_against_the_reference(case):
    mode, freq = sc.case_parts(case)
    vel, solar = sc.velocities(INP, mode)
    identical = True
    for mask, n_det in ((1, sc.case_dets(case)), (0, sc.N_SMALL)):
        want = sc.expected(case, mask)
        got = np.stack([dp.dipole(sc.pointing(INP, d, mask), vel=vel, solar=solar, cmb=INP["cmb"], freq=freq)
                        for d in range(n_det)])
        dev, ok = sc.deviation(got, want, case, INP)
        same = np.array_equal(got.view(np.uint64), want.view(np.uint64))
        identical &= same
        print(f"{case} mask {mask}: deviation {dev:.3f} eps*scale (allowed {10 * float(sc.gold()['err_' + case]):.2f}), "
              f"bit-identical {same}")
        assert ok
    assert np.array_equal(vel, INP["vel"]) if vel is not None else True      # the caller's velocity is not modified
    print(f"{case}: NumPy path bit-identical to the reference: {identical}")


def test_dipole_needs_a_velocity():
    with pytest.raises(RuntimeError, match="required"):
        dp.dipole(sc.pointing(INP, 0, 0))


def lonlat(v):
    return np.degrees(np.arctan2(v[1], v[0])) % 360.0, np.degrees(np.arcsin(v[2] / np.sqrt(np.sum(v * v))))


def test_solar_velocity_and_rotations():
    g = dp.solar_velocity("G")
    lon, lat = lonlat(g)
    assert abs(np.sqrt(np.sum(g * g)) - dp.solar_speed) < 1e-12
    assert abs(lon - dp.solar_gal_lon) < 1e-4 and abs(lat - dp.solar_gal_lat) < 1e-4
    g2c = dp.galactic_to_equatorial()
    assert np.max(np.abs(g2c @ g2c.T - np.eye(3))) < 1e-15 and abs(np.linalg.det(g2c) - 1.0) < 1e-15
    lon, lat = lonlat(g2c @ np.array([0.0, 0.0, 1.0]))
    assert abs(lon - 192.85948) < 1e-4 and abs(lat - 27.12825) < 1e-4
    lon, lat = lonlat(g2c @ np.array([1.0, 0.0, 0.0]))
    assert abs(lon - 266.40499) < 1e-4 and abs(lat + 28.93617) < 1e-4
    c2e = dp.equatorial_to_ecliptic()
    assert np.max(np.abs(c2e @ np.array([1.0, 0.0, 0.0]) - np.array([1.0, 0.0, 0.0]))) < 1e-15
    _, lat = lonlat(c2e @ np.array([0.0, 0.0, 1.0]))
    assert abs(lat - (90.0 - 23.4392911)) < 1e-3
    # the rotated velocities keep their length, and "E" is "C" rotated
    c, e = dp.solar_velocity("C"), dp.solar_velocity("E")
    assert np.allclose(c, g2c @ g, rtol=0, atol=1e-12) and np.allclose(e, c2e @ c, rtol=0, atol=1e-12)
    assert abs(np.sqrt(np.sum(e * e)) - dp.solar_speed) < 1e-12
    with pytest.raises(RuntimeError, match="coordinate"):
        dp.solar_velocity("X")


def test_orbital_velocity_stand_in():
    t = np.array([0.0, 0.25, 0.5]) * 365.25 * 86400
    v = synth.orbital_velocity(t)
    assert v.shape == (3, 3) and np.all(v[:, 2] == 0)
    assert np.allclose(np.sqrt(np.sum(v * v, axis=1)), 29.78, rtol=1e-15)
    assert np.allclose(v, 29.78 * np.array([[0, 1, 0], [-1, 0, 0], [0, -1, 0]]), atol=1e-13)
    assert np.allclose(synth.orbital_velocity(np.zeros(1), speed_kms=2.0, period_s=10.0, phase=np.pi / 2),
                       [[-2.0, 0.0, 0.0]], atol=1e-15)


# ---------------------------------------------------------------------------------------------- the operator
DETS = ["D0", "D1", "D2"]
VIEWS = [(3, 40), (40, 41), (90, 90), (120, 200)]


def small_data(units="K", signal=None, with_flags=True):
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults

    fp = Focalplane(DETS, INP["fp"][:3], sample_rate=1.0)
    ob = Observation(None, Telescope("dipole_tele", fp), sc.N, name="obs_dipole")
    ob.set_times(np.arange(sc.N, dtype=np.float64))
    ob.shared.create(defaults.boresight_radec, INP["bore"].copy())
    if with_flags:
        ob.shared.create(defaults.shared_flags, INP["flags"].copy())
    ob.shared.create(defaults.velocity, INP["vel"].copy())
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=units)
    if signal is not None:
        ob.detdata[defaults.det_data].data[:] = signal
    ob.intervals.create("some", VIEWS)
    data = Data()
    data.obs.append(ob)
    return data, ob


def operator(**kw):
    from toast_amd.ops import SimDipole

    return SimDipole(coord="G", **kw)


def in_views():
    inside = np.zeros(sc.N, dtype=bool)
    for first, last in VIEWS:
        inside[first:last] = True
    return inside


@pytest.mark.parametrize("mode", sc.MODES)
def test_operator_host_path(mode):
    """Views are respected, a flagged sample gets the value of the identity boresight, values are the fixture's."""
    case = f"{mode}_f150"
    data, ob = small_data(signal=INP["noise"][:3])
    operator(view="some", mode=mode, freq=150.0e9).apply(data, use_accel=False)
    got = ob.detdata["signal"].data
    inside = in_views()
    assert np.array_equal(got[:, ~inside], INP["noise"][:3][:, ~inside])
    want = sc.accumulated(INP["noise"][:3], sc.expected(case)[:3])
    dev, ok = sc.deviation(got[:, inside], want[:, inside], case, INP, before=INP["noise"][:3][:, inside])
    print(f"operator host path {case}: deviation {dev:.3f} eps*scale")
    assert ok
    # the identity boresight: the detector's own quaternion is the pointing
    vel, solar = sc.velocities(INP, mode)
    s = 4
    assert INP["flags"][s] & 1
    own = dp.dipole(INP["fp"][1][None, :], vel=None if vel is None else vel[s:s + 1], solar=solar, freq=150.0e9)
    assert got[1, s] == INP["noise"][1, s] + own[0]


def test_operator_add_then_subtract_and_units():
    data, ob = small_data(signal=INP["noise"][:3])
    operator().apply(data, use_accel=False)
    added = ob.detdata["signal"].data.copy()
    assert np.max(np.abs(added - INP["noise"][:3])) > 1e-3
    operator(subtract=True).apply(data, use_accel=False)
    back = ob.detdata["signal"].data
    assert np.max(np.abs(back - INP["noise"][:3])) <= 2 * sc.EPS * np.max(np.abs(INP["noise"][:3]))
    data_k, ob_k = small_data()
    data_m, ob_m = small_data(units="mK")
    for d in (data_k, data_m):
        operator(mode="solar").apply(d, use_accel=False)
    k, m = ob_k.detdata["signal"].data, ob_m.detdata["signal"].data
    assert np.max(np.abs(k)) > 1e-3 and np.array_equal(m, 1.0e3 * k)
    data_x, _ = small_data(units="Jy")
    with pytest.raises(RuntimeError, match="no conversion"):
        operator().apply(data_x, use_accel=False)


def test_operator_without_shared_flags_and_created_signal():
    """shared_flags=None: no flagging; a missing signal is created in det_data_units."""
    from toast_amd.data import defaults

    data, ob = small_data(with_flags=False)
    del ob.detdata[defaults.det_data]
    operator(shared_flags=None, det_data_units="uK", mode="total").apply(data, use_accel=False)
    assert ob.detdata["signal"].units == "uK"
    got = ob.detdata["signal"].data
    want = 1.0e6 * sc.expected("total_f0", mask=0)[:3]
    dev, ok = sc.deviation(got, want, "total_f0", INP, factor=1.0e6)
    print(f"operator without flags: deviation {dev:.3f} eps*scale")
    assert ok


def test_operator_traits():
    from toast_amd.ops import SimDipole

    op = SimDipole()
    assert (op.det_data, op.det_data_units, op.view, op.boresight, op.shared_flags, op.shared_flag_mask) == (
        "signal", "K", None, "boresight_radec", "flags", 1)
    assert (op.velocity, op.subtract, op.mode, op.coord, op.freq) == ("velocity", False, "total", "E", 0.0)
    assert (op.solar_speed, op.solar_gal_lat, op.solar_gal_lon, op.cmb) == (370.08, 48.25, 263.99, 2.72548)
    for bad in (dict(mode="both"), dict(coord="X"), dict(shared_flag_mask=-1)):
        with pytest.raises(TraitError):
            SimDipole(**bad)
    with pytest.raises(TraitError):
        op.mode = "lunar"
    req, prov = SimDipole(view="some").requires(), op.provides()
    assert req["shared"] == ["boresight_radec", "flags"] and req["detdata"] == ["signal"] and req["intervals"] == ["some"]
    assert prov["detdata"] == ["signal"] and prov["shared"] == []
