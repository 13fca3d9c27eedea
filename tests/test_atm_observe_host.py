"""AtmSim / ObserveAtmosphere without a GPU: the NumPy path against the reference's own outputs
(tests/golden/atm_observe.npz, written by tests/golden/make_golden_atm_observe.py from toast::atm_sim_observe and the
reference's ObserveAtmosphere._exec), the conditions the fixture stores, the validation errors, and the signature of
``_libtoast_hip.atm_sim_observe``.

Exact: every status, which samples were skipped (tod bits unchanged), which failed, every flag byte, operator outputs
at flagged samples.  Values: within ten times the reference's own stored deviation from the long-double chain, in the
same units eps * scale_i (the rule of tests/test_gpu_templates.py).  Measured here: the NumPy path of ``AtmSim.observe``
reproduces the reference's tod bit for bit in all eleven cases (deviation 1.2 .. 7.7, the reference's own figure); the
operator's host path deviates 15.3 where the reference deviates 10.0 (NumPy's asin / atan2 instead of libm's)."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import atm_observe_case as ac  # noqa: E402
from toast_amd import atm  # noqa: E402

G = np.load(ac.GOLD_PATH)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_numpy_path_against_the_reference(name):
    times, az, el, tod0 = ac.pointing(name)
    tod = tod0.copy()
    statuses = []
    for vol in ac.case_volumes(name):
        sim = ac.make_sim(vol)
        statuses.append(sim.observe(times, az, el, tod, ac.CASES[name].get("fixed_r", -1.0), use_accel=False))
        sim.close()
    ac.check_case(name, tod, statuses, tod0)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_fixture_conditions(name):
    """What keeps the comparison honest: no step point within 1e-9 cell widths of a cell face, no ray in cell
    (0, 0, 0), failures present but not dominant where the volume has holes; recomputed, not only read."""
    assert float(G[f"{name}_face"]) >= 1e-9
    assert not bool(G[f"{name}_cell0"])
    times, az, el, _ = ac.pointing(name)
    failed = np.zeros(times.size, dtype=bool)
    for k, vol in enumerate(ac.case_volumes(name)):
        ld = ac.longdouble_observe(vol, times, az, el, ac.CASES[name].get("fixed_r", -1.0))
        assert ld["face"] >= 1e-9 and not ld["cell0"]
        assert np.array_equal(ld["failed"], G[f"{name}_failed{k}"])
        assert np.array_equal(ld["skip"], G[f"{name}_skip{k}"])
        failed |= ld["failed"]
    if name in ac.HOLE_CASES:
        assert 1 <= failed.sum() <= times.size // 4
    else:
        assert failed.sum() == 0
    assert float(G[f"{name}_ref_dev"]) > 0 or times.size == 1


def test_cases_cover_the_edges():
    assert sorted({c["n"] for c in ac.CASES.values()}) == [1, 63, 64, 65, 257]
    steps = {n: [atm.ray_steps(g["xstep"], g["rmin"], g["rmax"], ac.CASES[n].get("fixed_r", -1.0), g["elmax"], g["zmax"])
                 for g, *_ in ac.case_volumes(n)] for n in ac.CASES}
    assert steps["full_n65"][0] == (15.0, 14)          # ended by rmax
    assert steps["zmax_n65"][0] == (15.0, 12)          # ended by r sin(elmax) >= zmax
    assert steps["rmin_n65"][0][0] == 45.0             # rmin above 1.5 xstep: 15 + 10 + 10 + 10
    assert steps["fixed_n64"][0] == (73.0, 1)
    assert steps["accum_n257"][1][0] == 85.0
    t, az, el, tod0 = ac.pointing("accum_n257")
    assert np.all(tod0 != 0) and np.any(az > 2 * np.pi) and np.any(az < 2 * np.pi)
    g = ac.BASE
    assert np.any(el > g["elmax"]) and np.any(el < g["elmin"]) and g["wx"] * g["wy"] * g["wz"] != 0


def test_operator_host_path():
    data, ob = ac.operator_data()
    ac.operator().apply(data, use_accel=False)
    ac.check_operator(ob.detdata["signal"].data, ob.detdata["flags"].data)


def test_operator_errors():
    from toast_amd.ops import ObserveAtmosphere

    data, ob = ac.operator_data()
    with pytest.raises(RuntimeError, match="absorption"):
        ObserveAtmosphere().apply(data, use_accel=False)
    with pytest.raises(NotImplementedError, match="sample_rate"):
        ac.operator(sample_rate=10.0).apply(data, use_accel=False)
    with pytest.raises(NotImplementedError, match="fade_time"):
        ac.operator(fade_time=1.0).apply(data, use_accel=False)
    # a slab that ends before the detector's last good sample / that is narrower than the scan
    sims = data["atm_sim"][ob.session.name]
    late = ac.volume("holes")
    late[0]["tmax"] = 105.0
    sims[0][0] = ac.make_sim(late)
    with pytest.raises(RuntimeError, match="Detector time"):
        ac.operator().apply(data, use_accel=False)
    narrow = ac.volume("holes")
    narrow[0]["azmax"] = 0.5
    sims[0][0] = ac.make_sim(narrow)
    with pytest.raises(RuntimeError, match="Detector Az/El"):
        ac.operator().apply(data, use_accel=False)


def test_std_range_from_the_reduction():
    """The device reduction hands over az of the first good sample and the extent of the wrapped offsets; where they
    span less than pi this is np.unwrap's range."""
    from toast_amd.ops import ObserveAtmosphere as Op

    rng = np.random.default_rng(5)
    for start in (0.1, 3.0, 6.2):
        az = np.mod(start + np.cumsum(rng.uniform(-0.02, 0.025, 400)), 2 * np.pi)
        d = az - az[0]
        d = np.where(d >= np.pi, d - 2 * np.pi, d)
        d = np.where(d < -np.pi, d + 2 * np.pi, d)
        assert d.max() - d.min() < np.pi
        lo, hi = Op._std_range_of(az[0] + d.min(), az[0] + d.max())
        want = Op._std_range(az)
        assert abs(lo - want[0]) < 1e-12 and abs(hi - want[1]) < 1e-12


def test_atmsim_validation():
    geom, ci, fi, re = ac.volume("holes")

    def build(**over):
        g = dict(geom)
        arrays = dict(compressed_index=ci, full_index=fi, realization=re)
        for k, v in over.items():
            (arrays if k in arrays else g)[k] = v
        return ac.make_sim((g, arrays["compressed_index"], arrays["full_index"], arrays["realization"]))

    sim = build()
    assert (sim.azmin, sim.azmax, sim.elmin, sim.elmax, sim.tmin, sim.tmax) == (0.3, 0.7, 0.6, 0.9, 100.0, 112.0)
    assert sim._nelem == re.size and sim._nn == ci.size and sim._xstride == ac.NY * ac.NZ and sim._cached
    for over, text in ((dict(azmin=0.7), "azmin >= azmax"), (dict(elmin=-0.1), "elmin < 0"),
                       (dict(elmax=1.6), "elmax > pi/2"), (dict(elmin=0.95), "elmin >= elmax"),
                       (dict(tmin=112.0), "tmin >= tmax"), (dict(nx=ac.NX + 1), "compressed_index"),
                       (dict(xstride=ac.NY * ac.NZ + 1), "strides"), (dict(zstride=0), "strides"),
                       (dict(full_index=fi[:-1]), "not consistent"), (dict(realization=re[:-1]), "not consistent"),
                       (dict(compressed_index=ci[:-1]), "compressed_index"), (dict(xstep=0.0), "positive")):
        with pytest.raises(RuntimeError, match=text):
            build(**over)
    with pytest.raises(NotImplementedError, match="CHOLMOD"):
        sim.simulate()
    t, az, el, tod = ac.pointing("holes_n65")
    with pytest.raises(RuntimeError, match="not consistent"):
        sim.observe(t, az[:-1], el, tod, use_accel=False)
    sim.close()
    with pytest.raises(RuntimeError, match="no cached observation"):
        sim.observe(t, az, el, tod, use_accel=False)


def test_malformed_volume_gives_status_not_a_fault():
    """Compressed entries far outside [0, nelem) and strides that leave the box end as status 1 with tod += 0."""
    geom, ci, fi, re = ac.volume("full")
    bad = ci.copy()
    bad[::7] = 2**40
    bad[3::11] = -(2**35)
    sim = ac.make_sim((geom, bad, fi, re))
    t, az, el, tod = ac.pointing("full_n64")
    assert sim.observe(t, az, el, tod, use_accel=False) == 1
    assert np.all(tod == 0)


def test_binding_signature():
    """_libtoast_hip.atm_sim_observe takes the argument list of the reference binding as atm.py:464-503 calls it."""
    from toast_amd import accel

    doc = accel.native().atm_sim_observe.__doc__
    names = ["times", "az", "el", "tod", "T0", "azmin", "azmax", "elmin", "elmax", "tmin", "tmax", "rmin", "rmax",
             "fixed_r", "zatm", "zmax", "wx", "wy", "wz", "xstep", "ystep", "zstep", "xstart", "delta_x", "ystart",
             "delta_y", "zstart", "delta_z", "maxdist", "nx", "ny", "nz", "xstride", "ystride", "zstride",
             "compressed_index", "full_index", "realization"]
    sig = doc.split("\n")[0]
    got = [part.strip().split(":")[0] for part in sig[sig.index("(") + 1:sig.rindex(")")].split(",")]
    assert got == names
    assert "-> int" in sig
    assert list(inspect.signature(atm.AtmSim.observe).parameters)[:6] == ["self", "times", "az", "el", "tod", "fixed_r"]
