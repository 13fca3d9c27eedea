"""GPU: the atmosphere-observation kernels (csrc/atm_observe.hip), ``AtmSim.observe`` on the device and
``ops.ObserveAtmosphere`` on device-resident data, against the reference's own outputs (tests/golden/atm_observe.npz).

Exact: every status, which samples were skipped (tod bits unchanged), which failed, every flag byte, operator outputs at
flagged samples; one launch of three rows and three launches of one row give the same bits, and so do the int32 / int64
index and the kernel with and without its one-cell cache.  Values: within ten times the reference's own stored deviation
from the long-double chain, in units eps * scale_i (the rule of tests/test_gpu_templates.py).  Every figure is printed
before it is asserted.

Measured on an MI355X (deviation of the device / of the reference, eps * scale_i): full_n1 1.242 / 1.242, full_n63
7.665 / 7.665, full_n64 4.900 / 5.087, full_n65 3.718 / 3.858, full_n257 6.846 / 6.846, holes_n257 5.360 / 6.178, holes_n65
5.703 / 5.703, zmax_n65 4.786 / 3.498, rmin_n65 5.361 / 4.811, fixed_n64 7.446 / 7.446, accum_n257 7.200 / 7.534 -- the C
ABI, ``AtmSim.observe`` and the binding alike; operator on resident data 15.287 / 9.960.  All exact comparisons held."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import atm_observe_case as ac  # noqa: E402

pytestmark = pytest.mark.gpu


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)
        accel_data_create(self.a, "test_atm")
        accel_data_update_device(self.a, "test_atm")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_atm")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_atm")


def abi_observe(name, index32=True, cell_cache=False):
    """toast_hip_atm_observe_dev on the slabs of a case: (tod after, statuses, tod before)."""
    from toast_amd import capi

    times, az, el, tod0 = ac.pointing(name)
    n = times.size
    bufs = [Dev(x) for x in (times, az, el, tod0)]
    statuses = []
    try:
        for vol in ac.case_volumes(name):
            sim = ac.make_sim(vol)
            geom = sim.geometry(ac.CASES[name].get("fixed_r", -1.0))
            idx = sim._compressed_index
            if index32:
                idx = np.where((idx >= 0) & (idx < sim._nelem), idx, -1).astype(np.int32)
            d_idx, d_real = Dev(idx), Dev(sim._realization)
            try:
                statuses.append(capi.dev.atm_observe(geom, d_idx.ptr, index32, d_real.ptr, 1, n, bufs[0].ptr, 0,
                                                     bufs[1].ptr, bufs[2].ptr, n, bufs[3].ptr, n, cell_cache=cell_cache))
            finally:
                d_idx.free()
                d_real.free()
                sim.close()
        return bufs[3].get(), statuses, tod0
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", list(ac.CASES))
def test_c_abi_against_the_reference(name):
    tod, statuses, tod0 = abi_observe(name)
    ac.check_case(name, tod, statuses, tod0)


@pytest.mark.parametrize("name", ["holes_n257", "rmin_n65", "fixed_n64"])
def test_kernel_options_give_the_same_bits(name):
    base, st, _ = abi_observe(name)
    for index32, cache in ((False, False), (True, True), (False, True)):
        tod, st2, _ = abi_observe(name, index32=index32, cell_cache=cache)
        assert st2 == st
        assert np.array_equal(tod.view(np.uint64), base.view(np.uint64)), (name, index32, cache)


@pytest.mark.parametrize("name", list(ac.CASES))
def test_atmsim_observe_on_the_device(name):
    times, az, el, tod0 = ac.pointing(name)
    tod = tod0.copy()
    statuses = []
    for vol in ac.case_volumes(name):
        sim = ac.make_sim(vol)
        statuses.append(sim.observe(times, az, el, tod, ac.CASES[name].get("fixed_r", -1.0), use_accel=True))
        # the volume stays resident between calls and goes with close()
        assert sim._dev_index is not None and sim._dev_index.on_device
        sim.close()
        assert sim._dev_index is None
    ac.check_case(name, tod, statuses, tod0)


def test_binding_on_host_arrays():
    """_libtoast_hip.atm_sim_observe with the reference's argument list (atm.py:464-503)."""
    from toast_amd.atm import atm_sim_observe

    name = "holes_n257"
    times, az, el, tod0 = ac.pointing(name)
    tod = tod0.copy()
    (g, ci, fi, re), = ac.case_volumes(name)
    status = atm_sim_observe(times, az, el, tod, g["T0"], g["azmin"], g["azmax"], g["elmin"], g["elmax"], g["tmin"],
                             g["tmax"], g["rmin"], g["rmax"], -1.0, g["zatm"], g["zmax"], g["wx"], g["wy"], g["wz"],
                             g["xstep"], g["ystep"], g["zstep"], g["xstart"], g["delta_x"], g["ystart"], g["delta_y"],
                             g["zstart"], g["delta_z"], g["maxdist"], g["nx"], g["ny"], g["nz"], g["ny"] * g["nz"],
                             g["nz"], 1, ci, fi, re)
    ac.check_case(name, tod, [status], tod0)


def test_batch_of_rows_gives_the_bits_of_single_rows():
    """observe_rows: one launch of 3 rows == three launches of one row (no result depends on the batch)."""
    from toast_amd.ops.sim_tod_atm_observe import quats_to_azel

    inp = ac.operator_inputs()
    n = ac.OP_N
    az = np.zeros((3, n))
    el = np.zeros((3, n))
    for d in range(3):
        az[d], el[d] = quats_to_azel(inp["quats"][d])
    sim = ac.make_sim(ac.volume("holes"))
    batch = inp["signal"].copy()
    st = sim.observe_rows(inp["times"], az, el, batch)
    single = inp["signal"].copy()
    st1 = [sim.observe_rows(inp["times"], az[d:d + 1].copy(), el[d:d + 1].copy(), single[d:d + 1]) for d in range(3)]
    sim.close()
    assert st == 1 and st1 == [1, 1, 1]
    assert np.array_equal(batch.view(np.uint64), single.view(np.uint64))
    assert np.any(batch != inp["signal"])


def resident_operator_run(detectors=None):
    from toast_amd.data import defaults

    data, ob = ac.operator_data()
    names = (defaults.det_data, defaults.det_flags, defaults.quats_azel, defaults.weights)
    for key in names:
        obj = ob.detdata[key]
        obj.accel_create(key)
        obj.accel_update_device()
    ac.operator().apply(data, detectors=detectors, use_accel=True)
    # resident data stays resident: the device copy is the current one until somebody asks for the host's
    assert ob.detdata[defaults.det_data].accel_in_use()
    signal = ob.detdata[defaults.det_data].data.copy()
    flags = ob.detdata[defaults.det_flags].data.copy()
    for key in names:
        if ob.detdata[key].accel_exists():
            ob.detdata[key].accel_delete()
    for slabs in data["atm_sim"][ob.session.name]:
        for sim in slabs:
            sim.close()
    return signal, flags


def test_operator_on_resident_data():
    signal, flags = resident_operator_run()
    ac.check_operator(signal, flags)


def test_operator_batch_gives_the_bits_of_single_detectors():
    signal, flags = resident_operator_run()
    inp = ac.operator_inputs()
    for d, det in enumerate(ac.OP_DETS):
        s1, f1 = resident_operator_run(detectors=[det])
        assert np.array_equal(s1[d].view(np.uint64), signal[d].view(np.uint64)), det
        assert np.array_equal(f1[d], flags[d])
        other = [k for k in range(3) if k != d]
        assert np.array_equal(s1[other], inp["signal"][other]) and np.array_equal(f1[other], inp["det_flags"][other])


def test_operator_device_matches_its_host_path_in_flags_and_errors():
    data, ob = ac.operator_data()
    sims = data["atm_sim"][ob.session.name]
    narrow = ac.volume("holes")
    narrow[0]["azmax"] = 0.5
    sims[0][0] = ac.make_sim(narrow)
    with pytest.raises(RuntimeError, match="Detector Az/El"):
        ac.operator().apply(data, use_accel=True)
    late = ac.volume("holes")
    late[0]["tmax"] = 105.0
    sims[0][0] = ac.make_sim(late)
    with pytest.raises(RuntimeError, match="Detector time"):
        ac.operator().apply(data, use_accel=True)


def test_malformed_volume_gives_status_not_a_fault():
    """Compressed entries far outside [0, nelem) (int64 index: the values reach the kernel as they are) end as status 1
    with tod += 0: the check comes before the load."""
    from toast_amd import capi

    geom, ci, fi, re = ac.volume("full")
    bad = ci.copy()
    bad[::7] = 2**40
    bad[3::11] = -(2**35)
    sim = ac.make_sim((geom, bad, fi, re))
    t, az, el, tod = ac.pointing("full_n64")
    bufs = [Dev(x) for x in (t, az, el, tod, bad, re)]
    try:
        st = capi.dev.atm_observe(sim.geometry(), bufs[4].ptr, False, bufs[5].ptr, 1, t.size, bufs[0].ptr, 0, bufs[1].ptr,
                                  bufs[2].ptr, t.size, bufs[3].ptr, t.size)
        assert st == 1
        assert np.all(bufs[3].get() == 0)
    finally:
        for b in bufs:
            b.free()
        sim.close()


def test_wide_scan_takes_the_host_range_and_matches_the_host_path():
    """A scan that wanders more than pi from its first good sample: the device reduction cannot reproduce np.unwrap's
    range, the operator gets it on the host for that detector, and the results are those of its host path -- flags
    and the set of observed samples exactly, values within 1e-11 of the largest (each path is within some ten
    eps * scale_i of the exact chain, fixture; scale_i is a sum of at most 15 terms of the size of the result)."""
    from toast_amd.ops import ObserveAtmosphere

    results = {}
    for use_accel in (False, True):
        data, ob, slabs = ac.wide_scan_data()
        for det in ("W0", "W1"):
            data["atm_sim"] = {ob.session.name: [[slabs[det]]]}
            ObserveAtmosphere(absorption="absorption").apply(data, detectors=[det], use_accel=use_accel)
        results[use_accel] = (ob.detdata["signal"].data.copy(), ob.detdata["flags"].data.copy())
        for sim in slabs.values():
            sim.close()
    (s_host, f_host), (s_dev, f_dev) = results[False], results[True]
    assert np.array_equal(f_dev, f_host)
    assert np.array_equal(s_dev != 0, s_host != 0)
    assert np.count_nonzero(s_host[0]) > 250 and 0 < np.count_nonzero(s_host[1]) < 20     # W1 wraps: az + 2 pi is skipped
    err = float(np.max(np.abs(s_dev - s_host)) / np.max(np.abs(s_host)))
    print(f"wide scan: device against host path {err:.3e} of the largest value")
    assert err <= 1e-11
