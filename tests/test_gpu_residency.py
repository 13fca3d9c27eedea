"""GPU: where every operator leaves the objects it touches.  ``det_data``, ``det_flags`` and ``shared_flags`` start
not registered on the device ("unregistered"), registered with the host copy current ("host") or current on the device
("device"); the operator runs under ``data.lazy_host`` True and False; afterwards ``(accel_exists(), accel_in_use())``
of every object it read or wrote is compared with the table below, and the timestreams and flags with those of the run
that started from host-only data -- bit for bit, except GroundFilter, whose fit sums with atomics (its own test's
bound: 1e-9 of the largest input).

The table was recorded from the operators while each still carried its own residency code; the shared helper of
``toast_amd.accel`` has to leave every object where they did.  Small cases on purpose: three or four detectors, a few
hundred to a few thousand samples, the builders of the per-operator tests."""

import functools

import numpy as np
import pytest

import demod_case as dc
import noise_estim_case as nc
import sim_noise_case as sc
import time_constant_case as tc
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.pixels import PixelData
from toast_amd.sim import create_ground_data

pytestmark = pytest.mark.gpu

STARTS = ("unregistered", "host", "device")
SIG, FLG, SHF = defaults.det_data, defaults.det_flags, defaults.shared_flags


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import capi

    assert capi.accel_enabled()
    capi.accel_assign_device(1, 0, 1.0, False)


def ground(n_det=3, n_samp=800):
    """A constant-elevation scan with several throws, noise plus a drift per detector, flagged samples."""
    data = create_ground_data(n_det=n_det, n_samp=n_samp, rate=20.0, n_obs=1, scan_rate_deg_s=10.0, seed=3)
    rng = np.random.default_rng(77)
    for ob in data.obs:
        sig = ob.detdata[SIG].data
        sig[:] = rng.standard_normal(sig.shape) + np.linspace(-1.0, 2.0, sig.shape[1])[None, :]
    return data


def put(obj, start):
    if start != "unregistered":
        obj.accel_create(obj._accel_name)
        if start == "device":
            obj.accel_update_device()


def start_from(data, start, extra=()):
    for ob in data.obs:
        for obj in [ob.detdata[SIG]] + [ob.detdata[k] for k in (FLG,) + tuple(extra) if k in ob.detdata]:
            put(obj, start)
        if SHF in ob.shared:
            put(ob.shared[SHF], start)


def objects(data, extra_detdata=(), extra_global=()):
    """name -> object, of everything the operator may have touched."""
    out = {}
    for iob, ob in enumerate(data.obs):
        for key in (SIG, FLG) + tuple(extra_detdata):
            if key in ob.detdata:
                out[f"{iob}:detdata:{key}"] = ob.detdata[key]
        if SHF in ob.shared:
            out[f"{iob}:shared:{SHF}"] = ob.shared[SHF]
    for key in extra_global:
        out[key] = data[key]
    return out


def finish(objs, extra=None):
    """(states, arrays): the states first -- reading ``.data`` afterwards moves the current side to the host."""
    states = {name: (bool(obj.accel_exists()), bool(obj.accel_in_use())) for name, obj in objs.items()}
    arrays = {name: np.array(obj.data) for name, obj in objs.items()}
    arrays.update(extra or {})
    return states, arrays


# ---- one function per operator: (start, lazy_host) -> (states, arrays)
def run_ground_filter(start, lazy):
    data = ground()
    data.lazy_host = lazy
    start_from(data, start)
    ops.GroundFilter(trend_order=1, filter_order=2, name="gf").apply(data)
    return finish(objects(data))


def run_poly_filter(start, lazy):
    data = ground()
    data.lazy_host = lazy
    start_from(data, start)
    op = ops.PolyFilter(order=2, view=None, name="pf")
    op.apply(data)
    return finish(objects(data), {"coeff": op.coefficients[data.obs[0].name]})


def run_poly_filter_2d(start, lazy):
    data = ground(n_det=4)
    data.lazy_host = lazy
    start_from(data, start)
    op = ops.PolyFilter2D(order=1, name="pf2d")
    op.apply(data)
    return finish(objects(data), {"coeff": op.coefficients[data.obs[0].name]})


def run_common_mode(start, lazy):
    data = ground()
    data.lazy_host = lazy
    start_from(data, start)
    ops.CommonModeFilter(name="cm").apply(data)
    return finish(objects(data))


def run_time_constant(start, lazy):
    data = tc.make_data()
    data.lazy_host = lazy
    start_from(data, start)
    ops.TimeConstant(tau_name="tau").apply(data)
    return finish(objects(data))


def run_noise_filter(start, lazy):
    data = ground()
    data.lazy_host = lazy
    start_from(data, start)
    ops.NoiseFilter(net_fit="closed_form", name="nf").apply(data)
    return finish(objects(data))


def run_noise_estim(start, lazy):
    data = nc.make_obs("cross_flags", n=2000)
    data.lazy_host = lazy
    start_from(data, start)
    ops.NoiseEstim(out_model="measured", **nc.OP_CASES["cross_flags"]["op"]).apply(data, use_accel=True)
    model = data.obs[0]["measured"]
    psds = {f"psd:{key}": np.array(model.psd(key)) for key in model.keys}
    return finish(objects(data), psds)


def run_sim_noise(start, lazy):
    data = sc.make_data(n_det=3, n_samp=1000)
    data.lazy_host = lazy
    start_from(data, start)
    ops.SimNoise(realization=2).apply(data, use_accel=True)
    return finish(objects(data))


def run_demodulate(start, lazy):
    G = dc.gold()
    data = dc.make_obs(G)
    data.lazy_host = lazy
    start_from(data, start)
    op = ops.Demodulate(stokes_weights=dc.fixed_weights_operator(dc.weight_table(G)), nskip=dc.NSKIP)
    out = op.apply(data, use_accel=True)
    objs = objects(data, extra_detdata=(op.stokes_weights.weights,))
    objs.update({"demod:" + name: obj for name, obj in objects(out).items()})
    return finish(objs)


def run_noise_weight(start, lazy):
    data = ground()
    data.lazy_host = lazy
    start_from(data, start)
    ops.NoiseWeight(det_data=SIG).apply(data, use_accel=True)
    return finish(objects(data))


def run_scan_mask(start, lazy):
    data = ground()
    data.lazy_host = lazy
    dp = ops.PointingDetectorSimple()
    ops.PixelsHealpix(detector_pointing=dp, nside=16, nest=True, create_dist="dist").apply(data)
    mask = PixelData(data["dist"], np.uint8, n_value=1)
    mask.data[:, ::3] = 1
    data["mask"] = mask
    start_from(data, start, extra=(defaults.pixels,))
    put(mask, start)
    ops.ScanMask(mask_key="mask", det_flags_value=4).apply(data, use_accel=True)
    return finish(objects(data, extra_detdata=(defaults.pixels,), extra_global=("mask",)))


def run_combine(start, lazy):
    data = ground()
    data.lazy_host = lazy
    rng = np.random.default_rng(5)
    for ob in data.obs:
        ob.detdata.create("other", dtype=np.float64, units=ob.detdata[SIG].units)
        ob.detdata["other"].data[:] = rng.standard_normal(ob.detdata[SIG].shape)
    start_from(data, start, extra=("other",))
    ops.Combine(op="subtract", first=SIG, second="other", result="diff").apply(data)
    return finish(objects(data, extra_detdata=("other", "diff")))


RUNNERS = {
    "GroundFilter": run_ground_filter, "PolyFilter": run_poly_filter, "PolyFilter2D": run_poly_filter_2d,
    "CommonModeFilter": run_common_mode, "TimeConstant": run_time_constant, "NoiseFilter": run_noise_filter,
    "NoiseEstim": run_noise_estim, "SimNoise": run_sim_noise, "Demodulate": run_demodulate,
    "NoiseWeight": run_noise_weight, "ScanMask": run_scan_mask, "Combine": run_combine,
}

#: relative to the largest input, for operators whose kernels sum with atomics; every other operator: bit for bit
TOLERANCE = {"GroundFilter": 1e-9}


@functools.lru_cache(maxsize=None)
def input_scale():
    return float(np.max(np.abs(ground().obs[0].detdata[SIG].data)))

# (accel_exists, accel_in_use): current on the device, registered with the host current, not registered
ON, HOST, OFF = (True, True), (True, False), (False, False)

# operator -> (start, lazy_host) -> {object: (accel_exists, accel_in_use)}
EXPECTED = {
    "GroundFilter": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "PolyFilter": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "PolyFilter2D": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "CommonModeFilter": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "TimeConstant": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": OFF,
                                 "1:detdata:signal": ON, "1:detdata:flags": ON, "1:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:shared:flags": OFF,
                                  "1:detdata:signal": OFF, "1:detdata:flags": OFF, "1:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": HOST,
                         "1:detdata:signal": ON, "1:detdata:flags": ON, "1:shared:flags": HOST},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:shared:flags": HOST,
                          "1:detdata:signal": OFF, "1:detdata:flags": OFF, "1:shared:flags": HOST},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON,
                           "1:detdata:signal": ON, "1:detdata:flags": ON, "1:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON,
                            "1:detdata:signal": ON, "1:detdata:flags": ON, "1:shared:flags": ON},
    },
    "NoiseFilter": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": HOST},
        ("host", False): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:shared:flags": HOST},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:shared:flags": ON},
    },
    "NoiseEstim": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": HOST, "0:shared:flags": HOST},
        ("host", False): {"0:detdata:signal": ON, "0:detdata:flags": HOST, "0:shared:flags": HOST},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "SimNoise": {
        ("unregistered", True): {"0:detdata:signal": ON},
        ("unregistered", False): {"0:detdata:signal": ON},
        ("host", True): {"0:detdata:signal": ON},
        ("host", False): {"0:detdata:signal": ON},
        ("device", True): {"0:detdata:signal": ON},
        ("device", False): {"0:detdata:signal": ON},
    },
    "Demodulate": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:detdata:weights": ON,
                                 "0:shared:flags": OFF, "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON,
                                 "demod:0:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:detdata:weights": ON,
                                  "0:shared:flags": OFF, "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON,
                                  "demod:0:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:weights": ON, "0:shared:flags": ON,
                         "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON, "demod:0:shared:flags": OFF},
        ("host", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:weights": ON,
                          "0:shared:flags": ON, "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON,
                          "demod:0:shared:flags": OFF},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:weights": ON,
                           "0:shared:flags": ON, "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON,
                           "demod:0:shared:flags": OFF},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:weights": ON,
                            "0:shared:flags": ON, "demod:0:detdata:signal": ON, "demod:0:detdata:flags": ON,
                            "demod:0:shared:flags": OFF},
    },
    "NoiseWeight": {
        ("unregistered", True): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": ON, "0:detdata:flags": OFF, "0:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": ON, "0:detdata:flags": HOST, "0:shared:flags": HOST},
        ("host", False): {"0:detdata:signal": ON, "0:detdata:flags": HOST, "0:shared:flags": HOST},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:shared:flags": ON},
    },
    "ScanMask": {
        ("unregistered", True): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                                 "0:shared:flags": OFF, "mask": ON},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                                  "0:shared:flags": OFF, "mask": ON},
        ("host", True): {"0:detdata:signal": HOST, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                         "0:shared:flags": HOST, "mask": ON},
        ("host", False): {"0:detdata:signal": HOST, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                          "0:shared:flags": HOST, "mask": ON},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                           "0:shared:flags": ON, "mask": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:pixels": ON,
                            "0:shared:flags": ON, "mask": ON},
    },
    "Combine": {
        ("unregistered", True): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:detdata:other": OFF,
                                 "0:detdata:diff": OFF, "0:shared:flags": OFF},
        ("unregistered", False): {"0:detdata:signal": OFF, "0:detdata:flags": OFF, "0:detdata:other": OFF,
                                  "0:detdata:diff": OFF, "0:shared:flags": OFF},
        ("host", True): {"0:detdata:signal": HOST, "0:detdata:flags": HOST, "0:detdata:other": HOST,
                         "0:detdata:diff": OFF, "0:shared:flags": HOST},
        ("host", False): {"0:detdata:signal": HOST, "0:detdata:flags": HOST, "0:detdata:other": HOST,
                          "0:detdata:diff": OFF, "0:shared:flags": HOST},
        ("device", True): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:other": ON, "0:detdata:diff": ON,
                           "0:shared:flags": ON},
        ("device", False): {"0:detdata:signal": ON, "0:detdata:flags": ON, "0:detdata:other": ON,
                            "0:detdata:diff": ON, "0:shared:flags": ON},
    },
}

_host_only = {}


def host_only_arrays(name):
    """The arrays of the run that started from host-only data (lazy host coherence), computed once per operator."""
    if name not in _host_only:
        _host_only[name] = RUNNERS[name]("unregistered", True)[1]
    return _host_only[name]


@pytest.mark.parametrize("lazy_host", [True, False])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("name", list(RUNNERS))
def test_operator_leaves_objects_where_it_did(name, start, lazy_host):
    states, arrays = RUNNERS[name](start, lazy_host)
    assert states == EXPECTED[name][(start, lazy_host)]
    want = host_only_arrays(name)
    assert sorted(arrays) == sorted(want)
    for key, value in want.items():
        if name in TOLERANCE and value.dtype.kind == "f":
            assert np.max(np.abs(arrays[key] - value)) <= TOLERANCE[name] * input_scale(), (name, key)
        else:
            assert np.array_equal(arrays[key], value, equal_nan=value.dtype.kind == "f"), (name, key)
