"""CPU: the host side of the time-constant feature -- the NumPy restatement of the single-pole convolution against the
outputs of the reference's own AlgorithmNumpy.convolve with a kernel function (tests/golden/time_constant*.npz, bit for
bit), fft.SinglePole as a kernel function, the argument checks of fft.convolve, and the operator's bookkeeping."""
import numpy as np
import pytest

import time_constant_case as tc


@pytest.fixture(scope="module")
def fixture():
    return tc.load_fixture()


@pytest.mark.parametrize("name", tc.FIXTURE_CASES)
@pytest.mark.parametrize("direction", ["convolve", "deconvolve"])
def test_restatement_equals_reference_fixture(fixture, name, direction):
    """Same standard as the oracle's (test_fft_oracle.py: np.array_equal with the reference's outputs)."""
    taus = fixture["taus"]
    data = np.tile(fixture[f"{name}_data"], (taus.size, 1))
    tc.single_pole_convolve(data, float(fixture[f"{name}_rate"]), taus, direction == "deconvolve")
    assert np.array_equal(data, fixture[f"{name}_out_{direction}"])


def test_fixture_reaches_the_lengths_it_is_meant_for(fixture):
    assert [int(fixture[f"{n}_n_fft"]) for n in tc.FIXTURE_CASES] == [4096, 8192, 8192, 32768]
    assert np.array_equal(fixture["taus"], [0.0, 1e-3, 3e-3, 10e-3, 50e-3])
    assert fixture["n3000_extents_convolve"].tolist() == [2, 17, 24, 16, 44]
    assert fixture["n3000_extents_deconvolve"].tolist() == [2, 21, 61, 101, 101]
    flagged = np.mean((fixture["n3000_flags_in"] & 1) != 0)
    assert 0.0005 < flagged < 0.006


@pytest.mark.parametrize("direction", ["convolve", "deconvolve"])
def test_restatement_extents_and_flags_equal_fixture(fixture, direction):
    taus = fixture["taus"]
    dec = direction == "deconvolve"
    assert np.array_equal(tc.single_pole_extents(3000, 200.0, taus, dec), fixture[f"n3000_extents_{direction}"])
    data = np.tile(fixture["n3000_data"], (taus.size, 1))
    flags = np.tile(fixture["n3000_flags_in"], (taus.size, 1))
    tc.convolve_with_flags(data, 200.0, taus, dec, flags, 1)
    assert np.array_equal(flags, fixture[f"n3000_flags_{direction}"])
    assert np.array_equal(data, fixture[f"n3000_out_{direction}"])


def test_single_pole_call_is_the_formula():
    from toast_amd.fft import SinglePole

    freqs = np.fft.rfftfreq(4096, d=1.0 / 37.0)
    taus = np.array([0.0, 1e-3, 50e-3])
    for dec in (False, True):
        k = SinglePole(taus, deconvolve=dec)
        for i, tau in enumerate(taus):
            got = k(i, freqs)
            assert got.dtype == np.complex128 and got.shape == freqs.shape
            assert np.array_equal(got, tc.pole_kernel(tau, freqs, dec))
            want = 1.0 + 1j * (2.0 * np.pi * tau * freqs)
            assert np.array_equal(got, want if dec else 1.0 / want)
    assert SinglePole(1e-3).deconvolve is False


def test_scalar_tau_broadcasts():
    from toast_amd.fft import SinglePole

    freqs = np.linspace(0.0, 100.0, 33)
    k = SinglePole(3e-3, deconvolve=True)
    assert np.array_equal(k(0, freqs), k(7, freqs))
    assert np.array_equal(k(4, freqs), tc.pole_kernel(3e-3, freqs, True))
    assert np.array_equal(k.taus(4), np.full(4, 3e-3))
    assert np.array_equal(SinglePole([1e-3, 2e-3]).taus(2), [1e-3, 2e-3])
    with pytest.raises(RuntimeError):
        SinglePole([1e-3, 2e-3]).taus(3)
    with pytest.raises(RuntimeError):
        SinglePole(np.zeros((2, 2)))


def test_single_pole_is_a_kernel_func_for_the_restated_algorithm(fixture):
    """The object in place of the kernel function: same outputs as the fixture."""
    from oracle import fft_oracle as fo
    from toast_amd.fft import SinglePole

    taus = fixture["taus"]
    rate = float(fixture["n1500_rate"])
    freq = np.fft.rfftfreq(fo.fft_length(1500), d=1.0 / rate)
    for direction in ("convolve", "deconvolve"):
        k = SinglePole(taus, deconvolve=direction == "deconvolve")
        for i in (1, 4):
            assert np.array_equal(k(i, freq), tc.pole_kernel(taus[i], freq, direction == "deconvolve"))


def test_convolve_argument_checks():
    """fft.py:774-802; they come before any device work."""
    from toast_amd import fft

    data = np.zeros((2, 64))
    pole = fft.SinglePole(1e-3)
    kf, kv = np.linspace(0, 1, 4), np.ones(4)
    with pytest.raises(RuntimeError, match="Cannot specify both"):
        fft.convolve(data, 10.0, kernel_freq=kf, kernels=kv, kernel_func=pole)
    with pytest.raises(RuntimeError, match="Cannot specify both"):
        fft.convolve(data, 10.0, kernel_freq=kf, kernel_func=pole)
    with pytest.raises(RuntimeError, match="Must specify either"):
        fft.convolve(data, 10.0)
    with pytest.raises(RuntimeError, match="Both flags and flag_mask"):
        fft.convolve(data, 10.0, flags=np.zeros((2, 64), np.uint8), kernel_func=pole)
    with pytest.raises(RuntimeError, match="Both flags and flag_mask"):
        fft.convolve(data, 10.0, flag_mask=1, kernel_func=pole)
    with pytest.raises(RuntimeError, match="algorithm"):
        fft.convolve(data, 10.0, kernel_func=pole, algorithm="nonuniform")
    with pytest.raises(RuntimeError, match="one value per timestream"):
        fft.convolve(data, 10.0, kernel_func=fft.SinglePole([1e-3, 2e-3, 3e-3]))
    assert not data.any()


def test_arbitrary_callable_still_raises():
    from toast_amd import fft

    with pytest.raises(NotImplementedError):
        fft.convolve(np.zeros((1, 64)), 10.0, kernel_func=lambda indx, freqs: np.ones(len(freqs), dtype=np.complex128))
    # ... also one that computes the same thing: only the SinglePole type says "analytic"
    with pytest.raises(NotImplementedError):
        fft.convolve(np.zeros((1, 64)), 10.0, kernel_func=lambda indx, freqs: tc.pole_kernel(1e-3, freqs, False))


def test_operator_traits_and_housekeeping():
    from toast_amd import ops
    from toast_amd.data import defaults

    op = ops.TimeConstant()
    want = dict(API=0, det_data=defaults.det_data, det_mask=defaults.det_mask_invalid, shared_flags=defaults.shared_flags,
                shared_flag_mask=defaults.shared_mask_invalid, det_flags=defaults.det_flags,
                det_flag_mask=defaults.det_mask_invalid, tau=None, tau_sigma=None, tau_name=None,
                tau_flag_mask=defaults.det_mask_invalid, batch=False, deconvolve=False, realization=0, debug=None)
    for k, v in want.items():
        assert getattr(op, k) == v, k
    req = op.requires()
    assert req["shared"] == [defaults.shared_flags] and req["detdata"] == [defaults.det_data, defaults.det_flags]
    assert not any(op.provides().values())
    op = ops.TimeConstant(det_flags=None, tau=1e-3, batch=True, debug="plots")
    req = op.requires()
    assert req["shared"] == [] and req["detdata"] == [defaults.det_data]
    with pytest.raises(RuntimeError, match="Either tau or tau_name"):
        ops.TimeConstant().apply(tc.make_data())


def test_operator_bookkeeping_restatement():
    """tau selection, tau_sigma, the NaN detector, the uid fallback and the shared-flag propagation of the host
    restatement that the GPU test compares the operator with."""
    from toast_amd import ops, rng
    from toast_amd.data import defaults
    from toast_amd.noise import name_UID

    data = tc.make_data()
    obs = data.obs[0]
    dets = obs.local_detectors
    taus, invalid = tc.operator_taus(obs, dets, tau_name="tau")
    assert invalid == ["D01"] and np.array_equal(taus, [2e-3, 0.0, 8e-3, 5e-3])
    taus, invalid = tc.operator_taus(obs, dets, tau=4e-3, tau_name="tau")
    assert invalid == [] and np.array_equal(taus, np.full(4, 4e-3))          # tau overrides tau_name
    t0, _ = tc.operator_taus(obs, dets, tau_name="tau", tau_sigma=0.1)
    t1, _ = tc.operator_taus(data.obs[1], dets, tau_name="tau", tau_sigma=0.1)
    t2, _ = tc.operator_taus(obs, dets, tau_name="tau", tau_sigma=0.1, realization=1)
    x = rng.random(1, sampler="gaussian", key=(1000, 123456), counter=(obs.session.uid, 0))[0]
    assert t0[0] == 2e-3 * (1 + x * 0.1) and t0[1] == 0.0
    assert t0[0] != t1[0] and t0[0] != t2[0]                                   # session and realization enter the stream
    assert np.all(np.abs(t0[[0, 2, 3]] / np.array([2e-3, 8e-3, 5e-3]) - 1) < 0.6)
    # without a uid column the detector's name is hashed
    nouid = tc.make_data(with_uid=False).obs[0]
    tn, _ = tc.operator_taus(nouid, dets, tau_name="tau", tau_sigma=0.1)
    x = rng.random(1, sampler="gaussian", key=(name_UID("D00"), 123456), counter=(nouid.session.uid, 0))[0]
    assert tn[0] == 2e-3 * (1 + x * 0.1)
    # the operator's own _get_tau agrees
    op = ops.TimeConstant(tau_name="tau", tau_sigma=0.1)
    assert [op._get_tau(obs, d) for d in ("D00", "D02", "D03")] == t0[[0, 2, 3]].tolist()
    assert np.isnan(op._get_tau(obs, "D01"))
    # shared flags inside the mask reach every detector's flags, those outside do not; the NaN detector is still convolved
    ref = tc.operator_reference(data, tau_name="tau")
    signal, flags, det_flags = ref[0]
    shared = obs.shared[defaults.shared_flags].data
    assert np.all(flags[:, (shared & 1) != 0] & 1)
    before = np.array([np.array(obs.detdata[defaults.det_flags][d]) for d in dets])
    bad = np.any(before & 1, axis=0) | ((shared & 1) != 0)
    near = np.convolve(bad.astype(np.int64), np.ones(2 * 120 + 1, dtype=np.int64), mode="same") > 0    # extents <= 101
    near[:120] = near[-120:] = True
    only16 = (shared == 16) & ~near
    assert np.any(only16) and not np.any(flags[:, only16] & 1)
    assert np.array_equal(flags[:, ~near], before[:, ~near])
    assert det_flags == {"D00": 0, "D01": defaults.det_mask_invalid, "D02": 0, "D03": 0}
    # ... with tau = 0: the mean of its padded series is removed
    d01 = np.array(obs.detdata[defaults.det_data]["D01"])
    assert not np.array_equal(signal[1], d01) and np.std(signal[1] - d01) < 0.05 * np.std(d01)
    # the inputs were not touched
    assert obs.local_detector_flags == {d: 0 for d in dets}
