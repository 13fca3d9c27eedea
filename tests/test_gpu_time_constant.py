"""GPU: the analytic single-pole kernel kind of the FFT pipelines (fft.SinglePole -> toast_hip_fft_convolve_pole*) and
ops.TimeConstant, against the outputs of the reference's own AlgorithmNumpy.convolve with a kernel function
(tests/golden/time_constant*.npz) and the host restatement of tests/time_constant_case.py.  Tolerances as in
test_gpu_fft.py: 1e-12 of the signal scale (1e-11 for the deconvolution), 1e-13 between the two pipelines."""
import numpy as np
import pytest

import time_constant_case as tc

pytestmark = pytest.mark.gpu

TOL = {"convolve": 1e-12, "deconvolve": 1e-11}


@pytest.fixture(scope="module")
def pf():
    from toast_amd import capi, fft

    assert capi.accel_enabled()
    capi.accel_assign_device(1, 0, 1.0, False)
    return fft


@pytest.fixture(scope="module")
def fixture():
    return tc.load_fixture()


@pytest.mark.parametrize("direction", ["convolve", "deconvolve"])
@pytest.mark.parametrize("name", tc.FIXTURE_CASES)
def test_reference_fixture(pf, fixture, name, direction):
    """Every fixture case through fft.convolve(kernel_func=SinglePole(...)): n1500 the rocFFT pipeline (k_fft_kernel_pole),
    n2049 / n3000 the self-paired rows of the fused one (k_fft_rows, unaligned / aligned pass 1), n9000 k_fft_rows_reg16.
    The fused cases once more through the rocFFT pipeline: the two agree to 1e-13."""
    taus = fixture["taus"]
    rate = float(fixture[f"{name}_rate"])
    data = np.tile(fixture[f"{name}_data"], (taus.size, 1))
    want = fixture[f"{name}_out_{direction}"]
    n_samp = data.shape[1]
    assert pf.fft_length(n_samp) == int(fixture[f"{name}_n_fft"])
    assert pf.implementation(n_samp) == ("rocfft" if name == "n1500" else "fused-3pass")
    kernel = pf.SinglePole(taus, deconvolve=direction == "deconvolve")
    got = data.copy()
    pf.convolve(got, rate, kernel_func=kernel)
    scale = np.max(np.abs(want))
    err = np.max(np.abs(got - want))
    print(f"{name} {direction}: max|got - want| / max|want| = {err / scale:.3e}")
    assert err < TOL[direction] * scale
    if name != "n1500":
        pf.select(True)
        try:
            assert pf.implementation(n_samp) == "rocfft"
            lib = data.copy()
            pf.convolve(lib, rate, kernel_func=kernel)
        finally:
            pf.select(False)
        print(f"{name} {direction}: fused against rocFFT {np.max(np.abs(got - lib)) / scale:.3e}")
        assert np.max(np.abs(lib - want)) < TOL[direction] * scale
        assert np.max(np.abs(got - lib)) < 1e-13 * scale


def test_convolve_deconvolve_argument_divides_by_the_object(pf, fixture):
    """deconvolve=True with a kernel function divides by what it returns (fft.py:331-334): dividing by 1 / K is the
    deconvolution, dividing by K the convolution."""
    taus = fixture["taus"]
    data = np.tile(fixture["n3000_data"], (taus.size, 1))
    for described, direction in ((False, "deconvolve"), (True, "convolve")):
        got = data.copy()
        pf.convolve(got, 200.0, kernel_func=pf.SinglePole(taus, deconvolve=described), deconvolve=True)
        want = fixture[f"n3000_out_{direction}"]
        assert np.max(np.abs(got - want)) < TOL[direction] * np.max(np.abs(want))


@pytest.mark.parametrize("direction", ["convolve", "deconvolve"])
def test_flags_and_extents(pf, fixture, direction):
    """The 3000-sample case with flags: impulse extents measured on the device and the extended flags, both exactly the
    reference's."""
    taus = fixture["taus"]
    invert = direction == "convolve"
    assert np.array_equal(pf.impulse_extents_pole(taus.size, 3000, 200.0, taus, invert), fixture[f"n3000_extents_{direction}"])
    data = np.tile(fixture["n3000_data"], (taus.size, 1))
    flags = np.tile(fixture["n3000_flags_in"], (taus.size, 1))
    pf.convolve(data, 200.0, flags=flags, flag_mask=1, kernel_func=pf.SinglePole(taus, deconvolve=not invert))
    assert np.array_equal(flags, fixture[f"n3000_flags_{direction}"])
    want = fixture[f"n3000_out_{direction}"]
    assert np.max(np.abs(data - want)) < TOL[direction] * np.max(np.abs(want))
    # a list of 1-D flag arrays takes the host route of the bookkeeping
    flist = [fixture["n3000_flags_in"].copy() for _ in range(taus.size)]
    d2 = np.tile(fixture["n3000_data"], (taus.size, 1))
    pf.convolve(d2, 200.0, flags=flist, flag_mask=1, kernel_func=pf.SinglePole(taus, deconvolve=not invert))
    assert np.array_equal(np.array(flist), flags) and np.array_equal(d2, data)


def test_all_samples_error_is_kept(pf):
    """tau = 5 s at 10 Hz: the response to an impulse in 64 samples never falls under 2 % of its peak (restatement: the
    walks reach both ends); the call raises before it touches data or flags, as the reference does (fft.py:871-873)."""
    assert tc.single_pole_extents(64, 10.0, [5.0], False).tolist() == [64]
    data = np.random.default_rng(1).standard_normal((1, 64))
    keep = data.copy()
    flags = np.zeros((1, 64), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="spreads to all samples"):
        pf.convolve(data, 10.0, flags=flags, flag_mask=1, kernel_func=pf.SinglePole(5.0))
    assert np.array_equal(data, keep) and not flags.any()


def test_row_indexing(pf):
    """convolve_buffer_pole on a 7-row buffer through data_index = [5, 0, 3, 6, 2]: tau goes with the position in the
    list, not with the buffer row; the other rows stay bit-identical."""
    rng = np.random.default_rng(31)
    rate, n_samp, rows = 200.0, 9000, 7
    idx = np.array([5, 0, 3, 6, 2], dtype=np.int32)
    taus = np.array([7e-3, 0.5e-3, 30e-3, 2e-3, 12e-3])
    buf = rng.standard_normal((rows, n_samp)) + np.linspace(-1, 2, n_samp)[None, :]
    for invert in (True, False):
        want = np.ascontiguousarray(buf[idx])
        tc.single_pole_convolve(want, rate, taus, not invert)
        got = buf.copy()
        pf.convolve_buffer_pole(got, idx, rate, taus, invert)
        assert np.max(np.abs(got[idx] - want)) < (1e-12 if invert else 1e-11) * np.max(np.abs(want))
        assert np.array_equal(got[[1, 4]], buf[[1, 4]])
    # a scalar tau is every row's
    want = np.ascontiguousarray(buf[idx])
    tc.single_pole_convolve(want, rate, 4e-3, False)
    got = buf.copy()
    pf.convolve_buffer_pole(got, idx, rate, 4e-3)
    assert np.max(np.abs(got[idx] - want)) < 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("n_samp", [1500, 9000])
def test_batches_keep_their_time_constants(pf, n_samp):
    """convolve_pole_dev in batches of two detectors (tau is indexed by det0 + position in the batch): both pipelines
    against the restatement; the fused kernels (n_samp 9000) equal the unbatched call bit for bit -- a row's arithmetic
    does not depend on its batch there, which rocFFT (n_samp 1500) does not promise for plans of different batch size."""
    import torch

    rng = np.random.default_rng(n_samp)
    rate = 200.0
    taus = np.array([1e-3, 3e-3, 10e-3, 50e-3, 6e-3])
    data = rng.standard_normal((5, n_samp)) + np.linspace(-1, 2, n_samp)[None, :]
    idx = np.arange(5, dtype=np.int32)
    out = []
    for max_batch in (0, 2):
        t = torch.from_numpy(data).cuda()
        pf.convolve_pole_dev(t.data_ptr(), idx, n_samp, rate, taus, True, max_batch=max_batch,
                             stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out.append(t.cpu().numpy())
    if pf.implementation(n_samp) == "fused-3pass":
        assert np.array_equal(out[0], out[1])
    want = data.copy()
    tc.single_pole_convolve(want, rate, taus, False)
    for got in out:
        assert np.max(np.abs(got - want)) < 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("n_samp", [720000, 1100003])
def test_long_lengths_both_directions(pf, n_samp):
    """n_fft 2^21 (LDS forward columns, 16-point register inverse columns) and 2^22 (odd length: the unaligned column
    passes, four columns per tile) against the restatement, both directions.  Then with the rows entry of the points
    switch away from its default: an analytic call has no 16-point row instantiation and runs the default one -- the
    same bits."""
    rng = np.random.default_rng(n_samp)
    rate = 200.0
    taus = np.array([2e-3, 20e-3])
    data = rng.standard_normal((2, n_samp)) + np.linspace(-1, 2, n_samp)[None, :]
    assert pf.implementation(n_samp) == "fused-3pass"
    got = {}
    for direction in ("convolve", "deconvolve"):
        want = data.copy()
        tc.single_pole_convolve(want, rate, taus, direction == "deconvolve")
        g = data.copy()
        pf.convolve(g, rate, kernel_func=pf.SinglePole(taus, deconvolve=direction == "deconvolve"))
        err = np.max(np.abs(g - want)) / np.max(np.abs(want))
        print(f"n_samp {n_samp} {direction}: {err:.3e}")
        assert err < TOL[direction]
        got[direction] = g
    try:
        pf.set_points(16, 0, 0)
        for direction in ("convolve", "deconvolve"):
            g = data.copy()
            pf.convolve(g, rate, kernel_func=pf.SinglePole(taus, deconvolve=direction == "deconvolve"))
            assert np.array_equal(g, got[direction]), direction
    finally:
        pf.set_points()


def _run_operator(resident, **traits):
    from toast_amd import ops
    from toast_amd.data import defaults

    data = tc.make_data()
    if resident:
        for ob in data.obs:
            dd = ob.detdata[defaults.det_data]
            dd.accel_create(defaults.det_data)
            dd.accel_update_device()
    ops.TimeConstant(**traits).apply(data)
    out = []
    for ob in data.obs:
        dd = ob.detdata[defaults.det_data]
        if resident:
            assert dd.accel_in_use()           # filtered in place, still resident
        dets = ob.local_detectors
        out.append((np.array(dd.data), np.array(ob.detdata[defaults.det_flags].data), dict(ob.local_detector_flags), dets))
    return out


@pytest.mark.parametrize("deconvolve", [False, True])
def test_operator(pf, deconvolve):
    """ops.TimeConstant on two observations x four detectors: tau from a focalplane column with one NaN, spread by
    tau_sigma, shared and detector flags -- against the host restatement; the device-resident and the host-resident
    route give identical arrays."""
    from toast_amd.data import defaults

    traits = dict(tau_name="tau", tau_sigma=0.1, deconvolve=deconvolve, realization=3)
    ref = tc.operator_reference(tc.make_data(), deconvolve=deconvolve, tau_name="tau", tau_sigma=0.1, realization=3)
    host = _run_operator(False, **traits)
    dev = _run_operator(True, **traits)
    tol = TOL["deconvolve" if deconvolve else "convolve"]
    for iob in range(tc.N_OBS):
        want_sig, want_flags, want_det = ref[iob]
        sig, flags, det_flags, dets = host[iob]
        assert det_flags == want_det and det_flags["D01"] == defaults.det_mask_invalid
        assert np.array_equal(flags, want_flags)
        assert np.max(np.abs(sig - want_sig)) < tol * np.max(np.abs(want_sig))
        assert np.array_equal(dev[iob][0], sig) and np.array_equal(dev[iob][1], flags) and dev[iob][2] == det_flags


def test_operator_without_flags_and_errors(pf):
    from toast_amd import ops
    from toast_amd.data import defaults

    ref = tc.operator_reference(tc.make_data(), tau=4e-3, use_flags=False)
    data = tc.make_data()
    before = [np.array(ob.detdata[defaults.det_flags].data) for ob in data.obs]
    ops.TimeConstant(tau=4e-3, tau_name="tau", det_flags=None, batch=True).apply(data)
    for iob, ob in enumerate(data.obs):
        sig = np.array(ob.detdata[defaults.det_data].data)
        assert np.max(np.abs(sig - ref[iob][0])) < 1e-12 * np.max(np.abs(ref[iob][0]))
        assert np.array_equal(np.array(ob.detdata[defaults.det_flags].data), before[iob])      # no flags are touched
        assert ob.local_detector_flags == {d: 0 for d in ob.local_detectors}                    # tau overrides the NaN column
    with pytest.raises(RuntimeError, match="Either tau or tau_name"):
        ops.TimeConstant(tau=None, tau_name=None).apply(tc.make_data())
