"""GPU: the random-stream and noise-simulation kernels (csrc/sim_noise.hip) against tests/golden/sim_noise.npz -- the
reference's own compiled streams and PSD interpolation (tests/golden/make_golden_sim_noise.py).

* uint64, uniform_01, uniform_m11: exact (integer arithmetic and correctly rounded IEEE operations).
* Gaussian: max relative distance <= 4 x gauss_ref_err.  The device ``log`` may be off by a full ulp where glibc's is
  below one; it enters once, the Horner steps are identical.
* Interpolated amplitudes: <= 4 x scale_ref_err of the stream's largest amplitude (the ``- psdshift`` cancellation
  makes per-element relative errors meaningless at zero-PSD bins).
* Timestreams: <= 10 x ts_ref_err of the stream's rms (rocFFT factors the length differently from pocketfft; the
  margin the template tests use over their measured host distance).
* Invariance: batch size, grouping of the detectors into calls and repetition do not change one bit.

Every figure is printed before it is asserted."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "workflows"))

import sim_noise_case as sc  # noqa: E402
from sim_noise_case import GOLD  # noqa: E402

pytestmark = pytest.mark.gpu

RATE = float(GOLD["psd_rate"])
FREQ = GOLD["psd_freq"]
TS_BOUND = 10.0 * float(GOLD["ts_ref_err"])


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)
        accel_data_create(self.a, "test_sim_noise")
        accel_data_update_device(self.a, "test_sim_noise")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_sim_noise")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_sim_noise")


def simulate(rz, tel, comp, obs, first, samples, det, psds, rate=RATE, freq=FREQ, start=None, **kw):
    """toast_hip_sim_noise_dev into a device buffer that holds ``start`` (zeros) before."""
    from toast_amd import capi

    n_rows = kw.pop("n_rows", len(det))
    buf = Dev(np.zeros((n_rows, samples)) if start is None else start)
    capi.dev.sim_noise(rz, tel, comp, obs, rate, first, samples, 2, det, freq, psds, buf.ptr, n_rows, **kw)
    capi.synchronize()
    out = buf.get()
    buf.free()
    return out


def test_device_streams():
    from toast_amd import capi, rng

    n = int(GOLD["rng_n"])
    cases = sc.rng_cases()
    gbound = 4.0 * float(GOLD["gauss_ref_err"])
    worst = 0.0
    for sampler, kind in sc.SAMPLERS.items():
        dtype = np.uint64 if kind == "uint64" else np.float64
        # all streams of the fixture in one launch, in reverse order in the output buffer (explicit offsets)
        offsets = [(len(cases) - 1 - i) * n for i in range(len(cases))]
        buf = Dev(np.zeros(len(cases) * n, dtype=dtype))
        rng.random_multi_device([n] * len(cases), [c[:2] for c in cases], [c[2:] for c in cases], buf.ptr, buf.a.size,
                                sampler=sampler, offsets=offsets)
        capi.synchronize()
        got = buf.get()
        buf.free()
        for i in range(len(cases)):
            g, want = got[offsets[i]:offsets[i] + n], GOLD[f"rng_{i}_{kind}"]
            if kind == "normal":
                worst = max(worst, float(np.max(np.abs(g - want) / np.abs(want))))
            else:
                assert np.array_equal(g, want), (sampler, i)
    counters = GOLD["rng_tail_counter"]
    buf = Dev(np.zeros(counters.size))
    rng.random_multi_device([1] * counters.size, [(11, 12)] * counters.size, [(0, int(c)) for c in counters], buf.ptr,
                            counters.size)
    capi.synchronize()
    tail = buf.get()
    with pytest.raises(RuntimeError, match="beyond the output"):
        capi.dev.rng_multi("normal", [8], [0], [0], [0], [0], buf.ptr, 4)
    buf.free()
    want = GOLD["rng_tail_normal"]
    worst_tail = float(np.max(np.abs(tail - want) / np.abs(want)))
    print(f"gaussian: max relative distance {worst:.3e} (streams), {worst_tail:.3e} (outer polynomials); bound {gbound:.3e}")
    assert max(worst, worst_tail) <= gbound


def test_device_interpolated_scale():
    from toast_amd import capi

    psds = GOLD["psd_psds"]
    bound = 4.0 * float(GOLD["scale_ref_err"])
    for samples in (3000, 12345):
        n_psd = capi.sim_noise_fft_length(samples, 2) // 2 + 1
        buf = Dev(np.full((psds.shape[0], n_psd), np.nan))
        capi.dev.sim_noise_psd_interp(RATE, samples, 2, FREQ, psds, buf.ptr)
        capi.synchronize()
        got = buf.get()
        buf.free()
        host = capi.tod_sim_noise_psd_interp(RATE, samples, 2, FREQ, psds)
        bins = GOLD[f"interp_{samples}_bins"]
        want = GOLD[f"interp_{samples}"]
        dist = float(np.max(np.max(np.abs(got[:, bins] - want), axis=1) / np.max(want, axis=1)))
        dist_all = float(np.max(np.max(np.abs(got - host), axis=1) / np.max(host, axis=1)))
        print(f"scale, samples {samples}: distance {dist:.3e} (fixture bins), {dist_all:.3e} (all bins, host entry); "
              f"bound {bound:.3e}")
        assert np.all(got[:, 0] == 0) and np.all(np.isfinite(got))
        assert max(dist, dist_all) <= bound


def test_device_timestreams():
    for name in sc.TS_CASES:
        rz, tel, comp, obs, first, samples, det, psds, want = sc.ts_case(name)
        got = simulate(rz, tel, comp, obs, first, samples, det, psds)
        dist = sc.rel_rms(got, want)
        print(f"timestream case {name} (firstsamp {first}, samples {samples}): distance {dist:.3e} of the rms, "
              f"bound {TS_BOUND:.3e}")
        assert dist <= TS_BOUND, name


def test_device_mixing_matrix_call():
    """The fixture's non-diagonal case through the C ABI: CSR by stream, two streams share row 1."""
    rz, tel, comp, obs, first, samples, det, psds, want = sc.ts_case("mix")
    mat = GOLD["ts_mix_matrix"]
    ptr, rows, weights = [0], [], []
    for s in range(mat.shape[1]):
        for r in range(mat.shape[0]):
            if mat[r, s] != 0:
                rows.append(r)
                weights.append(mat[r, s])
        ptr.append(len(rows))
    before = 1e-3 * np.linspace(-1.0, 1.0, 3 * samples).reshape(3, samples)
    got = simulate(rz, tel, comp, obs, first, samples, det, psds, start=before, n_rows=3, mix_ptr=ptr, mix_row=rows,
                   mix_weight=weights)
    noise_rms = np.sqrt(np.mean((want - before) ** 2, axis=1))
    dist = float(np.max(np.max(np.abs(got - want), axis=1) / noise_rms))
    print(f"mixing case: distance {dist:.3e} of the noise rms, bound {TS_BOUND:.3e}")
    assert dist <= TS_BOUND
    from toast_amd import capi

    with pytest.raises(RuntimeError, match="outside det_data"):
        simulate(rz, tel, comp, obs, first, samples, det, psds, n_rows=2, mix_ptr=ptr, mix_row=rows, mix_weight=weights)
    del capi


def test_invariance():
    rz, tel, comp, obs, first, samples, det, psds, _ = sc.ts_case("a")
    together = simulate(rz, tel, comp, obs, first, samples, det, psds)
    assert np.array_equal(together, simulate(rz, tel, comp, obs, first, samples, det, psds))     # twice
    for i in range(det.size):
        alone = simulate(rz, tel, comp, obs, first, samples, det[i:i + 1], psds[i:i + 1])
        assert np.array_equal(alone[0], together[i]), i
    for max_batch in (1, 2):
        assert np.array_equal(simulate(rz, tel, comp, obs, first, samples, det, psds, max_batch=max_batch), together)
    # shared rows in one batch and in separate batches
    mat_ptr, mat_row, mat_w = [0, 2, 4, 5], [0, 1, 1, 2, 0], [1.0, 0.5, 0.25, -2.0, 3.0]
    mixed = [simulate(rz, tel, comp, obs, first, samples, det, psds, mix_ptr=mat_ptr, mix_row=mat_row, mix_weight=mat_w,
                      max_batch=mb) for mb in (0, 1, 2)]
    assert np.array_equal(mixed[0], mixed[1]) and np.array_equal(mixed[0], mixed[2])


def test_operator_on_resident_data(monkeypatch):
    from toast_amd import ops
    from toast_amd.data import defaults

    results = {}
    for where in ("host", "device"):
        data = sc.make_data(n_det=3, n_samp=3000)
        dd = data.obs[0].detdata[defaults.det_data]
        dd.data[:] = 1e-3
        if where == "device":
            dd.accel_create(defaults.det_data)
            dd.accel_update_device()
            dd.accel_used(True)
        ops.SimNoise(realization=2, component=5).apply(data)       # the path follows the data
        assert dd.accel_in_use() == (where == "device")
        results[where] = dd.data.copy()
    noise = results["host"] - 1e-3
    dist = float(np.max(np.max(np.abs(results["device"] - results["host"]), axis=1) / np.sqrt(np.mean(noise**2, axis=1))))
    print(f"operator, resident det_data against the host path: distance {dist:.3e} of the noise rms, bound {TS_BOUND:.3e}")
    assert dist <= TS_BOUND and np.std(noise) > 0
    # the fixture's mixing case through the operator (its timestamps give a rate a few 1e-15 off 37 Hz: the fixture's
    # rate is handed to the operator instead)
    import test_sim_noise_host as th
    import toast_amd.ops.sim_tod_noise as mod

    monkeypatch.setattr(mod, "rate_from_times", lambda t: RATE)
    data, want = th.mix_observation()
    ops.SimNoise(realization=1, component=3).apply(data, use_accel=True)
    got = data.obs[0].detdata[defaults.det_data].data
    noise_rms = np.sqrt(np.mean((want - th.mix_before()) ** 2, axis=1))
    dist = float(np.max(np.max(np.abs(got - want), axis=1) / noise_rms))
    print(f"operator, mixing case on the device: distance {dist:.3e} of the noise rms, bound {TS_BOUND:.3e}")
    assert dist <= TS_BOUND


def test_full_length_and_spectrum():
    from toast_amd import capi

    # cfg-3 length: 720 000 samples at 200 Hz, fftlen 2^21
    freq, psd = sc.stat_psd()
    samples, rate, n_det = 720000, 200.0, 4
    from toast_amd.noise import AnalyticNoise

    an = AnalyticNoise(detectors=["d"], rate={"d": rate}, fmin={"d": 1e-5}, fknee={"d": 0.05}, alpha={"d": 1.0},
                       NET={"d": 50e-6})
    f200, p200 = np.asarray(an.freq("d")), np.tile(np.asarray(an.psd("d")), (n_det, 1))
    assert capi.sim_noise_fft_length(samples, 2) == 1 << 21
    det = np.array([0, 1, 1000, 4294967295], dtype=np.uint64)
    # The real check at this length is the device against the host entries.  The run under fft.select(True) is kept for
    # the day the fused inverse passes are fed: today the device transform is rocFFT under both settings (DESIGN.md
    # section 7b), so that comparison is between two runs of the same plans and can only show 0.
    from toast_amd import fft

    device = simulate(1, 2, 0, 3, 0, samples, det, p200, rate=rate, freq=f200)
    was_forced = fft.implementation(samples) == "rocfft"     # (a fused length: "rocfft" only when forced)
    fft.select(True)
    try:
        forced = simulate(1, 2, 0, 3, 0, samples, det, p200, rate=rate, freq=f200)
    finally:
        fft.select(was_forced)
    host = np.zeros((n_det, samples))
    capi.tod_sim_noise_timestream_batch(1, 2, 0, 3, rate, 0, 2, det, f200, p200, host)
    d_host = sc.rel_rms(device, host)
    d_forced = sc.rel_rms(device, forced)
    print(f"720 000 samples: device against the host entries {d_host:.3e} of the rms; bound {TS_BOUND:.3e}; under "
          f"fft.select(True) (the same rocFFT plans today) {d_forced:.3e}")
    assert d_host <= TS_BOUND and d_forced <= TS_BOUND
    # the periodogram check of test_sim_noise_host.py on device output
    n_det, samples, rate = sc.STAT["n_det"], sc.STAT["samples"], sc.STAT["rate"]
    ts = simulate(0, 1, 0, 2, 0, samples, np.arange(n_det, dtype=np.uint64), np.tile(psd, (n_det, 1)), rate=rate,
                  freq=freq)
    scale = capi.tod_sim_noise_psd_interp(rate, samples, 2, freq, psd[None, :])[0]
    rows = sc.spectrum_check(ts, scale)
    for k0, k1, ratio, sigma in rows:
        print(f"modes {k0:5d} .. {k1:5d}: periodogram / PSD = {ratio:.4f}, sigma {sigma:.4f}, "
              f"{(ratio - 1) / sigma:+.2f} sigma")
    for k0, k1, ratio, sigma in rows:
        assert abs(ratio - 1.0) <= 5.0 * sigma, (k0, k1, ratio, sigma)


def test_workflow_with_simulated_noise():
    import sim_satellite_simple as wf

    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        data = wf.main(["--sim-noise", "--destripe"])
    text = out.getvalue()
    print(text)
    iterations = int(re.search(r"PCG iterations (\d+)", text).group(1))
    assert 0 < iterations < 50          # converged before iter_max
    m = data["mapmaker_map"].data
    assert np.all(np.isfinite(m)) and np.std(m) > 0
