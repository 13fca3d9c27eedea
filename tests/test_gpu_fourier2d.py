"""GPU: the Fourier2D template (csrc/fourier2d.hip) against tests/golden/fourier2d.npz -- the results of the reference's
own methods (tests/golden/make_golden_fourier2d.py) on the inputs of tests/fourier2d_case.py -- through the C ABI and
through the class on device-resident buffers.

Bit-exact on the device, and asserted as equality: the norms, ``project_signal`` in one detector group (the reference's own
sequence of roundings: the amplitude that is there, then one rounded product per detector), ``add_to_signal`` (the sum over
the modes is taken in the order of NumPy's pairwise sum, and detector groups do not change it), ``apply_precond``.

Bounds that were measured, not guessed (the ``yard_*`` entries of the fixture, per case):

* ``project_signal`` with the detectors split over the grid takes its sum in another order: ten times the reference's own
  deviation from the exactly summed value (``math.fsum`` of the rounded products), in units of ``eps sum|terms|``; the
  reference's figure is 0.96 to 2.5 over the cases;
* the prior is a circular convolution of up to twice SciPy's length with rocFFT's twiddles: eight times the LARGEST
  distance of the reference from the same convolution summed directly in ``longdouble``, 2.85e-16 of ``max|out|``.

End to end: ``MapMaker`` over [Offset, Fourier2D] against the amplitudes and the residual history of the reference's
``solve()`` with the prior inside the left-hand side (the ``e2e_*`` entries).  The same solve runs in the order-exact mode
of the scatter with the template on its NumPy host path and on the device; both are bounded by ten times the measured
distance of the host run to the reference (``E2E_HOST_DISTANCE``; see there).  The test prints every figure before it
asserts.  It compares trajectories only: the reference's residual does not fall within the 8 iterations of the case, so
nothing here shows how well such a solve converges.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fourier2d_case as fc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "fourier2d.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
# Measured distance of MapMaker with the host-path template to the reference's solve() on an MI355X, relative to the
# largest amplitude / per entry of the residual history.  The prior's filter spans eleven decades (1 / fcorr with the floor
# at 1e-6 of the amplitude), so the solve amplifies the roundings of the dot products far more than the three-template case
# of test_gpu_templates.py does.  The device run of the same measurement gave 6.61e-12 / 3.33e-12 / 1.68e-12.
E2E_HOST_DISTANCE = {"baselines": 4.41e-12, "fourier2d": 2.20e-12, "history": 1.17e-12}


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)     # (its own host key)
        accel_data_create(self.a, "test_fourier2d")
        accel_data_update_device(self.a, "test_fourier2d")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_fourier2d")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_fourier2d")


def _to_device(data, keys=(fc.DET_DATA,)):
    for ob in data.obs:
        for key in keys:
            dd = ob.detdata[key]
            if not dd.accel_exists():
                dd.accel_create(key)
            if not dd.accel_in_use():
                dd.accel_update_device()


def _template(name, **extra):
    from toast_amd.templates import Fourier2D

    layout, traits = fc.CASES[name]
    data = fc.build(layout)
    tmpl = fc.configure(Fourier2D(name=name, **{**traits, **extra}))
    tmpl.data = data
    return data, tmpl


def _resident(tmpl, values):
    z = tmpl.zeros()
    z.local[:] = values
    z.accel_resident(f"{tmpl.name}_test")
    return z


def _view_offsets(name, iob):
    """Amplitude offsets of the views of one observation, from the fixture's flat list."""
    layout, _ = fc.CASES[name]
    n_before = sum(len(v) for v in fc.view_samples(layout)[:iob])
    return GOLD[f"{name}_view_offset"][n_before:n_before + len(fc.view_samples(layout)[iob])]


@pytest.mark.parametrize("name", list(fc.DEVICE_CASES))
def test_c_abi_matches_reference(name):
    from toast_amd import capi
    from toast_amd.accel import native

    layout, traits = fc.CASES[name]
    data = fc.build(layout)
    nmode = int(GOLD[f"{name}_nmode"])
    n_local = int(GOLD[f"{name}_n_local"])
    rows, cols = fc.sample_subset(layout)
    templates = [GOLD[f"{name}_T_obs{iob}"] for iob in range(len(data.obs))]
    add_scale, proj_scale = fc.term_scales(name, templates)
    f_project = 10.0 * float(GOLD[f"{name}_yard_project"])
    D = capi.dev
    start = fc.amplitudes(n_local, 2)
    amps = Dev(fc.amplitudes(n_local, 1))
    norms = Dev(np.full(n_local, -1.0))
    runs = (("one group", 1), ("three groups", 3), ("rule", 0), ("one group again", 1), ("rule again", 0))
    results = {label: Dev(start) for label, _ in runs}
    want_norms = np.zeros(n_local)      # the reference's sums (fourier2d.py:342-365) for EVERY sample, on the host
    for iob, ob in enumerate(data.obs):
        dets = list(ob.local_detectors)
        n_det = len(dets)
        sig = Dev(ob.detdata[fc.DET_DATA].data)
        flg = Dev(ob.detdata[fc.DET_FLAGS].data)
        idx = np.arange(n_det, dtype=np.int32)
        t = Dev(templates[iob])
        w = np.ones(n_det) if traits["noise_model"] is None else np.array([ob[fc.NOISE].detector_weight(d) for d in dets])
        w2 = Dev(np.array([templates[iob][k] ** 2 * w[k] for k in range(n_det)]))
        ivl = ob.intervals[fc.VIEW].data
        voff = _view_offsets(name, iob)
        n_samp = ob.n_local_samples
        D.fourier2d_norms(nmode, w2.ptr, voff, idx, flg.ptr, fc.DET_FLAG_MASK, n_det, n_samp, ivl, norms.ptr)
        for off, (first, last) in zip(voff, fc.view_samples(layout)[iob]):
            norms_view = want_norms[off:off + (last - first) * nmode].reshape(-1, nmode)
            for k in range(n_det):
                good = ((ob.detdata[fc.DET_FLAGS].data[k, first:last] & fc.DET_FLAG_MASK) == 0).astype(np.float64)
                norms_view += np.outer(good, w2.a[k])
        for label, n_group in runs:
            D.fourier2d_project_signal(nmode, t.ptr, voff, results[label].ptr, idx, sig.ptr, n_samp, ivl, n_group=n_group)
        # d + M a: the detector groups do not change a bit
        sig3 = Dev(ob.detdata[fc.DET_DATA].data)
        D.fourier2d_add_to_signal(nmode, t.ptr, voff, amps.ptr, idx, sig.ptr, n_samp, ivl, n_group=1)
        D.fourier2d_add_to_signal(nmode, t.ptr, voff, amps.ptr, idx, sig3.ptr, n_samp, ivl, n_group=0)
        got = sig.get()
        assert np.array_equal(got, sig3.get())
        err = np.abs(got[:, cols[iob]] - GOLD[f"{name}_add_obs{iob}"]) / (EPS * add_scale[iob])
        print(f"{name}: add_to_signal obs{iob}, worst deviation from the fixture {err.max():.2f} eps sum|terms|")
        assert np.array_equal(got[:, cols[iob]], GOLD[f"{name}_add_obs{iob}"])
        outside = np.ones(n_samp, dtype=bool)
        for first, last in fc.view_samples(layout)[iob]:
            outside[first:last] = False
        assert np.array_equal(got[:, outside], ob.detdata[fc.DET_DATA].data[:, outside])
        for d in (sig, sig3, flg, t, w2):
            d.free()
    got_norms = norms.get().reshape(-1, nmode)
    assert np.array_equal(got_norms[rows], GOLD[f"{name}_norms"])
    # every amplitude belongs to a view: none keeps the -1 it was filled with, and all equal the host's sums
    want_norms[want_norms != 0] = 1.0 / want_norms[want_norms != 0]
    assert np.array_equal(got_norms.reshape(-1), want_norms)
    zero = fc.all_flagged_row(layout)
    if zero is not None:
        assert np.all(got_norms[zero] == 0.0)
    proj = {k: v.get().reshape(-1, nmode) for k, v in results.items()}
    assert np.array_equal(proj["one group"][rows], GOLD[f"{name}_project"])
    assert np.array_equal(proj["one group"], proj["one group again"])
    assert np.array_equal(proj["rule"], proj["rule again"])
    for label in ("three groups", "rule"):
        err = np.abs(proj[label][rows] - GOLD[f"{name}_project"]) / (EPS * proj_scale)
        print(f"{name}: project_signal, {label}: worst deviation from the fixture {err.max():.2f} eps sum|terms| "
              f"(bound {f_project:.2f}); differs from one group in {np.count_nonzero(proj[label] != proj['one group'])} values")
        assert np.all(err <= f_project)
    if layout == "wide":
        assert np.any(proj["rule"] != proj["one group"])       # the rule did split the detectors
    # preconditioner: one multiply per amplitude
    out = Dev(np.full(n_local, -3.0))
    D.fourier2d_apply_precond(n_local, norms.ptr, amps.ptr, out.ptr)
    assert np.array_equal(out.get(), amps.a * got_norms.reshape(-1))
    if zero is not None:
        assert np.all(out.get().reshape(-1, nmode)[zero] == 0.0)
    # prior, view after view, on top of an output that is not zero
    from toast_amd.templates.fourier2d import half_complex, prior_fft_length

    pout = Dev(np.full(n_local, 0.5))
    scale = GOLD[f"{name}_filter_scale"]
    cum = 0
    for iob in range(len(data.obs)):
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            filt = GOLD[f"{name}_invcorr_{iob}_{ivw}"]
            n_fft = prior_fft_length(last - first, filt.size)
            spec = Dev(half_complex(np.fft.rfft(filt, n_fft), n_fft))
            work = Dev(np.zeros(2 * nmode * n_fft))
            off = int(_view_offsets(name, iob)[ivw])
            D.fourier2d_add_prior(nmode, last - first, amps.ptr + 8 * off, pout.ptr + 8 * off, filt.size, n_fft, spec.ptr,
                                  scale, work.ptr)
            native().accel_synchronize()
            spec.free()
            work.free()
    bound = 8.0 * float(GOLD["yard_prior_max"]) * float(GOLD[f"{name}_prior_max"])
    err = np.abs(pout.get().reshape(-1, nmode)[rows] - GOLD[f"{name}_prior"]).max()
    print(f"{name}: add_prior, distance to the fixture {err:.3e} = {err / float(GOLD[f'{name}_prior_max']):.2e} max|out| "
          f"(bound {bound:.3e} = {8.0 * float(GOLD['yard_prior_max']):.2e} max|out|)")
    assert err <= bound
    for d in [amps, norms, out, pout] + list(results.values()):
        d.free()


def test_views_are_clipped_to_the_observation():
    """A view that starts before sample 0 and ends past the last one is clipped to [0, n_samp); the amplitude offset stays
    that of the view's own first sample, so the amplitudes of the samples cut away are neither read nor written."""
    from toast_amd import capi
    from toast_amd.capi import interval_dtype

    name = "m37"
    layout, _ = fc.CASES[name]
    ob = fc.build(layout).obs[0]
    nmode, n_samp, before, after = int(GOLD[f"{name}_nmode"]), ob.n_local_samples, 5, 7
    templates = GOLD[f"{name}_T_obs0"]
    n_det = templates.shape[0]
    idx = np.arange(n_det, dtype=np.int32)
    n_amp = (before + n_samp + after) * nmode
    inside = slice(before * nmode, (before + n_samp) * nmode)
    wide, exact = np.zeros(1, dtype=interval_dtype), np.zeros(1, dtype=interval_dtype)
    wide["first"], wide["last"] = -before, n_samp + after
    exact["first"], exact["last"] = 0, n_samp
    t = Dev(templates)
    w2 = Dev(templates ** 2)
    flg = Dev(ob.detdata[fc.DET_FLAGS].data)
    got = {}
    for label, ivl, voff in (("wide", wide, np.array([0], dtype=np.int64)),
                             ("exact", exact, np.array([before * nmode], dtype=np.int64))):
        sig = Dev(ob.detdata[fc.DET_DATA].data)
        proj = Dev(fc.amplitudes(n_amp, 2))
        norms = Dev(np.full(n_amp, -1.0))
        amps = Dev(fc.amplitudes(n_amp, 1))
        D = capi.dev
        D.fourier2d_project_signal(nmode, t.ptr, voff, proj.ptr, idx, sig.ptr, n_samp, ivl, n_group=0)
        D.fourier2d_norms(nmode, w2.ptr, voff, idx, flg.ptr, fc.DET_FLAG_MASK, n_det, n_samp, ivl, norms.ptr)
        D.fourier2d_add_to_signal(nmode, t.ptr, voff, amps.ptr, idx, sig.ptr, n_samp, ivl, n_group=0)
        got[label] = (proj.get(), norms.get(), sig.get())
        for d in (sig, proj, norms, amps):
            d.free()
    for d in (t, w2, flg):
        d.free()
    for a, b in zip(got["wide"], got["exact"]):
        assert np.array_equal(a, b)
    proj, norms, sig = got["wide"]
    outside = np.ones(n_amp, dtype=bool)
    outside[inside] = False
    assert np.array_equal(proj[outside], fc.amplitudes(n_amp, 2)[outside]) and np.all(norms[outside] == -1.0)
    assert np.all(norms[inside] != -1.0) and np.any(proj[inside] != fc.amplitudes(n_amp, 2)[inside])
    assert np.any(sig != ob.detdata[fc.DET_DATA].data)


@pytest.mark.parametrize("name", list(fc.DEVICE_CASES))
def test_class_on_resident_buffers(name):
    from toast_amd.accel import accel_data_present

    layout, _ = fc.CASES[name]
    data, tmpl = _template(name)
    nmode = tmpl.nmode
    assert tmpl.supports_accel()
    rows, cols = fc.sample_subset(layout)
    dets = tmpl.detectors()
    assert tmpl._n_local == int(GOLD[f"{name}_n_local"])
    # the norms were computed on the device at set-up and stay there
    assert tmpl._mirrors["norms"].on_device and tmpl._mirrors["norms"].stale
    # so were the prior's spectra and work rows: the PCG loop allocates nothing
    assert tmpl._work[0] != 0 and len(tmpl._prior_views) == sum(len(v) for v in fc.view_samples(layout))
    assert np.array_equal(tmpl._norms.reshape(-1, nmode)[rows], GOLD[f"{name}_norms"])
    _to_device(data)
    proj = _resident(tmpl, fc.amplitudes(tmpl._n_local, 2))
    tmpl.project_signal_multi(dets, proj, n_group=1)
    assert proj.accel_in_use()
    assert np.array_equal(proj.local.reshape(-1, nmode)[rows], GOLD[f"{name}_project"])
    again = _resident(tmpl, fc.amplitudes(tmpl._n_local, 2))
    tmpl.project_signal_multi(dets, again)
    twice = _resident(tmpl, fc.amplitudes(tmpl._n_local, 2))
    tmpl.project_signal_multi(dets, twice)
    assert np.array_equal(again.local, twice.local)
    templates = [GOLD[f"{name}_T_obs{iob}"] for iob in range(len(data.obs))]
    _, proj_scale = fc.term_scales(name, templates)
    f_project = 10.0 * float(GOLD[f"{name}_yard_project"])
    err = np.abs(again.local.reshape(-1, nmode)[rows] - GOLD[f"{name}_project"]) / (EPS * proj_scale)
    print(f"{name}: project_signal_multi by the rule, worst deviation {err.max():.2f} eps sum|terms| (bound {f_project:.2f})")
    assert np.all(err <= f_project)
    amps = _resident(tmpl, fc.amplitudes(tmpl._n_local, 1))
    tmpl.add_to_signal_multi(dets, amps)
    for iob, ob in enumerate(data.obs):
        assert np.array_equal(ob.detdata[fc.DET_DATA].data[:, cols[iob]], GOLD[f"{name}_add_obs{iob}"]), (name, iob)
    out = _resident(tmpl, -3.0)
    tmpl.apply_precond(amps, out)
    assert out.accel_in_use()
    assert np.array_equal(out.local, amps.local * tmpl._norms)
    zero = fc.all_flagged_row(layout)
    if zero is not None:
        assert np.all(tmpl._norms.reshape(-1, nmode)[zero] == 0.0) and np.all(out.local.reshape(-1, nmode)[zero] == 0.0)
    pout = _resident(tmpl, 0.5)
    amps.accel_resident()
    tmpl.add_prior(amps, pout)
    assert pout.accel_in_use() and tmpl._work[0] != 0
    bound = 8.0 * float(GOLD["yard_prior_max"]) * float(GOLD[f"{name}_prior_max"])
    err = np.abs(pout.local.reshape(-1, nmode)[rows] - GOLD[f"{name}_prior"]).max()
    print(f"{name}: add_prior on resident vectors, distance to the fixture {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    work = tmpl._work
    amps.accel_resident()
    pout.accel_resident()
    tmpl.add_prior(amps, pout)
    assert tmpl._work == work            # nothing is allocated after the first call
    # clear() leaves nothing registered
    keys = tmpl.device_tables()
    assert len(keys) >= 2 and all(accel_data_present(k) for k in keys)
    tmpl.clear()
    assert not any(accel_data_present(k) for k in keys)
    assert tmpl.device_tables() == [] and tmpl._work == (0, 0)
    for z in (proj, again, twice, amps, out, pout):
        z.clear()


def _e2e(host_template):
    from toast_amd import capi, ops
    from toast_amd.data import defaults
    from toast_amd.templates import Fourier2D, Offset

    class HostFourier2D(Fourier2D):
        def supports_accel(self):
            return False

    cls = HostFourier2D if host_template else Fourier2D
    data, cfg = fc.build_e2e()
    was = capi.get_deterministic()
    capi.set_deterministic(True)
    try:
        dp = ops.PointingDetectorSimple()
        pix = ops.PixelsHealpix(detector_pointing=dp, nside=cfg["nside"], nest=True)
        sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", hwp_angle=defaults.hwp_angle)
        binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=True)
        tm = ops.TemplateMatrix(templates=[
            Offset(step_time=cfg["step_time"], noise_model=defaults.noise_model, name="baselines"),
            cls(order=cfg["order"], fit_subharmonics=cfg["fit_subharmonics"], noise_model=defaults.noise_model,
                correlation_length=cfg["correlation_length"], correlation_amplitude=cfg["correlation_amplitude"],
                name="fourier2d")])
        mm = ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=tm, iter_min=cfg["iters"],
                          iter_max=cfg["iters"], convergence=1e-30, keep_solver_products=True)
        mm.apply(data)
    finally:
        capi.set_deterministic(was)
    amps = data["mm_solve_amplitudes"]
    assert list(amps.keys()) == list(fc.E2E_NAMES)
    return {k: amps[k].local.copy() for k in fc.E2E_NAMES}, {k: amps[k].local_flags.copy() for k in fc.E2E_NAMES}, \
        np.array(mm.history), tuple(mm.lhs_route)


def test_mapmaker_over_offset_and_fourier2d_equals_reference_solve():
    want_hist = GOLD["e2e_history"]

    def distance(amps, hist):
        d = {k: float(np.abs(amps[k] - GOLD[f"e2e_amplitudes_{k}"]).max() / np.abs(GOLD[f"e2e_amplitudes_{k}"]).max())
             for k in fc.E2E_NAMES}
        d["history"] = float(np.max(np.abs(hist - want_hist) / want_hist))
        return d

    h_amps, h_flags, h_hist, h_route = _e2e(host_template=True)
    assert len(h_hist) == len(want_hist)
    host = distance(h_amps, h_hist)
    print("E2E host-path template, distance to the reference:", "  ".join(f"{k} {v:.2e}" for k, v in host.items()))
    d_amps, d_flags, d_hist, d_route = _e2e(host_template=False)
    assert d_route == ("sequence",) and len(d_hist) == len(want_hist)
    dev = distance(d_amps, d_hist)
    print("E2E device template, distance to the reference:   ", "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for amps, flags in ((h_amps, h_flags), (d_amps, d_flags)):
        for k in fc.E2E_NAMES:
            assert amps[k].size == GOLD[f"e2e_amplitudes_{k}"].size
            assert np.array_equal(flags[k], GOLD[f"e2e_flags_{k}"]), k
    for k, figure in E2E_HOST_DISTANCE.items():
        assert host[k] <= 10.0 * figure, ("host path", k, host[k], figure)
        assert dev[k] <= 10.0 * figure, ("device", k, dev[k], figure)
