"""GPU: the GainTemplate kernels (k_legendre_* of csrc/template_basis.hip) against tests/golden/gain_template.npz -- the
results of the reference's own methods (tests/golden/make_golden_gain_template.py) on the inputs of
tests/gain_template_case.py -- through the C ABI and through the class on device-resident buffers.

Bit-exact on the device: amplitude layout, ``n_local``, and ``add_to_signal`` against the template's own host path (an
explicit ascending-k loop).  Against the REFERENCE ``add_to_signal`` cannot be bit-exact from order 2 on (another
evaluation of the Legendre polynomials, see toast_amd/templates/gaintemplate.py); the host path is bounded there.

The reductions are taken in another ORDER than NumPy's and are compared under bounds that were measured, not guessed.
For the fixture's inputs the reference's own results deviate from exactly summed values (the generator's docstring has
the three definitions; it prints these figures) by at most

    project_signal   1.32 eps (PRESET + sum|terms|)           per case 0.51 1.32 0.37 0.98 0.42 0.98
    inverse Gram     0.63 eps cond(G) max|G^-1|               per case 0.63 0.63 0.28 0.28 0.11 0.13, cond up to 21.4
    add_to_signal    8.33 eps (|s| + |est| sum|T_k a_k|)      per case 0.89 1.22 6.30 6.30 8.33 8.33

and the device gets an order of magnitude over those figures for its different summation tree (the rule of
tests/test_gpu_templates.py): 13.2, 6.3 and 83.3.  ``apply_precond`` adds the rounding of a dot product of ``norder``
terms to the error of the matrix: ``(6.3 cond + norder) eps max|G^-1| sum|a|`` per amplitude.  The Gram matrix itself has
no figure of the reference's (it only keeps the inverse): the C-ABI test bounds it by the depth of the device's own
summation tree -- 16 strided adds per lane, 6 butterfly steps, 4 waves, 2 chunks: 28 additions and one product rounding
on every path, 14.5 eps sum|terms|, taken as 16.

End to end: ``MapMaker`` over [Offset, GainTemplate] against the amplitudes and the residual history of the reference's
``solve()`` (the ``e2e_*`` entries of the fixture), in the order-exact mode of the scatter, with the template on its
NumPy host path (``supports_accel`` answers no) and on the device.  The host path's distance to the reference was
measured on an MI355X: 3.67e-14 / 5.84e-15 of the largest amplitude for baselines / gain and 6.61e-14 relative in the
history (``E2E_HOST_DISTANCE``; the device run of the same session: 3.53e-14 / 6.00e-15 / 7.50e-14).  BOTH runs are
bounded by ten times the host figures and, independently, by the project's parity bar of 1e-10 relative.  The test
prints all figures before it asserts.

Measured on the same MI355X for the record (the tests print them): the device's projection lies within 1.34 eps
sum|terms| of the fixture and 0.51 of the exact sums, its inverse Gram matrices within 0.63 eps cond max|G^-1|; at the
C-ABI shapes projection and Gram matrix lie within 0.69 and 1.31 eps sum|terms| of the exact sums; the workflow recovers
the injected drift to 6e-13 of its rms.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gain_template_case as gc  # noqa: E402
import templates_case as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "gain_template.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
F_PROJECT, F_INVERSE, F_ADD, F_GRAM = 13.2, 6.3, 83.3, 16.0
# measured distance of MapMaker with the host-path template to the reference's solve() (see the module docstring)
E2E_HOST_DISTANCE = {"baselines": 3.67e-14, "gain": 5.84e-15, "history": 6.61e-14}
PARITY = 1.0e-10


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)     # (its own host key)
        accel_data_create(self.a, "test_gain")
        accel_data_update_device(self.a, "test_gain")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_gain")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_gain")


def _to_device(data, keys=(tc.DET_DATA,)):
    for ob in data.obs:
        for key in keys:
            dd = ob.detdata[key]
            if not dd.accel_exists():
                dd.accel_create(key)
            if not dd.accel_in_use():
                dd.accel_update_device()


def _resident(tmpl, values):
    z = tmpl.zeros()
    z.local[:] = values
    z.accel_resident(f"{tmpl.name}_test")
    return z


def _host_class():
    from toast_amd.templates import GainTemplate

    class HostGain(GainTemplate):
        def supports_accel(self):
            return False

    return HostGain


def _make(name, cls=None):
    from toast_amd.templates import GainTemplate

    traits, det_flags = gc.template_traits(name)
    data = gc.build()
    tmpl = gc.configure((cls or GainTemplate)(name=name, **traits), det_flags=det_flags)
    tmpl.data = data
    return data, tmpl


def _add_scale(data, tmpl, amps):
    from toast_amd.templates.subharmonic import legendre_basis

    ob = data.obs[0]
    norder = tmpl.order + 1
    basis = legendre_basis(norder, ob.n_local_samples)
    mag = np.abs(basis[None, :, :] * amps.reshape(-1, norder)[:, :, None]).sum(axis=1)
    return np.abs(ob.detdata[tc.DET_DATA].data) + np.abs(ob.detdata[gc.ESTIMATE].data) * mag


# ------------------------------------------------------------------ 1. the fixture's cases through the class
@pytest.mark.parametrize("name", list(gc.CASES))
def test_device_matches_reference(name):
    data, tmpl = _make(name)
    assert tmpl.supports_accel()
    norder = tmpl.order + 1
    dets = tmpl.detectors()
    assert tmpl._n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal([tmpl._det_start[d] for d in dets], GOLD[f"{name}_det_start"])
    # preconditioner: Gram matrices from the device (all samples, no flags), inverted on the host
    ref = GOLD[f"{name}_precond"]
    worst = max(np.abs(tmpl._precond[b] - ref[b]).max() / (EPS * np.linalg.cond(ref[b]) * np.abs(ref[b]).max())
                for b in range(ref.shape[0]))
    print(f"{name}: inverse Gram, worst deviation {worst:.2f} eps cond max|G^-1| (bound {F_INVERSE})")
    assert worst <= F_INVERSE
    _to_device(data)
    # M^T d onto the preset amplitudes, with the flags; twice for the bits
    scale = GOLD[f"{name}_project_scale"]
    proj = _resident(tmpl, gc.PRESET)
    tmpl.project_signal_multi(dets, proj)
    first = proj.local.copy()
    err = np.abs(first - GOLD[f"{name}_project"]) / (EPS * scale)
    print(f"{name}: project_signal, worst deviation from the fixture {err.max():.2f} eps sum|terms| (bound {F_PROJECT}); "
          f"from the exact sums {(np.abs(first - GOLD[f'{name}_project_exact']) / (EPS * scale)).max():.2f}")
    assert np.all(err <= F_PROJECT)
    again = _resident(tmpl, gc.PRESET)
    tmpl.project_signal_multi(dets, again)
    assert np.array_equal(again.local, first)
    # d + M a: the device equals the host path bit for bit; the host path lies within its bound of the reference
    values = tc.amplitudes(tmpl._n_local, 1)
    host_data, host = _make(name, _host_class())
    add_scale = _add_scale(host_data, host, values)
    h_amps = host.zeros()
    h_amps.local[:] = values
    for det in dets:
        host.add_to_signal(det, h_amps)
    want = host_data.obs[0].detdata[tc.DET_DATA].data
    amps = _resident(tmpl, values)
    tmpl.add_to_signal_multi(dets, amps)
    got = data.obs[0].detdata[tc.DET_DATA].data
    assert np.array_equal(got, want)
    err = np.abs(want - GOLD[f"{name}_add_obs0"]) / (EPS * add_scale)
    print(f"{name}: add_to_signal, host path from the fixture {err.max():.2f} eps (|s| + |est| sum|T a|) (bound {F_ADD})")
    assert np.all(err <= F_ADD)
    if tmpl.order <= 1:
        assert np.array_equal(got, GOLD[f"{name}_add_obs0"])
    # preconditioner applied to resident vectors
    out = _resident(tmpl, 0.0)
    tmpl.apply_precond(amps, out)
    assert out.accel_in_use()
    bound = EPS * np.array([(F_INVERSE * np.linalg.cond(p) + norder) * np.abs(p).max() for p in ref]).repeat(norder) * \
        np.abs(values).reshape(-1, norder).sum(axis=1).repeat(norder)
    assert np.all(np.abs(out.local - GOLD[f"{name}_precond_out"]) <= bound)
    tmpl.clear()
    host.clear()
    for z in (proj, again, amps, out):
        z.clear()


# ------------------------------------------------------------------ 2. the kernels at the shapes that can go wrong
VIEWS = [(0, 1), (3, 5), (6, 9), (11, 4107), (4108, 8205), (8206, 8270)]      # 1, 2, 3, 4096, 4097 and 64 samples
N_SAMP = 8271                                                                # odd: every other row starts 8 bytes off


@pytest.mark.parametrize("norder", [1, 2, 9])
def test_kernels_short_views_chunk_edges_and_alignment(norder):
    """C ABI.  Views of 1, 2 and 3 samples (np.linspace's special cases), of exactly one reduction chunk and one sample
    more, starting on odd samples of an odd-length row; signal, estimate and flag rows permuted differently (so the
    16-byte alignment of signal and estimate differs from row to row), amplitude blocks in another order than the rows;
    30 % flags plus unrelated bits; the last view fully flagged."""
    from toast_amd import capi
    from toast_amd.capi import interval_dtype
    from toast_amd.templates.subharmonic import legendre_basis

    D = capi.dev
    rng = np.random.default_rng(23 + norder)
    n_det, n_view = 3, len(VIEWS)
    ivl = np.zeros(n_view, dtype=interval_dtype)
    ivl["first"], ivl["last"] = [v[0] for v in VIEWS], [v[1] for v in VIEWS]
    sig0 = rng.standard_normal((n_det, N_SAMP))
    est0 = 2.0 + rng.standard_normal((n_det + 1, N_SAMP))       # one row more than the signal
    flags = (rng.random((n_det, N_SAMP)) < 0.3).astype(np.uint8) | 2 | ((rng.random((n_det, N_SAMP)) < 0.5).astype(np.uint8) * 4)
    flags[:, VIEWS[-1][0]:VIEWS[-1][1]] |= 1
    amps = rng.standard_normal(n_det * n_view * norder)
    offs = (np.array([2, 0, 1]) * n_view * norder).astype(np.int64)
    rows = np.array([1, 2, 0], dtype=np.int32)
    erows = np.array([3, 0, 2], dtype=np.int32)
    frows = np.array([0, 2, 1], dtype=np.int32)
    weights = np.array([1.0, 0.5, 4.0])          # powers of two: dividing them out is exact
    d_sig, d_est, d_amps, d_flags = Dev(sig0), Dev(est0), Dev(amps), Dev(flags)
    # ---- add_to_signal: bit for bit an explicit ascending-k loop
    D.gain_add_to_signal(norder, offs, d_amps.ptr, rows, d_sig.ptr, erows, d_est.ptr, N_SAMP, ivl)
    want = sig0.copy()
    for k in range(n_det):
        for v, (first, last) in enumerate(VIEWS):
            basis = legendre_basis(norder, last - first)
            a = amps[offs[k] + v * norder:][:norder]
            gain = np.zeros(last - first)
            for order in range(norder):
                gain += basis[order] * a[order]
            want[rows[k], first:last] += est0[erows[k], first:last] * gain
    got_sig = d_sig.get()
    assert np.array_equal(got_sig, want)
    assert np.array_equal(d_est.get(), est0)
    # ---- projection of the seeded signal onto preset amplitudes, and the Gram matrices
    d_sig2, d_out = Dev(sig0), Dev(np.full(amps.size, gc.PRESET))
    D.gain_project_signal(norder, offs, d_out.ptr, rows, d_sig2.ptr, erows, d_est.ptr, frows, d_flags.ptr, 1, N_SAMP, ivl)
    got = d_out.get()
    d_gram = Dev(np.full((n_det, n_view, norder, norder), -1.0))
    D.gain_precond_build(norder, erows, d_est.ptr, weights, N_SAMP, ivl, d_gram.ptr)
    gram = d_gram.get()
    worst_p = worst_g = 0.0
    for k in range(n_det):
        for v, (first, last) in enumerate(VIEWS):
            basis = legendre_basis(norder, last - first)
            good = (flags[frows[k], first:last] & 1) == 0
            est = est0[erows[k], first:last]
            w = est * sig0[rows[k], first:last]
            for r in range(norder):
                terms = (w * basis[r])[good]
                exact = math.fsum([gc.PRESET] + list(terms))
                worst_p = max(worst_p, abs(got[offs[k] + v * norder + r] - exact) / (EPS * (gc.PRESET + np.abs(terms).sum())))
                for c in range(norder):
                    terms = (basis[r] * est) * (basis[c] * est)      # ALL samples: no flags in the Gram matrix
                    worst_g = max(worst_g, abs(gram[k, v, r, c] / weights[k] - math.fsum(terms)) / (EPS * np.abs(terms).sum()))
    print(f"{norder} terms: project {worst_p:.2f}, Gram {worst_g:.2f} eps sum|terms| from the exact sums "
          f"(bounds {F_PROJECT}, {F_GRAM})")
    assert worst_p <= F_PROJECT and worst_g <= F_GRAM
    assert np.array_equal(gram, gram.transpose(0, 1, 3, 2))
    # the fully flagged view keeps the preset exactly
    v = n_view - 1
    for k in range(n_det):
        assert np.all(got[offs[k] + v * norder:][:norder] == gc.PRESET)
    # without flags every sample counts (flag pointer 0)
    d_out2 = Dev(np.full(amps.size, gc.PRESET))
    D.gain_project_signal(norder, offs, d_out2.ptr, rows, d_sig2.ptr, erows, d_est.ptr, None, 0, 1, N_SAMP, ivl)
    got2 = d_out2.get()
    for k in range(n_det):
        first, last = VIEWS[-1]
        terms = est0[erows[k], first:last] * sig0[rows[k], first:last]       # order 0 of the fully flagged view
        i = offs[k] + v * norder
        assert abs(got2[i] - math.fsum([gc.PRESET] + list(terms))) <= F_PROJECT * EPS * (gc.PRESET + np.abs(terms).sum())
        assert got2[i] != gc.PRESET
    # identical bits in a second run
    d_out.a[:] = gc.PRESET
    d_out3 = Dev(np.full(amps.size, gc.PRESET))
    D.gain_project_signal(norder, offs, d_out3.ptr, rows, d_sig2.ptr, erows, d_est.ptr, frows, d_flags.ptr, 1, N_SAMP, ivl)
    assert np.array_equal(d_out3.get(), got)
    D.gain_precond_build(norder, erows, d_est.ptr, weights, N_SAMP, ivl, d_gram.ptr)
    assert np.array_equal(d_gram.get(), gram)
    for d in (d_sig, d_est, d_amps, d_flags, d_sig2, d_out, d_out2, d_out3, d_gram):
        d.free()


@pytest.mark.parametrize("norder", [1, 2, 9])
def test_both_legendre_templates_run_the_same_arithmetic(norder):
    """C ABI.  SubHarmonic and GainTemplate are two policies of one kernel family, so with an estimate that is exactly 1.0,
    no flags and amplitudes preset to 0.0 GainTemplate's projection and Gram matrices are SubHarmonic's bit for bit:
    ``1.0 * s`` and ``T_k * 1.0`` are exact, both sum the same lane partials through the same butterflies and wave order,
    and both add the chunks in chunk order starting from 0.0.  ``add_to_signal`` is not compared: the two round
    differently there (``s += T_k a_k`` in place against ``s + e * sum``), and each has its own bit-exact test."""
    from toast_amd import capi
    from toast_amd.capi import interval_dtype

    D = capi.dev
    rng = np.random.default_rng(41 + norder)
    n_det, n_view = 3, len(VIEWS)
    ivl = np.zeros(n_view, dtype=interval_dtype)
    ivl["first"], ivl["last"] = [v[0] for v in VIEWS], [v[1] for v in VIEWS]
    sig0 = rng.standard_normal((n_det, N_SAMP))
    est0 = np.ones((n_det + 1, N_SAMP))
    n_amp = n_det * n_view * norder
    offs = (np.array([2, 0, 1]) * n_view * norder).astype(np.int64)
    rows = np.array([1, 2, 0], dtype=np.int32)
    erows = np.array([3, 0, 2], dtype=np.int32)
    weights = np.array([1.0, 0.5, 4.0])
    d_sig, d_est = Dev(sig0), Dev(est0)
    # ---- projection: SubHarmonic assigns (whatever was there), GainTemplate adds onto 0.0
    d_sub, d_gain = Dev(np.full(n_amp, -7.0)), Dev(np.zeros(n_amp))
    D.subharmonic_project_signal(norder, offs, d_sub.ptr, rows, d_sig.ptr, N_SAMP, ivl)
    D.gain_project_signal(norder, offs, d_gain.ptr, rows, d_sig.ptr, erows, d_est.ptr, None, 0, 1, N_SAMP, ivl)
    sub, gain = d_sub.get(), d_gain.get()
    assert np.all(sub != -7.0) and np.all(sub != 0.0)
    assert np.array_equal(gain, sub)
    # ---- Gram matrices: SubHarmonic without flags counts every sample, GainTemplate never counts
    d_gsub, d_ggain = Dev(np.full((n_det, n_view, norder, norder), -1.0)), Dev(np.full((n_det, n_view, norder, norder), -2.0))
    d_ngood = Dev(np.full((n_det, n_view), -1, dtype=np.int64))
    D.subharmonic_precond_build(norder, None, 0, 0, weights, N_SAMP, ivl, d_gsub.ptr, d_ngood.ptr)
    D.gain_precond_build(norder, erows, d_est.ptr, weights, N_SAMP, ivl, d_ggain.ptr)
    gsub, ggain = d_gsub.get(), d_ggain.get()
    assert np.all(gsub[:, :, 0, 0] == weights[:, None] * np.array([last - first for first, last in VIEWS]))
    assert np.array_equal(ggain, gsub)
    assert np.array_equal(d_ngood.get(), np.tile([last - first for first, last in VIEWS], (n_det, 1)))
    assert np.array_equal(d_sig.get(), sig0) and np.array_equal(d_est.get(), est0)
    for d in (d_sig, d_est, d_sub, d_gain, d_gsub, d_ggain, d_ngood):
        d.free()


def test_kernels_refuse_too_many_terms():
    from toast_amd import capi
    from toast_amd.capi import interval_dtype

    D = capi.dev
    n = D.subharmonic_max_terms() + 1
    assert n == 10
    ivl = np.zeros(1, dtype=interval_dtype)
    ivl["first"], ivl["last"] = 0, 100
    rows, offs = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    d_sig, d_est, d_amps = Dev(np.ones((1, 100))), Dev(np.ones((1, 100))), Dev(np.zeros(n))
    d_gram = Dev(np.zeros((1, 1, n, n)))
    with pytest.raises(RuntimeError, match="terms"):
        D.gain_add_to_signal(n, offs, d_amps.ptr, rows, d_sig.ptr, rows, d_est.ptr, 100, ivl)
    with pytest.raises(RuntimeError, match="terms"):
        D.gain_project_signal(n, offs, d_amps.ptr, rows, d_sig.ptr, rows, d_est.ptr, None, 0, 0, 100, ivl)
    with pytest.raises(RuntimeError, match="terms"):
        D.gain_precond_build(n, rows, d_est.ptr, np.ones(1), 100, ivl, d_gram.ptr)
    assert np.all(d_sig.get() == 1.0) and np.all(d_amps.get() == 0.0)
    for d in (d_sig, d_est, d_amps, d_gram):
        d.free()


# ------------------------------------------------------------------ 3. adjointness
def test_adjointness_without_flags():
    """<M a, y> = <a, M^T y> on two observations with ragged views, without flags (with flags the reference's two
    directions use different masks)."""
    from toast_amd.templates import GainTemplate

    data = gc.build("long", first_only=False)
    tmpl = gc.configure(GainTemplate(name="g", order=3, template_name=gc.ESTIMATE), view=tc.VIEW, det_flags=None)
    tmpl.data = data
    dets = tmpl.detectors()
    y = {ob.name: ob.detdata[tc.DET_DATA].data.copy() for ob in data.obs}
    _to_device(data)
    mty = _resident(tmpl, 0.0)
    tmpl.project_signal_multi(dets, mty)
    a = tc.amplitudes(tmpl._n_local, 4)
    for ob in data.obs:
        ob.detdata[tc.DET_DATA].data[:] = 0
    _to_device(data)
    amps = _resident(tmpl, a)
    tmpl.add_to_signal_multi(dets, amps)
    lhs_terms = np.concatenate([(ob.detdata[tc.DET_DATA].data * y[ob.name]).reshape(-1) for ob in data.obs])
    rhs_terms = a * mty.local
    lhs, rhs = math.fsum(lhs_terms), math.fsum(rhs_terms)
    # both sides are sums of n_samp * n_term products rounded once each
    bound = 64 * EPS * (np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum())
    print(f"<Ma, y> = {lhs!r}, <a, M^T y> = {rhs!r}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 1.0
    tmpl.clear()
    for z in (mty, amps):
        z.clear()


# ------------------------------------------------------------------ 4. clear()
def test_clear_releases_what_the_template_registered():
    """``clear()`` leaves nothing of the template on the device -- its preconditioner, the estimate it uploaded -- and a
    second ``_initialize`` gives the same preconditioner bit for bit."""
    from toast_amd.accel import accel_data_present
    from toast_amd.templates import GainTemplate

    data = gc.build("long", first_only=False)
    tmpl = gc.configure(GainTemplate(name="gain", order=2, template_name=gc.ESTIMATE, noise_model=tc.NOISE), view=tc.VIEW)
    tmpl.data = data

    def precond():
        amps, out = _resident(tmpl, tc.amplitudes(tmpl._n_local, 3)), _resident(tmpl, -3.0)
        tmpl.apply_precond(amps, out)
        assert out.accel_in_use()
        result = out.local.copy()
        amps.clear()
        out.clear()
        return result

    first = precond()
    assert np.all(first != -3.0)
    _to_device(data)
    proj = _resident(tmpl, 0.0)
    tmpl.project_signal_multi(tmpl.detectors(), proj)
    proj.clear()
    estimates = [ob.detdata[gc.ESTIMATE] for ob in data.obs]
    assert all(e.accel_exists() for e in estimates)
    mirrors = list(tmpl._mirrors.values())
    assert len(mirrors) == 1
    assert all(m.on_device and accel_data_present(m.buffer, m.name) for m in mirrors)
    tmpl.clear()
    assert not any(m.on_device or m.stale or accel_data_present(m.buffer, m.name) for m in mirrors)
    assert not any(e.accel_exists() or e.accel_in_use() for e in estimates)
    assert tmpl._borrowed == [] and tmpl._created == []
    # an estimate somebody else put on the device is left there
    _to_device(data, keys=(gc.ESTIMATE,))
    tmpl._initialize(data)
    assert np.array_equal(precond(), first)
    tmpl.clear()
    assert all(e.accel_exists() for e in estimates)


# ------------------------------------------------------------------ 5. end to end
def _e2e(host_template):
    from toast_amd import capi, ops
    from toast_amd.data import defaults
    from toast_amd.templates import GainTemplate, Offset

    cls = _host_class() if host_template else GainTemplate
    data, cfg = gc.build_e2e()
    was = capi.get_deterministic()
    capi.set_deterministic(True)
    try:
        dp = ops.PointingDetectorSimple()
        pix = ops.PixelsHealpix(detector_pointing=dp, nside=cfg["nside"], nest=True)
        sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", hwp_angle=defaults.hwp_angle)
        binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=True)
        tm = ops.TemplateMatrix(templates=[
            Offset(step_time=cfg["step_time"], noise_model=defaults.noise_model, name="baselines"),
            cls(order=cfg["order"], template_name=gc.ESTIMATE, noise_model=defaults.noise_model, name="gain")])
        mm = ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=tm, iter_min=cfg["iters"],
                          iter_max=cfg["iters"], convergence=1e-30, keep_solver_products=True)
        mm.apply(data)
    finally:
        capi.set_deterministic(was)
    amps = data["mm_solve_amplitudes"]
    assert list(amps.keys()) == list(gc.E2E_NAMES)
    return {k: amps[k].local.copy() for k in gc.E2E_NAMES}, {k: amps[k].local_flags.copy() for k in gc.E2E_NAMES}, \
        np.array(mm.history), tuple(mm.lhs_route)


def test_mapmaker_over_offset_and_gain_equals_reference_solve():
    want_hist = GOLD["e2e_history"]

    def distance(amps, hist):
        d = {k: float(np.abs(amps[k] - GOLD[f"e2e_amplitudes_{k}"]).max() / np.abs(GOLD[f"e2e_amplitudes_{k}"]).max())
             for k in gc.E2E_NAMES}
        d["history"] = float(np.max(np.abs(hist - want_hist) / want_hist))
        return d

    h_amps, h_flags, h_hist, h_route = _e2e(host_template=True)
    assert len(h_hist) == len(want_hist)
    host = distance(h_amps, h_hist)
    print("E2E host-path template, distance to the reference:", "  ".join(f"{k} {v:.2e}" for k, v in host.items()))
    d_amps, d_flags, d_hist, d_route = _e2e(host_template=False)
    assert d_route == ("sequence",) and h_route == ("sequence",) and len(d_hist) == len(want_hist)
    dev = distance(d_amps, d_hist)
    print("E2E device template, distance to the reference:   ", "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for amps, flags in ((h_amps, h_flags), (d_amps, d_flags)):
        for k in gc.E2E_NAMES:
            assert amps[k].size == GOLD[f"e2e_amplitudes_{k}"].size
            assert np.array_equal(flags[k], GOLD[f"e2e_flags_{k}"]), k
            assert not np.any(amps[k][GOLD[f"e2e_flags_{k}"] != 0]), k
    for k, figure in E2E_HOST_DISTANCE.items():
        assert host[k] <= PARITY and dev[k] <= PARITY, (k, host[k], dev[k])
        assert host[k] <= 10.0 * figure, ("host path", k, host[k], figure)
        assert dev[k] <= 10.0 * figure, ("device", k, dev[k], figure)


# ------------------------------------------------------------------ 6. the workflow
def test_workflow_recovers_an_injected_gain_drift(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "workflows"))
    import sim_satellite_simple as wf

    base = ["--ndet", "4", "--minutes", "5", "--rate", "20", "--nside", "64"]
    data = wf.main(base + ["--noise-free", "--gain-drift", "2"])
    out = capsys.readouterr().out
    print(out)
    amps = data["mapmaker_solve_amplitudes"]
    assert set(amps.keys()) == {"baselines", "gain"}
    hist = np.array(data["gain_drift_history"])
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    injected, recovered = data["gain_drift_injected"], data["gain_drift_recovered"]
    assert injected.shape == recovered.shape == (4, 3)
    # order 0 relative to its mean over the detectors: a common gain is a brighter sky
    diff = recovered - injected
    diff[:, 0] -= diff[:, 0].mean()
    rms = float(np.sqrt(np.mean(injected ** 2)))
    print(f"gain drift: largest error of the recovered amplitudes {np.abs(diff).max():.3e}, rms of the injected ones {rms:.3e}, "
          f"ratio {np.abs(diff).max() / rms:.3e} (bound 1e-3)")
    assert "injected" in out and "recovered" in out
    assert np.abs(diff).max() <= 1e-3 * rms
    # without the flag the keys are what they were: the solver's products are not kept, nothing of the drift is there
    for extra in (["--destripe"], []):
        data = wf.main(base + extra)
        assert "mapmaker_map" in data
        assert not any(k.startswith("gain_drift") or k == "mapmaker_solve_amplitudes" for k in data)
        assert all(wf.GAIN_ESTIMATE not in ob.detdata for ob in data.obs)
