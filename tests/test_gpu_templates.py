"""GPU: the SubHarmonic and Periodic templates (csrc/template_basis.hip) against tests/golden/templates_basis.npz -- the
results of the reference's own methods (tests/golden/make_golden_templates.py) on the inputs of tests/templates_case.py --
through the C ABI and through the classes on device-resident buffers.

Bit-exact on the device: amplitude layout, ``n_local``, SubHarmonic ``add_to_signal``; Periodic bin index, hits, flags,
``add_to_signal``, ``apply_precond``.

The three reductions are taken in another ORDER than NumPy's and are compared under bounds that were measured, not
guessed.  For the fixture's inputs the reference's own results deviate from the exactly summed values (``math.fsum`` of
the rounded products; the Gram matrices and their inverses in exact rational arithmetic) by at most

    SubHarmonic project_signal   0.69 eps sum|signal_i T_k|          (np.dot)
    Gram matrix                  1.99 eps sum|T_r T_c|               (np.dot)
    inverse of the Gram matrix   0.32 eps cond(G) max|G^-1|          (np.linalg.inv)
    Periodic project_signal      3.10 eps sum|terms|                 (np.add.at: one sample after the other)

and the device gets an order of magnitude over those figures for its different summation tree: 6.9, 20 and 31 times
``eps sum|terms|`` per amplitude, and 3.2 ``eps cond(G) max|G^-1|`` for the inverse.  cond(G) reaches 110 at order 8 (64
samples, 30 % flagged).  ``apply_precond`` adds the rounding of a dot product of ``norder`` terms to the error of the
matrix: ``(3.2 cond + norder) eps max|G^-1| sum|a|`` per amplitude.

End to end: ``MapMaker`` over [Offset, SubHarmonic, Periodic] against the amplitudes and the residual history of the
reference's ``solve()`` (the ``e2e_*`` entries of the fixture).  The same solve runs twice in the order-exact mode of the
scatter: with the two templates on their NumPy host path (their ``supports_accel`` answers no, the pipelines run them on
the host) and on the device.  The host path's distance to the reference was measured on an MI355X: 9.1e-15 / 6.6e-15 /
8.4e-15 of the largest amplitude for baselines / subharmonic / ground and 1.4e-14 relative in the history (the sweeps
are the reference's NumPy, the rest of the chain takes its sums in the reference's order; what is left are the 3 x 3
inversions and the dot products of the solve).  BOTH runs are bounded by ten times those figures (``E2E_HOST_DISTANCE``):
the host run so that the solver path itself -- layout across templates, preconditioner, the assigning projection inside
the PCG -- is held to the reference, the device run for its other summation tree.  The test prints all figures before it
asserts.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import templates_case as tc  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "templates_basis.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
F_PROJECT, F_GRAM, F_INVERSE, F_PERIODIC = 6.9, 20.0, 3.2, 31.0
# measured distance of MapMaker with host-path templates to the reference's solve() (see the module docstring)
E2E_HOST_DISTANCE = {"baselines": 9.1e-15, "subharmonic": 6.6e-15, "ground": 8.4e-15, "history": 1.4e-14}


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)     # (its own host key)
        accel_data_create(self.a, "test_templates")
        accel_data_update_device(self.a, "test_templates")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_templates")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_templates")


def _to_device(data, keys=(tc.DET_DATA,)):
    for ob in data.obs:
        for key in keys:
            dd = ob.detdata[key]
            if not dd.accel_exists():
                dd.accel_create(key)
            if not dd.accel_in_use():
                dd.accel_update_device()


def _subharmonic(name):
    from toast_amd.templates import SubHarmonic

    layout, traits = tc.SUBHARMONIC_CASES[name]
    data = tc.build(layout)
    tmpl = tc.configure(SubHarmonic(name=name, **traits))
    tmpl.data = data
    return data, tmpl


def _periodic(name, **extra):
    from toast_amd.templates import Periodic

    layout, traits = tc.PERIODIC_CASES[name]
    data = tc.build(layout)
    tmpl = tc.configure(Periodic(name=name, **{**traits, **extra}))
    tmpl.data = data
    return data, tmpl


def _resident(tmpl, values):
    z = tmpl.zeros()
    z.local[:] = values
    z.accel_resident(f"{tmpl.name}_test")
    return z


def _subharmonic_terms(name):
    """Per amplitude: exact sum of signal_i T_k(r_i) (fsum of the rounded products) and sum of their magnitudes."""
    from toast_amd.templates.subharmonic import legendre_basis

    layout, traits = tc.SUBHARMONIC_CASES[name]
    data = tc.build(layout)
    norder = traits["order"] + 1
    exact, scale = [], []
    for det in ("d0", "d1", "d2"):
        for iob, ob in enumerate(data.obs):
            if det not in ob.local_detectors:
                continue
            for first, last in tc.LAYOUTS[layout]["obs"][iob]["views"]:
                basis = legendre_basis(norder, last - first)
                for k in range(norder):
                    terms = ob.detdata[tc.DET_DATA][det, first:last] * basis[k]
                    exact.append(math.fsum(terms))
                    scale.append(np.abs(terms).sum())
    return np.array(exact), np.array(scale)


@pytest.mark.parametrize("name", list(tc.SUBHARMONIC_CASES))
def test_subharmonic_device_matches_reference(name):
    data, tmpl = _subharmonic(name)
    norder = tmpl.order + 1
    dets = tmpl.detectors()
    assert tmpl._n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal([tmpl._det_start[d] for d in dets], GOLD[f"{name}_det_start"])
    # preconditioner: Gram matrices from the device, inverted on the host
    ref = GOLD[f"{name}_precond"]
    worst = 0.0
    for blk in range(ref.shape[0]):
        cond = np.linalg.cond(ref[blk])
        err = np.abs(tmpl._precond[blk] - ref[blk]).max() / (EPS * cond * np.abs(ref[blk]).max())
        worst = max(worst, err)
    print(f"{name}: inverse Gram, worst deviation {worst:.2f} eps cond max|G^-1| (bound {F_INVERSE})")
    assert worst <= F_INVERSE
    _to_device(data)
    # M^T d: assigned, no flags; twice for the bits
    exact, scale = _subharmonic_terms(name)
    proj = _resident(tmpl, 123.0)
    tmpl.project_signal_multi(dets, proj)
    first = proj.local.copy()
    err = np.abs(first - GOLD[f"{name}_project"]) / (EPS * scale)
    print(f"{name}: project_signal, worst deviation from the fixture {err.max():.2f} eps sum|terms| (bound {F_PROJECT}); "
          f"from the exact sums {(np.abs(first - exact) / (EPS * scale)).max():.2f}")
    assert np.all(err <= F_PROJECT)
    again = _resident(tmpl, -7.0)
    tmpl.project_signal_multi(dets, again)
    assert np.array_equal(again.local, first)
    # d + M a: bit for bit
    amps = _resident(tmpl, tc.amplitudes(tmpl._n_local, 1))
    tmpl.add_to_signal_multi(dets, amps)
    for iob, ob in enumerate(data.obs):
        assert np.array_equal(ob.detdata[tc.DET_DATA].data, GOLD[f"{name}_add_obs{iob}"]), (name, iob)
    # preconditioner applied to resident vectors
    out = _resident(tmpl, 0.0)
    tmpl.apply_precond(amps, out)
    assert out.accel_in_use()
    bound = EPS * np.array([(F_INVERSE * np.linalg.cond(p) + norder) * np.abs(p).max() for p in ref]).repeat(norder) * \
        np.abs(amps.local).reshape(-1, norder).sum(axis=1).repeat(norder)
    assert np.all(np.abs(out.local - GOLD[f"{name}_precond_out"]) <= bound)
    tmpl.clear()
    for z in (proj, again, amps, out):
        z.clear()


def test_subharmonic_kernels_short_views_and_gram():
    """C ABI: views of one and two samples at order 8 (np.linspace's special cases), an unaligned row, a view of more
    than one reduction chunk; the Gram matrix against exactly summed products; two runs, identical bits."""
    from toast_amd import capi
    from toast_amd.capi import interval_dtype
    from toast_amd.templates.subharmonic import legendre_basis

    D = capi.dev
    rng = np.random.default_rng(11)
    n_det, n_samp, norder = 3, 9001, 9
    views = [(0, 1), (3, 5), (6, 9), (11, 8500), (8501, 9001)]
    ivl = np.zeros(len(views), dtype=interval_dtype)
    ivl["first"], ivl["last"] = [v[0] for v in views], [v[1] for v in views]
    sig0 = rng.standard_normal((n_det, n_samp))
    flags = (rng.random((n_det, n_samp)) < 0.3).astype(np.uint8) | 2
    for first, last in views[:3]:
        flags[:, first:last] = 2
    amps = rng.standard_normal(n_det * len(views) * norder)
    offs = (np.array([2, 0, 1]) * len(views) * norder).astype(np.int64)     # blocks in another order than the rows
    rows = np.array([1, 2, 0], dtype=np.int32)
    d_sig, d_amps, d_flags = Dev(sig0), Dev(amps), Dev(flags)
    D.subharmonic_add_to_signal(norder, offs, d_amps.ptr, rows, d_sig.ptr, n_samp, ivl)
    want = sig0.copy()
    for k, row in enumerate(rows):
        for v, (first, last) in enumerate(views):
            basis = legendre_basis(norder, last - first)
            a = amps[offs[k] + v * norder:][:norder]
            for order in range(norder):
                want[row, first:last] += basis[order] * a[order]
    assert np.array_equal(d_sig.get(), want)
    # projection of the seeded signal, and the Gram matrices
    d_sig2, d_out = Dev(sig0), Dev(np.full(amps.size, 9.0))
    D.subharmonic_project_signal(norder, offs, d_out.ptr, rows, d_sig2.ptr, n_samp, ivl)
    got = d_out.get()
    d_gram = Dev(np.zeros((n_det, len(views), norder, norder)))
    d_ngood = Dev(np.zeros((n_det, len(views)), dtype=np.int64))
    weights = np.array([1.0, 0.5, 3.0])
    D.subharmonic_precond_build(norder, rows, d_flags.ptr, 1, weights, n_samp, ivl, d_gram.ptr, d_ngood.ptr)
    gram, ngood = d_gram.get(), d_ngood.get()
    worst_p = worst_g = 0.0
    for k, row in enumerate(rows):
        for v, (first, last) in enumerate(views):
            basis = legendre_basis(norder, last - first)
            good = (flags[row, first:last] & 1) == 0
            assert ngood[k, v] == np.count_nonzero(good)
            for r in range(norder):
                terms = sig0[row, first:last] * basis[r]
                worst_p = max(worst_p, abs(got[offs[k] + v * norder + r] - math.fsum(terms)) / (EPS * np.abs(terms).sum()))
                for c in range(norder):
                    terms = basis[r][good] * basis[c][good]
                    worst_g = max(worst_g, abs(gram[k, v, r, c] / weights[k] - math.fsum(terms)) / (EPS * np.abs(terms).sum()))
    print(f"order 8 kernels: project {worst_p:.2f}, Gram {worst_g:.2f} eps sum|terms| from the exact sums "
          f"(bounds {F_PROJECT}, {F_GRAM})")
    assert worst_p <= F_PROJECT and worst_g <= F_GRAM
    assert np.array_equal(gram, gram.transpose(0, 1, 3, 2))
    # identical bits in a second run
    d_out.a[:] = 0
    D.subharmonic_project_signal(norder, offs, d_out.ptr, rows, d_sig2.ptr, n_samp, ivl)
    assert np.array_equal(d_out.get(), got)
    D.subharmonic_precond_build(norder, rows, d_flags.ptr, 1, weights, n_samp, ivl, d_gram.ptr, d_ngood.ptr)
    assert np.array_equal(d_gram.get(), gram)
    with pytest.raises(RuntimeError, match="terms"):
        D.subharmonic_add_to_signal(D.subharmonic_max_terms() + 1, offs, d_amps.ptr, rows, d_sig.ptr, n_samp, ivl)
    for d in (d_sig, d_amps, d_flags, d_sig2, d_out, d_gram, d_ngood):
        d.free()


def test_subharmonic_view_without_good_sample_raises_on_device():
    from toast_amd.templates import SubHarmonic

    data = tc.build("long")
    first, last = tc.LAYOUTS["long"]["obs"][0]["views"][2]
    data.obs[0].detdata[tc.DET_FLAGS].data[1, first:last] |= tc.DET_FLAG_MASK
    with pytest.raises(np.linalg.LinAlgError, match="detector d1, observation obs0, view 2 has no unflagged sample"):
        tc.configure(SubHarmonic(name="s", order=2)).data = data


def _periodic_terms(name):
    layout, _ = tc.PERIODIC_CASES[name]
    data = tc.build(layout)
    exact, scale = [], []
    for det in ("d0", "d1", "d2"):
        for iob, ob in enumerate(data.obs):
            if det not in ob.local_detectors:
                continue
            index = GOLD[f"{name}_index_obs{iob}"]
            good = (index >= 0) & ((ob.detdata[tc.DET_FLAGS][det] & tc.DET_FLAG_MASK) == 0)
            for b in range(int(GOLD[f"{name}_obs_nbins"][iob])):
                terms = np.concatenate([[0.5], ob.detdata[tc.DET_DATA][det][good & (index == b)]])
                exact.append(math.fsum(terms))
                scale.append(np.abs(terms).sum())
    return np.array(exact), np.array(scale)


@pytest.mark.parametrize("name", list(tc.PERIODIC_CASES))
def test_periodic_device_matches_reference(name):
    from toast_amd import capi

    data, tmpl = _periodic(name)
    dets = tmpl.detectors()
    assert tmpl._n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal([tmpl._det_start[d] for d in dets], GOLD[f"{name}_det_offset"])
    assert np.array_equal([tmpl._obs_nbins[i] for i in range(len(data.obs))], GOLD[f"{name}_obs_nbins"])
    # hits and flags were counted on the device; the index rows were computed there
    assert tmpl._mirrors["hits"].on_device
    assert np.array_equal(tmpl._amp_hits, GOLD[f"{name}_hits"])
    assert np.array_equal(tmpl._amp_flags.astype(np.uint8), GOLD[f"{name}_flags"])
    assert np.any(tmpl._amp_flags & (tmpl._amp_hits >= tmpl.minimum_bin_hits))
    for iob, ob in enumerate(data.obs):
        assert tmpl._index[iob].on_device and tmpl._index[iob].stale
        assert np.array_equal(tmpl._host_index(iob, ob)[0], GOLD[f"{name}_index_obs{iob}"])
        assert not tmpl._index[iob].stale
    _to_device(data)
    exact, scale = _periodic_terms(name)
    results = {}
    for label, path in (("lds", capi.dev.PERIODIC_PATH_LDS), ("atomic", capi.dev.PERIODIC_PATH_ATOMIC)):
        proj = _resident(tmpl, 0.5)
        tmpl.project_signal_multi(dets, proj, path=path)
        results[label] = proj.local.copy()
        err = np.abs(results[label] - GOLD[f"{name}_project"]) / (EPS * scale)
        print(f"{name}: project_signal ({label}), worst deviation from the fixture {err.max():.2f} eps sum|terms| "
              f"(bound {F_PERIODIC}); from the exact sums {(np.abs(results[label] - exact) / (EPS * scale)).max():.2f}")
        assert np.all(err <= F_PERIODIC)
        proj.clear()
    again = _resident(tmpl, 0.5)
    tmpl.project_signal_multi(dets, again)          # by the rule: the order-deterministic LDS form
    assert np.array_equal(again.local, results["lds"])
    amps = _resident(tmpl, tc.amplitudes(tmpl._n_local, 2))
    tmpl.add_to_signal_multi(dets, amps)
    for iob, ob in enumerate(data.obs):
        assert np.array_equal(ob.detdata[tc.DET_DATA].data, GOLD[f"{name}_add_obs{iob}"]), (name, iob)
    out = _resident(tmpl, -3.0)
    tmpl.apply_precond(amps, out)
    assert out.accel_in_use()
    assert np.array_equal(out.local, GOLD[f"{name}_precond_out"])
    tmpl.clear()
    for z in (again, amps, out):
        z.clear()


@pytest.mark.parametrize("sequence", ["written_on_device", "uploaded_then_dropped", "never_registered"])
def test_device_mirror(sequence):
    """The coherence states of ``DeviceMirror`` on eight float64 values."""
    from toast_amd import capi
    from toast_amd.accel import accel_data_present
    from toast_amd.templates import DeviceMirror

    values = np.arange(8, dtype=np.float64) + 1.0
    if sequence == "written_on_device":
        mirror, x = DeviceMirror(np.full(8, 9.0), "test_mirror").create(zero_out=True), Dev(values)
        assert mirror.on_device and not mirror.stale
        capi.dev.vec_axpby(8, 2.0, x.ptr, 1.0, mirror.ptr)       # 2 x onto the zeros (toast_hip_vec_axpby_dev)
        mirror.written()
        assert mirror.stale and np.array_equal(mirror.buffer, np.full(8, 9.0))
        assert np.array_equal(mirror.host, 2.0 * values) and not mirror.stale
        mirror.buffer[0] = -1.0
        assert mirror.host[0] == -1.0                            # (a second fetch would bring the 2 back)
        x.free()
        mirror.drop()
    elif sequence == "uploaded_then_dropped":
        mirror, y = DeviceMirror(values.copy(), "test_mirror"), Dev(np.zeros(8))
        assert mirror.upload() is mirror and mirror.on_device and not mirror.stale
        assert accel_data_present(mirror.buffer, mirror.name)
        capi.dev.vec_axpby(8, 1.0, mirror.upload().ptr, 0.0, y.ptr)
        assert np.array_equal(y.get(), values)
        y.free()
        mirror.drop()
        assert np.array_equal(mirror.host, values)
    else:
        mirror = DeviceMirror(values.copy(), "test_mirror")
        mirror.drop()
        assert np.array_equal(mirror.host, values)
    assert not mirror.on_device and not mirror.stale and not accel_data_present(mirror.buffer, mirror.name)


@pytest.mark.parametrize("kind", ["offset", "subharmonic", "periodic"])
def test_clear_releases_what_the_template_registered(kind):
    """``clear()`` leaves nothing of the template on the device, and a second ``_initialize`` gives the same
    preconditioner bit for bit (Fourier2D: test_gpu_fourier2d.py, through ``device_tables()``)."""
    from toast_amd.accel import accel_data_present
    from toast_amd.templates import Offset, Periodic, SubHarmonic

    data = tc.build("tiny")
    tmpl = {"offset": lambda: Offset(name="off", step_time=5.0, noise_model=tc.NOISE),
            "subharmonic": lambda: SubHarmonic(name="sub", **tc.SUBHARMONIC_CASES["sub0"][1]),
            "periodic": lambda: Periodic(name="per", **tc.PERIODIC_CASES["per_bins"][1])}[kind]()
    tc.configure(tmpl).data = data

    def precond():
        amps, out = _resident(tmpl, tc.amplitudes(tmpl._n_local, 3)), _resident(tmpl, -3.0)
        tmpl.apply_precond(amps, out)
        assert out.accel_in_use()
        result = out.local.copy()
        amps.clear()
        out.clear()
        return result

    first = precond()
    assert np.any(first != -3.0)
    mirrors = list(tmpl._mirrors.values()) + list(getattr(tmpl, "_index", {}).values())
    assert len(mirrors) == (3 if kind == "periodic" else 1)
    assert all(m.on_device and accel_data_present(m.buffer, m.name) for m in mirrors)
    tmpl.clear()
    assert not any(m.on_device or m.stale or accel_data_present(m.buffer, m.name) for m in mirrors)
    tmpl._initialize(data)
    assert np.array_equal(precond(), first)
    tmpl.clear()


def test_periodic_per_detector_key_device_equals_host_path():
    from toast_amd.templates import Periodic

    def build():
        data = tc.build("tiny")
        for iob, ob in enumerate(data.obs):
            ob.detdata.create("det_az", dtype=np.float64)
            ob.detdata.create("det_az_flags", dtype=np.uint8)
            rng = np.random.default_rng(90 + iob)
            ob.detdata["det_az"].data[:] = ob.shared[tc.KEY].data[None, :] + 3.0 * np.arange(len(ob.local_detectors))[:, None]
            ob.detdata["det_az_flags"].data[:] = (rng.random(ob.detdata["det_az"].data.shape) < 0.1) * tc.KEY_FLAG_MASK
        tmpl = tc.configure(Periodic(name="p", key="det_az", flags="det_az_flags", flag_mask=tc.KEY_FLAG_MASK,
                                     is_detdata_key=True, bins=6))
        return data, tmpl

    data_h, host = build()
    host.data = data_h
    hits_dev, flags_dev = host._amp_hits.copy(), host._amp_flags.copy()
    host.clear()
    host._amp_hits[:] = 0
    host._amp_flags[:] = False
    host._init_hits_host(data_h)
    assert np.array_equal(hits_dev, host._amp_hits) and np.array_equal(flags_dev, host._amp_flags)
    data_d, dev = build()
    dev.data = data_d
    for iob, ob in enumerate(data_d.obs):
        assert np.array_equal(dev._host_index(iob, ob), host._host_index(iob, data_h.obs[iob]))
    _to_device(data_d)
    values = tc.amplitudes(dev._n_local, 3)
    a_h = host.zeros()
    a_h.local[:] = values
    for det in host.detectors():
        host.add_to_signal(det, a_h)
    a_d = _resident(dev, values)
    dev.add_to_signal_multi(dev.detectors(), a_d)
    for ob_h, ob_d in zip(data_h.obs, data_d.obs):
        assert np.array_equal(ob_h.detdata[tc.DET_DATA].data, ob_d.detdata[tc.DET_DATA].data)
    p_h = host.zeros()
    for det in host.detectors():
        host.project_signal(det, p_h)
    _to_device(data_d)
    p_d = _resident(dev, 0.0)
    dev.project_signal_multi(dev.detectors(), p_d)
    # sum of the magnitudes of the terms of every amplitude: the host path over |signal|
    data_a, mag = build()
    for ob in data_a.obs:
        ob.detdata[tc.DET_DATA].data[:] = np.abs(ob.detdata[tc.DET_DATA].data)
    mag.data = data_a
    scale = mag.zeros()
    for det in mag.detectors():
        mag._project_signal(det, scale, use_accel=False)
    assert np.all(np.abs(p_d.local - p_h.local) <= F_PERIODIC * EPS * scale.local)
    assert np.any(p_h.local != 0)


def test_adjointness_without_flags():
    """<M a, y> = <a, M^T y> for both templates on inputs without flags (with flags the reference's two directions use
    different masks)."""
    from toast_amd.templates import Periodic, SubHarmonic

    for make in (lambda: SubHarmonic(name="s", order=3), lambda: Periodic(name="p", key=tc.KEY, bins=9, minimum_bin_hits=0)):
        data = tc.build("long")
        tmpl = tc.configure(make(), det_flags=None)
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
        print(f"{tmpl.name}: <Ma, y> = {lhs!r}, <a, M^T y> = {rhs!r}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound and abs(lhs) > 1.0
        tmpl.clear()


def _mapmaker(templates, n_det=4, n_samp=6000, use_templates_accel=True):
    from toast_amd import ops
    from toast_amd.data import defaults
    from toast_amd.sim import create_ground_data

    data = create_ground_data(n_det=n_det, n_samp=n_samp, rate=20.0, az_min_deg=40.0, az_max_deg=70.0, scan_rate_deg_s=1.0,
                              fov_deg=4.0, seed=5)
    rng = np.random.default_rng(3)
    for ob in data.obs:
        az = ob.shared[defaults.azimuth].data
        sig = ob.detdata[defaults.det_data].data
        for d in range(sig.shape[0]):
            sig[d] = rng.standard_normal(sig.shape[1]) + 5.0 * np.sin(az / 7.0) + 0.002 * np.arange(sig.shape[1])
    dp = ops.PointingDetectorSimple()
    pix = ops.PixelsHealpix(detector_pointing=dp, nside=64, nest=True, view=defaults.scanning_interval)
    sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", view=defaults.scanning_interval)
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=True)
    tm = ops.TemplateMatrix(templates=templates, view=defaults.scanning_interval)
    mm = ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=tm, iter_min=8, iter_max=8,
                      convergence=1e-30, keep_solver_products=True)
    mm.apply(data)
    return data, mm


def _e2e(host_templates, deterministic=True):
    from toast_amd import capi, ops
    from toast_amd.data import defaults
    from toast_amd.templates import Offset, Periodic, SubHarmonic

    class HostSubHarmonic(SubHarmonic):
        def supports_accel(self):
            return False

    class HostPeriodic(Periodic):
        def supports_accel(self):
            return False

    sub_cls, per_cls = (HostSubHarmonic, HostPeriodic) if host_templates else (SubHarmonic, Periodic)
    data, cfg = tc.build_e2e()
    was = capi.get_deterministic()
    capi.set_deterministic(deterministic)
    try:
        dp = ops.PointingDetectorSimple()
        pix = ops.PixelsHealpix(detector_pointing=dp, nside=cfg["nside"], nest=True)
        sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", hwp_angle=defaults.hwp_angle)
        binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=True)
        tm = ops.TemplateMatrix(templates=[
            Offset(step_time=cfg["step_time"], noise_model=defaults.noise_model, name="baselines"),
            sub_cls(order=cfg["order"], noise_model=defaults.noise_model, name="subharmonic"),
            per_cls(key=tc.KEY, bins=cfg["bins"], minimum_bin_hits=cfg["minimum_bin_hits"], name="ground")])
        mm = ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=tm, iter_min=cfg["iters"],
                          iter_max=cfg["iters"], convergence=1e-30, keep_solver_products=True)
        mm.apply(data)
    finally:
        capi.set_deterministic(was)
    amps = data["mm_solve_amplitudes"]
    assert list(amps.keys()) == list(tc.E2E_NAMES)
    return {k: amps[k].local.copy() for k in tc.E2E_NAMES}, {k: amps[k].local_flags.copy() for k in tc.E2E_NAMES}, \
        np.array(mm.history), tuple(mm.lhs_route)


def test_mapmaker_over_three_templates_equals_reference_solve():
    want_hist = GOLD["e2e_history"]

    def distance(amps, hist):
        d = {k: float(np.abs(amps[k] - GOLD[f"e2e_amplitudes_{k}"]).max() / np.abs(GOLD[f"e2e_amplitudes_{k}"]).max())
             for k in tc.E2E_NAMES}
        d["history"] = float(np.max(np.abs(hist - want_hist) / want_hist))
        return d

    h_amps, h_flags, h_hist, h_route = _e2e(host_templates=True)
    assert len(h_hist) == len(want_hist)
    host = distance(h_amps, h_hist)
    print("E2E host-path templates, distance to the reference:", "  ".join(f"{k} {v:.2e}" for k, v in host.items()))
    d_amps, d_flags, d_hist, d_route = _e2e(host_templates=False)
    assert d_route == ("sequence",) and len(d_hist) == len(want_hist)
    dev = distance(d_amps, d_hist)
    print("E2E device templates, distance to the reference:   ", "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for amps, flags in ((h_amps, h_flags), (d_amps, d_flags)):
        for k in tc.E2E_NAMES:
            assert amps[k].size == GOLD[f"e2e_amplitudes_{k}"].size
            assert np.array_equal(flags[k], GOLD[f"e2e_flags_{k}"]), k
            assert not np.any(amps[k][GOLD[f"e2e_flags_{k}"] != 0]), k
    for k, figure in E2E_HOST_DISTANCE.items():
        assert host[k] <= 10.0 * figure, ("host path", k, host[k], figure)
        assert dev[k] <= 10.0 * figure, ("device", k, dev[k], figure)


def test_mapmaker_over_three_templates_runs_the_sequence():
    from toast_amd.data import defaults
    from toast_amd.templates import Offset, Periodic, SubHarmonic

    data, mm = _mapmaker([Offset(step_time=10.0, noise_model=defaults.noise_model, name="baselines"),
                          SubHarmonic(order=2, noise_model=defaults.noise_model, name="subharmonic"),
                          Periodic(key=defaults.azimuth, bins=12, name="ground")])
    assert mm.lhs_route == ("sequence",)
    amps = data["mm_solve_amplitudes"]
    assert set(amps.keys()) == {"baselines", "subharmonic", "ground"}
    for v in amps.values():
        assert np.all(np.isfinite(v.local)) and np.any(v.local != 0)
    hist = np.array(mm.history)
    print("residual history over [Offset, SubHarmonic, Periodic]:", hist)
    assert np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    assert np.all(np.isfinite(data["mm_map"].data))


def test_mapmaker_with_one_offset_still_takes_the_fused_path():
    from toast_amd.data import defaults
    from toast_amd.templates import Offset

    _, mm = _mapmaker([Offset(step_time=10.0, noise_model=defaults.noise_model, name="baselines")])
    assert len(mm.lhs_route) > 0 and all(r in ("packed", "fused") for r in mm.lhs_route)


def test_workflow_with_both_template_flags(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "workflows"))
    import ground_filter_mapmaker as wf

    data = wf.main(["--ndet", "4", "--minutes", "5", "--rate", "20", "--nside", "64", "--iter", "4", "--subharmonic", "2",
                    "--periodic-az", "16"])
    out = capsys.readouterr().out
    assert "relative residual" in out
    assert set(data["mapmaker_solve_amplitudes"].keys()) == {"baselines", "subharmonic", "ground"}
    # with neither flag the template list is the one Offset it always was
    data = wf.main(["--ndet", "4", "--minutes", "5", "--rate", "20", "--nside", "64", "--iter", "2"])
    assert set(data["mapmaker_solve_amplitudes"].keys()) == {"baselines"}
