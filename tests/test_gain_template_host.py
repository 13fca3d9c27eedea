"""Host path of ``toast_amd.templates.GainTemplate`` against tests/golden/gain_template.npz -- the results of the
reference's own methods (tests/golden/make_golden_gain_template.py) on the inputs of tests/gain_template_case.py -- and,
beyond what the reference can pin (two observations, ragged views), against plain NumPy loops written here.

Bounds.  For the fixture's inputs the reference's own results deviate from exactly summed values (basis from the
three-term recurrence; see the generator's docstring for the three definitions) by at most

    project_signal   1.32 eps (PRESET + sum|terms|)           per case 0.51 1.32 0.37 0.98 0.42 0.98
    inverse Gram     0.63 eps cond(G) max|G^-1|               per case 0.63 0.63 0.28 0.28 0.11 0.13, cond up to 21.4
    add_to_signal    8.33 eps (|s| + |est| sum|T_k a_k|)      per case 0.89 1.22 6.30 6.30 8.33 8.33

and this implementation gets an order of magnitude over those figures (the rule of tests/test_gpu_templates.py): 13.2,
6.3 and 83.3.  ``apply_precond`` adds the rounding of a dot product of ``norder`` terms to the error of the matrix:
``(6.3 cond + norder) eps max|G^-1| sum|a|`` per amplitude.  ``add_to_signal`` is bit-identical to the reference up to
order 1, where the recurrence and the reference's monomials are the same basis.
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

GOLD = np.load(os.path.join(HERE, "golden", "gain_template.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
F_PROJECT, F_INVERSE, F_ADD = 13.2, 6.3, 83.3


def make(name, cls=None):
    from toast_amd.templates import GainTemplate

    traits, det_flags = gc.template_traits(name)
    data = gc.build()
    tmpl = gc.configure((cls or GainTemplate)(name=name, **traits), det_flags=det_flags)
    tmpl.data = data
    return data, tmpl


def add_scale(data, tmpl, amps):
    """|s| + |est| sum_k |T_k a_k| per sample of the fixture's one observation, before the add."""
    from toast_amd.templates.subharmonic import legendre_basis

    ob = data.obs[0]
    norder = tmpl.order + 1
    basis = legendre_basis(norder, ob.n_local_samples)
    mag = np.abs(basis[None, :, :] * amps.reshape(-1, norder)[:, :, None]).sum(axis=1)
    return np.abs(ob.detdata[tc.DET_DATA].data) + np.abs(ob.detdata[gc.ESTIMATE].data) * mag


def precond_out_bound(ref_precond, amps, norder):
    per_block = np.array([(F_INVERSE * np.linalg.cond(p) + norder) * np.abs(p).max() for p in ref_precond])
    return EPS * per_block.repeat(norder) * np.abs(amps).reshape(-1, norder).sum(axis=1).repeat(norder)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_host_path_matches_reference(name):
    data, tmpl = make(name)
    norder = tmpl.order + 1
    dets = tmpl.detectors()
    assert tmpl._n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal([tmpl._det_start[d] for d in dets], GOLD[f"{name}_det_start"])
    ref = GOLD[f"{name}_precond"]
    assert tmpl._precond.shape == ref.shape
    worst = max(np.abs(tmpl._precond[b] - ref[b]).max() / (EPS * np.linalg.cond(ref[b]) * np.abs(ref[b]).max())
                for b in range(ref.shape[0]))
    print(f"{name}: inverse Gram, worst deviation {worst:.2f} eps cond max|G^-1| (bound {F_INVERSE})")
    assert worst <= F_INVERSE
    # M^T d onto the preset amplitudes, with the flags
    proj = tmpl.zeros()
    proj.local[:] = gc.PRESET
    for det in dets:
        tmpl.project_signal(det, proj)
    err = np.abs(proj.local - GOLD[f"{name}_project"]) / (EPS * GOLD[f"{name}_project_scale"])
    print(f"{name}: project_signal, worst deviation from the fixture {err.max():.2f} eps sum|terms| (bound {F_PROJECT})")
    assert np.all(err <= F_PROJECT)
    assert np.all(np.abs(proj.local - gc.PRESET) > 1.0)
    # d + M a
    amps = tmpl.zeros()
    amps.local[:] = tc.amplitudes(tmpl._n_local, 1)
    scale = add_scale(data, tmpl, amps.local)
    for det in dets:
        tmpl.add_to_signal(det, amps)
    got, want = data.obs[0].detdata[tc.DET_DATA].data, GOLD[f"{name}_add_obs0"]
    err = np.abs(got - want) / (EPS * scale)
    print(f"{name}: add_to_signal, worst deviation from the fixture {err.max():.2f} eps (|s| + |est| sum|T a|) (bound {F_ADD})")
    if tmpl.order <= 1:
        assert np.array_equal(got, want)
    else:
        assert np.all(err <= F_ADD)
    out = tmpl.zeros()
    tmpl.apply_precond(amps, out)
    assert np.all(np.abs(out.local - GOLD[f"{name}_precond_out"]) <= precond_out_bound(ref, amps.local, norder))
    tmpl.clear()


def test_gram_matrix_ignores_the_flags():
    """The reference's preconditioner sums over ALL samples: the same template without solver flags has the same one."""
    _, with_flags = make("g4")
    from toast_amd.templates import GainTemplate

    data = gc.build()
    traits, _ = gc.template_traits("g4")
    plain = gc.configure(GainTemplate(name="plain", **traits), det_flags=None)
    plain.data = data
    assert np.array_equal(with_flags._precond, plain._precond)


def _two_observations(order):
    from toast_amd.templates import GainTemplate

    data = gc.build("long", first_only=False)
    tmpl = gc.configure(GainTemplate(name="two", order=order, template_name=gc.ESTIMATE, noise_model=tc.NOISE), view=tc.VIEW)
    tmpl.data = data
    return data, tmpl


def test_two_observations_and_ragged_views_are_consistent():
    """Layout, both sweeps and ``apply_precond`` mean the same amplitudes: detector-major, then observation, then view,
    the offset advancing in every method, the estimate sliced to the view.  Checked against a plain loop."""
    from toast_amd.templates.subharmonic import legendre_basis

    order = 3
    norder = order + 1
    data, tmpl = _two_observations(order)
    cfg = tc.LAYOUTS["long"]["obs"]
    # layout: d0 and d2 live in both observations (3 + 2 views), d1 in the first only
    assert tmpl._det_start == {"d0": 0, "d1": 5 * norder, "d2": 8 * norder} and tmpl._n_local == 13 * norder
    a = tc.amplitudes(tmpl._n_local, 5)
    sig0 = [ob.detdata[tc.DET_DATA].data.copy() for ob in data.obs]
    want_sig = [s.copy() for s in sig0]
    want_proj, scale_proj, want_prec = np.zeros(a.size), np.zeros(a.size), np.zeros(a.size)
    off = 0
    for det in ("d0", "d1", "d2"):
        for iob, ob in enumerate(data.obs):
            if det not in cfg[iob]["dets"]:
                continue
            row = list(cfg[iob]["dets"]).index(det)
            weight = ob[tc.NOISE].detector_weight(det)
            for first, last in cfg[iob]["views"]:
                basis = legendre_basis(norder, last - first)
                est = ob.detdata[gc.ESTIMATE].data[row, first:last]
                gain = np.zeros(last - first)
                for k in range(norder):
                    gain += basis[k] * a[off + k]
                want_sig[iob][row, first:last] += est * gain
                good = (ob.detdata[tc.DET_FLAGS].data[row, first:last] & tc.DET_FLAG_MASK) == 0
                gram = np.zeros((norder, norder))
                for r in range(norder):
                    terms = (est * sig0[iob][row, first:last] * basis[r])[good]
                    want_proj[off + r] = math.fsum([gc.PRESET] + list(terms))
                    scale_proj[off + r] = gc.PRESET + np.abs(terms).sum()
                    for c in range(norder):
                        gram[r, c] = weight * math.fsum((basis[r] * est) * (basis[c] * est))
                want_prec[off:off + norder] = np.linalg.solve(gram, a[off:off + norder])
                off += norder
    assert off == tmpl._n_local
    proj = tmpl.zeros()
    proj.local[:] = gc.PRESET
    for det in tmpl.detectors():
        tmpl.project_signal(det, proj)
    # two roundings per term and a summation tree of at most 4100 terms: (2 + log2(4100)) eps sum|terms| < 16 eps sum|terms|
    assert np.all(np.abs(proj.local - want_proj) <= 16 * EPS * scale_proj)
    amps = tmpl.zeros()
    amps.local[:] = a
    for det in tmpl.detectors():
        tmpl.add_to_signal(det, amps)
    for iob, ob in enumerate(data.obs):
        assert np.array_equal(ob.detdata[tc.DET_DATA].data, want_sig[iob]), iob
        assert np.any(want_sig[iob] != sig0[iob])
    out = tmpl.zeros()
    tmpl.apply_precond(amps, out)
    # a solve against an explicit inverse: both within a few eps cond(G) of the true solution; cond < 100 at order 3
    assert np.all(np.abs(out.local - want_prec) <= 1e-12 * np.abs(want_prec).reshape(-1, norder).max(axis=1).repeat(norder))
    # the second observation's amplitudes are used: changing one of them changes only that observation's signal
    for ob, s in zip(data.obs, sig0):
        ob.detdata[tc.DET_DATA].data[:] = s
    amps.local[:] = 0.0
    amps.local[tmpl._det_start["d0"] + 3 * norder] = 1.0      # d0, observation 1, view 0, order 0
    tmpl.add_to_signal("d0", amps)
    assert np.array_equal(data.obs[0].detdata[tc.DET_DATA].data, sig0[0])
    first, last = cfg[1]["views"][0]
    changed = data.obs[1].detdata[tc.DET_DATA].data != sig0[1]
    assert changed[0, first:last].all() and changed.sum() == last - first
    tmpl.clear()


def test_singular_blocks_raise_with_names():
    from toast_amd.templates import GainTemplate

    data = gc.build("long", first_only=False)
    data.obs[1].detdata[gc.ESTIMATE].data[1, 560:1160] = 0.0      # d2 is row 1 of the second observation
    tmpl = gc.configure(GainTemplate(name="g", order=2, template_name=gc.ESTIMATE), view=tc.VIEW)
    with pytest.raises(np.linalg.LinAlgError, match="detector d2, observation obs1, view 1 has a signal estimate that is zero"):
        tmpl.data = data
    # a view of two samples cannot carry three terms
    data = gc.build("short", first_only=False)
    tmpl = gc.configure(GainTemplate(name="g", order=2, template_name=gc.ESTIMATE), view=tc.VIEW)
    with pytest.raises(np.linalg.LinAlgError, match="detector d0, observation obs0, view 1 has 2 samples for 3 terms"):
        tmpl.data = data
    # ... and does at order 1
    tmpl = gc.configure(GainTemplate(name="g", order=1, template_name=gc.ESTIMATE), view=tc.VIEW)
    tmpl.data = gc.build("short", first_only=False)
    assert np.all(np.isfinite(tmpl._precond))


def test_set_up_errors():
    from toast_amd.templates import GainTemplate

    data = gc.build()
    with pytest.raises(RuntimeError, match="template_name"):
        gc.configure(GainTemplate(name="g", order=1)).data = data
    with pytest.raises(RuntimeError, match="observation obs0 has no detdata 'nowhere'"):
        gc.configure(GainTemplate(name="g", order=1, template_name="nowhere")).data = data
    data.obs[0].detdata.create("est32", dtype=np.float32)
    with pytest.raises(RuntimeError, match="float64"):
        gc.configure(GainTemplate(name="g", order=1, template_name="est32")).data = data
    data = gc.build()
    data.obs[0].detdata.create("sig32", dtype=np.float32)
    tmpl = gc.configure(GainTemplate(name="g", order=1, template_name=gc.ESTIMATE))
    tmpl.det_data = "sig32"
    with pytest.raises(RuntimeError, match="float64"):
        tmpl.data = data


def test_detectors_need_an_estimate():
    """Only detectors present in ``template_name`` take part."""
    from toast_amd.templates import GainTemplate

    data = tc.build("long")
    del data.obs[1:]
    ob = data.obs[0]
    ob.detdata.create(gc.ESTIMATE, dtype=np.float64, detectors=["d0", "d2"])
    ob.detdata[gc.ESTIMATE].data[:] = 1.5
    tmpl = gc.configure(GainTemplate(name="g", order=1, template_name=gc.ESTIMATE))
    tmpl.data = data
    assert tmpl.detectors() == ["d0", "d2"] and tmpl._n_local == 4


def test_order_above_the_device_limit_runs_on_the_host():
    from toast_amd import capi
    from toast_amd.templates import GainTemplate

    limit = capi.dev.subharmonic_max_terms()
    assert limit == 9
    data = gc.build()
    tmpl = gc.configure(GainTemplate(name="g", order=limit, template_name=gc.ESTIMATE))
    tmpl.data = data
    assert not tmpl.supports_accel()
    assert gc.configure(GainTemplate(name="g", order=limit - 1, template_name=gc.ESTIMATE)).supports_accel()
    amps = tmpl.zeros()
    amps.local[:] = 1.0
    before = data.obs[0].detdata[tc.DET_DATA].data.copy()
    tmpl.add_to_signal("d0", amps)
    assert np.any(data.obs[0].detdata[tc.DET_DATA].data[0] != before[0])
    assert tmpl._precond.shape == (3, limit + 1, limit + 1)
