"""Host: the Fourier2D template on its NumPy / SciPy path against tests/golden/fourier2d.npz -- the results of the
reference's own methods (tests/golden/make_golden_fourier2d.py) on the inputs of tests/fourier2d_case.py -- and the
additions to the data model it needs.  No device.

Layout, basis, norms and ``project_signal`` are sequences of single roundings in a fixed order and are compared for
equality.  ``add_to_signal`` (NumPy's pairwise sum) and the prior (SciPy's convolution, which picks its method) may take
their sums in another order with another build of those libraries, so they get the bounds of the GPU tests: ten times the
reference's own deviation from the exact sum, and eight times its largest distance from the ``longdouble`` convolution
(the ``yard_*`` entries of the fixture, measured by the generator).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import fourier2d_case as fc  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "fourier2d.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps


def _template(name, **extra):
    from toast_amd.templates import Fourier2D

    layout, traits = fc.CASES[name]
    data = fc.build(layout)
    tmpl = fc.configure(Fourier2D(name=name, **{**traits, **extra}))
    tmpl.data = data
    return data, tmpl


def _amps(tmpl, values):
    z = tmpl.zeros()
    z.local[:] = values
    return z


@pytest.mark.parametrize("name", list(fc.CASES))
def test_host_path_matches_reference(name):
    layout, _ = fc.CASES[name]
    data, tmpl = _template(name)
    nmode = tmpl.nmode
    rows, cols = fc.sample_subset(layout)
    assert nmode == int(GOLD[f"{name}_nmode"]) and tmpl._n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal(np.concatenate([tmpl._obs_view_offset[i] for i in range(len(data.obs))]), GOLD[f"{name}_view_offset"])
    z = tmpl.zeros()
    assert np.array_equal(np.array(z.local_ranges), GOLD[f"{name}_local_ranges"]) and not np.any(z.local_flags)
    templates = []
    for iob, ob in enumerate(data.obs):
        t = np.array([tmpl._templates[iob][d] for d in ob.local_detectors])
        assert np.array_equal(t, GOLD[f"{name}_T_obs{iob}"]), iob
        fc.check_rank(t)
        templates.append(t)
        for ivw, filt in enumerate(tmpl._filters[iob]):
            want = GOLD[f"{name}_invcorr_{iob}_{ivw}"]
            first, last = fc.view_samples(layout)[iob][ivw]
            assert filt.size == want.size == (last - first) - (last - first) % 2
            assert np.array_equal(filt, want)      # the same rfft / irfft on the same expressions
    assert np.array_equal(np.concatenate([tmpl._filter_floored[i] for i in range(len(data.obs))]), GOLD[f"{name}_floored"][:, 0])
    assert np.array_equal(tmpl._filter_scale, GOLD[f"{name}_filter_scale"])
    if layout == "wide" and nmode <= 70:
        assert np.linalg.matrix_rank(templates[0]) == nmode      # full column rank
    assert np.array_equal(tmpl._norms.reshape(-1, nmode)[rows], GOLD[f"{name}_norms"])
    zero = fc.all_flagged_row(layout)
    if zero is not None:
        assert np.all(tmpl._norms.reshape(-1, nmode)[zero] == 0.0)
    add_scale, proj_scale = fc.term_scales(name, templates)
    # M^T d on top of amplitudes that are not zero
    proj = _amps(tmpl, fc.amplitudes(tmpl._n_local, 2))
    for det in tmpl.detectors():
        tmpl.project_signal(det, proj)
    assert np.array_equal(proj.local.reshape(-1, nmode)[rows], GOLD[f"{name}_project"])
    # d + M a
    amps = _amps(tmpl, fc.amplitudes(tmpl._n_local, 1))
    for det in tmpl.detectors():
        tmpl.add_to_signal(det, amps)
    f_add = 10.0 * float(GOLD[f"{name}_yard_add"])
    for iob, ob in enumerate(data.obs):
        err = np.abs(ob.detdata[fc.DET_DATA].data[:, cols[iob]] - GOLD[f"{name}_add_obs{iob}"]) / (EPS * add_scale[iob])
        print(f"{name}: add_to_signal obs{iob}, worst deviation from the fixture {err.max():.2f} eps sum|terms| (bound {f_add:.2f})")
        assert np.all(err <= f_add)
    out = _amps(tmpl, -3.0)
    tmpl.apply_precond(amps, out)
    assert np.array_equal(out.local, amps.local * tmpl._norms)
    if zero is not None:
        assert np.all(out.local.reshape(-1, nmode)[zero] == 0.0)
    out = _amps(tmpl, 0.5)
    tmpl.add_prior(amps, out)
    bound = 8.0 * float(GOLD["yard_prior_max"]) * float(GOLD[f"{name}_prior_max"])
    err = np.abs(out.local.reshape(-1, nmode)[rows] - GOLD[f"{name}_prior"]).max()
    print(f"{name}: add_prior, distance to the fixture {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    tmpl.clear()


def test_floor_is_active_in_the_fixture():
    assert GOLD["floor_floored"][:, 0].max() > 100 and GOLD["m7_floored"][:, 0].max() > 0


def test_focalplane_field_of_view():
    from toast_amd.data import Focalplane, detector_direction

    quats = fc.focalplane_quats(5)
    fp = Focalplane([f"d{k}" for k in range(5)], quats)
    mincos = min(detector_direction(q)[2] for q in quats)
    assert fp.field_of_view == 1.01 * 2.0 * np.arccos(mincos)
    assert abs(fp.field_of_view - 1.01 * 2.0 * np.radians(0.9)) < 1.0e-9
    # boresight detectors only: one degree
    fp = Focalplane(["a", "b"], np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)))
    assert fp.field_of_view == np.radians(1.0)
    assert Focalplane(["a"], [[0.0, 0.0, 0.0, 1.0]], field_of_view=0.25).field_of_view == 0.25
    # the rotated boresight of a quaternion about x by 90 degrees points along -y
    s = np.sqrt(0.5)
    assert np.allclose(detector_direction([s, 0.0, 0.0, s]), [0.0, -1.0, 0.0], atol=1e-15)


def test_amplitudes_local_ranges():
    from toast_amd.data import Comm
    from toast_amd.templates import Amplitudes

    comm = Comm()
    a = Amplitudes(comm, 10, 10, local_ranges=[(0, 4), (13, 6)])
    assert a.local_ranges == [(0, 4), (13, 6)] and a.n_local == 10 and a.local_indices is None
    a.local[:] = np.arange(10.0)
    b = a.duplicate()
    assert b.local_ranges == a.local_ranges and np.array_equal(b.local, a.local)
    assert a.dot(b) == float(np.sum(np.arange(10.0) ** 2))
    assert Amplitudes(comm, 10, 10).local_ranges is None
    with pytest.raises(RuntimeError):
        Amplitudes(comm, 10, 10, local_ranges=[(0, 4), (13, 5)])
    with pytest.raises(RuntimeError):
        Amplitudes(comm, 12, 10, local_ranges=[(0, 4), (13, 6)])
    with pytest.raises(NotImplementedError):
        Amplitudes(comm, 10, 10, local_indices=np.arange(10))

    class TwoProcesses:
        comm_world = comm_group = object()
        world_size = group_size = 2

    with pytest.raises(NotImplementedError):
        Amplitudes(TwoProcesses(), 10, 10, local_ranges=[(0, 10)])


def test_the_three_raises():
    from toast_amd.templates import Fourier2D

    data = fc.build("short")
    with pytest.raises(RuntimeError, match="debug_plots"):
        fc.configure(Fourier2D(name="f", debug_plots="plots")).data = data
    data.obs[0].intervals.create("one", [(10, 60), (70, 71)])
    data.obs[1].intervals.create("one", [(0, 500)])
    with pytest.raises(ValueError, match=r"view 1 of observation obs0"):
        fc.configure(Fourier2D(name="f"), view="one").data = data

    data = fc.build("short")

    class TwoProcesses:
        comm_world = comm_group = object()
        world_size = group_size = 2

    data.comm = TwoProcesses()
    with pytest.raises(NotImplementedError):
        fc.configure(Fourier2D(name="f")).data = data


def test_supports_accel_on_either_side_of_the_cap():
    from toast_amd import capi
    from toast_amd.templates import Fourier2D

    cap = capi.dev.fourier2d_max_modes()
    assert cap >= 39
    assert Fourier2D(order=3, fit_subharmonics=True).supports_accel()
    order = 1
    while (2 * order) ** 2 + 1 <= cap:
        order += 1
    assert not Fourier2D(order=order, fit_subharmonics=False).supports_accel()
    assert Fourier2D(order=order - 1, fit_subharmonics=False).supports_accel()
    assert not Fourier2D(**{k: v for k, v in fc.CASES["above"][1].items()}).supports_accel()


def test_trait_audit_is_clean_for_fourier2d():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import audit_traits

    if not os.path.isdir(audit_traits.REF):
        pytest.skip("the reference sources are not on this machine")
    assert "Fourier2D" in audit_traits.ours() and "Fourier2D" in audit_traits.ref_classes()
    assert [d for d in audit_traits.differences() if d[0] == "Fourier2D"] == []
