"""tests/templates_reference.py held on the CPU: the plain reference that tests/test_gpu_templates_grid.py compares the
HIP kernels with must itself be right, and must notice one lost sample.

* ``basis`` equals ``toast_amd.templates.subharmonic.legendre_basis`` bit for bit.  Against the same recurrence carried in
  ``np.longdouble`` (r from a long-double ``linspace``) its largest distance over 1..9 terms and lengths 1, 2, 3, 64 and
  4097 is 9.67 eps (BASIS_DISTANCE_EPS; T_6 at 64 samples, where the step 2 / 63 is no double and T_k' grows like k^2;
  2 / 4096 is exact and 4097 samples stay below 4.5 eps; |T_k| <= 1, so eps is an absolute unit): a deterministic CPU
  figure, asserted with a factor 2.
* On the inputs of tests/templates_case.py the reference reproduces the ``*_index_obs*``, ``*_hits`` and ``*_add_obs*``
  entries of tests/golden/templates_basis.npz (results of the reference implementation's own methods) bit for bit, and
  the fixture's projections lie within the derived bounds of the exact sums.
* The fixture's SubHarmonic preconditioner blocks P are ``numpy.linalg.inv`` of Gram matrices G' that were summed in
  NumPy's order: |G' - G| <= E = gamma(m) S w elementwise.  ``inv`` solves G' X = I by LU with partial pivoting, whose
  columns satisfy |G' P - I| <= gamma(3n) |L||U||P| (Higham, Theorem 9.4), and (|L||U|)_ik <= n rho max|G'| with the growth
  factor rho <= 2^(n-1).  So  |G P - I| <= E |P| + gamma(3n) n 2^(n-1) (max|G| + max E) colsum|P|, G being the exact
  weighted Gram matrix of the reference.  Crude in rho, and still eight orders below one lost sample.
* Self-sensitivity: with one sample dropped from a grid case the reference moves by more than 1000 times the bound.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import templates_case as tc  # noqa: E402
import templates_reference as tr  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "templates_basis.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
LD = np.longdouble
ALL_DETS = ("d0", "d1", "d2")
BASIS_DISTANCE_EPS = 9.67


def test_basis_equals_the_host_path_and_the_long_double_recurrence():
    from toast_amd.templates.subharmonic import legendre_basis

    worst = 0.0
    for norder in range(1, 10):
        for length in (1, 2, 3, 64, 4097):
            b = tr.basis(norder, length)
            assert b.dtype == np.float64 and np.array_equal(b, legendre_basis(norder, length)), (norder, length)
            wide = tr.basis(norder, length, dtype=LD)
            assert wide.dtype == LD
            worst = max(worst, float(np.abs(b.astype(LD) - wide).max() / EPS))
    assert np.array_equal(tr.basis(9, 1)[:, 0], [1, -1, 1, -1, 1, -1, 1, -1, 1])
    assert np.array_equal(tr.basis(3, 2), [[1, 1], [-1, 1], [1, 1]])
    print(f"basis: largest distance to the long-double recurrence {worst:.3f} eps (recorded {BASIS_DISTANCE_EPS})")
    assert worst <= 2.0 * BASIS_DISTANCE_EPS
    assert worst >= 0.5 * BASIS_DISTANCE_EPS          # (the recorded figure is this one)


def _layout(case_layout, per_obs):
    """Detector-major amplitude offsets: {(det, iob): offset}, n_local.  ``per_obs[iob]`` amplitudes per detector."""
    obs = tc.LAYOUTS[case_layout]["obs"]
    offsets, off = {}, 0
    for det in ALL_DETS:
        for iob, ocfg in enumerate(obs):
            if det in ocfg["dets"]:
                offsets[(det, iob)] = off
                off += per_obs[iob]
    return offsets, off


@pytest.mark.parametrize("name", list(tc.SUBHARMONIC_CASES))
def test_reference_reproduces_the_subharmonic_fixture(name):
    layout, traits = tc.SUBHARMONIC_CASES[name]
    norder = traits["order"] + 1
    data = tc.build(layout)
    obs = tc.LAYOUTS[layout]["obs"]
    offsets, n_local = _layout(layout, [len(o["views"]) * norder for o in obs])
    assert n_local == int(GOLD[f"{name}_n_local"])
    assert np.array_equal([offsets[(d, 0)] for d in ALL_DETS], GOLD[f"{name}_det_start"])
    amps = tc.amplitudes(n_local, 1)
    worst_p = worst_g = LD(0)
    for iob, ob in enumerate(data.obs):
        dets = list(obs[iob]["dets"])
        views = obs[iob]["views"]
        rows = list(range(len(dets)))
        offs = [offsets[(d, iob)] for d in dets]
        signal = ob.detdata[tc.DET_DATA].data
        flags = ob.detdata[tc.DET_FLAGS].data
        assert np.array_equal(tr.subharmonic_add(signal, rows, offs, amps, views, norder), GOLD[f"{name}_add_obs{iob}"])
        sums = tr.subharmonic_project(signal, rows, views, norder)
        weights = [0.5 + 0.75 * ALL_DETS.index(d) if traits["noise_model"] is not None else 1.0 for d in dets]
        gram, ngood = tr.subharmonic_gram(flags, rows, tc.DET_FLAG_MASK, weights, views, norder)
        assert np.all(ngood > 0)
        exact = (gram.hi.astype(LD) + gram.lo.astype(LD)) * np.asarray(weights, dtype=LD)[:, None, None, None]
        _, g_bound = tr.gram_check(exact, gram, weights)
        for k in range(len(dets)):
            for v in range(len(views)):
                sl = slice(offs[k] + v * norder, offs[k] + (v + 1) * norder)
                got = GOLD[f"{name}_project"][sl]
                one = tr.Sums(*(a[k, v] for a in sums))
                frac = tr.fraction_of(tr.deviation(got, one), tr.gamma(one.m - 1) * one.S)
                worst_p = max(worst_p, frac.max())
                p = GOLD[f"{name}_precond"][sl.start // norder].astype(LD)
                resid = np.abs(exact[k, v] @ p - np.eye(norder, dtype=LD))
                bound = g_bound[k, v] @ np.abs(p) + tr.gamma(3 * norder) * norder * 2.0 ** (norder - 1) * \
                    (np.abs(exact[k, v]).max() + g_bound[k, v].max()) * np.abs(p).sum(axis=0)[None, :]
                worst_g = max(worst_g, tr.fraction_of(resid, bound).max())
    print(f"{name}: fixture projection {float(worst_p):.3f} of gamma(m-1) S; |G P - I| {float(worst_g):.2e} of its bound")
    assert worst_p <= 1 and worst_g <= 1


@pytest.mark.parametrize("name", list(tc.PERIODIC_CASES))
def test_reference_reproduces_the_periodic_fixture(name):
    layout, traits = tc.PERIODIC_CASES[name]
    data = tc.build(layout)
    obs = tc.LAYOUTS[layout]["obs"]
    nbins_obs, setup = [], []
    for iob, ob in enumerate(data.obs):
        key = np.asarray(ob.shared[tc.KEY].data, dtype=np.float64).reshape(1, -1)
        kflags = None if traits["flags"] is None else np.asarray(ob.shared[tc.KEY_FLAGS].data).reshape(1, -1)
        inview = np.zeros(key.shape, dtype=bool)
        for first, last in obs[iob]["views"]:
            inview[:, first:last] = True
        if kflags is not None:
            inview &= (kflags & traits["flag_mask"]) == 0
        omin, omax = key[inview].min(), key[inview].max()
        if traits["bins"] is not None:
            nbins, incr = traits["bins"], (omax - omin) / traits["bins"]
        else:
            incr = float(traits["increment"])
            nbins = int((omax - omin) / incr)
        assert (omin, incr, nbins) == (GOLD[f"{name}_obs_min"][iob], GOLD[f"{name}_obs_incr"][iob], GOLD[f"{name}_obs_nbins"][iob])
        index, clamped = tr.periodic_index(key, kflags, traits["flag_mask"], obs[iob]["views"], omin, incr, nbins)
        assert index.dtype == np.int32 and np.array_equal(index[0], GOLD[f"{name}_index_obs{iob}"])
        assert clamped > 0 or traits["bins"] is None
        nbins_obs.append(nbins)
        setup.append(index)
    offsets, n_local = _layout(layout, nbins_obs)
    assert n_local == int(GOLD[f"{name}_n_local"])
    amps = tc.amplitudes(n_local, 2)
    worst = LD(0)
    for iob, ob in enumerate(data.obs):
        dets, nbins, index = list(obs[iob]["dets"]), nbins_obs[iob], setup[iob]
        rows = list(range(len(dets)))
        signal = ob.detdata[tc.DET_DATA].data
        flags = ob.detdata[tc.DET_FLAGS].data
        hits = tr.periodic_hits(index, None, flags, rows, tc.DET_FLAG_MASK, nbins, len(dets), 0, signal.shape[1])
        a_in = [amps[offsets[(d, iob)]:][:nbins] for d in dets]
        assert np.array_equal(tr.periodic_add(signal, rows, index, None, a_in, nbins), GOLD[f"{name}_add_obs{iob}"])
        a0 = np.full((len(dets), nbins), 0.5)
        sums, _ = tr.periodic_project(signal, rows, index, None, flags, rows, tc.DET_FLAG_MASK, nbins, a0)
        assert np.array_equal(sums.m, hits)
        for k, d in enumerate(dets):
            sl = slice(offsets[(d, iob)], offsets[(d, iob)] + nbins)
            assert np.array_equal(hits[k], GOLD[f"{name}_hits"][sl])
            one = tr.Sums(*(a[k] for a in sums))
            worst = max(worst, tr.fraction_of(tr.deviation(GOLD[f"{name}_project"][sl], one), tr.periodic_bound(one, a0[k])).max())
    print(f"{name}: fixture projection {float(worst):.3f} of gamma(m) (|a0| + S)")
    assert worst <= 1


def test_reference_notices_one_dropped_sample():
    # Periodic: one sample that takes part loses its bin
    case = tr.periodic_sweep(7, "random", "shared")
    rows, flag_rows, nbins = case["rows"], case["flag_rows"], case["nbins"]
    d = 1
    i = int(np.argmax(np.where(case["good"][d], np.abs(case["signal"][rows[d]]), 0.0)))
    b = int(case["index"][0, i])
    index = case["index"].copy()
    index[0, i] = -1
    sums, _ = tr.periodic_project(case["signal"], rows, index, None, case["flags"], flag_rows, tr.DET_MASK, nbins, case["a0"])
    moved = tr.deviation(sums.hi[d, b], tr.Sums(*(a[d, b] for a in case["project"])))
    bound = tr.periodic_bound(case["project"], case["a0"])[d, b]
    print(f"periodic: one dropped sample moves the sum by {float(moved / bound):.2e} bounds")
    assert sums.m[d, b] == case["project"].m[d, b] - 1 and moved > 1000 * bound
    # SubHarmonic: the view of 4097 samples without its sample 2000 (a zero term)
    sub = tr.subharmonic_grid()
    view = sub["views"][9]
    assert view[1] - view[0] == 4097
    signal = sub["signal"].copy()
    signal[sub["rows"][0], view[0] + 2000] = 0.0
    sums = tr.subharmonic_project(signal, sub["rows"][:1], [view], tr.SUBH_MAX_TERMS)
    full = tr.Sums(*(a[0, 9] for a in sub["project"]))
    moved = tr.deviation(sums.hi[0, 0], full)
    bound = tr.gamma(full.m - 1) * full.S
    print("subharmonic: one dropped sample moves the sums by", " ".join(f"{float(x):.1e}" for x in moved / bound), "bounds")
    assert moved[0] > 1000 * bound[0] and np.count_nonzero(moved > 1000 * bound) >= 5
