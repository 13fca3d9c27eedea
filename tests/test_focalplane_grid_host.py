"""Host: the inputs and plain references of tests/focalplane_grid.py, before any device result is judged by them.

* The Fourier2D layout has the view lengths, the adjacency, the clipping and the sentinel gaps its docstring lists.
* The plain Fourier2D references, applied to the layouts of tests/fourier2d_case.py, reproduce the results of the
  reference implementation's own methods (tests/golden/fourier2d.npz) on the fixture's sample subset: equality for the
  norms and the projection, the fixture's own bounds for add_to_signal (ten times the reference's deviation from the exact
  sum) and the prior (eight times its largest distance from the longdouble convolution).
* Every synthetic prior case prints ``d_ref``, the distance of the reference's own call (scipy.signal.convolve, "same")
  from the longdouble window relative to max|out|: the GPU test's bound is 8 x max(d_ref, yard) x max|out|.
* tests/golden/poly2d_grid.npz / poly2d_grid_o3.npz: the host emulation of the device algorithm agrees with the stored
  coefficients of the reference's kernel within the stored bounds; exclusion share, engineered samples, statuses.
* ``batches_o3`` has the tiles and views the GPU test needs; the tiles per batch are the launcher's to say.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import focalplane_grid as G  # noqa: E402
import fourier2d_case as fc  # noqa: E402
import poly2d_host as P  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "fourier2d.npz"), allow_pickle=False)
EPS = np.finfo(np.float64).eps
YARD = float(GOLD["yard_prior_max"])


# ------------------------------------------------------------------------------------ Fourier2D
def test_fourier2d_layout_has_the_shapes_it_is_there_for():
    views, clipped = G.F2D_VIEWS, G.f2d_clipped()
    lengths = [b - a for a, b in clipped]
    assert sorted(lengths) == [0, 1, 2, 3, 255, 256, 257, 511, 512, 513]
    assert G.F2D_N_SAMP % 2 == 1 and 2300 <= sum(lengths) <= 2400 and G.f2d_tiles() == 14
    assert sum(first < 0 for first, _ in views) == 1 and sum(last > G.F2D_N_SAMP for _, last in views) == 1
    assert sum(views[v][1] == views[v + 1][0] and lengths[v] > 0 and lengths[v + 1] > 0 for v in range(len(views) - 1)) == 2
    e = G.F2D_EMPTY_VIEW
    assert lengths[e] == 0 and lengths[e - 1] > 0 and lengths[e + 1] > 0
    assert {a % 2 for (a, b) in clipped if b > a} == {0, 1}
    assert all(clipped[v][1] <= clipped[v + 1][0] for v in range(len(views) - 1))        # ascending, never overlapping
    inside = np.zeros(G.F2D_N_SAMP, dtype=bool)
    for a, b in clipped:
        inside[a:b] = True
    assert inside[G.F2D_ALL_FLAGGED] and 0 < np.count_nonzero(~inside) < 120
    assert list(G.F2D_BLOCK_ORDER) != sorted(G.F2D_BLOCK_ORDER) and sorted(G.F2D_BLOCK_ORDER) == list(range(len(views)))
    for nmode in G.F2D_NMODES:
        offsets, size, used = G.f2d_amp_layout(nmode)
        blocks = sorted((int(offsets[v]), int(offsets[v]) + (views[v][1] - views[v][0]) * nmode) for v in range(len(views)))
        assert blocks[0][0] >= 3 and blocks[-1][1] < size
        assert all(blocks[k + 1][0] - blocks[k][1] >= 3 for k in range(len(blocks) - 1))     # sentinel slots between the blocks
        assert np.count_nonzero(used) == sum(lengths) * nmode
        # the clipped views: the amplitudes of the samples cut away lie inside a block and are not used
        assert not used[offsets[0]:offsets[0] + 5 * nmode].any() and used[offsets[0] + 5 * nmode]
        assert not used[offsets[9] + 513 * nmode:offsets[9] + 519 * nmode].any() and used[offsets[9] + 513 * nmode - 1]
    for n_det in G.F2D_NDETS:
        case = G.f2d_case(7, n_det)
        assert case["signal"].shape[0] == n_det + 1 and sorted(set(range(n_det + 1)) - set(case["rows"])) != []
        unlisted = (set(range(n_det + 1)) - set(case["rows"])).pop()
        assert np.all(case["signal"][unlisted] == G.SENTINEL)
        assert n_det < 5 or not np.array_equal(case["rows"], case["flag_rows"])
        listed = case["flags"][case["flag_rows"]]
        assert np.all(listed[:, G.F2D_ALL_FLAGGED] & G.DET_FLAG_MASK)
        assert 0.2 < np.mean((case["flags"] & G.DET_FLAG_MASK) != 0) < 0.4 and np.any(case["flags"] & G.DET_FLAG_OTHER)
        assert np.all(case["amps"][~case["used"]][:3] == G.SENTINEL)
    assert np.count_nonzero(G.f2d_table(19, 9, "random") == 0.0) > 9
    for nmode in G.F2D_NMODES:
        assert np.linalg.matrix_rank(G.f2d_table(nmode, 70)) == nmode      # real mode sets: full column rank


def _fixture_layout(name, iob):
    """Views, offsets and buffers of one observation of a fixture case, in the form the references take."""
    layout, traits = fc.CASES[name]
    data = fc.build(layout)
    ob = data.obs[iob]
    views = fc.view_samples(layout)[iob]
    n_before = sum(len(v) for v in fc.view_samples(layout)[:iob])
    offsets = GOLD[f"{name}_view_offset"][n_before:n_before + len(views)]
    dets = list(ob.local_detectors)
    w = np.ones(len(dets)) if traits["noise_model"] is None else np.array([ob[fc.NOISE].detector_weight(d) for d in dets])
    return ob, views, offsets, w, len(data.obs)


@pytest.mark.parametrize("name", list(fc.DEVICE_CASES))
def test_plain_references_reproduce_the_reference_fixture(name):
    layout, _ = fc.CASES[name]
    nmode, n_local = int(GOLD[f"{name}_nmode"]), int(GOLD[f"{name}_n_local"])
    rows, cols = fc.sample_subset(layout)
    amps, proj = fc.amplitudes(n_local, 1), fc.amplitudes(n_local, 2)
    norms = np.full(n_local, -1.0)
    n_obs = _fixture_layout(name, 0)[4]
    templates = [GOLD[f"{name}_T_obs{iob}"] for iob in range(n_obs)]
    add_scale, _ = fc.term_scales(name, templates)
    f_add = 10.0 * float(GOLD[f"{name}_yard_add"])
    for iob in range(n_obs):
        ob, views, offsets, w, _ = _fixture_layout(name, iob)
        t = templates[iob]
        sig, flg = ob.detdata[fc.DET_DATA].data, ob.detdata[fc.DET_FLAGS].data
        idx = np.arange(t.shape[0])
        args = (nmode, views, ob.n_local_samples, offsets)
        got = G.f2d_add(sig, idx, t, amps, *args)
        err = np.abs(got[:, cols[iob]] - GOLD[f"{name}_add_obs{iob}"]) / (EPS * add_scale[iob])
        print(f"{name}: plain add_to_signal obs{iob}, worst deviation from the fixture {err.max():.2f} eps sum|terms| (bound {f_add:.2f})")
        assert np.all(err <= f_add)
        proj = G.f2d_project(sig, idx, t, proj, *args)
        w2 = np.array([(t[d] * t[d]) * w[d] for d in range(t.shape[0])])
        norms = G.f2d_norms(flg, idx, fc.DET_FLAG_MASK, w2, norms, *args)
    assert np.array_equal(proj.reshape(-1, nmode)[rows], GOLD[f"{name}_project"])
    assert np.array_equal(norms.reshape(-1, nmode)[rows], GOLD[f"{name}_norms"]) and not np.any(norms == -1.0)
    zero = fc.all_flagged_row(layout)
    if zero is not None:
        assert np.all(norms.reshape(-1, nmode)[zero] == 0.0)
    # the split projection's truth and bound hold the reference's own sequence, with room
    ob, views, offsets, w, _ = _fixture_layout(name, 0)
    t = templates[0]
    idx = np.arange(t.shape[0])
    args = (ob.detdata[fc.DET_DATA].data, idx, t, fc.amplitudes(n_local, 2), nmode, views, ob.n_local_samples, offsets)
    truth, bound = G.f2d_project_truth(*args)
    seq = G.f2d_project(*args)
    err = np.abs(seq.astype(G.LD) - truth).astype(np.float64)
    frac = np.max(err[bound > 0] / bound[bound > 0])
    print(f"{name}: sequential projection of obs0, worst fraction of the derived bound {frac:.3f}")
    assert np.all(err <= bound) and np.all(err[bound == 0] == 0)
    # the prior: the longdouble window of the plain reference on the fixture's filters, against the fixture
    scale = GOLD[f"{name}_filter_scale"]
    out = np.full(n_local, 0.5).reshape(-1, nmode)
    av = amps.reshape(-1, nmode)
    cum = 0
    for iob in range(n_obs):
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            filt = GOLD[f"{name}_invcorr_{iob}_{ivw}"]
            n, shift = last - first, (filt.size - 1) // 2
            for m in range(nmode):
                full = np.convolve(av[cum:cum + n, m].astype(G.LD), (filt * scale[m]).astype(G.LD))
                out[cum:cum + n, m] = (G.LD(0.5) + full[shift:shift + n]).astype(np.float64)
            cum += n
    bound = 8.0 * YARD * float(GOLD[f"{name}_prior_max"])
    err = np.abs(out[rows] - GOLD[f"{name}_prior"]).max()
    print(f"{name}: longdouble window against the fixture {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def _prior_cases():
    for shape in G.PRIOR_SHAPES:
        yield shape + (1,)
    for shape in G.PRIOR_DOUBLED:
        yield shape + (2,)


def test_prior_window_is_the_same_mode_of_the_reference_call():
    """d_ref of every case: the scipy path stays inside 8 x max(d_ref, yard) of its own distance trivially; what is
    checked is that the window of the direct sum IS the "same" mode, also for F > L and odd F, and that d_ref is the size of
    rounding and not of a shifted window."""
    from toast_amd.templates.fourier2d import prior_fft_length

    short = 0
    for view_len, filter_len in G.PRIOR_SHAPES:
        n_fft = prior_fft_length(view_len, filter_len)
        short += n_fft < 64
        assert n_fft % 2 == 0 and n_fft >= view_len + filter_len - 1
        for nmode in G.PRIOR_NMODES:
            got = G.prior_scipy(view_len, filter_len, nmode)
            d, peak = G.prior_distance(got, view_len, filter_len, nmode)
            d_ref = d / peak
            bound = 8.0 * max(d_ref, YARD) * peak
            print(f"prior L {view_len} F {filter_len} nmode {nmode} n_fft {n_fft}: d_ref {d_ref:.3e} max|out|, max|out| {peak:.3e}, "
                  f"bound {bound:.3e}")
            assert d <= bound and d_ref < 1e-14 and peak > 1.0
    assert short >= 3
    assert {f % 2 for _, f in G.PRIOR_SHAPES} == {0, 1} and any(f > l for l, f in G.PRIOR_SHAPES)
    assert [prior_fft_length(l, f) for l, f in G.PRIOR_SHAPES[:4]] == [2, 2, 4, 16]


# ------------------------------------------------------------------------------------ PolyFilter2D
_fixtures = {}


def test_poly2d_edge_layout():
    lengths = [max(0, min(int(b), G.EDGE_N_SAMP) - max(int(a), 0)) for a, b in zip(G.EDGE_STARTS, G.EDGE_STOPS)]
    assert sorted(lengths) == [0, 1, 2, 255, 256, 257, 513]
    assert G.EDGE_STARTS[0] < 0 and G.EDGE_STOPS[-1] > G.EDGE_N_SAMP and G.EDGE_STARTS[-1] == G.EDGE_N_SAMP - 1
    assert G.EDGE_STOPS[0] == G.EDGE_STARTS[1] and lengths[2] == 0 and lengths[1] > 0 and lengths[3] > 0
    groups = G.edge_groups()
    assert tuple(np.bincount(groups)) == G.EDGE_GROUP_SIZES and 1 in G.EDGE_GROUP_SIZES
    assert np.count_nonzero(np.diff(groups) != 0) > len(groups) // 2          # interleaved in list order
    # the engineered samples are consecutive slots of the 513-sample view and start a wave of the solve at every order
    v = 5
    assert lengths[v] == 513 and G.EDGE_STARTS[v] <= G.EDGE_FIRST and G.EDGE_FIRST + 8 <= G.EDGE_STOPS[v]
    assert (G.EDGE_FIRST - G.EDGE_STARTS[v]) % 64 == 0


@pytest.mark.parametrize("name", list(G.EDGE_CASES))
def test_poly2d_edge_emulation_against_reference_fixture(name):
    case, ref_coeff, excluded, bounds = G.edge_fixture_case(name, _fixtures)
    fix = _fixtures[G.EDGE_FIXTURES[name]]
    order, n_mode = case["order"], case["n_mode"]
    assert np.max(np.abs(case["templates"] - fix[f"{name}_templates"])) <= 1e-15
    again = P.excluded_systems(case)
    print(f"{name}: excluded {100 * np.mean(excluded):.2f} % of {excluded.size} systems")
    assert np.array_equal(again, excluded) and np.mean(excluded) <= P.MAX_EXCLUDED
    assert min(G.EDGE_GROUP_SIZES[1:]) < n_mode or order == 0          # a group with fewer detectors than modes
    sig, flags, coeff, status, sweeps = P.emulate(case)
    assert sweeps <= 12
    # a quarter of the stored bound: the bound is four times what this very comparison measured
    P.check_result(case, ref_coeff, excluded, {k: v / 4 * (1 + 1e-12) for k, v in bounds.items()}, sig, flags, coeff,
                   label=f"emulation {name}")
    smax = np.nanmax(np.abs(case["signal"][case["sig_rows"]]))
    assert bounds["filtered"] <= 1e-10 * smax
    # the engineered samples have the ranks they are there for
    g0 = np.flatnonzero(case["det_group"] == 0)
    n_good = np.count_nonzero(P.good_mask(case, np.arange(case["n_samp"]))[g0], axis=0)
    assert n_good[G.E_GROUP_FLAGGED] == 0 and n_good[G.E_SHARED] == 0 and n_good[G.E_ONE_GOOD] == 1
    assert n_mode == 1 or 0 < n_good[G.E_FEW_GOOD] < n_mode
    assert n_good[G.E_NAN_GOOD] == g0.size and n_good[G.E_NAN_FLAGGED] == g0.size - 1 and n_good[G.E_ZERO] == g0.size - 1
    span = np.arange(G.EDGE_FIRST, G.EDGE_FIRST + 8)
    assert list(status[span, 0]) == G.edge_statuses(order)
    for s in (G.E_GROUP_FLAGGED, G.E_SHARED, G.E_ZERO, G.E_NAN_GOOD):
        assert np.all(coeff[s, 0] == 0) and np.all(flags[case["flag_rows"][g0], s] & P.POLY_MASK)
    assert np.any(coeff[G.E_ONE_GOOD, 0] != 0) and np.all(np.isfinite(coeff))
    assert np.isnan(sig[case["sig_rows"][g0[1]], G.E_NAN_FLAGGED]) and np.isnan(sig[case["sig_rows"][g0[2]], G.E_NAN_GOOD])
    # every status an order can have, within one 64-sample span of one group -- and within one wave of the solve
    wave = {0: 64, 1: 16, 2: 4, 3: 4}[order]
    assert (G.EDGE_FIRST - 780) % wave == 0
    assert set(status[G.EDGE_FIRST:G.EDGE_FIRST + min(wave, 8), 0]) == ({0, 1, 3} if order == 0 else {0, 1, 2, 3})
    # the other groups: one detector, fewer detectors than modes
    inside = P.view_samples(case)
    if order > 0:
        assert not np.any(status[inside, 1] == 0) and np.any(status[inside, 1] == 2)
    assert np.all(status[inside] >= 0) and np.all(np.delete(status, inside, axis=0) == -1)


def test_poly2d_empty_group_case():
    case, compact = G.build_empty_group_case(), G.build_empty_group_case(compact=True)
    assert case["n_group"] == 3 and sorted(set(case["det_group"])) == [0, 2]
    assert compact["n_group"] == 2 and np.array_equal(compact["det_group"] * 2, case["det_group"])
    assert np.array_equal(case["templates"], compact["templates"])
    assert case["starts"][0] < 0 and case["stops"][0] > case["n_samp"]
    sig, flags, coeff, status, _ = P.emulate(case)
    csig, cflags, ccoeff, cstatus, _ = P.emulate(compact)
    assert np.all(coeff[:, 1] == 0) and np.all(status[:, 1] == 1)
    assert np.array_equal(sig, csig) and np.array_equal(flags, cflags)
    assert np.array_equal(coeff[:, [0, 2]], ccoeff) and np.array_equal(status[:, [0, 2]], cstatus)


def test_poly2d_batches_case():
    """Per system the scratch holds 65 moments and projections plus 16 coefficients as doubles and a 4-byte status
    (csrc/poly2d_filter.hip): with 64 groups a tile of 256 samples takes 10.7 MB of the 96 MiB, nine tiles a batch.  The
    figure itself is the launcher's (``filter_poly2d_batch_tiles``, asserted by the GPU test); here: the case has the
    tiles and the views that make three batches with a view across the first boundary and one starting on the second."""
    tile0, n_tile = G.batch_tiles()
    assert n_tile >= 20
    n = (G.BATCH_STOPS - G.BATCH_STARTS + G.TILE - 1) // G.TILE
    assert any(t0 < 9 < t0 + k for t0, k in zip(tile0, n))          # a view across tile 9 | 10
    assert 18 in tile0                                             # a view starting on tile 18
    assert tuple(np.bincount(np.repeat(np.arange(64), G.BATCH_GROUP_SIZES))) == (24,) * 4 + (2,) * 60
    pieces = G.batch_pieces()
    assert all((b - a + G.TILE - 1) // G.TILE <= 3 for a, b in pieces)
    assert {b - a for a, b in pieces} >= {513, 257, 256, 255, 2, 1}
    covered = np.zeros(G.BATCH_N_SAMP, dtype=int)
    for a, b in pieces:
        covered[a:b] += 1
    want = np.zeros(G.BATCH_N_SAMP, dtype=int)
    for a, b in zip(G.BATCH_STARTS, G.BATCH_STOPS):
        want[a:b] = 1
    assert np.array_equal(covered, want)
    case = G.build_batches_case()
    assert case["n_group"] == 64 and case["order"] == 3 and case["n_det"] == 216
    assert tuple(np.bincount(case["det_group"])) == G.BATCH_GROUP_SIZES


def test_query_entries_are_host_arithmetic():
    """The two entries the GPU tests read their branch from make no device call: they answer without a GPU."""
    from toast_amd import capi

    groups, tiles = capi.dev.fourier2d_groups, capi.dev.filter_poly2d_batch_tiles
    n_tile = G.f2d_tiles()
    assert [groups(n, n_tile, 0) for n in G.F2D_NDETS] == [1, 1, 2, 3, 18]       # "5 become 3 and 2, 9 three groups of 3"
    assert all(groups(n, n_tile, n + 3) == n and groups(n, n_tile, 1) == 1 for n in G.F2D_NDETS)
    assert groups(70, 1024, 0) == 1 and groups(0, n_tile, 0) == 0
    per_batch = [tiles(3, g) for g in (1, 2, 64, 65535)]
    print(f"filter_poly2d_batch_tiles at order 3 for 1, 2, 64 and 65535 groups: {per_batch}")
    assert per_batch[0] >= 2 * per_batch[1] >= 2 and per_batch[2] >= 1 and per_batch[3] == 1      # never below one tile
    assert tiles(0, 64) > tiles(1, 64) > tiles(2, 64) > tiles(3, 64)
    assert tiles(-1, 1) == 0 and tiles(4, 1) == 0 and tiles(3, 0) == 0 and tiles(3, 65536) == 0
