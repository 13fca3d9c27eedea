"""CPU: the algorithm of ops.FilterBin against the reference's own run (tests/golden/filterbin.npz, produced by
tests/golden/make_golden_filterbin.py from src/toast/ops/filterbin.py), with no device.

``filterbin_case.NumpyBackend`` restates in NumPy what the device hands over -- the unnormalised blocks of the arrowhead
normal matrix and the counts of good non-zero samples --; the operator's own host code (``regress`` / ``solve_blocks`` /
``trim_intervals`` of toast_amd/ops/filterbin.py: the two maskings, the normalisation D^-1/2 M D^-1/2, the block
elimination and the choice of route) does the rest.  Flags and routes must agree exactly; the filtered signal's distance
max |delta| / rms(signal) is printed per case.  Its largest value is the algorithm distance E_host that
tests/test_gpu_filterbin.py quotes."""
import numpy as np
import pytest

import filterbin_case as FC
import golden_util as gu
from toast_amd.ops import filterbin as FB


def run_host(case):
    """-> (filtered signal, detector flags, shared flags, regress result, kept intervals, dense names)."""
    cfg = case["cfg"]
    n = cfg["n_samp"]
    signal, flags, shared = case["signal"].copy(), case["dflags"].copy(), case["shared"].copy()
    k = 1 if cfg["poly"] is None else cfg["poly"] + 1
    kept = []
    if cfg["poly"] is not None:
        bad = (shared & FC.SHARED_FLAG_MASK) != 0
        kept, flagged = FB.trim_intervals([(int(a), int(b)) for a, b in case["spans"]], n, bad, k)
        for first, last in flagged:
            shared[first:last] |= FC.FILTER_FLAG_MASK
    starts, stops = [s[1] for s in kept], [s[2] for s in kept]
    dense = FC.dense_templates(case)
    first, last = FC.row_spans(dense)
    backend = FC.NumpyBackend(dense, starts, stops, k, signal, flags, shared)
    res = FB.regress(backend, cfg["n_det"], n, first, last, starts, stops, k, cfg["limit"])
    names = FB.dense_template_names(cfg["hwp"], cfg["ground"], cfg["poly"], cfg["split"], FC.LEFTRIGHT, FC.RIGHTLEFT)
    return signal, flags, shared, res, kept, names


def amplitudes_by_name(res, d, kept, names):
    amps = {names[t]: res["amp_d"][d, t] for t in np.nonzero(res["act_d"][d])[0]}
    for v, (index, _, _) in enumerate(kept):
        for j in np.nonzero(res["act_p"][d, v])[0]:
            amps[f"poly-{j}-interval-{index}"] = res["amp_p"][d, v, j]
    return amps


@pytest.fixture(scope="module")
def fixture():
    return gu.load("filterbin")


@pytest.mark.parametrize("name", list(FC.CASES))
def test_algorithm_against_the_reference_run(fixture, name):
    case = FC.load_case(fixture, name)
    signal, flags, shared, res, kept, names = run_host(case)
    assert np.array_equal(shared, case["shared_out"])
    assert np.array_equal(flags, case["flags_out"])
    assert np.array_equal(res["route"], case["routes"])
    detflags = np.where(res["flag_detector"], FC.FILTER_FLAG_MASK, 0) | np.where(
        res["route"] == FB.ROUTE_REJECTED, FC.FILTER_DETECTOR_MASK, 0)
    assert np.array_equal(detflags, case["detflags"])
    rms = np.sqrt(np.mean(case["signal"] ** 2))
    dist = np.max(np.abs(signal - case["out"])) / rms
    print(f"\nfilterbin host {name}: max |delta filtered| / rms(signal) = {dist:.3e}  fast route {res['fast'].tolist()}")
    assert dist < 1e-10                       # the parity bar
    # amplitudes: the same templates survive; the values agree where the reference inverted (they are not unique under
    # the pseudo-inverse)
    for d in range(case["cfg"]["n_det"]):
        want = {x: case["amps"][d, i] for i, x in enumerate(case["amp_names"]) if not np.isnan(case["amps"][d, i])}
        if case["routes"][d] not in (FB.ROUTE_INV, FB.ROUTE_PINV):
            assert want == {}
            continue
        got = amplitudes_by_name(res, d, kept, names)
        assert sorted(got) == sorted(want)
        if case["routes"][d] == FB.ROUTE_INV:
            scale = max(abs(v) for v in want.values())
            worst = max(abs(got[x] - want[x]) for x in want) / scale
            assert worst < 1e-10, (name, d, worst)


def test_planted_edges_are_in_the_fixture(fixture):
    case = FC.load_case(fixture, "all")
    assert np.max(case["spans"][:, 1] - case["spans"][:, 0]) > 1024 and case["spans"][-1, 1] > case["cfg"]["n_samp"]
    assert case["routes"][int(case["planted_dead_detector"])] == FB.ROUTE_NOFIT
    d = int(case["planted_dead_direction_det"])
    dropped = [x for i, x in enumerate(case["amp_names"]) if x.endswith(FC.LEFTRIGHT) and np.isnan(case["amps"][d, i])]
    assert len(dropped) == 5 and case["routes"][d] == FB.ROUTE_INV
    short = int(case["planted_short_interval"])
    assert not any(x.endswith(f"-interval-{short}") for x in case["amp_names"])
    assert sorted(set(FC.load_case(fixture, n)["routes"].tolist()) for n in ("pinv", "reject")) == [{1}, {2}]
    # the HWP angle starts at exactly 0: the sine rows start one sample late (SparseTemplates.trim)
    first, _ = FC.row_spans(FC.dense_templates(case))
    assert list(first[:4]) == [0, 1, 0, 1]


def test_fast_route_is_the_reference_route_where_it_is_taken(fixture):
    """Block elimination and the reference's inverse of the full matrix give the same amplitudes; with a limit the bound
    cannot clear, every detector takes the reference route."""
    case = FC.load_case(fixture, "all")
    cfg = case["cfg"]
    _, _, _, res, kept, _ = run_host(case)
    assert res["fast"][[0, 1, 2, 4, 6]].all()
    case["cfg"] = dict(cfg, limit=1e-30)            # nothing is below it: inverse for everybody, but the bound ...
    _, _, _, res_fast, _, _ = run_host(case)
    case["cfg"] = dict(cfg, limit=0.5)              # ... cannot clear this one
    signal_ref, _, _, res_ref, _, _ = run_host(case)
    assert not res_ref["fast"].any() and set(res_ref["route"].tolist()) <= {FB.ROUTE_PINV, FB.ROUTE_NOFIT}
    scale = np.max(np.abs(res["amp_d"]))
    assert np.max(np.abs(res_fast["amp_d"] - res["amp_d"])) <= 1e-12 * scale
    # pseudo-inverse of a regular matrix (cut at 1e-10 of the largest singular value): the same cleaned signal
    assert np.max(np.abs(signal_ref - case["out"])) < 1e-9 * np.sqrt(np.mean(case["signal"] ** 2))


def test_solve_blocks_matches_a_dense_least_squares_fit():
    """A small random arrowhead system: the amplitudes equal np.linalg.lstsq on the explicit unit-norm template matrix."""
    rng = np.random.default_rng(5)
    n, nd, k = 700, 3, 2
    starts, stops = [10, 260, 480], [250, 470, 690]
    dense = rng.standard_normal((nd, n))
    signal = rng.standard_normal((2, n)) + 3.0
    flags = (rng.random((2, n)) < 0.1).astype(np.uint8)
    shared = (rng.random(n) < 0.05).astype(np.uint8)
    backend = FC.NumpyBackend(dense, starts, stops, k, signal.copy(), flags, shared)
    first, last = FC.row_spans(dense)
    res = FB.regress(backend, 2, n, first, last, starts, stops, k, 1e-6)
    assert res["fast"].all() and np.all(res["route"] == FB.ROUTE_INV)
    for d in range(2):
        good = ((shared & FC.SHARED_FLAG_MASK) == 0) & ((flags[d] & FC.DET_FLAG_MASK) == 0)
        rows = [r for r in dense]
        for a, b in zip(starts, stops):
            for row in FC.interval_polynomials(a, b, k):
                full = np.zeros(n)
                full[a:b] = row
                rows.append(full)
        F = np.array(rows)
        F /= np.sqrt(np.sum((F * good) ** 2, axis=1))[:, None]
        want = np.linalg.lstsq((F * good).T, signal[d] * good, rcond=None)[0]
        got = np.concatenate([res["amp_d"][d], res["amp_p"][d].ravel()])
        assert np.max(np.abs(got - want)) < 1e-11 * np.max(np.abs(want))
        assert np.max(np.abs(backend.signal[d] - (signal[d] - want @ F))) < 1e-11 * np.max(np.abs(signal[d]))


def test_flag_mask_overlap_checks_and_unsupported_traits():
    """filterbin.py:726-744: the four checks raise before anything else happens; what is left out raises too."""
    from toast_amd import ops
    from toast_amd.sim import create_ground_data

    data = create_ground_data(n_det=2, n_samp=400, rate=20.0)
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=8, nest=True)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU")

    def binner(**kw):
        return ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=weights, **kw)

    with pytest.raises(RuntimeError, match="binning"):
        ops.FilterBin(name="fb").apply(data)
    for traits, bin_traits, what in (
            (dict(filter_flag_mask=4, det_flag_mask=3), {}, "det flag mask"),
            (dict(filter_flag_mask=4, det_flag_mask=4, shared_flag_mask=3), {}, "shared mask"),
            (dict(filter_flag_mask=4, det_flag_mask=4, shared_flag_mask=4), dict(det_flag_mask=3), "det bin mask"),
            (dict(filter_flag_mask=4, det_flag_mask=4, shared_flag_mask=4), dict(det_flag_mask=4, shared_flag_mask=3),
             "shared bin mask")):
        with pytest.raises(RuntimeError, match=f"does not overlap with {what}"):
            ops.FilterBin(name="fb", binning=binner(**bin_traits), **traits).apply(data)
    for trait, value in (("write_obs_matrix", True), ("deproject_map", "map.fits"), ("precomputed_templates", "key"),
                         ("ground_filter_bin_width", 0.01), ("ground_template_time_step", 10), ("maskfile", "mask.fits")):
        with pytest.raises(NotImplementedError, match=trait):
            ops.FilterBin(name="fb", binning=binner(), **{trait: value}).apply(data)
    names = FB.dense_template_names(2, 3, 1, True, "lr", "rl")
    assert names == ["HWPSS-cos-1", "HWPSS-sin-1", "HWPSS-cos-2", "HWPSS-sin-2", "ground-poly-2-lr", "ground-poly-2-rl",
                     "ground-poly-3-lr", "ground-poly-3-rl"]
