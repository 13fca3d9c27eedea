"""The ObserveAtmosphere operator-kernel cases without a GPU (tests/atm_operator_case.py): the conditions that keep the
device comparisons of tests/test_gpu_atm_operator_grid.py honest, and the host restatements of k_atm_good_ranges,
k_atm_flag_failed and k_atm_finish against ``ObserveAtmosphere._observe_host`` -- code that
tests/test_atm_observe_host.py ties to the reference's own run.

Conditions, for every pointing of the observe_quats and operator cases: no step point within 1e-9 cell widths of a cell
face, no ray in cell (0, 0, 0), every az / el at least 1e-6 rad inside the cone (an ulp of another libm cannot flip a
skip), and where a volume has holes at least one good sample of a row fails and at most a quarter of them.  A row of one
sample cannot meet both halves of the last condition; it applies to the rows of 64 samples and more.

Restatements: flags equal the host path's byte for byte; values lie within ``FINISH_ROUNDINGS`` eps * scale_i of the
long-double finish of the same scratch rows (measured here: the restatement reproduces the host path bit for bit, worst
ratio of the host path's error to the bound 0.28)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import atm_observe_case as ac  # noqa: E402
import atm_operator_case as oc  # noqa: E402


def test_shapes_cover_the_edges():
    assert {255, 256, 257, 513} <= set(oc.N) and set(oc.N_OBSERVE) <= set(oc.N) and set(oc.N_FINISH) <= set(oc.N)
    assert oc.layout(257, True) == (257 + 37, 19) and oc.layout(257, False) == (257, 0)
    buf = oc.embed(np.ones((2, 5)), True, oc.SENTINEL, n_rows=4, at=[3, 1])
    assert buf.shape == (4, 42) and np.all(buf[[3, 1], 19:24] == 1) and np.sum(buf == 1) == 10
    for entries in (1, 3, 4, 5):
        tables = oc.row_tables(entries, 4, entries)
        assert all(np.unique(t).size == entries and t.max() < entries + 2 for t in tables)
        assert not any(np.array_equal(t, np.arange(entries)) for t in tables)
        assert len({t.tobytes() for t in tables}) == (4 if entries > 1 else 2)


@pytest.mark.parametrize("n", oc.N)
def test_range_rows(n):
    """The readout inputs: elevations in [0.1, 1.4], az over the full circle, the wrap points on both sides of phi = 0."""
    quats, wrap = oc.range_rows(n)
    az, el = oc.longdouble_azel(quats)
    assert np.all(np.abs(np.sqrt((quats**2).sum(-1)) - 1) < 1e-2) and np.any(np.abs((quats**2).sum(-1) - 1) > 1e-5)
    assert el.min() >= 0.1 - 1e-9 and el.max() <= 1.4 + 1e-9 and az.min() >= 0 and az.max() <= oc.TWOPI
    assert wrap.sum() == min(n, 4)
    if n >= 4:
        assert float(az[3, 0]) == oc.TWOPI                      # phi = 0
        assert float(az[3, 1]) > 6.28 and 0 < float(az[3, 2]) < 1e-15 and 0 < float(az[3, 3]) < 1e-14
    if n >= 63:
        assert az[3].max() - az[3].min() > 6.0
        host = [oc.ranges_host(np.ones(n), az[k].astype(np.float64), el[k].astype(np.float64)) for k in range(5)]
        assert az[1].max() - az[1].min() > 6.0 and host[1][6] - host[1][5] < 0.3       # crosses 0 / 2 pi
        assert host[2][6] - host[2][5] >= np.pi                                         # sweeps more than pi
        assert host[0][6] - host[0][5] < 0.4


def test_host_readout_deviation():
    """What the device readout is held to four times of: ``quats_to_azel`` against the long-double evaluation."""
    from toast_amd.ops.sim_tod_atm_observe import quats_to_azel

    worst = 0.0
    for n in oc.N:
        quats, wrap = oc.range_rows(n)
        az_ld, el_ld = oc.longdouble_azel(quats)
        az, el = quats_to_azel(quats.reshape(-1, 4))
        worst = max(worst, oc.azel_deviation(az.reshape(wrap.shape), el.reshape(wrap.shape), az_ld, el_ld, wrap))
    print(f"host readout: {worst:.3f} eps * max(1, |value|)")
    assert 0 < worst < 64


@pytest.mark.parametrize("n", oc.N)
def test_flag_patterns(n):
    for entries in (1, 3, 5):
        for name in oc.PATTERNS:
            pat = oc.flag_pattern(name, n, entries, 1)
            if pat is None:
                assert n <= 256 and name in ("s256", "from256")
                continue
            det, shared = pat
            good = np.stack([oc.good_host(None if det is None else det[e], shared, n) for e in range(entries)])
            want = {"first": [0], "last": [n - 1], "s256": [256], "from256": list(range(256, n)), "none": [],
                    "outside": list(range(n)), "neither": list(range(n))}
            if name in want:
                assert np.nonzero(good[0])[0].tolist() == want[name], name
            if name == "outside" and n >= 63:
                assert np.any(det != 0) and np.any(shared != 0)
            if name == "none" and entries > 1 and n >= 63:
                assert good[1].any()                   # a row with good samples next to the empty one
            if name == "random" and n >= 255:
                assert 0.55 < good.mean() < 0.85


def test_flag_failed_case():
    good, atm, flags, enable = oc.flag_failed_case(257, 4, 3)
    after, n_bad = oc.flag_failed_host(good, atm, flags, enable, 2)
    assert enable.tolist() == [1, 0, 1, 1] and n_bad[1] == 0 and np.all(n_bad[[0, 2, 3]] >= 4)
    assert np.array_equal(after[1], flags[1]) and np.all((after & ~np.uint8(2)) == (flags & ~np.uint8(2)))
    for e in (0, 2, 3):
        raised = (good[e] != 0) & np.isin(np.abs(atm[e]), [0.0, 1e-31])
        assert np.all(after[e, raised] & 2) and n_bad[e] == raised.sum()
        assert np.any((good[e] == 0) & (atm[e] == 0.0)) and np.any(np.isnan(atm[e]) & (good[e] != 0))
        assert np.any((good[e] != 0) & (atm[e] == 1e-30) & (after[e] == flags[e]) & (flags[e] & 2 == 0))


def check_conditions(kinds, times, quats, good, holes):
    face, cell0, failed, margin = oc.observe_conditions(kinds, times, quats, good)
    assert face >= 1e-9 and not cell0 and margin >= 1e-6
    if holes and failed.size >= 48:
        assert 1 <= failed.sum() <= failed.size // 4, (kinds, failed.sum(), failed.size)
    if not holes:
        assert failed.sum() == 0
    return failed


@pytest.mark.parametrize("entries", oc.OBSERVE_ENTRIES)
@pytest.mark.parametrize("n", oc.N_OBSERVE)
def test_observe_case_conditions(n, entries):
    times, quats, flags = oc.observe_case(n, entries)
    assert ac.BASE["tmin"] < times.min() and times.max() < ac.BASE["tmax"]
    for e in range(entries):
        good = oc.good_host(flags[e], None, n)
        assert good.sum() >= 0.6 * n
        for kinds in oc.OBSERVE_VOLUMES:
            check_conditions(kinds, times, quats[e], good, kinds != ("full",))


def test_two_pointings_conditions():
    t, quats = oc.two_pointings()
    times = np.array([t, t])
    face, cell0, failed, margin = oc.observe_conditions(("holes",), times, quats[:, 0], np.ones(2))
    assert face >= 1e-9 and not cell0 and margin >= 1e-2 and failed.tolist() == [True, False]


@pytest.mark.parametrize("view", oc.VIEW_FORMS)
def test_operator_case_conditions(view):
    inp = oc.operator_inputs()
    assert ac.BASE["tmin"] < inp["times"].min() and inp["times"].max() < ac.BASE["tmax"]
    assert len(oc.OP_DETS) == 4 and oc.OP_N == 600 and oc.OP_VIEWS == [(0, 257), (257, 600)]
    for variant in ("defaults", "no_det_flags", "no_shared_flags"):
        for first, last, kinds in oc.operator_views(view):
            for d in range(len(oc.OP_DETS)):
                good = oc.operator_good(variant, d, first, last)
                if variant != "no_det_flags" and d == oc.OP_WHOLLY_FLAGGED and (first, last) == oc.OP_VIEWS[0]:
                    assert not good.any()
                    continue
                assert good.sum() > 0.4 * good.size
                check_conditions(kinds, inp["times"][first:last], inp["quats"][d, first:last], good, True)


@pytest.mark.parametrize("view", oc.VIEW_FORMS)
@pytest.mark.parametrize("variant", list(oc.VARIANTS))
def test_restatements_against_the_host_path(variant, view):
    """good_host, flag_failed_host and finish_host chained as the device path chains its kernels give the flags of
    ``_observe_host`` exactly and its values within the rounding bound of k_atm_finish."""
    from toast_amd.data import defaults

    data, ob, detectors = oc.operator_data(variant)
    oc.operator_of(variant, view).apply(data, detectors=detectors, use_accel=False)
    oc.close_sims(data, ob)
    signal, flags, ld_signal, scale_i = oc.restated_operator(variant, view)
    got = ob.detdata[defaults.det_data].data
    inp = oc.operator_inputs(oc.VARIANTS[variant].get("nnz", 3))
    if flags is None:
        assert defaults.det_flags not in ob.detdata
    else:
        assert np.array_equal(ob.detdata[defaults.det_flags].data, flags)
        named = [oc.OP_DETS.index(d) for d in (detectors or oc.OP_DETS)]
        if "det_flags" not in oc.VARIANTS[variant].get("traits", {}):
            assert np.any(flags[named] != inp["det_flags"][named])            # a slab with holes raised some
    seen = scale_i > 0                                                           # good samples of the named detectors
    changed = got.view(np.uint64) != inp["signal"].view(np.uint64)
    assert not np.any(changed & ~seen) and changed.sum() > 0.5 * seen.sum()
    assert np.array_equal(changed, signal.view(np.uint64) != inp["signal"].view(np.uint64))
    err = np.abs(got.astype(oc.L) - ld_signal)[seen] / (oc.FINISH_ROUNDINGS * oc.EPS * scale_i[seen])
    same = int(np.sum(got.view(np.uint64) == signal.view(np.uint64)))
    print(f"{variant} view={view}: host path error / bound {float(err.max()):.3f}; {same} of {got.size} samples carry "
          f"the restatement's bits")
    assert err.max() <= 1.0
