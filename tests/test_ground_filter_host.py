"""CPU: the yardstick of tests/test_gpu_ground_filter_grid.py (tests/ground_filter_case.py).

* The long double truth against the reference's compiled kernels (tests/golden/cov_filter.npz) and the oracle.
* The bound resolves one lost sample: an fp64 evaluation without one sample at a slice boundary is at least 100 bounds
  from the truth in every diagonal Gram entry and every projection whose template is non-zero there.
* The bound can be met: the oracle's NumPy fp64 evaluation (pairwise sums) lies inside it on every case of the grids.
"""
import numpy as np
import pytest

import golden_util as gu
import ground_filter_case as gc
from oracle import ground_filter as GF


def test_case_flags_have_bits_inside_and_outside_the_masks():
    case = gc.template_grid_case(23, "legendre", "random")
    common, det_bad = gc.masks_of(case)
    flags = case["flag_buffer"][case["flag_index"]]
    # good samples with a non-zero byte, bad samples with bits outside the mask: `flags != 0` is not `flags & mask`
    assert np.count_nonzero((flags != 0) & ~det_bad) > 0.9 * np.count_nonzero(~det_bad)
    assert np.count_nonzero(det_bad & ((flags & ~np.uint8(gc.DET_MASK)) != 0)) > 0
    assert np.count_nonzero(common & (case["shared_flags"] != 0)) > 0.9 * np.count_nonzero(common)
    assert abs(np.mean(~common) - gc.SHARED_FRACTION) < 0.01 and abs(np.mean(det_bad[0]) - gc.DET_FRACTION) < 0.01
    assert np.all(det_bad[gc.TEMPLATE_GRID_ALL[0]])
    d = gc.TEMPLATE_GRID_ONE_GOOD[0]
    assert np.count_nonzero(~det_bad[d]) == 1 and np.count_nonzero(~det_bad[d] & common) == 1
    assert not np.array_equal(case["signal_index"], case["flag_index"])
    assert not np.array_equal(case["signal_index"], np.arange(case["n_det"]))
    assert np.array_equal(case["signal_buffer"][case["signal_index"]], case["signal"])
    # nothing counts with mask 0 or without flags
    for kind in ("mask0", "none"):
        common, det_bad = gc.masks_of(gc.template_grid_case(23, "legendre", kind))
        assert np.all(common) and not np.any(det_bad)
    # the indicator / split kind has entries that are exactly zero, and others
    t = gc.cached_truth(gc.template_grid_case(8, "indicator", "random"))[0]
    assert np.count_nonzero(t["gram_common_norm"] == 0) >= 8 and np.count_nonzero(t["gram_common_norm"]) >= 8
    # the zero row of every detector, every row of the detector without a good sample
    assert np.count_nonzero(t["proj_norm"] == 0) >= gc.TEMPLATE_GRID_DETS + 7


def test_truth_against_reference_fixture_and_oracle():
    g = gu.load("cov_filter")
    templates = np.vstack([g["gf_trend"], g["gf_poly"]])
    sig, good = g["gf_signal"], g["gf_good"] != 0
    common = good[0] | good[1]
    det_bad = common[None, :] & ~good
    t = gc.truth_from_masks(templates, sig, common, det_bad)
    seq = gc.sequential_distance_from_masks(templates, sig, common, det_bad, t)
    # the reference's invcov of a detector is G - D_d; its norm is that of its own terms
    for d in range(2):
        want_i = t["gram_common"] - t["gram_flagged"][d]
        norm_i = t["gram_common_norm"] - t["gram_flagged_norm"][d]
        g1 = gc.truth_from_masks(templates, sig[d:d + 1], good[d], np.zeros((1, sig.shape[1]), dtype=bool))
        assert gc.distance(want_i, g1["gram_common"], g1["gram_common_norm"]) < 1e-18      # long double against long double: 2^-64 = 5e-20
        seq_i = gc.sequential_distance_from_masks(templates, sig[d:d + 1], good[d], np.zeros((1, sig.shape[1]), dtype=bool), g1)
        figures = dict(ref_proj=gc.distance(g[f"gf_proj{d}"], t["proj"][d], t["proj_norm"][d]),
                       ref_invcov=gc.distance(g[f"gf_invcov{d}"], g1["gram_common"], g1["gram_common_norm"]),
                       oracle_proj=gc.distance(GF.bin_proj(sig[d], templates, good[d]), t["proj"][d], t["proj_norm"][d]),
                       oracle_invcov=gc.distance(GF.bin_invcov(templates, good[d]), g1["gram_common"], g1["gram_common_norm"]))
        print(f"fixture detector {d}: {figures}; sequential {seq['proj']:.3e} (proj) {seq_i['gram_common']:.3e} (invcov)")
        # the compiled reference IS the sequential evaluation (up to how its compiler contracts the products)
        assert figures["ref_proj"] <= gc.FACTOR * seq["proj"] and figures["oracle_proj"] <= gc.FACTOR * seq["proj"]
        assert figures["ref_invcov"] <= gc.FACTOR * seq_i["gram_common"]
        assert figures["oracle_invcov"] <= gc.FACTOR * seq_i["gram_common"]
        assert np.max(np.abs(norm_i - g1["gram_common_norm"])) <= 1e-12 * np.max(norm_i)
        assert t["n_flagged"][d] == np.count_nonzero(common & ~good[d])
        got = gc.subtract_expected(sig[d], templates, g[f"gf_coeff{d}"], 3)
        assert np.array_equal(got, sig[d] - g[f"gf_fit{d}"])


def _largest_cases():
    return [gc.template_grid_case(65, "legendre", "random"), gc.length_grid_case(131149, 23), gc.nonfinite_case(32)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_bound_resolves_one_lost_edge_sample(which):
    """A kernel that loses the sample on either side of a slice boundary, or the last one, cannot pass."""
    case = _largest_cases()[which]
    n, nt, templates = case["n_samp"], case["n_template"], case["templates"]
    t, seq = gc.cached_truth(case)
    bound = gc.bounds(seq)
    common, det_bad = gc.masks_of(case)
    weakest = dict(gram=np.inf, proj=np.inf)
    for i in [e for e in gc.SLICE_EDGES if e < n] + [n - 1]:
        # the sample is good for everybody in the truth (its terms are added where the case has it bad) and left out of
        # the fp64 evaluation
        ti = templates[:, i].astype(gc.L)
        assert np.all(templates[:, i] != 0)
        extra = 0 if common[i] else 1
        want = np.diag(t["gram_common"]) + extra * ti * ti
        norm = np.diag(t["gram_common_norm"]) + extra * templates[:, i] ** 2
        without = common.copy()
        without[i] = False
        diag = np.array([np.sum((templates[r] * templates[r])[without]) for r in range(nt)])
        weakest["gram"] = min(weakest["gram"], float(np.min(np.abs(diag.astype(gc.L) - want) / norm)) / bound["gram_common"])
        for d in range(case["n_det"]):
            s_i = case["signal"][d, i]
            extra = 0 if (common[i] and not det_bad[d, i]) else 1
            want = t["proj"][d] + extra * ti * gc.L(s_i)
            norm = t["proj_norm"][d] + extra * np.abs(templates[:, i] * s_i)
            good = without & ~det_bad[d]
            p = np.array([np.sum((templates[r] * case["signal"][d])[good]) for r in range(nt)])
            weakest["proj"] = min(weakest["proj"], float(np.min(np.abs(p.astype(gc.L) - want) / norm)) / bound["proj"])
    print(f"n_samp {n}, n_template {nt}: one lost edge sample is at least {weakest['gram']:.3g} bounds (Gram diagonal), "
          f"{weakest['proj']:.3g} bounds (projections) from the truth")
    assert weakest["gram"] >= 100 and weakest["proj"] >= 100


def _check_reference_within_bound(case, label):
    """GF.bin_proj for every detector; GF.bin_invcov on the common mask and, as the sum over the flagged samples alone, on
    the flagged masks of four detectors (the python double loop of bin_invcov is what limits the number): the ones flagged
    everywhere / nearly everywhere and two with random flags."""
    t, seq = gc.cached_truth(case)
    bound = gc.bounds(seq)
    assert all(b < 1e-3 / case["n_samp"] for b in bound.values())
    common, det_bad = gc.masks_of(case)
    templates = case["templates"]
    figures = dict(proj=0.0, gram_flagged=0.0)
    for d in range(case["n_det"]):
        good = (common & ~det_bad[d]).astype(np.uint8)
        p = GF.bin_proj(np.where(good, case["signal"][d], 0.0), templates, good)
        figures["proj"] = max(figures["proj"], gc.distance(p, t["proj"][d], t["proj_norm"][d]))
    figures["gram_common"] = gc.distance(GF.bin_invcov(templates, common.astype(np.uint8)), t["gram_common"],
                                         t["gram_common_norm"])
    most = np.argsort(t["n_flagged"])[::-1]
    for d in sorted(set(most[:2]) | set(range(min(2, case["n_det"])))):
        flagged = (common & det_bad[d]).astype(np.uint8)
        figures["gram_flagged"] = max(figures["gram_flagged"], gc.distance(
            GF.bin_invcov(templates, flagged), t["gram_flagged"][d], t["gram_flagged_norm"][d]))
    print(f"{label}: " + ", ".join(f"{k} {figures[k]:.3e} / {bound[k]:.3e}" for k in sorted(bound)))
    for k in bound:
        assert figures[k] <= bound[k], (label, k)


@pytest.mark.parametrize("nt,kind,flag_kind", gc.template_grid())
def test_reference_within_bound_template_grid(nt, kind, flag_kind):
    _check_reference_within_bound(gc.template_grid_case(nt, kind, flag_kind), f"n_template {nt} {kind} {flag_kind}")


@pytest.mark.parametrize("n_samp", gc.SAMPLE_LENGTHS)
def test_reference_within_bound_length_grid(n_samp):
    for nt in gc.LENGTH_GRID_COUNTS:
        _check_reference_within_bound(gc.length_grid_case(n_samp, nt), f"n_samp {n_samp} n_template {nt}")


@pytest.mark.parametrize("nt", [8, 32])
def test_reference_within_bound_nonfinite_case(nt):
    _check_reference_within_bound(gc.nonfinite_case(nt), f"non-finite case n_template {nt}")
