#!/usr/bin/env python3
"""Generate tests/golden/poly_filter_edges.npz: the polynomial filter on ILL-CONDITIONED good-sample patterns, with a
high-precision truth.

Every case is one interval of one detector whose good samples form a contiguous stretch (or two): a leading stretch of
50 / 25 / 10 / 5 % of the interval, a middle or a trailing stretch of 10 %, 5 % at each end, and -- as a control --
90 % good at random, each at order 1, 3, 5, 8, 12 and 15, plus one interval of about 9000 samples that the path rule sends to
the two-pass kernels.  The bad samples are flagged partly in the shared flags, partly in the detector flags, partly in both.

Stored per case (the signal is rebuilt by the tests from tests/poly_filter_host.py):

* `truth`: the least-squares residual on ALL samples of the interval.  The templates are `poly_filter_host.legendre`
  evaluated in double -- they are the model --; only the solve runs in mpmath at 120 digits (normal equations: with
  cond(T)^2 <= 1e45 that leaves more than 60 correct digits).  Rounded to double.
* `ref`: what the reference's own NumPy kernel (src/toast/ops/polyfilter/kernels_numpy.py:10-83, parsed where it lies
  as in make_golden_poly_filter.py, called with inclusive stops) makes of the same input, and from it
  `ref_err_good` / `ref_err_all` = max |ref - truth| / max |signal| on the good / on all samples of the interval.
* `cond`: the 2-norm condition number of the templates restricted to the good samples.
* `cls`: bit 1 good-checked (ref_err_good <= 1e-9), bit 2 all-checked (good-checked and ref_err_all <= 1e-9), bit 4
  rank-deficient (cond >= 1e12 and not good-checked).  The caps are conditions on the cases, not tolerances: the
  reference alone decides the class, and the counts the tests rely on are asserted below.

* `op_*`: the operator-level case of tests/test_gpu_poly_filter_edges.py (`poly_filter_host.edge_operator_inputs`: a
  simulated ground observation, one detector with only the first 10 % of every throw good, order 5): the throws and
  `op_host_err_good`, the largest distance on the good samples of that detector between the double-precision
  `poly_filter_host.filter_polynomial` -- what the operator test compares with -- and the 120-digit solve.

Build container only (needs mpmath and the reference); the fixture is committed.

    python tests/golden/make_golden_poly_filter_edges.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import poly_filter_host as H  # noqa: E402
from make_golden_poly_filter import arange_ok, load_reference_kernel  # noqa: E402

ORDERS = (1, 3, 5, 8, 12, 15)
MASKS = ("lead50", "lead25", "lead10", "lead5", "mid10", "trail10", "ends5", "rand90")
SHARED_MASK, DET_MASK = 16, 7
GOOD, ALL, RANK = 1, 2, 4
CAP = 1e-9


def good_mask(name, length, seed):
    good = np.zeros(length, dtype=bool)
    if name.startswith("lead"):
        good[:int(round(length * int(name[4:]) / 100.0))] = True
    elif name == "mid10":
        good[int(0.45 * length):int(0.45 * length) + int(round(0.1 * length))] = True
    elif name == "trail10":
        good[length - int(round(0.1 * length)):] = True
    elif name == "ends5":
        w = int(round(0.05 * length))
        good[:w] = True
        good[length - w:] = True
    elif name == "rand90":
        good[:] = H.hashed_uniform(seed + 5000, length) < 0.9
    else:
        raise ValueError(name)
    return good


def split_flags(good, start, n_samp, seed):
    """Shared and detector flags whose union (under the masks) is exactly ~good inside the interval; bits outside the
    masks are set at random everywhere, and the samples outside the interval carry random masked bits too."""
    u = H.hashed_uniform(seed + 6000, n_samp)
    v = H.hashed_uniform(seed + 7000, n_samp)
    bad = v < 0.3                                   # outside the interval: anything
    bad[start:start + good.size] = ~good
    in_shared = bad & ((u < 0.4) | (u >= 0.8))
    in_det = bad & (u >= 0.4)
    shared = np.where(in_shared, 16, 0).astype(np.uint8) | np.where(v < 0.5, 2, 0).astype(np.uint8)
    det_bits = np.array([1, 2, 4, 3, 5, 6, 7], dtype=np.uint8)[(u * 7000).astype(np.int64) % 7]
    det = np.where(in_det, det_bits, 0).astype(np.uint8) | np.where(v > 0.6, 64, 0).astype(np.uint8)
    assert np.array_equal(H.combined_flags(shared, SHARED_MASK, det, DET_MASK)[start:start + good.size] == 0, good)
    assert np.any(in_shared & ~in_det) and np.any(in_det & ~in_shared)
    return shared, det


def mp_truth(templates, good, signal):
    """signal - T^T c on all samples, c the least-squares solution over the good samples, solved at 120 digits."""
    import mpmath as mp

    mp.mp.dps = 120
    n = templates.shape[0]
    tg = [[mp.mpf(float(v)) for v in templates[k][good]] for k in range(n)]
    sg = [mp.mpf(float(v)) for v in signal[good]]
    gram = mp.matrix(n, n)
    rhs = mp.matrix(n, 1)
    for r in range(n):
        for c in range(r, n):
            gram[r, c] = gram[c, r] = mp.fdot(tg[r], tg[c])
        rhs[r] = mp.fdot(tg[r], sg)
    coeff = mp.lu_solve(gram, rhs)
    # the solve kept its digits: the normal-equation residual is tiny against the right-hand side
    back = gram * coeff - rhs
    assert max(abs(back[r]) for r in range(n)) <= mp.mpf(10) ** -70 * max(abs(rhs[r]) for r in range(n))
    out = np.empty(signal.size)
    for i in range(signal.size):
        out[i] = float(mp.mpf(float(signal[i])) - mp.fsum(coeff[k] * mp.mpf(float(templates[k][i])) for k in range(n)))
    return out


def draw_length(rng, lo, hi):
    while True:
        length = int(rng.integers(lo, hi))
        if arange_ok(length):
            return length


def make_case(kernel, order, name, length, seed, rng):
    start = int(rng.integers(3, 40))
    n_samp = start + length + int(rng.integers(5, 30))
    row = int(rng.integers(0, 3))
    good = good_mask(name, length, seed)
    assert np.count_nonzero(good) > order + 1
    shared, det = split_flags(good, start, n_samp, seed)
    signal = H.poly_case_signals(seed, 3, n_samp)[row]
    seg = signal[start:start + length]
    templates = H.legendre(length, order + 1)
    truth = mp_truth(templates, good, seg)
    work = signal.copy()
    kernel(order, H.combined_flags(shared, SHARED_MASK, det, DET_MASK), [work], np.array([start]),
           np.array([start + length - 1]))
    assert np.array_equal(work[:start], signal[:start]) and np.array_equal(work[start + length:], signal[start + length:])
    ref = work[start:start + length]
    scale = np.max(np.abs(seg))
    err_good = float(np.max(np.abs(ref - truth)[good]) / scale)
    err_all = float(np.max(np.abs(ref - truth)) / scale)
    cond = float(np.linalg.cond(templates[:, good].T))
    cls = 0
    if err_good <= CAP:
        cls |= GOOD
        if err_all <= CAP:
            cls |= ALL
    elif cond >= 1e12:
        cls |= RANK
    print(f"order {order:2d} {name:8s} L {length:5d} good {np.count_nonzero(good):5d} cond {cond:8.1e} "
          f"ref_err good {err_good:8.1e} all {err_all:8.1e} class {cls}", flush=True)
    return dict(order=np.array(order), mask=np.array(MASKS.index(name)), seed=np.array(seed), n_samp=np.array(n_samp),
                start=np.array(start), stop=np.array(start + length), row=np.array(row), shared=shared, det=det,
                truth=truth, ref=ref, ref_err_good=np.array(err_good), ref_err_all=np.array(err_all), cond=np.array(cond),
                cls=np.array(cls))


def check_classes(cases):
    """The conditions the tests lean on (tests/test_poly_filter_host.py re-checks them from the committed file)."""
    cls = np.array([int(c["cls"]) for c in cases])
    cond = np.array([float(c["cond"]) for c in cases])
    good = (cls & GOOD) != 0
    both = (cls & ALL) != 0
    rank = (cls & RANK) != 0
    assert np.count_nonzero(good) >= 30
    assert np.count_nonzero(good & (cond >= 1e4)) >= 10
    assert np.count_nonzero(both & (cond >= 1e2)) >= 8
    assert np.count_nonzero(rank) >= 3 and not np.any(rank & good) and np.all(cond[rank] >= 1e12)
    for c in cases:
        if int(c["cls"]) & GOOD:
            assert float(c["ref_err_good"]) <= CAP
        if int(c["cls"]) & ALL:
            assert float(c["ref_err_all"]) <= CAP
    return int(np.count_nonzero(good)), int(np.count_nonzero(both)), int(np.count_nonzero(rank))


def operator_case():
    from toast_amd.sim import create_ground_data

    data = create_ground_data(**H.EDGE_OPERATOR_SIM)
    ob = data.obs[0]
    starts = np.array([iv.first for iv in ob.intervals["scanning"]], dtype=np.int64)
    stops = np.array([iv.last for iv in ob.intervals["scanning"]], dtype=np.int64)
    signal, det_flags = H.edge_operator_inputs(starts, stops, ob.n_local_samples)
    shared = np.array(ob.shared["flags"].data)
    shared_mask, det_mask = H.EDGE_OPERATOR_MASKS
    flags = H.combined_flags(shared, shared_mask, det_flags[H.EDGE_OPERATOR_DET], det_mask)
    row = signal[H.EDGE_OPERATOR_DET]
    host = row.copy()
    _, status = H.filter_polynomial(H.EDGE_OPERATOR_ORDER, flags, host, starts, stops)
    assert np.all(status == H.FITTED)
    worst = 0.0
    for a, b in zip(starts, stops):
        good = flags[a:b] == 0
        assert 0.08 * (b - a) <= np.count_nonzero(good) <= 0.1 * (b - a) and not np.any(good[int(0.1 * (b - a)) + 1:])
        truth = mp_truth(H.legendre(b - a, H.EDGE_OPERATOR_ORDER + 1), good, row[a:b])
        worst = max(worst, float(np.max(np.abs(host[a:b] - truth)[good]) / np.max(np.abs(row))))
    print(f"operator case: {starts.size} throws of {int(np.min(stops - starts))}-{int(np.max(stops - starts))} samples, "
          f"host restatement within {worst:.1e} of the truth on the good samples")
    assert worst <= CAP
    return {"op_starts": starts, "op_stops": stops, "op_host_err_good": np.array(worst)}


def main():
    kernel = load_reference_kernel()
    rng = np.random.default_rng(20261019)
    cases = []
    seed = 300
    for order in ORDERS:
        for name in MASKS:
            # 5 % of the interval must still hold more samples than terms; a few intervals of about 1500
            lo, hi = (1300, 1500) if (order, name) in ((3, "lead10"), (8, "ends5"), (15, "lead50")) else (400, 640)
            cases.append(make_case(kernel, order, name, draw_length(rng, lo, hi), seed, rng))
            seed += 10
    # longer than the single-pass stage cap (7424): the rule sends it to the two-pass kernels; 10 % = about 900 good samples
    cases.append(make_case(kernel, 5, "lead10", draw_length(rng, 8800, 9200), seed, rng))
    counts = check_classes(cases)
    print("good-checked %d, all-checked %d, rank-deficient %d of %d cases" % (counts + (len(cases),)))
    out = {"n_cases": np.array(len(cases)), "shared_mask": np.array(SHARED_MASK), "det_mask": np.array(DET_MASK)}
    for i, c in enumerate(cases):
        out.update({f"c{i}_{k}": v for k, v in c.items()})
    out.update(operator_case())
    path = os.path.join(HERE, "poly_filter_edges.npz")
    np.savez_compressed(path, **out)
    z = np.load(path, allow_pickle=False)
    assert set(z.files) == set(out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
