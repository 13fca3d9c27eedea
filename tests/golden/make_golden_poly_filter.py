#!/usr/bin/env python3
"""Generate tests/golden/poly_filter.npz by RUNNING THE REFERENCE'S OWN kernels.

* `filter_polynomial_numpy` (src/toast/ops/polyfilter/kernels_numpy.py:10-83) is pure NumPy: this script parses the
  reference file where it lies, compiles only that function from its syntax tree (decorator dropped, nothing copied
  into the repository) and runs it once per detector with that detector's flag vector.  The NumPy kernel treats
  `stops` as INCLUSIVE while the compiled kernel -- the reference's default, which the device follows -- treats it as
  exclusive, so it is called with `stops - 1`; both then filter the same samples on the same x grid.  Its
  `np.arange` grid has one element too many for ~8 % of the interval lengths (a shape error), so the interval
  lengths are drawn among those where `arange` gives exactly L elements, and that is asserted.
* `sum_detectors` / `subtract_mean` come from the compiled reference bindings (oracle.load_ref()).

The inputs are rebuilt by the tests from tests/poly_filter_host.py (hash-generated doubles), so the fixture holds only
flags, interval lists and the reference's outputs.  Build container only; the fixture is committed.

    python tests/golden/make_golden_poly_filter.py
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/src/toast/ops/polyfilter/kernels_numpy.py"

import poly_filter_host as H  # noqa: E402


def load_reference_kernel():
    tree = ast.parse(open(REF).read(), REF)
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "filter_polynomial_numpy"]
    assert len(funcs) == 1
    funcs[0].decorator_list = []      # @kernel(...)
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, REF, "exec"), ns)
    return ns["filter_polynomial_numpy"]


def arange_ok(length):
    xstart, xstop, dx = (1.0 / length) - 1.0, (1.0 / length) + 1.0, 2.0 / length
    return np.arange(start=xstart, stop=xstop, step=dx).size == length


def draw_length(rng, lo, hi):
    while True:
        length = int(rng.integers(lo, hi))
        if arange_ok(length):
            return length


def poly_case(kernel, rng, order, n_det, n_samp, seed):
    # ragged intervals with gaps; the last one runs past n_samp and is clipped
    starts, stops = [], []
    cursor = int(rng.integers(0, 7))
    while True:
        length = draw_length(rng, 60, 420)
        if cursor + length + 40 >= n_samp:
            break
        starts.append(cursor)
        stops.append(cursor + length)
        cursor += length + int(rng.integers(0, 25))
    tail = n_samp - cursor
    assert tail > order + 1 and arange_ok(tail)
    starts.append(cursor)
    stops.append(n_samp + 13)
    starts, stops = np.array(starts, dtype=np.int64), np.array(stops, dtype=np.int64)
    dead = 2                       # an interval without a single good sample
    flags = (rng.random((n_det, n_samp)) < 0.10).astype(np.uint8)
    for d in range(n_det):
        for k in range(len(starts)):
            a, b = starts[k], min(stops[k], n_samp)
            if rng.random() < 0.5:          # a flagged block of up to 30 % of the interval
                w = int(rng.integers(1, max(2, int(0.3 * (b - a)))))
                o = int(rng.integers(a, b - w + 1))
                flags[d, o:o + w] = 1
        flags[d, starts[dead]:stops[dead]] = 1
    flags *= np.array([1, 2, 4, 1, 2, 4], dtype=np.uint8)[:n_det, None]     # any non-zero value counts
    for d in range(n_det):
        for k in range(len(starts)):
            if k != dead:
                a, b = starts[k], min(stops[k], n_samp)
                assert np.count_nonzero(flags[d, a:b] == 0) >= 0.5 * (b - a)
    signals = H.poly_case_signals(seed, n_det, n_samp)
    out = signals.copy()
    ref_stops = np.minimum(stops, n_samp) - 1           # inclusive stops for the NumPy kernel
    coeff = np.zeros((n_det, len(starts), order + 1))
    for d in range(n_det):
        row = out[d].copy()
        kernel(order, flags[d], [row], starts, ref_stops)
        out[d] = row
        # the reference's coefficients, recomputed the way it computes them (lstsq, rcond=-1)
        for k in range(len(starts)):
            a, b = starts[k], min(stops[k], n_samp)
            good = flags[d, a:b] == 0
            if not np.any(good):
                continue
            t = H.legendre(b - a, order + 1)
            coeff[d, k] = np.linalg.lstsq(t[:, good].T, signals[d, a:b][good], rcond=-1)[0]
            assert np.max(np.abs(signals[d, a:b] - coeff[d, k] @ t - out[d, a:b])) < 1e-9
    outside = np.ones(n_samp, dtype=bool)
    for a, b in zip(starts, stops):
        outside[a:b] = False
    assert np.array_equal(out[:, outside], signals[:, outside])
    assert np.array_equal(out[:, starts[dead]:stops[dead]], signals[:, starts[dead]:stops[dead]])
    return dict(order=np.array(order), seed=np.array(seed), n_det=np.array(n_det), n_samp=np.array(n_samp), starts=starts,
                stops=stops, dead=np.array(dead), flags=flags, out=out, coeff=coeff)


def common_mode_case(ref, rng):
    n_rows, n_flag_rows, n_det, n_samp, seed = 10, 9, 7, 23007, 77
    det_index = np.array([8, 1, 5, 0, 9, 3, 6], dtype=np.int64)      # permuted rows of larger buffers
    flag_index = np.array([2, 7, 0, 8, 4, 1, 5], dtype=np.int64)
    signals = H.common_mode_signals(seed, n_rows, n_samp)
    shared = ((rng.random(n_samp) < 0.05) * 1 + (rng.random(n_samp) < 0.05) * 4).astype(np.uint8)
    shared_mask = 1
    det_flags = ((rng.random((n_flag_rows, n_samp)) < 0.10) * 2 + (rng.random((n_flag_rows, n_samp)) < 0.10) * 8).astype(np.uint8)
    det_mask = 2
    nobody = 11111                 # a sample nobody hits: every listed detector flags it, the shared flag is clear
    shared[nobody] = 0
    det_flags[flag_index, nobody] = 2
    total = np.zeros(n_samp)
    hits = np.zeros(n_samp, dtype=np.int64)
    ref.sum_detectors(det_index, flag_index, shared, shared_mask, signals, det_flags, det_mask, total, hits)
    assert hits[nobody] == 0 and hits.max() == n_det
    summed = total.copy()
    out = signals.copy()
    ref.subtract_mean(det_index, out, total, hits)
    # the subtraction is one IEEE operation per sample: the tests rebuild the filtered signal from the mean
    want = signals.copy()
    want[det_index] -= total[None, :]
    assert np.array_equal(out, want)
    chk_sum, chk_hits = np.zeros(n_samp), np.zeros(n_samp, dtype=np.int64)
    H.sum_detectors(det_index, flag_index, shared, shared_mask, signals, det_flags, det_mask, chk_sum, chk_hits)
    assert np.array_equal(chk_sum, summed) and np.array_equal(chk_hits, hits)
    return dict(cm_seed=np.array(seed), cm_n_rows=np.array(n_rows), cm_det_index=det_index, cm_flag_index=flag_index,
                cm_shared=shared, cm_shared_mask=np.array(shared_mask), cm_det_flags=det_flags, cm_det_mask=np.array(det_mask),
                cm_sum=summed, cm_mean=total, cm_hits=hits, cm_nobody=np.array(nobody))


def main():
    import oracle

    ref = oracle.load_ref()
    assert ref is not None, "build oracle/_ref first"
    kernel = load_reference_kernel()
    rng = np.random.default_rng(20261016)
    out = {}
    cases = [(0, 4), (1, 5), (3, 6), (5, 4), (8, 5)]
    for i, (order, n_det) in enumerate(cases):
        case = poly_case(kernel, rng, order, n_det, 2400, seed=100 + i)
        out.update({f"p{i}_{k}": v for k, v in case.items()})
    out["n_poly_cases"] = np.array(len(cases))
    out.update(common_mode_case(ref, rng))
    path = os.path.join(HERE, "poly_filter.npz")
    np.savez_compressed(path, **out)
    z = np.load(path, allow_pickle=False)
    assert set(z.files) == set(out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
