#!/usr/bin/env python3
"""Generate tests/golden/poly2d.npz by RUNNING THE REFERENCE'S OWN kernel `filter_poly2D_numpy`
(src/toast/ops/polyfilter/kernels_numpy.py:86-97): this script parses the reference file where it lies, compiles only
that function from its syntax tree (decorator dropped, nothing copied into the repository) and calls it once per view
with the [n_samp][n_det] signals and masks the reference's operator builds (polyfilter.py:306-327).  The compiled
`filter_poly2D_solve` needs LAPACK, which the oracle build does not link; the NumPy kernel is the same DGELSS call
through `np.linalg.lstsq(..., rcond=1e-6)`.

The inputs are rebuilt by the tests from tests/poly2d_host.py (hash-generated), so the fixture holds, per case: the
flag seed, the templates, the reference kernel's output -- the coefficients of every (sample, group) inside the views --,
the systems left out of the value comparison (bit-packed) and the measured bounds.  The kernel's only output is the
coefficients; the filtered signal and the updated flags of the reference's operator follow from them by
polyfilter.py:345-381, which tests/poly2d_host.apply_coefficients restates -- storing them as well would take 2 MB more
than a committed file may have.

Exclusion: a system with an eigenvalue ratio in [0.5e-6, 2e-6] (SVD of A) may be solved at either rank and is left out
of the value comparison; at most 10 % of a case's systems, else the flag seed is raised and the masks are redrawn.
Bounds: 4 x max |reference - host emulation of the device algorithm| over the compared systems, for the filtered
signal, the fit T c and the coefficients; a filtered-signal bound above 1e-10 max|signal| fails the generator.
Build container only; the fixture is committed.

    python tests/golden/make_golden_poly2d.py
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/src/toast/ops/polyfilter/kernels_numpy.py"

import poly2d_host as P  # noqa: E402


def load_reference_kernel():
    tree = ast.parse(open(REF).read(), REF)
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "filter_poly2D_numpy"]
    assert len(funcs) == 1
    funcs[0].decorator_list = []      # @kernel(...)
    mod = ast.Module(body=funcs, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, REF, "exec"), ns)
    return ns["filter_poly2D_numpy"]


def reference_coefficients(kernel, case):
    coeff = np.zeros((case["n_samp"], case["n_group"], case["n_mode"]))
    for first, last in zip(case["starts"], case["stops"]):
        first, last = max(int(first), 0), min(int(last), case["n_samp"])
        signals, masks = P.reference_inputs(case, first, last)
        out = np.zeros((last - first, case["n_group"], case["n_mode"]))
        kernel(case["det_group"], case["templates"], signals, masks, out)
        coeff[first:last] = out
    return coeff


def measure(case, ref_coeff, excluded):
    """max |reference - emulation| over the compared systems: filtered signal, fit, coefficients."""
    ref_sig, ref_flags, ref_fit = P.apply_coefficients(case, ref_coeff)
    emu_sig, emu_flags, emu_coeff, _, sweeps = P.emulate(case)
    _, _, emu_fit = P.apply_coefficients(case, emu_coeff)
    assert np.array_equal(ref_flags, emu_flags), "the emulation flags other samples than the reference"
    cmp = P.compared(case, excluded)
    rows = case["sig_rows"]
    good = np.zeros_like(cmp)
    good[:, P.view_samples(case)] = P.good_mask(case)
    sel = cmp & good
    assert np.array_equal(np.isnan(ref_sig), np.isnan(emu_sig)) and np.array_equal(np.isnan(ref_sig), np.isnan(case["signal"]))
    d_sig = np.nanmax(np.abs(ref_sig[rows][sel] - emu_sig[rows][sel]))
    d_fit = np.max(np.abs(ref_fit[cmp] - emu_fit[cmp]))
    samples = P.view_samples(case)
    d_coeff = np.max(np.abs(ref_coeff[samples] - emu_coeff[samples])[~excluded])
    # everything that is not a good detector-sample inside a view keeps its bits, in both
    untouched = np.ones(case["signal"].shape, dtype=bool)
    untouched[np.ix_(rows, samples)] = ~P.good_mask(case)
    for got in (ref_sig, emu_sig):
        assert np.array_equal(got[untouched], case["signal"][untouched], equal_nan=True)
    return np.array([d_sig, d_fit, d_coeff]), sweeps


def main():
    kernel = load_reference_kernel()
    out = {}
    for name in P.CASES:
        seed = 8000 + 100 * list(P.CASES).index(name)
        while True:
            case = P.build_case(name, seed)
            excluded = P.excluded_systems(case)
            if np.mean(excluded) <= P.MAX_EXCLUDED:
                break
            seed += 10
        ref_coeff = reference_coefficients(kernel, case)
        samples = P.view_samples(case)
        # the engineered samples do what they are there for
        g0 = np.flatnonzero(case["det_group"] == 0)
        n_good = np.count_nonzero(P.good_mask(case, np.arange(case["n_samp"]))[g0], axis=0)
        assert n_good[P.S_GROUP_FLAGGED] == 0 and n_good[P.S_SHARED] == 0 and n_good[P.S_ONE_GOOD] == 1
        assert case["n_mode"] == 1 or 0 < n_good[P.S_FEW_GOOD] < case["n_mode"]
        for s in (P.S_GROUP_FLAGGED, P.S_SHARED, P.S_ZERO):
            assert np.all(ref_coeff[s, 0] == 0)
        assert np.any(ref_coeff[P.S_ONE_GOOD, 0] != 0) and np.all(np.isfinite(ref_coeff))
        diffs, sweeps = measure(case, ref_coeff, excluded)
        bounds = 4.0 * diffs
        smax = np.nanmax(np.abs(case["signal"]))
        assert bounds[0] <= 1e-10 * smax, (name, bounds, smax)
        print(f"{name}: seed {seed}, {excluded.size} systems, excluded {100 * np.mean(excluded):.2f} %, "
              f"Jacobi sweeps <= {sweeps}, bounds filtered {bounds[0]:.3e} fit {bounds[1]:.3e} coeff {bounds[2]:.3e}, "
              f"max|signal| {smax:.2f}")
        out[f"{name}_seed"] = np.array(seed)
        out[f"{name}_templates"] = case["templates"]
        out[f"{name}_coeff"] = ref_coeff[samples]
        out[f"{name}_excluded"] = np.packbits(excluded.astype(np.uint8).ravel())
        out[f"{name}_bounds"] = bounds
    # the NaN in a good sample: the reference is bypassed there (it would hand the NaN to LAPACK); the expected result is
    # the rule of the device entry: zero coefficients, flagged, signal untouched
    case = P.build_nan_case()
    s = P.NAN_CASE["sample"]
    clean = dict(case)
    clean["signal"] = case["signal"].copy()
    clean["signal"][P.NAN_CASE["det"], s] = 1.0
    ref_coeff = reference_coefficients(kernel, clean)
    ref_coeff[s] = 0.0
    diffs, _ = measure(case, ref_coeff, np.zeros((case["n_samp"], 1), dtype=bool))
    out["nan_coeff"] = ref_coeff
    out["nan_bounds"] = 4.0 * diffs
    print(f"nan case: bounds {out['nan_bounds']}")
    path = os.path.join(HERE, "poly2d.npz")
    np.savez_compressed(path, **out)
    z = np.load(path, allow_pickle=False)
    assert set(z.files) == set(out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
