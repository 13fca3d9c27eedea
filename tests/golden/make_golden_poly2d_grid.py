#!/usr/bin/env python3
"""Generate tests/golden/poly2d_grid.npz (edges_o0 .. edges_o2) and tests/golden/poly2d_grid_o3.npz (edges_o3) exactly as
tests/golden/make_golden_poly2d.py generates poly2d.npz: the reference's own kernel `filter_poly2D_numpy`
(src/toast/ops/polyfilter/kernels_numpy.py:86-97) is compiled from the syntax tree of the reference file where it lies --
nothing of it is copied -- and called once per view of the ``edges_o*`` cases of tests/focalplane_grid.py, whose inputs
the tests rebuild from hashes.  Per case the fixture holds the flag seed, the templates, the reference kernel's
coefficients inside the views, the bit-packed exclusion mask and the bounds 4 x max |reference - host emulation| for the
filtered signal, the fit and the coefficients.  The coefficients of the four cases together (1284 samples x 5 groups x
30 modes) do not fit one committed file, so order 3 has its own.

The sample with a NaN in a GOOD detector is not handed to the reference's kernel as it is (it would pass the NaN to
LAPACK): the kernel sees 1.0 there, and the expected coefficients of that one system are the rule of the device entry,
zeros -- as for the ``nan`` case of make_golden_poly2d.py.

The conditions of make_golden_poly2d.py hold: at most 10 % of a case's systems in the border band of eigenvalue ratios
(else the flag seed is raised), a filtered-signal bound above 1e-10 max|signal| fails the generator, every file stays
below 1 MB.  Build container only; the fixtures are committed.

    python tests/golden/make_golden_poly2d_grid.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import focalplane_grid as G  # noqa: E402
import make_golden_poly2d as M  # noqa: E402
import poly2d_host as P  # noqa: E402


def main():
    kernel = M.load_reference_kernel()
    files = {}
    for name, cfg in G.EDGE_CASES.items():
        seed = 8800 + 100 * cfg["order"]
        while True:
            case = G.build_edge_case(name, seed)
            excluded = P.excluded_systems(case)
            if np.mean(excluded) <= P.MAX_EXCLUDED:
                break
            seed += 10
        ref_coeff = M.reference_coefficients(kernel, G.nan_free(case))
        ref_coeff[G.E_NAN_GOOD, 0] = 0.0
        samples = P.view_samples(case)
        # the engineered samples do what they are there for
        g0 = np.flatnonzero(case["det_group"] == 0)
        n_good = np.count_nonzero(P.good_mask(case, np.arange(case["n_samp"]))[g0], axis=0)
        assert n_good[G.E_GROUP_FLAGGED] == 0 and n_good[G.E_SHARED] == 0 and n_good[G.E_ONE_GOOD] == 1
        assert case["n_mode"] == 1 or 0 < n_good[G.E_FEW_GOOD] < case["n_mode"]
        assert n_good[G.E_NAN_GOOD] == g0.size and n_good[G.E_NAN_FLAGGED] == g0.size - 1
        for s in (G.E_GROUP_FLAGGED, G.E_SHARED, G.E_ZERO):
            assert np.all(ref_coeff[s, 0] == 0)
        assert np.any(ref_coeff[G.E_ONE_GOOD, 0] != 0) and np.all(np.isfinite(ref_coeff))
        diffs, sweeps = M.measure(case, ref_coeff, excluded)
        bounds = 4.0 * diffs
        smax = np.nanmax(np.abs(case["signal"][case["sig_rows"]]))
        assert bounds[0] <= 1e-10 * smax, (name, bounds, smax)
        print(f"{name}: seed {seed}, {excluded.size} systems, excluded {100 * np.mean(excluded):.2f} %, "
              f"Jacobi sweeps <= {sweeps}, bounds filtered {bounds[0]:.3e} fit {bounds[1]:.3e} coeff {bounds[2]:.3e}, "
              f"max|signal| {smax:.2f}")
        out = files.setdefault(G.EDGE_FIXTURES[name], {})
        out[f"{name}_seed"] = np.array(seed)
        out[f"{name}_templates"] = case["templates"]
        out[f"{name}_coeff"] = ref_coeff[samples]
        out[f"{name}_excluded"] = np.packbits(excluded.astype(np.uint8).ravel())
        out[f"{name}_bounds"] = bounds
    for file, out in files.items():
        path = os.path.join(HERE, file)
        np.savez_compressed(path, **out)
        z = np.load(path, allow_pickle=False)
        assert set(z.files) == set(out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
