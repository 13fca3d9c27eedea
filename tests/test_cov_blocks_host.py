"""CPU: the checks of tests/cov_blocks_case.py must pass on the faithful plain-double emulation of k_cov_invert and must
BITE -- each of five deliberately wrong emulations has to fail at least one assertion.  The same check functions run on
the device in tests/test_gpu_cov_blocks.py; nothing here runs a wrong kernel on a GPU.  With mpmath at hand the truth in
tests/golden/cov_blocks.npz, the stored figures of the reference restatement and the in-band share of the threshold
ladders are derived again from the fixture's own blocks."""
import numpy as np
import pytest

import cov_blocks_case as C


def test_fixture_holds_every_family():
    for nnz in C.NNZ:
        T = C.load(nnz)
        want = {f"cond_{rc:.0e}" for rc in C.RCONDS} | {"diag_exact", "ladder", "spacer", "tiny_offdiag", "subnormal"}
        want |= set(C.DEAD)
        if nnz < 4:
            want |= {"scan_one_hit", "scan_one_angle", "scan_two_angles", "scan_close", "scan_spread"}
        assert want <= set(T.family), want - set(T.family)
        assert T.n > max(C.SIZES) and T.compared.sum() > 200
        # rank-deficient scanning blocks are there in bulk, with a true rcond of rounding size and either sign
        if nnz == 3:
            thin = T.is_in("scan_one_hit", "scan_one_angle", "scan_two_angles")
            assert thin.sum() >= 100 and (np.abs(T.rc[thin]) < 1e-14).all()
        print(f"nnz={nnz}: {T.n} blocks, {int(T.compared.sum())} compared, ref_rc_err {T.ref_rc_err:.3f}, "
              f"ref_inv_err {T.ref_inv_err:.3f}, band {T.band:.3e}")


def test_checks_pass_on_the_faithful_emulation():
    figures = C.check_all(C.emulation, label="emulation ")
    for nnz, fam in figures.items():
        assert max(a for a, _ in fam.values()) <= C.load(nnz).rc_bound
        assert max(b for _, b in fam.values()) <= C.load(nnz).inv_bound


WRONG = {
    # (one rotation diagonalises a 2 x 2 block: a one-sweep cap is wrong from nnz 3 on)
    "one_sweep": ((3, 4), dict(sweeps=1)),
    "strict_threshold": (C.NNZ, dict(strict=True)),
    "no_eigenvector_update": (C.NNZ, dict(update_v=False)),
    "emin_from_zero": (C.NNZ, dict(emin0=0.0)),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_checks_fail_on_a_wrong_emulation(name):
    """Every nnz on its own: the wrong variant has to be caught at each nnz where it is wrong."""
    for nnz in WRONG[name][0]:
        T = C.load(nnz)
        run = C.emulation(nnz, **WRONG[name][1])
        with pytest.raises(AssertionError):
            C.check_inversion(run, T, label=f"{name} ")
            C.check_rcond_only(run, T, label=f"{name} ")
            for tau in C.TAUS:
                C.check_threshold(run, T, tau, label=f"{name} ")


def test_checks_fail_on_swapped_packed_entries():
    """Two packed entries of the nnz 4 block swapped on the way in ((0, 3) and (1, 1): neighbours in the packing)."""
    T = C.load(4)
    with pytest.raises(AssertionError):
        C.check_inversion(C.emulation(4, swap=(3, 4)), T, label="swapped ")


def test_strict_threshold_is_caught_by_the_exact_blocks_alone():
    """``>`` for ``>=`` changes nothing but the blocks at exactly tau: the figures pass, the decision check does not."""
    T = C.load(3)
    run = C.emulation(3, strict=True)
    C.check_inversion(run, T, label="strict ")
    with pytest.raises(AssertionError, match="exactly tau"):
        C.check_threshold(run, T, 1e-6, label="strict ")


def test_truth_and_reference_figures_rederived():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    rc_err = inv_err = 0.0
    for nnz in C.NNZ:
        T = C.load(nnz)
        full = C.unpack(T.packed, nnz)
        rc = np.full(T.n, np.nan, dtype=C.LD)
        inv = np.full(T.packed.shape, np.nan, dtype=C.LD)
        emin = np.full(T.n, np.nan)
        for i in np.flatnonzero(T.finite):
            a = mpmath.matrix(full[i].tolist())
            ev = mpmath.eigsy(a, eigvals_only=True)
            lo, hi = min(ev), max(ev)
            r = lo / hi if hi > 0 else mpmath.mpf(0)
            h = float(r)
            rc[i] = C.LD(h) + C.LD(float(r - mpmath.mpf(h)))
            emin[i] = float(lo)
            if T.compared[i]:
                x = mpmath.inverse(a)
                flat = [x[k, m] for k in range(nnz) for m in range(k, nnz)]
                for j, e in enumerate(flat):
                    h = float(e)
                    inv[i, j] = C.LD(h) + C.LD(float(e - mpmath.mpf(h)))
        fin = T.finite
        assert np.max(np.abs(rc[fin] - T.rc[fin])) <= 2.0 ** -60, "the stored rcond is not the truth"
        assert (np.abs(emin[fin] - T.emin[fin]) <= 1e-30 * np.abs(T.emax[fin])).all()
        cmp_ = T.compared
        assert np.max(np.abs(inv[cmp_] - T.inv[cmp_]) / np.abs(T.inv[cmp_]).max(axis=1, keepdims=True)) <= 2.0 ** -60
        rc_err = max(rc_err, float(np.max(np.abs(T.ref_cond[cmp_].astype(C.LD) - rc[cmp_]) / C.EPS)))
        err = np.abs(T.ref_inv[cmp_].astype(C.LD) - inv[cmp_]).max(axis=1)
        inv_err = max(inv_err, float(np.max(err * emin[cmp_] * rc[cmp_] / C.EPS)))
        for tau in C.TAUS:
            ladder = T.is_in("ladder") & (T.tau == tau)
            share = float(np.mean(np.abs(rc[ladder] - C.LD(tau)) <= T.band))
            print(f"nnz={nnz} tau={tau:g}: {share:.0%} of {int(ladder.sum())} rungs inside the band")
            assert share <= 0.1
    T = C.load(3)
    print(f"re-derived ref_rc_err {rc_err:.6f} (stored {T.ref_rc_err:.6f}), ref_inv_err {inv_err:.6f} "
          f"(stored {T.ref_inv_err:.6f})")
    assert abs(rc_err - T.ref_rc_err) <= 1e-9 * T.ref_rc_err
    assert abs(inv_err - T.ref_inv_err) <= 1e-9 * T.ref_inv_err
