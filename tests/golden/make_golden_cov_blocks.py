#!/usr/bin/env python3
"""Generate tests/golden/cov_blocks.npz: per-pixel covariance blocks at the numeric edges with their truth from 50-digit
arithmetic (mpmath), for tests/test_cov_blocks_host.py and tests/test_gpu_cov_blocks.py.

Per nnz = 2, 3, 4 and per block (families: tests/cov_blocks_case.py): the packed upper triangle as the doubles the kernel
reads; of that rounded matrix emin, emax, rcond = emin / emax (0 when emax <= 0) from ``mpmath.eigsy`` and the inverse
from ``mpmath.inverse`` (blocks with rcond >= 1e-13; rcond and the inverse as hi + lo pairs of doubles); what the
reference restatement -- ``make_golden_mapmaker.cov_eigendecompose_diag``, NumPy ``eigh`` in place of LAPACK dsyev,
threshold 0 -- made of the block.  ``ref_rc_err`` / ``ref_inv_err`` are the restatement's largest error figures over all
compared blocks of all nnz; the tests give the code under test 4 x those.

The threshold ladders need the band (4 ref_rc_err eps) before they exist, so the figures are measured twice: over the
other families first, which places the rungs, then over everything, which is what is stored; the in-band share of the
ladders is asserted with the stored band.

Build container only (mpmath, oracle/_ref):      python tests/golden/make_golden_cov_blocks.py
"""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cov_blocks_case as C  # noqa: E402
import make_golden_mapmaker as mg  # noqa: E402

mpmath.mp.dps = 60
PER_LEVEL, PER_KIND, N_ONE = 40, 40, 30


def hi_lo(x):
    hi = float(x)
    return hi, float(x - mpmath.mpf(hi))


def truth(full):
    """(emin, emax, (rc_hi, rc_lo), inverse hi [blk], inverse lo [blk]) of one block; nan for a non-finite one."""
    nnz = full.shape[0]
    nanv = np.full(C.blk(nnz), np.nan)
    if not np.isfinite(full).all():
        return np.nan, np.nan, (np.nan, np.nan), nanv, nanv
    a = mpmath.matrix(full.tolist())
    ev = mpmath.eigsy(a, eigvals_only=True)
    emin, emax = min(ev), max(ev)
    rc = emin / emax if emax > 0 else mpmath.mpf(0)
    if rc < 1e-13:
        return float(emin), float(emax), hi_lo(rc), nanv, nanv
    inv = mpmath.inverse(a)
    pairs = [hi_lo(inv[k, m]) for k in range(nnz) for m in range(k, nnz)]
    return float(emin), float(emax), hi_lo(rc), np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def restatement(packed, nnz):
    """The reference restatement at threshold 0 on the finite blocks -> (cond, inverse); nan elsewhere."""
    ok = np.isfinite(packed).all(axis=1)
    data = np.ascontiguousarray(packed[ok]).reshape(-1)
    cond = np.zeros(int(ok.sum()))
    with np.errstate(all="ignore"):
        mg.cov_eigendecompose_diag(1, int(ok.sum()), nnz, data, cond, 0.0)
    ref_cond, ref_inv = np.full(packed.shape[0], np.nan), np.full(packed.shape, np.nan)
    ref_cond[ok], ref_inv[ok] = cond, data.reshape(-1, C.blk(nnz))
    return ref_cond, ref_inv


def arrays(nnz, entries):
    """Fixture arrays of one nnz from [(family, block[, tau, side])]."""
    names = sorted({e[0] for e in entries})
    packed = np.stack([C.pack(e[1]) for e in entries])
    t = [truth(C.unpack(p, nnz)) for p in packed]
    ref_cond, ref_inv = restatement(packed, nnz)
    return dict(packed=packed, family=[e[0] for e in entries], names=names,
                tau=np.array([e[2] if len(e) > 2 else np.nan for e in entries]),
                side=np.array([e[3] if len(e) > 2 else 0 for e in entries], dtype=np.int8),
                emin=np.array([x[0] for x in t]), emax=np.array([x[1] for x in t]),
                rc_hi=np.array([x[2][0] for x in t]), rc_lo=np.array([x[2][1] for x in t]),
                inv_hi=np.stack([x[3] for x in t]), inv_lo=np.stack([x[4] for x in t]), ref_cond=ref_cond, ref_inv=ref_inv)


def as_npz(per_nnz, nnz1, ref_rc_err, ref_inv_err):
    families = sorted({f for a in per_nnz.values() for f in a["names"]} | {f for f, _ in nnz1})
    z = dict(families=np.array(families), ref_rc_err=np.float64(ref_rc_err), ref_inv_err=np.float64(ref_inv_err),
             packed_1=np.array([v for _, v in nnz1]), family_1=np.array([families.index(f) for f, _ in nnz1], dtype=np.int16))
    for nnz, a in per_nnz.items():
        for key, val in a.items():
            if key == "family":
                val = np.array([families.index(f) for f in val], dtype=np.int16)
            if key != "names":
                z[f"{key}_{nnz}"] = val
    return z


class Mem:
    """What cov_blocks_case.Blocks reads of an npz, before there is a file."""

    def __init__(self, z):
        self.z = z

    def __getitem__(self, key):
        return np.array(self.z[key])


def ref_figures(per_nnz, nnz1):
    """The restatement's largest figures over the compared blocks of all nnz."""
    z = Mem(as_npz(per_nnz, nnz1, 1.0, 1.0))
    rc_err = inv_err = 0.0
    for nnz in per_nnz:
        T = C.Blocks(z, nnz)
        rc_err = max(rc_err, float(np.max(C.rc_figure(T.ref_cond, T)[T.compared])))
        inv_err = max(inv_err, float(np.max(C.inv_figure(T.ref_inv, T)[T.compared])))
    return rc_err, inv_err


def join(a, b):
    out = {}
    for key in a:
        if key == "names":
            out[key] = sorted(set(a[key]) | set(b[key]))
        elif key == "family":
            out[key] = a[key] + b[key]
        else:
            out[key] = np.concatenate([a[key], b[key]])
    return out


def main():
    rng = np.random.default_rng(20261019)
    scan = C.scanning(rng, PER_KIND)
    base = {}
    for nnz in C.NNZ:
        entries = C.conditioned(rng, nnz, PER_LEVEL)
        if nnz == 3:
            entries += scan
        elif nnz == 2:
            entries += [(f, b[1:, 1:].copy()) for f, b in scan]
        # the degenerate blocks in the middle of the buffer, the exactly decidable ones after them
        half = len(entries) // 2
        entries = entries[:half] + C.degenerate(rng, nnz) + entries[half:] + C.diagonal_exact(nnz)
        base[nnz] = arrays(nnz, entries)
        print(f"nnz={nnz}: {len(entries)} blocks before the ladders")
    nnz1 = [(f, float(b[0, 0])) for f, b in scan]
    for _ in range(N_ONE):
        x = 10.0 ** rng.uniform(-8, 8)
        nnz1 += [("one_positive", x), ("one_negative", -x * rng.uniform(0.5, 2.0)), ("one_zero", 0.0), ("one_nan", np.nan)]
    rc0, inv0 = ref_figures(base, nnz1)
    band0 = C.FACTOR * rc0 * C.EPS
    print(f"without the ladders: ref_rc_err {rc0:.3f}, ref_inv_err {inv0:.3f}; rungs from 8 x {band0:.3e}")
    every = {nnz: join(base[nnz], arrays(nnz, C.ladders(rng, nnz, band0))) for nnz in C.NNZ}
    ref_rc_err, ref_inv_err = ref_figures(every, nnz1)
    print(f"ref_rc_err {ref_rc_err:.3f}   ref_inv_err {ref_inv_err:.3f}   (restatement, all compared blocks, eps = 2^-52)")
    z = as_npz(every, nnz1, ref_rc_err, ref_inv_err)
    mem = Mem(z)
    for nnz in C.NNZ:
        T = C.Blocks(mem, nnz)
        data, cond = C.jacobi_invert(T.packed, nnz, 0.0, True)
        rcf, invf = C.rc_figure(cond, T), C.inv_figure(data, T)
        reff, refi = C.rc_figure(T.ref_cond, T), C.inv_figure(T.ref_inv, T)
        for f, cnt, a, b, c, d in C.per_family(T, T.compared, rcf, invf, reff, refi):
            print(f"nnz={nnz} {f:16s} n={cnt:3d}  emulation {a:7.3f} / {b:7.3f}   restatement {c:7.3f} / {d:7.3f}")
        for tau in C.TAUS:
            ladder = T.is_in("ladder") & (T.tau == tau)
            inside = np.asarray(np.abs(T.rc - C.LD(tau)) <= T.band) & ladder
            share = inside.sum() / ladder.sum()
            print(f"nnz={nnz} tau={tau:g}: {int(ladder.sum())} rungs, {share:.0%} inside the band of {T.band:.3e}")
            assert share <= 0.1
        # the exactly decidable blocks are what they say, to the bit
        exact = T.is_in("diag_exact")
        want = np.where(T.side == 1, T.tau, np.nextafter(T.tau, 0.0))
        assert np.array_equal((T.rc[exact]).astype(np.float64), want[exact])
    np.savez(C.FIXTURE, **z)
    print(f"{C.FIXTURE}: {os.path.getsize(C.FIXTURE)} bytes, "
          + ", ".join(f"nnz {n}: {every[n]['packed'].shape[0]} blocks" for n in C.NNZ) + f", nnz 1: {len(nnz1)}")


if __name__ == "__main__":
    main()
