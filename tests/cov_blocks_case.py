"""Per-pixel covariance blocks at the numeric edges: the block families of tests/golden/cov_blocks.npz, a plain-double
emulation of k_cov_invert (toast_amd/csrc/kernels.hip), the two error figures and the check functions that
tests/test_cov_blocks_host.py runs on the emulation and tests/test_gpu_cov_blocks.py on the device.  NumPy only.

The fixture (tests/golden/make_golden_cov_blocks.py) holds, per nnz = 2, 3, 4 and per block: the packed upper triangle
as the doubles the kernel reads, and of THAT rounded matrix the eigenvalue extremes, rcond = emin / emax (0 when
emax <= 0, as in toast_map_cov.cpp:342) and the inverse from 50-digit arithmetic, rcond and the inverse as hi + lo pairs
of doubles; also what the NumPy ``eigh`` restatement of cov_eigendecompose_diag (make_golden_mapmaker.py) gave.

Error figures, both in units of eps = 2^-52:

* rcond:    |cond - rcond_true| / eps -- absolute, rcond is an eigenvalue error already divided by emax;
* inverse:  max_ij |X_ij - (A^-1)_ij| emin_true rcond_true / eps -- the error over eps kappa ||A^-1||_2, the form a
  backward-stable eigen-inverse obeys.

They are compared for blocks with rcond_true >= 1e-12.  ``ref_rc_err`` / ``ref_inv_err`` of the fixture are the largest
figures of the restatement; the code under test gets FACTOR = 4 times those (the margin test_gpu_noise_estim.py and
test_gpu_demod.py give a device algorithm over the reference's own distance from the truth: cyclic Jacobi and dsyev are
different algorithms with the same error form).  The band inside which a threshold decision may go either way is
4 ref_rc_err eps around the threshold.  A block that the code cut although its true rcond is above the threshold by less
than the band is in one of the two legal states and is left out of the inverse figure (its inverse is zero by design).

The ``subnormal`` block is left out of every figure: the squares of its entries underflow, so the kernel's sweep test sees
offn == 0 and takes the diagonal as it stands; only its two-state and neighbour properties are checked.  The NaN and inf
blocks are dense, as a sum of w w^T with one bad weight is: the rotations spread the NaN over the whole block and it is
cut.  (An exactly diagonal block with a NaN on its diagonal is never rotated; the kernel's emin / emax scan skips the NaN
and keeps the block.  A scatter cannot produce one, what dsyev makes of it cannot be established without LAPACK, and it is
not in the fixture.)"""
import os

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_blocks.npz")
NNZ = (2, 3, 4)
RCONDS = (1.0, 1e-1, 1e-2, 1e-4, 1e-6, 1e-8, 1e-10, 1e-12)
#: the thresholds the project and its tests use
TAUS = (1e-8, 1e-6, 1e-3, 1e-1)
MAIN_THRESHOLD = 1e-12
COMPARE_RCOND = 1e-12
FACTOR = 4
SIZES = (1, 255, 256, 257)
#: families whose blocks must come out as a zero block with cond == 0 for every positive threshold
DEAD = ("zero", "negative", "indefinite", "nan_offdiag", "nan_diag", "inf_diag", "inf_offdiag")
NO_FIGURE = ("subnormal",)


def blk(nnz):
    return nnz * (nnz + 1) // 2


def pack(full):
    iu = np.triu_indices(full.shape[-1])
    return np.ascontiguousarray(full[..., iu[0], iu[1]])


def unpack(packed, nnz):
    packed = np.asarray(packed)
    iu = np.triu_indices(nnz)
    full = np.zeros(packed.shape[:-1] + (nnz, nnz), dtype=packed.dtype)
    full[..., iu[0], iu[1]] = packed
    full[..., iu[1], iu[0]] = packed
    return full


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ block families
def random_orthogonal(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def rotated(rng, lam, scale=1.0):
    """Q diag(lam) Q^T x scale, symmetric to the bit."""
    q = random_orthogonal(rng, len(lam))
    a = (q * np.asarray(lam, dtype=np.float64)) @ q.T
    return 0.5 * (a + a.T) * scale


def spectrum(rng, nnz, rcond):
    """Eigenvalues from 1 down to rcond, the inner ones log-uniform between."""
    lam = np.ones(nnz)
    lam[-1] = rcond
    lam[1:-1] = rcond ** rng.random(nnz - 2)
    return lam


def conditioned(rng, nnz, per_level):
    out = []
    for rc in RCONDS:
        for _ in range(per_level):
            out.append((f"cond_{rc:.0e}", rotated(rng, spectrum(rng, nnz, rc), 10.0 ** rng.uniform(-6, 6))))
    return out


def scanning(rng, per_kind):
    """IQU blocks sum s w w^T, w = (1, eta cos 2 psi, eta sin 2 psi), added up in double as a scatter would."""
    def block(psi, s, eta):
        w = np.stack([np.ones_like(psi), eta * np.cos(2 * psi), eta * np.sin(2 * psi)], axis=1)
        acc = np.zeros((3, 3))
        for wi, si in zip(w, s):
            acc += (si * wi)[:, None] * wi[None, :]
        return 0.5 * (acc + acc.T)

    out = []
    for kind in ("scan_one_hit", "scan_one_angle", "scan_two_angles", "scan_close", "scan_spread"):
        for _ in range(per_kind):
            eta = rng.uniform(0.5, 1.0)
            scale = 10.0 ** rng.uniform(-3, 3)
            if kind == "scan_one_hit":
                psi = rng.uniform(0, np.pi, 1)
            elif kind == "scan_one_angle":
                psi = np.full(rng.integers(2, 30), rng.uniform(0, np.pi))
            elif kind == "scan_two_angles":
                two = rng.uniform(0, np.pi, 2)
                psi = two[rng.integers(0, 2, rng.integers(2, 30))]
                psi[:2] = two
            elif kind == "scan_close":
                psi = rng.uniform(0, np.pi) + 10.0 ** rng.uniform(-7, -1) * rng.random(rng.integers(3, 41))
            else:
                psi = rng.uniform(0, np.pi, rng.integers(3, 201))
            out.append((kind, block(psi, scale * rng.uniform(0.5, 2.0, psi.size), eta)))
    return out


def diagonal_exact(nnz):
    """diag(s, s/2.., s tau) with s a power of two: Jacobi does nothing and the kernel's rcond is tau to the bit; each
    paired with nextafter(tau, 0).  -> (family, block, tau, +1 at tau | -1 just below)"""
    out = []
    for tau in TAUS + (MAIN_THRESHOLD,):
        for j, e in enumerate((-20, -3, 0, 7, 30)):
            s = 2.0 ** e
            for t, side in ((tau, 1), (np.nextafter(tau, 0.0), -1)):
                d = np.full(nnz, 0.5 * s)
                d[j % nnz] = s * t
                d[(j + 1) % nnz] = s
                out.append(("diag_exact", np.diag(d), tau, side))
    return out


def ladders(rng, nnz, band):
    """Rotated blocks with rcond tau +- 8 band 2^k, k = 0..9 (tau (1 +- delta) with delta = 8 band 2^k / tau: the band is
    absolute in rcond, as the rcond figure is)."""
    out = []
    for tau in TAUS:
        for k in range(10):
            for sign in (1.0, -1.0):
                lam = spectrum(rng, nnz, tau + sign * 8.0 * band * 2.0 ** k)
                out.append(("ladder", rotated(rng, lam, 2.0 ** int(rng.integers(-10, 11))), tau, 0))
    return out


def degenerate(rng, nnz):
    """Every degenerate block between two ordinary ones (family ``spacer``)."""
    def good():
        return rotated(rng, spectrum(rng, nnz, 0.3), 10.0 ** rng.uniform(-2, 2))

    nan_off, nan_diag, inf_diag, inf_off = good(), good(), good(), good()
    nan_off[0, nnz - 1] = nan_off[nnz - 1, 0] = np.nan
    nan_diag[1, 1] = np.nan
    inf_diag[nnz - 1, nnz - 1] = np.inf
    inf_off[0, 1] = inf_off[1, 0] = np.inf
    tiny = np.diag(np.arange(1.0, nnz + 1)) * 3.0
    tiny[~np.eye(nnz, dtype=bool)] = 3.0e-200
    lam_ind = spectrum(rng, nnz, 0.2)
    lam_ind[-1] = -0.5
    bad = [("zero", np.zeros((nnz, nnz))), ("negative", -good()), ("indefinite", rotated(rng, lam_ind, 7.0)),
           ("nan_offdiag", nan_off), ("nan_diag", nan_diag), ("inf_diag", inf_diag), ("inf_offdiag", inf_off),
           ("tiny_offdiag", tiny), ("subnormal", good() * 1e-310)]
    out = [("spacer", good())]
    for b in bad:
        out += [b, ("spacer", good())]
    return out


# ------------------------------------------------------------------------------------------ the kernel in plain doubles
def jacobi_invert(packed, nnz, threshold, invert, sweeps=30, strict=False, update_v=True, swap=None, emin0=1.0e100):
    """k_cov_invert<nnz> on [n, blk] packed blocks in NumPy doubles: the same sweep test, rotation formulas, sweep cap,
    emin / emax scan, threshold test and packing, every product and sum rounded once (the library is built with
    -ffp-contract=off).  -> (data, cond).  The keyword arguments make the deliberately wrong variants of
    tests/test_cov_blocks_host.py: fewer sweeps, ``>`` for ``>=``, no eigenvector update, two packed entries swapped on
    the way in, another start value of emin."""
    src = np.array(packed, dtype=np.float64).reshape(-1, blk(nnz))
    n = src.shape[0]
    if nnz == 1:
        out = src.copy()
        if invert:
            nz = out[:, 0] != 0
            with np.errstate(all="ignore"):
                out[nz, 0] = 1.0 / out[nz, 0]
        return out, np.ones(n)
    load = src
    if swap is not None:
        load = src.copy()
        load[:, list(swap)] = src[:, list(swap)[::-1]]
    a = unpack(load, nnz)
    v = np.broadcast_to(np.eye(nnz), a.shape).copy()
    active = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            offn, diag = np.zeros(n), np.zeros(n)
            for k in range(nnz):
                diag = diag + a[:, k, k] * a[:, k, k]
                for m in range(k + 1, nnz):
                    offn = offn + a[:, k, m] * a[:, k, m]
            active &= ~((offn <= 1e-34 * diag) | (offn == 0.0))
            if not active.any():
                break
            for p in range(nnz - 1):
                for q in range(p + 1, nnz):
                    apq = a[:, p, q]
                    rot = (active & (apq != 0.0))[:, None]
                    theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    cs = (1.0 / np.sqrt(t * t + 1.0))[:, None]
                    sn = t[:, None] * cs
                    cp, cq = a[:, :, p].copy(), a[:, :, q].copy()
                    a[:, :, p] = np.where(rot, cs * cp - sn * cq, cp)
                    a[:, :, q] = np.where(rot, sn * cp + cs * cq, cq)
                    rp, rq = a[:, p, :].copy(), a[:, q, :].copy()
                    a[:, p, :] = np.where(rot, cs * rp - sn * rq, rp)
                    a[:, q, :] = np.where(rot, sn * rp + cs * rq, rq)
                    if update_v:
                        vp, vq = v[:, :, p].copy(), v[:, :, q].copy()
                        v[:, :, p] = np.where(rot, cs * vp - sn * vq, vp)
                        v[:, :, q] = np.where(rot, sn * vp + cs * vq, vq)
        emin, emax = np.full(n, emin0), np.zeros(n)
        for k in range(nnz):
            emin = np.where(a[:, k, k] < emin, a[:, k, k], emin)
            emax = np.where(a[:, k, k] > emax, a[:, k, k], emax)
        rc = np.where(emax > 0.0, emin / np.where(emax > 0.0, emax, 1.0), 0.0)
        ok = (rc > threshold) if strict else (rc >= threshold)
        out = src.copy()
        if invert:
            off = 0
            for k in range(nnz):
                for m in range(k, nnz):
                    acc = np.zeros(n)
                    for e in range(nnz):
                        acc = acc + v[:, k, e] * v[:, m, e] / a[:, e, e]
                    out[:, off] = np.where(ok, acc, 0.0)
                    off += 1
        return out, np.where(ok, rc, 0.0)


def emulation(nnz, **wrong):
    """The ``run(packed, threshold, invert) -> (data, cond)`` of the check functions, on the emulation."""
    return lambda packed, threshold, invert: jacobi_invert(packed, nnz, threshold, invert, **wrong)


# ------------------------------------------------------------------------------------------ fixture and figures
class Blocks:
    """The blocks of one nnz with their truth; arrays are read-only and shared by every test."""

    def __init__(self, z, nnz):
        self.nnz = nnz
        self.names = [str(s) for s in z["families"]]
        g = lambda key: z[f"{key}_{nnz}"]                                             # noqa: E731
        self.packed = g("packed")
        self.family = np.array([self.names[i] for i in g("family")])
        self.tau, self.side = g("tau"), g("side")
        self.emin, self.emax = g("emin"), g("emax")
        with np.errstate(invalid="ignore"):
            self.rc = g("rc_hi").astype(LD) + g("rc_lo").astype(LD)
            self.inv = g("inv_hi").astype(LD) + g("inv_lo").astype(LD)
        self.ref_cond, self.ref_inv = g("ref_cond"), g("ref_inv")
        self.ref_rc_err, self.ref_inv_err = float(z["ref_rc_err"]), float(z["ref_inv_err"])
        self.rc_bound, self.inv_bound = FACTOR * self.ref_rc_err, FACTOR * self.ref_inv_err
        self.band = FACTOR * self.ref_rc_err * EPS
        self.finite = np.isfinite(self.packed).all(axis=1)
        figured = self.finite & ~np.isin(self.family, NO_FIGURE)
        with np.errstate(invalid="ignore"):
            self.compared = figured & (self.rc >= COMPARE_RCOND)
        self.figured = figured
        self.n = self.packed.shape[0]
        for a in (self.packed, self.tau, self.side, self.emin, self.emax, self.rc, self.inv, self.ref_cond, self.ref_inv):
            a.setflags(write=False)

    def is_in(self, *families):
        return np.isin(self.family, families)

    def kinds(self):
        """Family groups of the printout: the conditioned blocks by level, the rest by family."""
        return [f for f in self.names if (self.family == f).any()]


_LOADED = {}


def load(nnz):
    if "z" not in _LOADED:
        _LOADED["z"] = np.load(FIXTURE)
    if nnz not in _LOADED:
        _LOADED[nnz] = Blocks(_LOADED["z"], nnz)
    return _LOADED[nnz]


def load_nnz1():
    """(values [n], family names [n]) of the 1 x 1 blocks."""
    if "z" not in _LOADED:
        _LOADED["z"] = np.load(FIXTURE)
    z = _LOADED["z"]
    names = [str(s) for s in z["families"]]
    return z["packed_1"], np.array([names[i] for i in z["family_1"]])


def rc_figure(cond, T):
    """|cond - rcond_true| / eps per block (nan where there is no truth)."""
    return np.asarray(np.abs(np.asarray(cond).astype(LD) - T.rc) / LD(EPS), dtype=np.float64)


def inv_figure(data, T):
    """max_ij |X_ij - (A^-1)_ij| emin rcond / eps per block (nan where there is no truth)."""
    err = np.abs(np.asarray(data).astype(LD) - T.inv).max(axis=1)
    return np.asarray(err * T.emin.astype(LD) * T.rc / LD(EPS), dtype=np.float64)


def per_family(T, sel, *figures):
    """[(family, count, largest of every figure)] over the selected blocks."""
    rows = []
    for f in T.kinds():
        m = sel & (T.family == f)
        if m.any():
            rows.append((f, int(m.sum())) + tuple(float(np.max(fig[m])) for fig in figures))
    return rows


def two_states(data, cond, threshold):
    """Per block: (kept, cut) -- kept: cond >= threshold (> 0 for threshold 0 is not asked); cut: cond == +0.0 and a block
    of +0.0."""
    cut = (bits(cond) == 0) & (bits(data) == 0).all(axis=1)
    with np.errstate(invalid="ignore"):
        kept = np.asarray(cond) >= threshold
    return kept, cut


# ------------------------------------------------------------------------------------------ checks
def check_inversion(run, T, label=""):
    """All families in one buffer, threshold 1e-12, invert: both figures within FACTOR x the restatement's.
    -> {family: (rcond figure, inverse figure)}."""
    data, cond = run(T.packed, MAIN_THRESHOLD, True)
    assert data.shape == T.packed.shape and cond.shape == (T.n,)
    kept, cut = two_states(data, cond, MAIN_THRESHOLD)
    above = np.asarray(T.rc - LD(MAIN_THRESHOLD) > LD(T.band))
    must_keep = T.compared & above
    in_band_cut = T.compared & ~above & cut
    sel = T.compared & ~in_band_cut
    rcf, invf = rc_figure(cond, T), inv_figure(data, T)
    out = {}
    for f, cnt, a, b in per_family(T, sel, rcf, invf):
        print(f"{label}nnz={T.nnz} invert {f:16s} n={cnt:3d}  rcond figure {a:8.3f} (bound {T.rc_bound:.3f})"
              f"  inverse figure {b:8.3f} (bound {T.inv_bound:.3f})")
        out[f] = (a, b)
    print(f"{label}nnz={T.nnz} invert: restatement {T.ref_rc_err:.3f} / {T.ref_inv_err:.3f}, "
          f"worst {np.max(rcf[sel]):.3f} / {np.max(invf[sel]):.3f}, {int(in_band_cut.sum())} cut inside the band")
    part = T.figured | T.is_in(*DEAD)
    assert (kept | cut)[part].all(), "a block is neither kept nor a zero block with cond 0"
    assert kept[must_keep].all(), "a block above the threshold by more than the band was cut"
    assert np.isfinite(data[sel]).all()
    assert np.max(rcf[sel]) <= T.rc_bound, ("rcond figure", float(np.max(rcf[sel])), T.rc_bound)
    assert np.max(invf[sel]) <= T.inv_bound, ("inverse figure", float(np.max(invf[sel])), T.inv_bound)
    return out


def check_rcond_only(run, T, label=""):
    """invert = 0 leaves the data alone and gives the cond of invert = 1; threshold 0 (covariance_rcond's call): every
    cond >= 0 and finite, exactly 0 where the true rcond is below -band, within the band of the truth elsewhere."""
    d0, c0 = run(T.packed, MAIN_THRESHOLD, False)
    _, c1 = run(T.packed, MAIN_THRESHOLD, True)
    assert same_bits(d0, T.packed), "invert = 0 wrote into the data"
    assert same_bits(c0, c1), "invert = 0 and invert = 1 disagree on cond"
    d, c = run(T.packed, 0.0, False)
    assert same_bits(d, T.packed)
    assert np.isfinite(c).all() and (c >= 0).all()
    below = T.figured & np.asarray(T.rc < -LD(T.band))
    assert (c[below] == 0.0).all(), "a block with a negative true rcond did not get cond 0"
    rest = T.figured & ~below
    rcf = rc_figure(c, T)
    for f, cnt, a in per_family(T, rest, rcf):
        print(f"{label}nnz={T.nnz} rcond-only threshold 0 {f:16s} n={cnt:3d}  rcond figure {a:8.3f} (bound {T.rc_bound:.3f})")
    assert np.max(rcf[rest]) <= T.rc_bound, ("rcond figure at threshold 0", float(np.max(rcf[rest])), T.rc_bound)
    return c


def check_threshold(run, T, tau, label=""):
    """Every block whose true rcond is off tau by more than the band takes the true decision; kept blocks are finite and
    pass the inverse bound, cut ones are zero with cond 0; blocks inside the band are in one of the two states; the
    diagonal blocks at exactly tau are kept, those at nextafter(tau, 0) cut.  -> (data, cond)"""
    data, cond = run(T.packed, tau, True)
    kept, cut = two_states(data, cond, tau)
    part = T.figured | T.is_in(*DEAD)
    assert (kept ^ cut)[part].all(), "a block is not in exactly one of the two states"
    dist = np.asarray(np.abs(T.rc - LD(tau)))
    decided = T.figured & (dist > T.band)
    want_kept = decided & np.asarray(T.rc >= LD(tau))
    want_cut = (decided & ~want_kept) | T.is_in(*DEAD)
    ladder = T.is_in("ladder") & (T.tau == tau)
    share = float(np.mean(~decided[ladder]))
    invf = inv_figure(data, T)
    worst = float(np.max(invf[want_kept]))
    print(f"{label}nnz={T.nnz} tau={tau:g}: {int(want_kept.sum())} kept, {int(want_cut.sum())} cut, "
          f"{int((T.figured & ~decided).sum())} inside the band ({share:.0%} of the ladder), "
          f"inverse figure of the kept {worst:.3f} (bound {T.inv_bound:.3f})")
    assert share <= 0.1
    assert kept[want_kept].all(), "a block above tau by more than the band was cut"
    assert cut[want_cut].all(), "a block below tau by more than the band (or a degenerate one) was kept"
    assert np.isfinite(data[want_kept]).all()
    assert worst <= T.inv_bound, ("inverse figure", worst, T.inv_bound)
    exact = T.is_in("diag_exact") & (T.tau == tau)
    assert (exact & (T.side == 1)).sum() >= 3 and (exact & (T.side == -1)).sum() >= 3
    at = exact & (T.side == 1)
    assert kept[at].all() and (cond[at] == tau).all(), "a diagonal block at exactly tau was cut (>= in the reference)"
    assert cut[exact & (T.side == -1)].all(), "a diagonal block at nextafter(tau, 0) was kept"
    return data, cond


def check_degenerate(run, T, full=None):
    """NaN, inf, zero, negative and indefinite blocks: a zero block and cond == 0 for a positive threshold; the blocks
    before and after every degenerate one have the bits they have when run alone."""
    data, cond = run(T.packed, MAIN_THRESHOLD, True) if full is None else full
    dead = T.is_in(*DEAD)
    assert dead.sum() >= len(DEAD)
    _, cut = two_states(data, cond, MAIN_THRESHOLD)
    assert cut[dead].all(), list(T.family[dead & ~cut])
    odd = np.flatnonzero(dead | T.is_in("tiny_offdiag", "subnormal"))
    for i in odd:
        for j in (i - 1, i + 1):
            assert T.family[j] == "spacer"
            d1, c1 = run(T.packed[j:j + 1], MAIN_THRESHOLD, True)
            assert same_bits(d1[0], data[j]) and same_bits(c1, cond[j:j + 1]), (T.family[i], j)
            assert c1[0] >= 0.25 and np.isfinite(d1).all()


def check_sizes(run, T, full=None):
    """n_px of 1, 255, 256 and 257: the bits of the same blocks in the whole buffer."""
    data, cond = run(T.packed, MAIN_THRESHOLD, True) if full is None else full
    assert T.n > max(SIZES)
    for n in SIZES:
        d, c = run(T.packed[:n], MAIN_THRESHOLD, True)
        assert same_bits(d, data[:n]) and same_bits(c, cond[:n]), n


def check_nnz1(run1):
    """nnz 1: cond == 1 everywhere, zero included, as in the reference; the data is the correctly rounded reciprocal,
    0 left 0; invert = 0 leaves the data alone."""
    vals, fam = load_nnz1()
    for f in ("one_positive", "one_negative", "one_zero", "one_nan"):
        assert (fam == f).any(), f
    x = vals.reshape(-1, 1)
    with np.errstate(all="ignore"):
        want = np.where(x != 0, 1.0 / np.where(x != 0, x, 1.0), x)
    num = ~np.isnan(want)

    def reciprocal(d, n):
        # (the payload of a NaN's reciprocal is the divider's business: a NaN is asked for, not its bits)
        return np.isnan(d[~num[:n]]).all() and same_bits(d[num[:n]], want[:n][num[:n]])

    for thr in (0.0, 1e-6):
        d, c = run1(x, thr, True)
        assert (c == 1.0).all()
        assert reciprocal(d, x.shape[0])
        d, c = run1(x, thr, False)
        assert (c == 1.0).all() and same_bits(d, x)
    assert x.shape[0] > max(SIZES)
    for n in SIZES:
        d, c = run1(x[:n], 1e-6, True)
        assert reciprocal(d, n) and (c == 1.0).all()


def check_all(run_of, label=""):
    """Every check above on ``run_of(nnz)``; -> {nnz: {family: (rcond figure, inverse figure)}}."""
    figures = {}
    for nnz in NNZ:
        T, run = load(nnz), run_of(nnz)
        figures[nnz] = check_inversion(run, T, label)
        check_rcond_only(run, T, label)
        for tau in TAUS:
            check_threshold(run, T, tau, label)
        check_degenerate(run, T)
        check_sizes(run, T)
    check_nnz1(run_of(1))
    return figures
