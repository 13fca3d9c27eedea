"""Plain statements of the SubHarmonic and Periodic template operations (csrc/template_basis.hip) on bare arrays, with
rounding bounds that are derived and not measured.  NumPy and ``math.fsum`` only: no device, no oracle, nothing of
``toast_amd.templates``.  Shared by tests/test_templates_reference_host.py (the reference itself is held to the fixture of
the reference implementation and to the host path) and tests/test_gpu_templates_grid.py (the HIP kernels at every term
count and bin path).

Conventions: ``signal`` / ``flags`` are [n_row][n_samp] buffers, ``rows[d]`` names the row of detector ``d``; ``views`` is
a list of (first, last) sample ranges, clipped to [0, n_samp) here as the library clips them.

Exact and bit-exact results
  * ``basis``: the fp64 Legendre rows as the kernels state them: ``np.linspace(-1, 1, length)`` and the recurrence
    ``(((2k - 1) r) T[k-1] - (k - 1) T[k-2]) / k`` with a true division.  Lengths 1 and 2 follow ``linspace``.
  * ``subharmonic_add``, ``periodic_add``: one rounding per product and per addition, ascending order: bit-exact.
  * ``periodic_index``, ``periodic_hits``: integers: exact.

Sums (``Sums``): the exact value of a sum of fp64 terms is held as an unevaluated pair hi + lo (``math.fsum`` of the terms
and ``math.fsum`` of the terms and -hi: what is left is below 2^-105 of the sum), next to S = sum |terms| and the term
count m.  The terms are the ROUNDED products (``signal_i * T_k(r_i)``, ``T_r T_c``): the library is built with
-ffp-contract=off and rounds every product once, to the same double, so the products add nothing to a bound.

Bounds, with u = 2^-53 and gamma(k) = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, §4.2: a sum
of m floating-point numbers taken in ANY order -- sequential, pairwise, butterflies, partial sums per chunk -- has
m - 1 additions on the path of every term, so it deviates from the exact sum by at most gamma(m - 1) S; additions of an
exact zero are exact and do not count):
  * SubHarmonic ``project_signal``: an amplitude is the sum of the m products of its view: gamma(m - 1) S.  One sample: exact.
  * SubHarmonic Gram matrix: the sum of m products, then one multiplication by the detector weight:
    (1 + theta_{m-1})(1 + delta) = 1 + theta_m: gamma(m) S w.
  * SubHarmonic ``apply_precond``: n products rounded once each and n - 1 additions (the first is onto 0.0): gamma(n)
    sum_c |P_rc x_c|.
  * Periodic ``project_signal``: what the amplitude held plus m samples, m + 1 values, m additions: gamma(m) (|a0| + S).  A
    bin without a term keeps its bits.
These bounds are loose for a tree sum (a butterfly's own bound is about gamma(log2 m)), and they are still at least eight
orders of magnitude below what one lost or doubled sample does to a sum (about S / m: m gamma(m) < 2e-7 for the 4e4
samples the tests use).  That is their purpose: any order of summation passes, any other set of terms does not.
"""
import math
from collections import namedtuple
from itertools import chain

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble has to be wider than a double for these references"
U = 2.0 ** -53

#: hi + lo: the exact sum; S: the sum of the magnitudes of the terms; m: the number of terms (arrays of one shape)
Sums = namedtuple("Sums", "hi lo S m")


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (1 - k * LD(U))


def exact_sum(terms):
    """(hi, lo, S) of a sequence of doubles."""
    terms = [float(t) for t in terms]
    hi = math.fsum(terms)
    lo = math.fsum(chain(terms, (-hi,)))
    return hi, lo, math.fsum(abs(t) for t in terms)


def deviation(got, sums):
    """|got - exact| as long doubles."""
    return np.abs((np.asarray(got, dtype=LD) - np.asarray(sums.hi, dtype=LD)) - np.asarray(sums.lo, dtype=LD))


def fraction_of(err, bound):
    """err / bound elementwise; where the bound is 0 the value must be exact: 0 or inf."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    safe = np.where(bound > 0, bound, 1)
    return np.where(bound > 0, err / safe, np.where(err == 0, LD(0), LD(np.inf)))


def clip_views(views, n_samp):
    return [(max(int(f), 0), min(int(l), int(n_samp))) for f, l in views]


# ------------------------------------------------------------------------------------ SubHarmonic
def basis(norder, length, dtype=np.float64):
    """[norder][length] Legendre rows of one view."""
    t = np.zeros((norder, length), dtype=dtype)
    r = np.linspace(dtype(-1.0), dtype(1.0), length, dtype=dtype)
    for k in range(norder):
        if k == 0:
            t[k] = 1
        elif k == 1:
            t[k] = r
        else:
            t[k] = ((2 * k - 1) * r * t[k - 1] - (k - 1) * t[k - 2]) / k
    return t


def subharmonic_add(signal, rows, offs, amps, views, norder):
    """signal[rows[d]][view] += sum_k T_k amps[offs[d] + view * norder + k], ascending k -> a new array."""
    out = np.array(signal, dtype=np.float64, copy=True)
    for d, row in enumerate(rows):
        for v, (first, last) in enumerate(clip_views(views, out.shape[1])):
            if last <= first:
                continue
            t = basis(norder, last - first)
            a = amps[offs[d] + v * norder:][:norder]
            for k in range(norder):
                out[row, first:last] += t[k] * a[k]
    return out


def subharmonic_project(signal, rows, views, norder):
    """Sums [n_det][n_view][norder] of signal_i T_k(r_i) over ALL samples of a view (no flags)."""
    views = clip_views(views, signal.shape[1])
    shape = (len(rows), len(views), norder)
    hi, lo, S, m = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    for v, (first, last) in enumerate(views):
        if last <= first:
            continue
        t = basis(norder, last - first)
        for d, row in enumerate(rows):
            for k in range(norder):
                hi[d, v, k], lo[d, v, k], S[d, v, k] = exact_sum(signal[row, first:last] * t[k])
            m[d, v] = last - first
    return Sums(hi, lo, S, m)


def subharmonic_gram(flags, flag_rows, mask, weights, views, norder):
    """(Sums [n_det][n_view][norder][norder] of T_r T_c over the unflagged samples -- unweighted: hi, lo and S are
    multiplied by the weight where they are compared, see ``gram_check`` --, ngood [n_det][n_view])."""
    n_samp = flags.shape[1] if flags is not None else max(int(l) for _, l in views)
    views = clip_views(views, n_samp)
    n_det = len(weights)
    shape = (n_det, len(views), norder, norder)
    hi, lo, S, m = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    ngood = np.zeros((n_det, len(views)), dtype=np.int64)
    for v, (first, last) in enumerate(views):
        if last <= first:
            continue
        t = basis(norder, last - first)
        for d in range(n_det):
            good = np.ones(last - first, dtype=bool)
            if flags is not None:
                good = (flags[flag_rows[d], first:last] & mask) == 0
            ngood[d, v] = np.count_nonzero(good)
            for r in range(norder):
                for c in range(r, norder):
                    e = exact_sum(t[r][good] * t[c][good])
                    for arr, x in zip((hi, lo, S), e):
                        arr[d, v, r, c] = arr[d, v, c, r] = x
            m[d, v] = ngood[d, v]
    return Sums(hi, lo, S, m), ngood


def gram_check(got, sums, weights):
    """(|got - exact sum * weight|, gamma(m) S w) for Gram matrices [n_det][n_view][n][n]."""
    w = np.asarray(weights, dtype=LD)[:, None, None, None]
    err = np.abs(np.asarray(got, dtype=LD) - (np.asarray(sums.hi, dtype=LD) + np.asarray(sums.lo, dtype=LD)) * w)
    return err, gamma(sums.m) * np.asarray(sums.S, dtype=LD) * np.abs(w)


def subharmonic_precond(precond, amp_in):
    """(P x, gamma(n) sum_c |P_rc x_c|) per block as long doubles: precond [n_block][n][n], amp_in [n_block * n]."""
    p = np.asarray(precond, dtype=LD)
    x = np.asarray(amp_in, dtype=LD).reshape(p.shape[0], 1, p.shape[1])
    prod = p * x
    return prod.sum(axis=2).reshape(-1), (gamma(p.shape[1]) * np.abs(prod).sum(axis=2)).reshape(-1)


# ------------------------------------------------------------------------------------ Periodic
def periodic_index(key, flags, mask, views, obs_min, incr, nbins):
    """int32 [n_row][n_samp]: ((key - obs_min) / incr) truncated and clamped to nbins - 1 for the samples of the views
    whose ``flags & mask`` is clear; -1 elsewhere.  Also returns how many values the clamp changed."""
    index = np.full(key.shape, -1, dtype=np.int32)
    clamped = 0
    for first, last in clip_views(views, key.shape[1]):
        if last <= first:
            continue
        b = ((key[:, first:last] - obs_min) / incr).astype(np.int32)
        clamped += int(np.count_nonzero(b >= nbins))
        b[b >= nbins] = nbins - 1
        if flags is not None:
            b[(flags[:, first:last] & mask) != 0] = -1
        index[:, first:last] = b
    return index, clamped


def periodic_takes_part(index, index_rows, flags, flag_rows, mask, nbins, n_det):
    """(bins [n_det][n_samp], good [n_det][n_samp]): a sample takes part when 0 <= index < nbins and its detector flag is
    clear."""
    bins = np.stack([index[index_rows[d] if index_rows is not None else 0] for d in range(n_det)])
    good = (bins >= 0) & (bins < nbins)
    if flags is not None:
        good &= np.stack([(flags[flag_rows[d]] & mask) == 0 for d in range(n_det)])
    return bins, good


def periodic_hits(index, index_rows, flags, flag_rows, mask, nbins, n_det, first, last):
    """int64 [n_det][nbins]: the samples of [first, last) that take part, per bin."""
    bins, good = periodic_takes_part(index, index_rows, flags, flag_rows, mask, nbins, n_det)
    first, last = max(first, 0), min(last, bins.shape[1])
    hits = np.zeros((n_det, nbins), dtype=np.int64)
    for d in range(n_det):
        if last > first:
            hits[d] = np.bincount(bins[d, first:last][good[d, first:last]], minlength=nbins)
    return hits


def periodic_add(signal, rows, index, index_rows, amps, nbins):
    """signal[rows[d]][i] += amps[d][index[i]] where the index is a bin (the key's flags only) -> a new array."""
    out = np.array(signal, dtype=np.float64, copy=True)
    bins, good = periodic_takes_part(index, index_rows, None, None, 0, nbins, len(rows))
    for d, row in enumerate(rows):
        out[row, good[d]] += amps[d][bins[d, good[d]]]
    return out


def periodic_project(signal, rows, index, index_rows, flags, flag_rows, mask, nbins, a0):
    """Sums [n_det][nbins] of a0 and the samples that take part; S and m count the samples only.  Also returns, per
    sample, whether it took part."""
    n_det = len(rows)
    bins, good = periodic_takes_part(index, index_rows, flags, flag_rows, mask, nbins, n_det)
    shape = (n_det, nbins)
    hi, lo, S, m = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64)
    for d, row in enumerate(rows):
        b = bins[d, good[d]]
        s = signal[row, good[d]]
        order = np.argsort(b, kind="stable")
        b, s = b[order], s[order]
        edges = np.searchsorted(b, np.arange(nbins + 1))
        s = s.tolist()
        for k in range(nbins):
            terms = s[edges[k]:edges[k + 1]]
            m[d, k] = len(terms)
            if len(terms) == 0:
                hi[d, k] = a0[d][k]
                continue
            hi[d, k], lo[d, k], _ = exact_sum([float(a0[d][k])] + terms)
            S[d, k] = math.fsum(abs(t) for t in terms)
    return Sums(hi, lo, S, m), good


def periodic_bound(sums, a0):
    return gamma(sums.m) * (np.abs(np.asarray(a0, dtype=LD)) + np.asarray(sums.S, dtype=LD))


# ------------------------------------------------------------------------------------ inputs of the grid tests
# One SubHarmonic layout for every term count: three detectors in a buffer of four rows of odd length (odd rows start on an
# odd double), the unused row 1 and the amplitude slots between the detectors' blocks hold SENTINEL.  View lengths sit on
# the wave (64) and on the reduction chunk (4096) and span three chunks (8193); one view is empty; starts are odd and even.
SENTINEL = -7.25e9
DET_MASK = 1
SUBH = dict(n_samp=24001, n_row=4, rows=(2, 0, 3), flag_rows=(1, 3, 0), weights=(1.0, 0.5, 3.0),
            views=((0, 1), (3, 5), (6, 9), (11, 74), (80, 80), (81, 145), (150, 215), (217, 4312), (4314, 8410),
                   (8411, 12508), (12510, 20703), (23990, 24001)),
            empty_view=4, flagged=(1, 5), block_order=(2, 0, 1), lead=3, gap=5)
SUBH_MAX_TERMS = 9
PERIODIC_CHUNK = 16384
PERIODIC_LDS_BINS = 1024

_CACHE = {}


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)


def subharmonic_grid():
    """The SubHarmonic inputs with the references at 9 terms, computed once: the values for n < 9 terms are the leading
    entries (the basis rows do not depend on the term count).  Callers must not write into it."""
    if "subh" not in _CACHE:
        cfg = SUBH
        rng = np.random.default_rng(4101)
        n_samp, n_row = cfg["n_samp"], cfg["n_row"]
        signal = rng.standard_normal((n_row, n_samp)) + 0.25
        signal[1] = SENTINEL
        flags = ((rng.random((n_row, n_samp)) < 0.3).astype(np.uint8) * DET_MASK) | \
            ((rng.random((n_row, n_samp)) < 0.2).astype(np.uint8) * 4) | 2
        d, v = cfg["flagged"]
        first, last = cfg["views"][v]
        flags[cfg["flag_rows"][d], first:last] |= DET_MASK
        project = subharmonic_project(signal, cfg["rows"], cfg["views"], SUBH_MAX_TERMS)
        gram, ngood = subharmonic_gram(flags, cfg["flag_rows"], DET_MASK, cfg["weights"], cfg["views"], SUBH_MAX_TERMS)
        _readonly(signal, flags, ngood, *project, *gram)
        _CACHE["subh"] = dict(cfg, signal=signal, flags=flags, project=project, gram=gram, ngood=ngood)
    return _CACHE["subh"]


def subharmonic_offsets(norder):
    """(amp_offsets of the three detectors, size of the amplitude buffer): blocks in another order than the rows, ``lead``
    unused slots in front and ``gap`` after every block."""
    block = len(SUBH["views"]) * norder
    offs = np.array([SUBH["lead"] + b * (block + SUBH["gap"]) for b in SUBH["block_order"]], dtype=np.int64)
    return offs, SUBH["lead"] + 3 * (block + SUBH["gap"])


def used_slots(offs, block, size):
    used = np.zeros(size, dtype=bool)
    for o in offs:
        used[o:o + block] = True
    return used


# Periodic sweeps: three chunks of 16384 samples, the last one partial, odd rows.
SWEEP = dict(n_samp=40001, n_row=4, rows=(2, 0, 3), flag_rows=(1, 3, 0), block_order=(1, 2, 0), lead=3, gap=5,
             index_rows=(2, 0, 1), period=9973.0)
SWEEP_NBINS = (1, 7, 255, 256, 257, 1024, 1025, 5000)
SWEEP_PATTERNS = ("sweep", "random", "single")
SWEEP_MODES = ("shared", "per_detector")


def periodic_offsets(nbins):
    offs = np.array([SWEEP["lead"] + b * (nbins + SWEEP["gap"]) for b in SWEEP["block_order"]], dtype=np.int64)
    return offs, SWEEP["lead"] + 3 * (nbins + SWEEP["gap"])


def sweep_index(nbins, pattern, mode, seed):
    """Hand-built int32 index rows [1 or 3][n_samp]: ``sweep`` a slow sine (one or two bins per 64 samples up to some
    tens of bins; with more bins the same sine crosses proportionally more, or it could not reach half of them in 626
    wave steps), ``random`` uniform bins, ``single`` the last bin.  About 10 % of the entries are -1 and about 2 % are no
    bins of the call: nbins, nbins + 5, 2^31 - 1."""
    rng = np.random.default_rng(seed)
    n_samp = SWEEP["n_samp"]
    n_irow = 3 if mode == "per_detector" else 1
    i = np.arange(n_samp)
    index = np.empty((n_irow, n_samp), dtype=np.int32)
    for r in range(n_irow):
        if pattern == "sweep":
            x = 0.5 + 0.5 * np.sin(2.0 * np.pi * (i + 777.0 * r) / SWEEP["period"])
            index[r] = np.minimum((x * nbins).astype(np.int64), nbins - 1)
        elif pattern == "random":
            index[r] = rng.integers(0, nbins, n_samp)
        else:
            index[r] = nbins - 1
    pure = index.copy()
    draw = rng.random(index.shape)
    index[draw < 0.10] = -1
    junk = np.array([nbins, nbins + 5, 2 ** 31 - 1], dtype=np.int64)[rng.integers(0, 3, index.shape)].astype(np.int32)
    index = np.where(draw > 0.98, junk, index)
    return index, pure


def periodic_sweep(nbins, pattern, mode, seed=None):
    """Inputs and references of one sweep case, computed once.  Callers must not write into it."""
    key = (nbins, pattern, mode)
    if key not in _CACHE:
        cfg = SWEEP
        if seed is None:
            seed = 5200 + 17 * SWEEP_NBINS.index(nbins) + 5 * SWEEP_PATTERNS.index(pattern) + SWEEP_MODES.index(mode)
        rng = np.random.default_rng(seed)
        n_samp, n_row = cfg["n_samp"], cfg["n_row"]
        index, pure = sweep_index(nbins, pattern, mode, seed + 1000)
        index_rows = cfg["index_rows"] if mode == "per_detector" else None
        signal = rng.standard_normal((n_row, n_samp)) + 0.25
        signal[1] = SENTINEL
        flags = ((rng.random((n_row, n_samp)) < 0.3).astype(np.uint8) * DET_MASK) | \
            ((rng.random((n_row, n_samp)) < 0.2).astype(np.uint8) * 4) | 2
        offs, size = periodic_offsets(nbins)
        a0 = rng.standard_normal((3, nbins)) + 2.0
        project, good = periodic_project(signal, cfg["rows"], index, index_rows, flags, cfg["flag_rows"], DET_MASK, nbins, a0)
        _readonly(signal, flags, index, pure, a0, good, *project)
        _CACHE[key] = dict(cfg, nbins=nbins, pattern=pattern, mode=mode, signal=signal, flags=flags, index=index, pure=pure,
                           index_rows=index_rows, offs=offs, size=size, a0=a0, project=project, good=good)
    return _CACHE[key]


def sweep_conditions(case):
    """What the sweep cases are for, from the reference alone -> dict of figures (asserted by the tests before any kernel
    runs)."""
    good, nbins, n_samp = case["good"], case["nbins"], case["n_samp"]
    bins, _ = periodic_takes_part(case["index"], case["index_rows"], None, None, 0, nbins, 3)
    chunk = np.arange(n_samp) // PERIODIC_CHUNK
    step = np.arange(n_samp) // 64
    out = dict(take_part=float(good.mean()), bins_hit=1.0, bins_in_all_chunks=n_samp, widest_step=0)
    for d in range(3):
        b = bins[d][good[d]]
        out["bins_hit"] = min(out["bins_hit"], np.unique(b).size / nbins)
        per_chunk = [np.bincount(b[chunk[good[d]] == c], minlength=nbins) > 0 for c in range(3)]
        out["bins_in_all_chunks"] = min(out["bins_in_all_chunks"], int(np.count_nonzero(per_chunk[0] & per_chunk[1] & per_chunk[2])))
        pairs = np.unique(step[good[d]].astype(np.int64) * (2 ** 31) + b)
        out["widest_step"] = max(out["widest_step"], int(np.bincount(pairs >> 31).max()))
    return out
