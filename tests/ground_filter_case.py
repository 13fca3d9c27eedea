"""The cases, the long double truth and the bound of the ground-filter grid tests (tests/test_ground_filter_host.py on the
host, tests/test_gpu_ground_filter_grid.py on the device: csrc/ground_filter.hip).  NumPy only.

A case (``make_case``) holds templates [n_template][n_samp], seeded normal signals and flag BYTES with random bits inside
and outside the masks (a kernel that tested ``flags != 0`` instead of ``flags & mask`` fails every case), the signal and
flag rows permuted inside larger buffers whose other rows are NaN / 0xff.

``truth`` evaluates what toast_hip_template_fit_dev promises in long double (64-bit mantissa), with the norm
sum |terms| of every entry.  Figures are distances ``max |got - truth| / sum |terms|`` over the entries of one quantity.
The bound of a case is FACTOR = 4 times ``sequential_distance``: the distance of the sums evaluated in fp64 in the
reference's own loop order (toast_tod_filter.cpp:160-215: ``proj[row] += t[i] * signal[i] * good[i]``, sample after
sample), i.e. the device is to be no further from the truth than four times the reference is (the rule of
tests/test_gpu_noise_estim.py).  The factor is not 1 because the one-pair path of k_template_gram_flagged adds the samples
of its queue sequentially in an arbitrary order: that IS the reference's arithmetic on permuted terms, and its distance
scatters around the reference's.  The bound is measured on the reference's arithmetic alone, never on the kernel.

A bad sample's signal counts as 0 whatever it holds (the contract pinned by test (c) of the device module); the
reference multiplies by ``good`` and would hand a NaN on.  ``truth`` and ``sequential_distance`` both replace the signal
of bad samples by 0, so a NaN or Inf there changes neither.
"""
import functools

import numpy as np

from oracle import ground_filter as GF

L = np.longdouble
FACTOR = 4
DET_MASK, SHARED_MASK = 0x06, 0x21
KINDS = ("legendre", "indicator")
FLAG_KINDS = ("none", "random", "all", "one_good", "mask0")
DET_FRACTION, SHARED_FRACTION = 0.02, 0.05

#: (a) both sides of every dispatch threshold of toast_hip_template_fit_dev (8 | 9, 16 | 17, 24 | 25, 32 | 33, 48 | 49) and
#: of the 256-pair threshold of k_template_gram_flagged (22 | 23)
TEMPLATE_COUNTS = (1, 2, 7, 8, 9, 16, 17, 22, 23, 24, 25, 32, 33, 48, 49, 65)
TEMPLATE_EXTRA_COUNTS = (8, 23, 49)
TEMPLATE_GRID_SAMPLES, TEMPLATE_GRID_DETS = 9001, 37
#: detectors of grid (a) flagged at every sample / at all but one: the first shares a wave with good detectors in every
#: instantiation, the second is the last detector, the one the clamped duplicates of the last wave repeat
TEMPLATE_GRID_ALL, TEMPLATE_GRID_ONE_GOOD = (5,), (36,)
#: (b) the edges of a wave (64), a block / tile (256), a queue block (1024), a projection slice (4096), a Gram slice (65536)
SAMPLE_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 131149)
LENGTH_GRID_COUNTS, LENGTH_GRID_DETS, LENGTH_GRID_ALL = (3, 23), 5, (2,)
#: the samples at which a slice of one of the kernels ends or begins
SLICE_EDGES = (4095, 4096, 65535, 65536)


def template_grid():
    """The (n_template, kind, flag_kind) of grid (a)."""
    out = [(nt, "legendre", "random") for nt in TEMPLATE_COUNTS]
    for nt in TEMPLATE_EXTRA_COUNTS:
        out += [(nt, "indicator", "random"), (nt, "indicator", "none"), (nt, "legendre", "none"), (nt, "legendre", "mask0")]
    return out


def template_grid_case(nt, kind, flag_kind):
    return cached_case(1000 + nt, TEMPLATE_GRID_SAMPLES, nt, TEMPLATE_GRID_DETS, kind, flag_kind, (DET_MASK, SHARED_MASK),
                       TEMPLATE_GRID_ALL, TEMPLATE_GRID_ONE_GOOD)


def length_grid():
    return [(n, nt) for n in SAMPLE_LENGTHS for nt in LENGTH_GRID_COUNTS]


def length_grid_case(n_samp, nt):
    return cached_case(2000 + nt, n_samp, nt, LENGTH_GRID_DETS, "legendre", "random", (DET_MASK, SHARED_MASK),
                       LENGTH_GRID_ALL, ())


def nonfinite_case(nt):
    """The case of test (c): 11 detectors are one full wave and a ragged one at 8 detectors per wave (n_template = 8) and
    six waves, the last with a clamped duplicate, at 2 per wave (n_template = 32)."""
    return cached_case(3000 + nt, 9001, nt, 11, "legendre", "random", (DET_MASK, SHARED_MASK), (), ())


# ---------------------------------------------------------------------------------------------------------- cases
def _flag_bytes(rng, flagged, mask):
    """Bytes drawn from all 256 values: ``byte & mask != 0`` exactly where ``flagged``."""
    values = np.arange(256, dtype=np.uint8)
    bad, fine = values[(values & mask) != 0], values[(values & mask) == 0]
    return np.where(flagged, bad[rng.integers(0, bad.size, flagged.shape)], fine[rng.integers(0, fine.size, flagged.shape)])


def indicator_templates(rng, n_samp, n_template):
    """Rows of disjoint 0/1 indicators (azimuth bins), split rows (a Legendre polynomial times a scan-direction mask) and,
    from three rows on, one row that is identically zero: Gram entries between two indicators or with the zero row, and
    projections on the zero row, are sums of exact zeros."""
    n_rest = n_template - (1 if n_template >= 3 else 0)
    n_ind = (n_rest + 1) // 2
    ibin = rng.integers(0, n_ind, n_samp)
    direction = rng.integers(-1, 2, n_samp)                 # -1 / 0 (turnaround) / +1
    x = np.sort(rng.uniform(-1, 1, n_samp))
    rows = [(ibin == b).astype(np.float64) for b in range(n_ind)]
    for k in range(n_rest - n_ind):
        rows.append(GF.legendre_templates(x, k // 2, k // 2 + 1)[0] * (direction != (1 if k % 2 else -1)))
    if n_template >= 3:
        rows.insert(n_template // 3, np.zeros(n_samp))
    return np.ascontiguousarray(np.vstack(rows))


def make_case(seed, n_samp, n_template, n_det, kind="legendre", flag_kind="random", masks=(DET_MASK, SHARED_MASK),
              all_flagged=None, one_good=None):
    """``flag_kind`` none: no flag arrays (NULL pointers); random: DET_FRACTION of a detector's and SHARED_FRACTION of the
    shared samples flagged; all / one_good: random, and the detectors ``all_flagged`` (default: the middle one) flagged at
    every sample / ``one_good`` (default: the last one) at every sample but one; mask0: the flags of random with both masks
    0, so that nothing counts.  ``all_flagged`` / ``one_good`` may be given with every kind that has flags."""
    assert kind in KINDS and flag_kind in FLAG_KINDS
    rng = np.random.default_rng([seed, n_samp, n_template, n_det])
    if kind == "legendre":
        templates = GF.legendre_templates(np.sort(rng.uniform(-1, 1, n_samp)), 0, n_template)
    else:
        templates = indicator_templates(rng, n_samp, n_template)
    signal = rng.standard_normal((n_det, n_samp))
    det_mask, shared_mask = masks
    shared_bad = rng.random(n_samp) < SHARED_FRACTION
    det_bad = rng.random((n_det, n_samp)) < DET_FRACTION
    if all_flagged is None:
        all_flagged = (n_det // 2,) if flag_kind == "all" else ()
    if one_good is None:
        one_good = (n_det - 1,) if flag_kind == "one_good" else ()
    for d in all_flagged:
        det_bad[d] = True
    for d in one_good:
        det_bad[d] = True
        common = np.flatnonzero(~shared_bad)
        det_bad[d, common[-1] if common.size else n_samp - 1] = False    # the last sample the shared flags leave
    det_flags = _flag_bytes(rng, det_bad, det_mask)
    shared_flags = _flag_bytes(rng, shared_bad, shared_mask)
    # rows permuted inside larger buffers; the rows no detector owns would show in every sum
    signal_index = rng.permutation(n_det + 3)[:n_det].astype(np.int32)
    flag_index = rng.permutation(n_det + 2)[:n_det].astype(np.int32)
    if n_det > 1 and np.array_equal(signal_index, flag_index):
        flag_index = flag_index[::-1].copy()
    signal_buffer = np.full((n_det + 3, n_samp), np.nan)
    signal_buffer[signal_index] = signal
    flag_buffer = np.full((n_det + 2, n_samp), 0xFF, dtype=np.uint8)
    flag_buffer[flag_index] = det_flags
    case = dict(n_samp=n_samp, n_template=n_template, n_det=n_det, kind=kind, flag_kind=flag_kind, templates=templates,
                signal=signal, signal_buffer=signal_buffer, signal_index=signal_index, flag_buffer=flag_buffer,
                flag_index=flag_index, shared_flags=shared_flags, det_mask=det_mask, shared_mask=shared_mask,
                with_flags=flag_kind != "none")
    if flag_kind == "mask0":
        case["det_mask"] = case["shared_mask"] = 0
    return case


@functools.lru_cache(maxsize=None)
def cached_case(*args):
    """One copy per argument list, shared by the tests of a module and never modified."""
    return make_case(*args)


def masks_of(case, signal=None):
    """(common_good [n_samp], det_bad [n_det][n_samp]) as the entry defines them."""
    n, n_det = case["n_samp"], case["n_det"]
    if not case["with_flags"]:
        return np.ones(n, dtype=bool), np.zeros((n_det, n), dtype=bool)
    common = (case["shared_flags"] & case["shared_mask"]) == 0
    det_bad = (case["flag_buffer"][case["flag_index"]] & case["det_mask"]) != 0
    return common, det_bad


# ---------------------------------------------------------------------------------------------------------- truth
def _ldot(a, b, chunk=512):
    """a @ b.T in long double, the samples added in chunks: numpy adds the terms of a long double product one after the
    other, so the rounding of a chunk grows with its length (about sqrt(chunk) x 2^-64 of the partial sums)."""
    parts = [a[:, i:i + chunk] @ b[:, i:i + chunk].T for i in range(0, a.shape[1], chunk)]
    return np.sum(np.array(parts, dtype=L), axis=0) if parts else np.zeros((a.shape[0], b.shape[0]), dtype=L)


def truth_from_masks(templates, signal, common_good, det_bad):
    """Long double sums and their norms.  ``signal`` [n_det][n_samp]; bad samples count as 0 whatever they hold."""
    n_det = signal.shape[0]
    nt = templates.shape[0]
    tl, ta = templates.astype(L), np.abs(templates)
    out = {}
    good = common_good[None, :] & ~det_bad
    sg = np.where(good, signal, 0.0)
    out["proj"] = _ldot(sg.astype(L), tl)
    out["proj_norm"] = np.ascontiguousarray((ta @ np.abs(sg).T).T)
    tg = tl[:, common_good]
    out["gram_common"] = _ldot(tg, tg)
    out["gram_common_norm"] = ta[:, common_good] @ ta[:, common_good].T
    out["gram_flagged"] = np.zeros((n_det, nt, nt), dtype=L)
    out["gram_flagged_norm"] = np.zeros((n_det, nt, nt))
    flagged = common_good[None, :] & det_bad
    out["n_flagged"] = np.count_nonzero(flagged, axis=1).astype(np.int64)
    for d in np.flatnonzero(out["n_flagged"]):
        tf = tl[:, flagged[d]]
        out["gram_flagged"][d] = _ldot(tf, tf)
        out["gram_flagged_norm"][d] = ta[:, flagged[d]] @ ta[:, flagged[d]].T
    return out


def truth(case, signal=None):
    common, det_bad = masks_of(case)
    return truth_from_masks(case["templates"], case["signal"] if signal is None else signal, common, det_bad)


_truths = {}


def cached_truth(case):
    """(truth, sequential distances) of a case, computed once and never modified."""
    if id(case) not in _truths:
        t = truth(case)
        _truths[id(case)] = (case, t, sequential_distance(case, t))
    return _truths[id(case)][1:]


def _sequential_rows(rows, weights, want, norm):
    """max over the rows of |cumsum(rows * weights)[-1] - want| / norm (entries with norm 0 are exact zeros: no share)."""
    if rows.shape[1] == 0:
        return 0.0
    seq = np.cumsum(rows * weights, axis=1)[:, -1]
    ok = norm > 0
    return float(np.max(np.abs(seq[ok].astype(L) - want[ok]) / norm[ok])) if np.any(ok) else 0.0


def sequential_distance_from_masks(templates, signal, common_good, det_bad, t):
    """The same sums in fp64 in the reference's loop order (np.cumsum adds strictly one term after the other):
    terms = (T_r * s) * good and (T_r * T_c) * good.  Samples with good == 0 add an exact 0 and are left out."""
    nt = templates.shape[0]
    out = dict(proj=0.0, gram_common=0.0, gram_flagged=0.0)
    good = common_good[None, :] & ~det_bad
    for d in range(signal.shape[0]):
        sel = good[d]
        out["proj"] = max(out["proj"], _sequential_rows(templates[:, sel], signal[d, sel][None, :], t["proj"][d],
                                                        t["proj_norm"][d]))
    flagged = common_good[None, :] & det_bad
    subsets = [("gram_common", common_good, t["gram_common"], t["gram_common_norm"])]
    subsets += [("gram_flagged", flagged[d], t["gram_flagged"][d], t["gram_flagged_norm"][d])
                for d in np.flatnonzero(t["n_flagged"])]
    for key, sel, want, norm in subsets:
        ts = np.ascontiguousarray(templates[:, sel])
        for r in range(nt):
            out[key] = max(out[key], _sequential_rows(ts[r:], ts[r][None, :], want[r, r:], norm[r, r:]))
    return out


def sequential_distance(case, t, signal=None):
    common, det_bad = masks_of(case)
    return sequential_distance_from_masks(case["templates"], case["signal"] if signal is None else signal, common,
                                          det_bad, t)


def bounds(seq):
    return {k: FACTOR * v for k, v in seq.items()}


def distance(got, want, norm):
    """max |got - truth| / norm over the entries with norm > 0; an entry with norm == 0 is a sum of exact zeros and must be
    exactly 0.0 (inf is returned otherwise, as for any entry that is not finite)."""
    got, want, norm = np.asarray(got), np.asarray(want), np.asarray(norm)
    assert got.shape == want.shape == norm.shape
    zero = norm == 0
    if np.any(got[zero] != 0.0) or not np.all(np.isfinite(got)):
        return np.inf
    if np.all(zero):
        return 0.0
    return float(np.max(np.abs(got[~zero].astype(L) - want[~zero]) / norm[~zero]))


def subtract_expected(signal, templates, coeff, first_template):
    """signal - fit with fit = the oracle's add_templates of the rows from ``first_template`` on into a zeroed row, template
    after template, in fp64: what toast_hip_template_subtract_dev gives bit for bit."""
    fit = np.zeros(signal.size)
    GF.add_templates(fit, templates[first_template:], coeff[first_template:])
    return signal - fit

