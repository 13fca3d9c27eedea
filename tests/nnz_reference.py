"""Extended-precision statements of the map-domain operations for any number of Stokes components
(nnz = 1 "I", 2 "QU", 3 "IQU", 4), with rounding bounds that are derived and not chosen.  Shared by
tests/test_nnz_reference_host.py (the CPU oracle must stay inside the bounds), tests/test_gpu_nnz.py (every launch
variant of the HIP kernels must) and tests/test_gpu_offset_steps.py (the offset-template kernels at every baseline
length).  Nothing here calls the code under test.

Every function returns the exact value (``np.longdouble``, unit roundoff 2^-64: its own rounding is 2^-11 of a double's
and is ignored), the sum of the magnitudes of what was added up and, for scatter sums, the number of terms.

Bounds, with u = 2^-53 and gamma(m) = m u / (1 - m u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1;
the library is built with -ffp-contract=off, so every product and sum is rounded once):

* scatter sums (build_noise_weighted, inverse covariance, offset_accumulate): a map element is what it held before plus
  n terms fl(fl(a b) c) -- two roundings each -- added in any order, n additions: |got - exact| <= gamma(n + 2) S with
  S = |initial| + sum |a b c|.  An element that receives no term keeps its bits.
* scan_map: v = fl(scale fl(sum_k fl(w_k m_k))) carries gamma(nnz + 1) (nnz products, nnz - 1 additions -- the first one
  is onto 0.0 and exact -- and the scale), the final d + v / d - v one more rounding: gamma(nnz + 3) M covers it with
  M = |d| + |scale| sum |w_k m_k|.  In the multiply mode the result is the product d v, whose error is relative to
  M = |d| |scale| sum |w_k m_k|.  With the zero switch d is 0 (also for a sample without a pixel: it is zeroed).
* offset_scan_project: a term is fl(fl(a - sum_k w_k m_k) dw): gamma(nnz + 2) (|a| + sum |w_k m_k|) |dw|; n of them are
  added to what the amplitude held, n additions: gamma(n + nnz + 2) S.
* hits are integers: exact.

The offset-template statements at any baseline length (tests/test_gpu_offset_steps.py):

* offset_add_to_signal: a sample of an unflagged amplitude is fl(d + a), ONE IEEE addition, and the correctly rounded sum
  is what a float64 addition returns: the statement is exact and the comparison is bit equality, everywhere -- samples of
  flagged amplitudes, samples outside the views and rows outside data_index hold what they held.
* offset_project_signal: the terms are the raw samples d_s (read, not computed: no rounding of their own); n of them are
  added, in any order, onto what the amplitude held: n additions, |got - exact| <= gamma(n) S with
  S = |initial| + sum |d_s| -- ``extra = 0``.  Flagged samples contribute an exact + 0.0 and are not terms.
* offset_clean_accumulate: a term is fl(fl(fl(d - a~) s) w_k) with a~ the amplitude or, flagged, 0 (the kernel's 0.0 + a is
  exact): fl(d - a~) = (d - a~)(1 + e1) errs RELATIVE to the exact difference, the two products add e2, e3:
  |term - (d - a~) s w_k| <= gamma(3) |(d - a~) s w_k|.  With the n additions: gamma(n + 3) S,
  S = |initial| + sum |(d - a~) s w_k| -- ``extra = 3``, one more than offset_accumulate.
* the packed sweeps (packed_pointing.hip) read the I weight from ``cal`` (checked equal to weights[..., 0] in every sample
  when the cache is written) and Q / U from ``qu`` (copies): the same operands, products and order as the kernels over the
  original arrays, fl(fl(a s) w_k) and fl(fl(a - sum_k fl(w_k m_k)) dw); the pair forms add the two detectors' terms of a
  sample before the run sum, which is one of the n additions.  ``extra = 2`` and ``extra = nnz + 2 = 5`` as above.
* flagged-sample counts are sums of 1.0 far below 2^53: exact integers.
* offset_variance: rint, one subtraction of integers (exact), one division, one comparison; one product and one division
  for the variance: the same IEEE operations in NumPy double -- bit equality."""
import numpy as np

import cases

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble has to be wider than a double for these references"
U = LD(2.0) ** -53

NNZ = (1, 2, 3, 4)

#: the shapes where the launch variants differ (odd detector counts, odd chunk starts, odd n_samp, ...)
CASES = {
    "odd_dets_odd_starts": dict(n_det=5, n_samp=3000, nside=64, n_split=3, gap=2),
    "odd_n_samp": dict(n_samp=3001, n_det=4, n_split=3, gap=2),
    "single_det": dict(n_det=1, n_samp=2048, nside=32),
    "short_intervals": dict(n_samp=60, n_split=20, gap=1, n_det=2, nside=16),
    "broken_pairs_indirect": dict(n_det=4, n_samp=2500, fp_roll=1, extra_rows=2, n_split=2, gap=5),
    "long_runs": dict(n_det=4, n_samp=4096, nside=8),
    "short_runs": dict(n_det=6, n_samp=6000, nside=2048, spin_period_s=3.0, spin_angle_deg=40.0),
    "no_flags": dict(with_det_flags=False, with_shared_flags=False),
}

#: baseline lengths at which the offset kernels change path: runs of 1, 2, one DPP row (16), half a wave (32), a wave (64),
#: two samples per lane times a wave (128: the packed sweeps' uniform amplitude look-up), a workgroup trip (256), a chunk
#: (1024), one amplitude per view and a step no view reaches; each with its neighbours (divisors that are and are not
#: powers of two)
STEPS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2500, 10**6)

#: view cases of the offset-template grid: make_case arguments and, where given, the views [first, last) that replace
#: the case's own.  long_odd_view: odd first sample, odd length, three chunks (steps 1023 / 1024 / 1025 put a baseline
#: boundary before, on and after the chunk boundary at sample 3 + 1024); even_views: even first samples and even lengths,
#: the middle one longer than a chunk -- with an even step no lane of the two-samples-per-lane kernels sees a boundary
#: between its samples.
VIEW_CASES = {
    "long_odd_view": (dict(n_det=5, n_samp=2600, nside=64), ((3, 2598),)),
    "odd_dets_odd_starts": (CASES["odd_dets_odd_starts"], None),
    "odd_n_samp": (CASES["odd_n_samp"], None),
    "short_intervals": (CASES["short_intervals"], None),
    "even_views": (dict(n_det=4, n_samp=3000, nside=64), ((0, 1000), (1002, 2050), (2052, 3000))),
}

#: (should_zero, should_subtract, should_scale) of scan_map
SCAN_MODES = {"zero": (True, False, False), "add": (False, False, False), "subtract": (False, True, False),
              "multiply": (False, False, True)}
MAP_DTYPES = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32}


def gamma(m):
    m = np.asarray(m, dtype=LD)
    return m * U / (1 - m * U)


_POINTING = {}


def intervals(views, rate=10.0):
    """Views [first, last) as an interval array."""
    ivl = np.zeros(len(views), dtype=cases.interval_dtype)
    for k, (first, last) in enumerate(views):
        ivl[k]["first"], ivl[k]["last"] = first, last
        ivl[k]["start"], ivl[k]["stop"] = first / rate, last / rate
    return ivl


def pointing(oracle, name):
    """(case, pointing) of CASES[name]: pixels, IQU weights, global2local and the number of local submaps from the CPU
    oracle's pointing chain.  Computed once per session; callers must not write into it."""
    if name not in _POINTING:
        kwargs, views = VIEW_CASES[name] if name in VIEW_CASES else (CASES[name], None)
        c = cases.make_case(**kwargs)
        if views is not None:
            c["intervals"] = intervals(views, c["rate"])
        ch = cases.run_chain(oracle, c)
        pt = dict(pixels=ch["pixels"], weights=ch["weights"], g2l=ch["g2l"], n_local=ch["zmap"].shape[0])
        for a in list(pt.values()) + [v for v in c.values() if isinstance(v, np.ndarray)]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _POINTING[name] = (c, pt)
    return _POINTING[name]


def weights_nnz(weights3, nnz, seed=99):
    """Weights of ``nnz`` components from IQU ones: I as a 2-D array (the I-only layout), (Q, U), IQU, IQU plus a seeded
    random fourth column."""
    if nnz == 1:
        return np.ascontiguousarray(weights3[:, :, 0])
    if nnz == 2:
        return np.ascontiguousarray(weights3[:, :, 1:])
    if nnz == 3:
        return np.ascontiguousarray(weights3)
    extra = np.random.default_rng(seed).standard_normal(weights3.shape[:2] + (1,))
    return np.ascontiguousarray(np.concatenate([weights3, extra], axis=2))


def seeded_map(shape, dtype, seed=31):
    """A map of any of the four map types: normal deviates (x 7 and rounded, zeros replaced, for the integer types)."""
    m = np.random.default_rng(seed).standard_normal(shape)
    if np.issubdtype(dtype, np.integer):
        m = np.round(7.0 * m)
        m[m == 0] = 3.0     # (no zero entries: every hit sample gets a map term)
    return np.ascontiguousarray(m.astype(dtype))


def view_samples(c):
    parts = [np.arange(int(iv["first"]), int(iv["last"]), dtype=np.int64) for iv in c["intervals"]]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def _unflagged(c, d, s, det_mask, shared_mask):
    good = np.ones(s.size, dtype=bool)
    if c["det_flags"].shape[1] == c["n_samp"]:
        good &= (c["det_flags"][c["flag_index"][d], s] & det_mask) == 0
    if c["shared_flags"].size == c["n_samp"]:
        good &= (c["shared_flags"][s] & shared_mask) == 0
    return good


def _wrow(c, weights, d, s, nnz):
    return weights[c["weight_index"][d]][s].reshape(s.size, nnz).astype(LD)


def _local(c, pt, p):
    """(hit, local flat pixel) of global pixels ``p``: no pixel or a submap that is not local is not a hit."""
    nps = c["n_pix_submap"]
    lsm = pt["g2l"][np.where(p >= 0, p // nps, 0)]
    hit = (p >= 0) & (lsm >= 0)
    return hit, np.where(hit, lsm * nps + p % nps, 0)


def amplitude_index(c, step, n_amp_views, shift=0):
    """Per sample the index of its baseline inside one detector's amplitudes (template_offset: the views follow each
    other, each with n_amp_views[v] steps of ``step`` samples); -1 outside the views.  ``shift`` moves every baseline
    boundary by that many samples: a wrong statement, for the tests that show that the bounds can fail."""
    out = np.full(c["n_samp"], -1, dtype=np.int64)
    run = 0
    for iv, n in zip(c["intervals"], n_amp_views):
        first, last = int(iv["first"]), int(iv["last"])
        out[first:last] = run + (np.arange(first, last) - first + shift) // step
        run += int(n)
    return out


def offset_layout(c, step, amp_offset=5, spare=3):
    """(n_amp_views, amp_offsets, n_amp) of an Offset template over the case's views, the first amplitude at
    ``amp_offset`` and ``spare`` unused ones at the end."""
    n_amp_views = np.array([-(-(int(v["last"]) - int(v["first"])) // step) for v in c["intervals"]], dtype=np.int64)
    per_det = int(n_amp_views.sum())
    amp_offsets = amp_offset + np.arange(c["n_det"], dtype=np.int64) * per_det
    return n_amp_views, amp_offsets, amp_offset + c["n_det"] * per_det + spare


class Scatter:
    """A scatter sum at the elements it touches: ``idx`` (sorted flat element numbers), and there the exact value
    ``total``, the magnitude sum ``mag`` (both [len(idx), n_value], initial contents included) and the number of terms
    ``n``; ``initial`` is what the output held before, [n_element, n_value] -- everywhere else it must still hold that."""

    def __init__(self, initial, elements, terms):
        self.initial = np.array(initial, dtype=np.float64).reshape(-1, terms[0].shape[1] if terms else 1)
        n_value = self.initial.shape[1]
        loc = np.concatenate(elements) if elements else np.zeros(0, dtype=np.int64)
        term = np.concatenate(terms) if terms else np.zeros((0, n_value), dtype=LD)
        self.idx, pos = np.unique(loc, return_inverse=True)
        self.total = self.initial[self.idx].astype(LD)
        self.mag = np.abs(self.total)
        self.n = np.zeros(self.idx.size, dtype=np.int64)
        np.add.at(self.total, pos, term)
        np.add.at(self.mag, pos, np.abs(term))
        np.add.at(self.n, pos, 1)

    def counts(self):
        """The number of terms of every element (the hit map of the pixel scatters)."""
        out = np.zeros(self.initial.shape[0], dtype=np.int64)
        out[self.idx] = self.n
        return out

    def excess(self, got, extra=2):
        """The largest |got - exact| / (gamma(n + extra) S) over the touched elements; inf when an element that
        received nothing differs from its initial contents in any bit."""
        got = np.asarray(got).reshape(self.initial.shape)
        rest = np.ones(self.initial.shape[0], dtype=bool)
        rest[self.idx] = False
        if not np.array_equal(got[rest], self.initial[rest]):
            return float("inf")
        return excess(got[self.idx], self.total, gamma(self.n + extra)[:, None] * self.mag)


def _scatter(c, pt, initial, det_mask, shared_mask, values, skip_non_local=False):
    """initial + the sum over the unflagged, pixelled samples inside the views of values(d, s) [len(s), n_value], per
    local pixel.  ``skip_non_local``: samples whose submap is not local contribute nothing (the offset kernels skip
    them); otherwise there must be none."""
    samples = view_samples(c)
    elements, terms = [], []
    for d in range(c["n_det"]):
        p = pt["pixels"][c["pixel_index"][d]][samples]
        good = (p >= 0) & _unflagged(c, d, samples, det_mask, shared_mask)
        s, p = samples[good], p[good]
        hit, loc = _local(c, pt, p)
        if skip_non_local:
            s, loc = s[hit], loc[hit]
        else:
            assert hit.all(), "the scatter kernels need every hit submap to be local"
        elements.append(loc)
        terms.append(values(d, s))
    return Scatter(initial, elements, terms)


def build_noise_weighted(c, pt, weights, nnz, zmap0, det_mask=1, shared_mask=1):
    """zmap0 + A^T N^-1 d: per local pixel and component the sum of tod x det_scale x w_k -> Scatter."""
    def values(d, s):
        t = c["tod"][c["data_index"][d]][s].astype(LD) * LD(c["det_scale"][d])
        return t[:, None] * _wrow(c, weights, d, s, nnz)

    return _scatter(c, pt, np.reshape(zmap0, (-1, nnz)), det_mask, shared_mask, values)


def inverse_covariance(c, pt, weights, nnz, cov0, det_mask=1, shared_mask=1):
    """cov0 + the packed upper triangle of sum det_scale w_j w_k -> Scatter; its counts() are the hits."""
    ju, ku = np.triu_indices(nnz)

    def values(d, s):
        w = _wrow(c, weights, d, s, nnz)
        return LD(c["det_scale"][d]) * w[:, ju] * w[:, ku]

    return _scatter(c, pt, np.reshape(cov0, (-1, ju.size)), det_mask, shared_mask, values)


def offset_accumulate(c, pt, weights, nnz, zmap0, step, n_amp_views, amp_offsets, amps, amp_flags, det_mask=1,
                      shared_mask=1, skip_non_local=False):
    """zmap0 + A^T N^-1 M a: build_noise_weighted of the timestream of unflagged baseline amplitudes -> Scatter."""
    aidx = amplitude_index(c, step, n_amp_views)

    def values(d, s):
        a = amp_offsets[d] + aidx[s]
        t = np.where(amp_flags[a] == 0, amps[a], 0.0).astype(LD) * LD(c["det_scale"][d])
        return t[:, None] * _wrow(c, weights, d, s, nnz)

    return _scatter(c, pt, np.reshape(zmap0, (-1, nnz)), det_mask, shared_mask, values, skip_non_local)


def offset_clean_accumulate(c, pt, weights, nnz, zmap0, step, n_amp_views, amp_offsets, amps, amp_flags, signal, det_mask=1,
                            shared_mask=1):
    """zmap0 + A^T N^-1 (d - M a): build_noise_weighted of the signal (rows by data_index) minus the timestream of
    unflagged baseline amplitudes -> Scatter (``extra = 3``)."""
    aidx = amplitude_index(c, step, n_amp_views)

    def values(d, s):
        a = amp_offsets[d] + aidx[s]
        t = signal[c["data_index"][d]][s].astype(LD) - np.where(amp_flags[a] == 0, amps[a], 0.0).astype(LD)
        return (t * LD(c["det_scale"][d]))[:, None] * _wrow(c, weights, d, s, nnz)

    return _scatter(c, pt, np.reshape(zmap0, (-1, nnz)), det_mask, shared_mask, values)


def offset_add_to_signal(c, step, n_amp_views, amp_offsets, amps, amp_flags, tod, shift=0):
    """tod + M a: every sample inside the views whose amplitude is unflagged gets the amplitude added (rows by
    data_index) -> the expected buffer, exact: a float64 addition IS the exact sum rounded once.  Bit equality."""
    want = np.array(tod, dtype=np.float64)
    aidx = amplitude_index(c, step, n_amp_views, shift)
    s = view_samples(c)
    for d in range(c["n_det"]):
        row = c["data_index"][d]
        a = amp_offsets[d] + aidx[s]
        on = amp_flags[a] == 0
        want[row, s[on]] = tod[row, s[on]] + amps[a[on]]
    return want


def offset_project_signal(c, step, n_amp_views, amp_offsets, amps0, amp_flags, flag_mask, use_flags, tod=None, shift=0):
    """amps0 + M^T d: per unflagged amplitude the sum of its samples (rows by data_index; ``use_flags``: of those whose
    detector flag, rows by flag_index, has no bit of ``flag_mask``) -> Scatter (``extra = 0``)."""
    tod = c["tod"] if tod is None else tod
    aidx = amplitude_index(c, step, n_amp_views, shift)
    samples = view_samples(c)
    elements, terms = [], []
    for d in range(c["n_det"]):
        a = amp_offsets[d] + aidx[samples]
        keep = amp_flags[a] == 0
        if use_flags:
            keep &= (c["det_flags"][c["flag_index"][d], samples] & flag_mask) == 0
        elements.append(a[keep])
        terms.append(tod[c["data_index"][d]][samples[keep]].astype(LD)[:, None])
    return Scatter(np.reshape(amps0, (-1, 1)), elements, terms)


def offset_count_flagged(c, step, n_amp_views, amp_offsets, flag_mask, n_amp, det_flags=None):
    """Per amplitude the number of samples whose detector flag (rows by flag_index) has a bit of ``flag_mask`` -> int64
    [n_amp], exact."""
    det_flags = c["det_flags"] if det_flags is None else det_flags
    aidx = amplitude_index(c, step, n_amp_views)
    s = view_samples(c)
    out = np.zeros(n_amp, dtype=np.int64)
    for d in range(c["n_det"]):
        bad = (det_flags[c["flag_index"][d], s] & flag_mask) != 0
        np.add.at(out, amp_offsets[d] + aidx[s][bad], 1)
    return out


def offset_variance(n_bad, amp_len, det_weight, good_fraction):
    """(flags uint8, variances) [n_det, n_len] of the Offset template's set-up from the flagged-sample counts ``n_bad``
    [n_det, n_len], the baseline lengths ``amp_len`` [n_len] and the detector weights: an amplitude is cut (flag 1,
    variance 0) when n_good / max(len, 1) <= good_fraction with n_good = len - rint(n_bad), the weight is not positive
    or the baseline is empty; else its variance is 1 / (weight x n_good).  The kernel's IEEE operations, in double."""
    length = np.asarray(amp_len, dtype=np.int64)[None, :]
    w = np.asarray(det_weight, dtype=np.float64)[:, None]
    n_good = length.astype(np.float64) - np.rint(np.asarray(n_bad, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        cut = (n_good / np.maximum(length, 1).astype(np.float64) <= good_fraction) | (w <= 0.0) | (length == 0)
        var = np.where(cut, 0.0, 1.0 / (w * n_good))
    return cut.astype(np.uint8), var


def offset_scan_project(c, pt, weights, nnz, mapdata, step, n_amp_views, amp_offsets, amps, amp_flags, out0, det_weights,
                        flag_mask, signal=None):
    """out0 + M^T N^-1 (M a - A z): per unflagged amplitude the sum over its unflagged samples of
    (a - sum_k w_k z_k) x det_weight, the map term only where the sample has a local pixel -> Scatter.  With ``signal``
    (a timestream buffer, rows by data_index) the sample of the signal stands for a: M^T N^-1 (d - A z), the solver's
    right-hand side."""
    aidx = amplitude_index(c, step, n_amp_views)
    m2 = mapdata.reshape(-1, nnz)
    samples = view_samples(c)
    use_flags = c["det_flags"].shape[1] == c["n_samp"]
    elements, terms, mags = [], [], []
    for d in range(c["n_det"]):
        a = amp_offsets[d] + aidx[samples]
        keep = amp_flags[a] == 0
        if use_flags:
            keep &= (c["det_flags"][c["flag_index"][d], samples] & flag_mask) == 0
        s, a = samples[keep], a[keep]
        hit, loc = _local(c, pt, pt["pixels"][c["pixel_index"][d]][s])
        prod = _wrow(c, weights, d, s, nnz) * m2[loc].astype(LD)
        av = (amps[a] if signal is None else signal[c["data_index"][d]][s]).astype(LD)
        dw = LD(det_weights[d])
        elements.append(a)
        terms.append(((av - np.where(hit, prod.sum(axis=1), 0)) * dw)[:, None])
        mags.append(((np.abs(av) + np.where(hit, np.abs(prod).sum(axis=1), 0)) * abs(dw))[:, None])
    ref = Scatter(np.reshape(out0, (-1, 1)), elements, terms)
    # the magnitude of a term is (|a| + sum |w z|) |dw|, not the |term| that Scatter added up
    ref.mag = np.abs(ref.initial[ref.idx].astype(LD))
    np.add.at(ref.mag, np.searchsorted(ref.idx, np.concatenate(elements)), np.concatenate(mags))
    return ref


def scan_map(c, pt, weights, nnz, mapdata, tod, scale, zero, subtract, mult):
    """Per sample inside the views d (op) scale x sum_k w_k m_k -> (exact, M), both [rows, n_samp]; M is 0 and the value
    the input where the kernel must not write (outside the views, other rows) or must write the input back."""
    want = tod.astype(LD)
    mag = np.zeros(tod.shape, dtype=LD)
    m2 = mapdata.reshape(-1, nnz)
    s = view_samples(c)
    sc = LD(scale)
    for d in range(c["n_det"]):
        row = c["data_index"][d]
        hit, loc = _local(c, pt, pt["pixels"][c["pixel_index"][d]][s])
        base = np.zeros(s.size, dtype=LD) if zero else tod[row][s].astype(LD)
        prod = _wrow(c, weights, d, s, nnz) * m2[loc].astype(LD)
        v, av = sc * prod.sum(axis=1), abs(sc) * np.abs(prod).sum(axis=1)
        if subtract:
            r, g = base - v, np.abs(base) + av
        elif mult:
            r, g = base * v, np.abs(base) * av
        else:
            r, g = base + v, np.abs(base) + av
        want[row, s] = np.where(hit, r, base)
        mag[row, s] = np.where(hit, g, 0)
    return want, mag


def excess(got, exact, bound):
    """The largest |got - exact| / bound (0 where both vanish, inf where only the bound does): <= 1 is inside."""
    err = np.abs(np.asarray(got).astype(LD) - exact)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), np.where(bound > 0, err / np.where(bound > 0, bound, 1), LD(np.inf)))
    return float(ratio.max()) if ratio.size else 0.0


def scan_excess(got, ref, nnz):
    want, mag = ref
    return excess(got, want, gamma(nnz + 3) * mag)
