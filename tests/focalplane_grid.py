"""Inputs and plain references for the grid tests of the two focal-plane operators (tests/test_focalplane_grid_host.py,
tests/test_gpu_fourier2d_grid.py, tests/test_gpu_poly2d_grid.py).  NumPy and the host-side data model only: no device, no
oracle, nothing of the reference tree at test time.

Fourier2D (csrc/fourier2d.hip).  ``f2d_case(nmode, n_det)`` builds one observation of an odd number of samples whose
views have the clipped lengths 0, 1, 2, 3, 255, 256, 257, 511, 512 and 513 -- the edges of the 256-sample tile that
``f2d_job_of_tile`` resolves --, one of them starting before sample 0, one ending past the last sample, two pairs
adjacent, the empty one between two others.  The amplitude blocks of the views lie in another order than the views with
sentinel slots between them; the block of a clipped view starts at the amplitude of its own UNCLIPPED first sample.
Detector rows are permuted inside a buffer with one unlisted sentinel row, flag rows are permuted differently.  The tables
are the real mode sets (``evaluate_template`` on ``fourier2d_case.focalplane_quats``) or a random table with exact zeros.

The references are the reference implementation's expressions (src/toast/templates/fourier2d.py:395-459) as the host path
of toast_amd/templates/fourier2d.py restates them; tests/test_fourier2d_host.py holds that host path to the reference
fixture, and tests/test_focalplane_grid_host.py holds the functions below to the same fixture:

    f2d_add            row + np.sum(a.reshape(-1, nmode) * T[d], 1)                                     bit equality
    f2d_project        amp += np.outer(row, T[d]), detector after detector                              bit equality (one group)
    f2d_project_truth  a0 + sum_d s_d T_dm in longdouble, with the bound for ANY order of the n_det + 1 terms:
                       gamma(n_det + 1) (|a0| + sum|s_d T_dm|) + n_det 2^-63 sum|...|;  gamma(k) = k u / (1 - k u),
                       u = 2^-53: one rounded product per term and at most n_det additions; the second summand is the
                       rounding of the longdouble sum itself
    f2d_norms          the sequential sum over the unflagged detectors of (T * T) * w, then 1 / x, 0 where it is 0
    prior_truth        per mode the "same" window full[(F - 1) // 2 : (F - 1) // 2 + L] of the direct convolution in
                       longdouble, times scale_m, on top of the output that was there

PolyFilter2D (csrc/poly2d_filter.hip).  A second case table next to ``poly2d_host.CASES``, built with the functions of
tests/poly2d_host.py:

    edges_o0 .. edges_o3   5 interleaved groups of 30, 1, 3, 12 and 7 detectors; views of 255 (starting before sample 0),
                           256 (adjacent), 0, 257, 2, 513 and 1 sample (the observation's last one, its view ending past
                           it); rows permuted in larger buffers whose unlisted rows hold a sentinel; eight engineered
                           samples at consecutive slots of group 0, aligned to a wave of the solve, so that the statuses
                           0, 1, 2 and 3 sit in neighbouring teams.  Held to the coefficients of the reference's own
                           kernel: tests/golden/poly2d_grid.npz (orders 0 to 2) and poly2d_grid_o3.npz
                           (tests/golden/make_golden_poly2d_grid.py; one file per 1 MB).
    empty_group_o1         three groups of which group 1 has no detector; one view clipped at both ends
    batches_o3             order 3, 64 groups (4 of 24 detectors, 60 of 2), 20 sample tiles in four views: more than two
                           batches of the launcher, one view across the first batch boundary, one starting on the second
"""
import numpy as np

import poly2d_host as P
import poly_filter_host as H

LD = np.longdouble
SENTINEL = -7.5e300
U = 2.0 ** -53

# ------------------------------------------------------------------------------------ Fourier2D: the layout
F2D_N_SAMP = 2401
# (first, last) as handed to the entries; clipped to [0, F2D_N_SAMP) by them
F2D_VIEWS = ((-5, 255), (255, 511), (520, 520), (521, 778), (780, 781), (782, 784), (785, 788), (790, 1301), (1301, 1813),
             (1888, 2407))
F2D_EMPTY_VIEW = 2
F2D_ALL_FLAGGED = 600                    # flagged in every detector: its norm is 0
F2D_BLOCK_ORDER = (7, 2, 0, 9, 4, 1, 8, 6, 3, 5)      # the views in the order of their amplitude blocks
F2D_NMODES = (5, 7, 17, 19, 37, 39)
F2D_NDETS = (1, 2, 5, 9, 70)
F2D_MODE_SETS = {5: (1, False), 7: (1, True), 17: (2, False), 19: (2, True), 37: (3, False), 39: (3, True)}
DET_FLAG_MASK, DET_FLAG_OTHER = 1, 4
TILE = 256                               # kThreads: samples per workgroup of the sweeps


def gamma(k):
    return k * U / (1.0 - k * U)


def f2d_clipped(views=F2D_VIEWS, n_samp=F2D_N_SAMP):
    """-> [(first, last)] clipped to the observation; an empty view keeps first == last."""
    out = []
    for first, last in views:
        a, b = max(first, 0), min(last, n_samp)
        out.append((a, max(a, b)))
    return out


def f2d_tiles(views=F2D_VIEWS, n_samp=F2D_N_SAMP):
    """Sample tiles of the sweeps over these views."""
    return sum((b - a + TILE - 1) // TILE for a, b in f2d_clipped(views, n_samp))


def f2d_amp_layout(nmode, views=F2D_VIEWS, n_samp=F2D_N_SAMP, order=F2D_BLOCK_ORDER):
    """-> (offsets int64 [n_view], size, used bool [size]): the block of view v holds (last - first) * nmode amplitudes of
    the UNCLIPPED view from offsets[v] on; blocks follow each other in ``order`` with 3 + (view % 4) unused slots in front
    of each.  ``used`` marks the amplitudes of the samples inside the observation: everything else is never written."""
    offsets = np.zeros(len(views), dtype=np.int64)
    at = 0
    for v in order:
        at += 3 + v % 4
        offsets[v] = at
        at += (views[v][1] - views[v][0]) * nmode
    size = at + 5
    used = np.zeros(size, dtype=bool)
    for v, ((first, last), (a, b)) in enumerate(zip(views, f2d_clipped(views, n_samp))):
        used[offsets[v] + (a - first) * nmode:offsets[v] + (b - first) * nmode] = True
    return offsets, size, used


def f2d_table(nmode, n_det, kind="modes"):
    """T[d][m]: the modes of the reference's basis at the detectors of ``fourier2d_case.focalplane_quats`` (the field of
    view as ``Focalplane`` derives it), or a random table of which one entry in seven is exactly 0."""
    if kind == "random":
        rng = np.random.default_rng(9100 + 100 * nmode + n_det)
        t = rng.standard_normal((n_det, nmode))
        t[rng.random((n_det, nmode)) < 1.0 / 7.0] = 0.0
        t.flat[0] = 0.0
        return t
    import fourier2d_case as fc
    from toast_amd.data import detector_direction
    from toast_amd.templates.fourier2d import evaluate_template

    order, subharmonics = F2D_MODE_SETS[nmode]
    xyz = np.array([detector_direction(q) for q in fc.focalplane_quats(n_det)])
    radius = 0.5 * 1.01 * 2.0 * np.arccos(np.min(xyz[:, 2]))
    out = np.array([evaluate_template(*np.arcsin([x, y]), radius, order, subharmonics) for x, y, _ in xyz])
    assert out.shape == (n_det, nmode)
    return out


_f2d_cases = {}


def f2d_case(nmode, n_det, kind="modes"):
    """The inputs of one (nmode, n_det): built once, shared, never modified."""
    key = (nmode, n_det, kind)
    if key in _f2d_cases:
        return _f2d_cases[key]
    rng = np.random.default_rng(9000 + 1000 * n_det + nmode)
    n_rows = n_det + 1
    rows = rng.permutation(n_rows)[:n_det].astype(np.int32)
    flag_rows = rng.permutation(n_rows)[:n_det].astype(np.int32)
    signal = np.full((n_rows, F2D_N_SAMP), SENTINEL)
    signal[rows] = rng.standard_normal((n_det, F2D_N_SAMP)) + 0.25 * np.arange(n_det)[:, None]
    flags = (rng.random((n_rows, F2D_N_SAMP)) < 0.3).astype(np.uint8) * DET_FLAG_MASK
    flags |= (rng.random((n_rows, F2D_N_SAMP)) < 0.2).astype(np.uint8) * DET_FLAG_OTHER
    flags[:, F2D_ALL_FLAGGED] |= DET_FLAG_MASK
    offsets, size, used = f2d_amp_layout(nmode)
    amps = rng.standard_normal(size)            # what add_to_signal and apply_precond read
    start = rng.standard_normal(size)           # what project_signal adds on top of
    amps[~f2d_blocks(nmode)] = SENTINEL
    start[~f2d_blocks(nmode)] = SENTINEL
    t = f2d_table(nmode, n_det, kind)
    weights = 0.5 + 0.75 * (np.arange(n_det) % 7)
    case = dict(nmode=nmode, n_det=n_det, n_samp=F2D_N_SAMP, views=F2D_VIEWS, rows=rows, flag_rows=flag_rows, signal=signal,
                flags=flags, offsets=offsets, size=size, used=used, amps=amps, start=start, T=t, weights=weights,
                w2=np.array([(t[d] * t[d]) * weights[d] for d in range(n_det)]).reshape(n_det, nmode))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _f2d_cases[key] = case
    return case


def f2d_blocks(nmode):
    """bool [size]: inside the amplitude block of a view (the samples cut off a clipped view included)."""
    offsets, size, _ = f2d_amp_layout(nmode)
    inside = np.zeros(size, dtype=bool)
    for v, (first, last) in enumerate(F2D_VIEWS):
        inside[offsets[v]:offsets[v] + (last - first) * nmode] = True
    return inside


def _view_slices(nmode, views, n_samp, offsets):
    """(samples of the observation, amplitudes) of every view that is not empty."""
    for v, ((first, _), (a, b)) in enumerate(zip(views, f2d_clipped(views, n_samp))):
        if b > a:
            at = int(offsets[v]) + (a - first) * nmode
            yield slice(a, b), slice(at, at + (b - a) * nmode)


# ------------------------------------------------------------------------------------ Fourier2D: the references
def f2d_add(signal, rows, t, amps, nmode, views, n_samp, offsets):
    """fourier2d.py:395-414 -> the signal buffer after add_to_signal of every listed detector."""
    out = np.array(signal)
    for d, row in enumerate(rows):
        for samples, block in _view_slices(nmode, views, n_samp, offsets):
            out[row, samples] = out[row, samples] + np.sum(amps[block].reshape(-1, nmode) * t[d], 1)
    return out


def f2d_project(signal, rows, t, start, nmode, views, n_samp, offsets):
    """fourier2d.py:416-435, detector after detector -> the amplitude vector."""
    out = np.array(start)
    for d, row in enumerate(rows):
        for samples, block in _view_slices(nmode, views, n_samp, offsets):
            amp_view = out[block].reshape(-1, nmode)
            amp_view[:] += np.outer(signal[row, samples], t[d])
    return out


def f2d_project_truth(signal, rows, t, start, nmode, views, n_samp, offsets):
    """-> (truth longdouble [size], bound float64 [size]) of the projection summed in any order; outside the views the
    truth is ``start`` and the bound 0."""
    truth = np.array(start, dtype=LD)
    mag = np.abs(truth)
    n_det = len(rows)
    for samples, block in _view_slices(nmode, views, n_samp, offsets):
        tv, mv = truth[block].reshape(-1, nmode), mag[block].reshape(-1, nmode)
        for d, row in enumerate(rows):
            term = signal[row, samples].astype(LD)[:, None] * t[d].astype(LD)[None, :]
            tv += term
            mv += np.abs(term)
        truth[block], mag[block] = tv.reshape(-1), mv.reshape(-1)
    bound = gamma(n_det + 1) * mag + n_det * 2.0 ** -63 * mag
    inside = np.zeros(truth.size, dtype=bool)
    for _, block in _view_slices(nmode, views, n_samp, offsets):
        inside[block] = True
    bound[~inside] = 0
    return truth, bound.astype(np.float64)


def f2d_norms(flags, flag_rows, mask, w2, fill, nmode, views, n_samp, offsets):
    """fourier2d.py:331-365 -> the norms vector; ``flags`` None: every sample is good.  ``fill`` where no view is."""
    out = np.array(fill, dtype=np.float64)
    for samples, block in _view_slices(nmode, views, n_samp, offsets):
        acc = np.zeros((samples.stop - samples.start, nmode))
        for d in range(w2.shape[0]):
            good = np.ones(acc.shape[0])
            if flags is not None:
                good[(flags[flag_rows[d], samples] & mask) != 0] = 0
            acc += np.outer(good, w2[d])
        nonzero = acc != 0
        acc[nonzero] = 1.0 / acc[nonzero]
        out[block] = acc.reshape(-1)
    return out


# ------------------------------------------------------------------------------------ Fourier2D: the prior
PRIOR_SHAPES = ((1, 1), (2, 1), (3, 2), (5, 8), (63, 62), (64, 64), (65, 128), (129, 127), (300, 299), (513, 512))
PRIOR_NMODES = (1, 5, 8, 39, 40)
PRIOR_DOUBLED = ((64, 64), (129, 127))
PRIOR_MAX_MODES = 40
PRIOR_FILL = 0.5


def prior_inputs(view_len, filter_len):
    """-> (in [L][40], filter [F], scale [40]): a decaying random filter, the scales of the class at its default
    amplitude (1, 2, 2, 4, ... times 10).  A case of ``nmode`` modes takes the first ``nmode`` columns."""
    rng = np.random.default_rng(9500 + 1000 * view_len + filter_len)
    a = rng.standard_normal((view_len, PRIOR_MAX_MODES))
    k = np.arange(filter_len)
    filt = rng.standard_normal(filter_len) * np.exp(-k / (1.0 + filter_len / 6.0))
    filt[0] = 1.0 + abs(filt[0])
    scale = np.full(PRIOR_MAX_MODES, 4.0)
    scale[0], scale[1:3] = 1.0, 2.0
    return a, filt, scale * 10.0


_prior = {}


def prior_truth(view_len, filter_len):
    """-> longdouble [L][40]: the window of scipy.signal.convolve(in[:, m], filter * scale_m, "same") -- samples
    (F - 1) // 2 .. (F - 1) // 2 + L of the full convolution -- by direct summation, WITHOUT the output it is added to."""
    key = (view_len, filter_len)
    if key not in _prior:
        a, filt, scale = prior_inputs(view_len, filter_len)
        full = np.zeros((view_len + filter_len - 1, PRIOR_MAX_MODES), dtype=LD)
        al = a.astype(LD)
        for k in range(filter_len):
            full[k:k + view_len] += al * (filt[k] * scale).astype(LD)[None, :]      # filter * scale_m: rounded, as handed over
        shift = (filter_len - 1) // 2
        _prior[key] = full[shift:shift + view_len]
    return _prior[key]


def prior_scipy(view_len, filter_len, nmode, fill=PRIOR_FILL):
    """The reference's own call (fourier2d.py:437-455) on the same inputs, on top of ``fill`` -> [L][nmode]."""
    import scipy.signal

    a, filt, scale = prior_inputs(view_len, filter_len)
    out = np.full((view_len, nmode), fill)
    for m in range(nmode):
        out[:, m] += scipy.signal.convolve(a[:, m], filt * scale[m], mode="same")
    return out


def prior_distance(got, view_len, filter_len, nmode, fill=PRIOR_FILL):
    """-> (max |got - (fill + truth)|, max |truth|) over the first ``nmode`` modes."""
    truth = prior_truth(view_len, filter_len)[:, :nmode]
    return float(np.max(np.abs(got.astype(LD) - (LD(fill) + truth)))), float(np.max(np.abs(truth)))


# ------------------------------------------------------------------------------------ PolyFilter2D: edge cases
EDGE_CASES = {f"edges_o{order}": dict(order=order) for order in range(4)}
EDGE_N_SAMP = 1300
EDGE_STARTS = np.array([-7, 255, 515, 517, 776, 780, 1299], dtype=np.int64)
EDGE_STOPS = np.array([255, 511, 515, 774, 778, 1293, 1304], dtype=np.int64)
EDGE_GROUP_SIZES = (30, 1, 3, 12, 7)
EDGE_N_DET = sum(EDGE_GROUP_SIZES)
# Engineered samples of group 0: eight consecutive slots of the 513-sample view from slot 64 on, so that they start a
# wave of the solve at every order (64, 16, 4 and 4 systems per wave).  Statuses at orders 1 to 3: 0 1 2 3 | 0 1 2 0.
EDGE_FIRST = 780 + 64
E_ZERO, E_GROUP_FLAGGED, E_ONE_GOOD, E_NAN_GOOD, E_NAN_FLAGGED, E_SHARED, E_FEW_GOOD, E_PLAIN = range(EDGE_FIRST, EDGE_FIRST + 8)
EDGE_FIXTURES = {"edges_o0": "poly2d_grid.npz", "edges_o1": "poly2d_grid.npz", "edges_o2": "poly2d_grid.npz",
                 "edges_o3": "poly2d_grid_o3.npz"}


def edge_groups():
    """The detectors of the five groups interleaved in list order."""
    labels = np.repeat(np.arange(len(EDGE_GROUP_SIZES)), EDGE_GROUP_SIZES)
    return labels[np.argsort(H.hashed_uniform(7501, EDGE_N_DET), kind="stable")].astype(np.int32)


def _random_inputs(base, seed, n_sig_rows, n_flag_rows, n_samp):
    s = np.arange(n_samp)
    signal = 6.0 + 2.0 * np.sin(s / 50.0)[None, :] + (H.hashed_uniform(base + 3, n_sig_rows * n_samp).reshape(n_sig_rows, n_samp) - 0.5) * np.sqrt(12.0)
    frac = P.BAD_FRACTIONS[(H.hashed_uniform(seed, n_samp) * P.BAD_FRACTIONS.size).astype(int)]
    det_flags = (H.hashed_uniform(seed + 1, n_flag_rows * n_samp).reshape(n_flag_rows, n_samp) < frac[None, :]).astype(np.uint8) * P.DET_MASK
    det_flags |= (H.hashed_uniform(seed + 2, n_flag_rows * n_samp).reshape(n_flag_rows, n_samp) < 0.2).astype(np.uint8) * P.DET_OTHER
    shared = (H.hashed_uniform(seed + 3, n_samp) < 0.03).astype(np.uint8) * P.SHARED_MASK
    shared |= (H.hashed_uniform(seed + 4, n_samp) < 0.2).astype(np.uint8) * P.SHARED_OTHER
    return signal, det_flags, shared


def build_edge_case(name, seed):
    """Inputs of ``edges_o*`` with flag seed ``seed``, in the form of ``poly2d_host.build_case``."""
    order = EDGE_CASES[name]["order"]
    n_det, n_group, n_mode = EDGE_N_DET, len(EDGE_GROUP_SIZES), (order + 1) ** 2
    templates, det_group, quats = P.case_templates(n_det, n_group, order, det_group=edge_groups())
    base = 7600 + 10 * order
    n_sig_rows, n_flag_rows = n_det + 4, n_det + 3
    sig_rows = np.argsort(H.hashed_uniform(base + 1, n_sig_rows))[:n_det].astype(np.int32)
    flag_rows = np.argsort(H.hashed_uniform(base + 2, n_flag_rows))[:n_det].astype(np.int32)
    signal, det_flags, shared = _random_inputs(base, seed, n_sig_rows, n_flag_rows, EDGE_N_SAMP)
    unlisted = np.setdiff1d(np.arange(n_sig_rows), sig_rows)
    signal[unlisted] = SENTINEL
    g0 = np.flatnonzero(det_group == 0)
    engineered = list(range(EDGE_FIRST, EDGE_FIRST + 8))
    shared[engineered] &= ~np.uint8(P.SHARED_MASK)
    shared[E_SHARED] |= P.SHARED_MASK
    clear = ~np.uint8(P.DET_MASK)
    signal[sig_rows, E_ZERO] = 0.0                                              # every good signal exactly 0: solved, c = 0
    det_flags[:, E_ZERO] &= clear
    det_flags[flag_rows[g0[0]], E_ZERO] |= P.DET_MASK
    det_flags[flag_rows[g0], E_GROUP_FLAGGED] |= P.DET_MASK                      # nobody good in group 0
    det_flags[flag_rows[g0], E_ONE_GOOD] |= P.DET_MASK
    det_flags[flag_rows[g0[g0.size // 2]], E_ONE_GOOD] &= clear                  # exactly one good detector
    det_flags[flag_rows[g0], E_NAN_GOOD] &= clear                                # a NaN in a good sample: not finite
    signal[sig_rows[g0[2]], E_NAN_GOOD] = np.nan
    det_flags[flag_rows[g0], E_NAN_FLAGGED] &= clear                             # a NaN under a flag: solved
    signal[sig_rows[g0[1]], E_NAN_FLAGGED] = np.nan
    det_flags[flag_rows[g0[1]], E_NAN_FLAGGED] |= P.DET_MASK
    if n_mode > 1:
        n_few = min(n_mode - 1, g0.size - 1)                                     # 0 < n_good < n_mode: truncated
        det_flags[flag_rows[g0], E_FEW_GOOD] |= P.DET_MASK
        det_flags[flag_rows[g0[:n_few]], E_FEW_GOOD] &= clear
    det_flags[flag_rows[g0], E_PLAIN] &= clear
    return dict(order=order, n_det=n_det, n_group=n_group, n_mode=n_mode, templates=templates, det_group=det_group,
                quats=quats, signal=signal, det_flags=det_flags, shared=shared, sig_rows=sig_rows, flag_rows=flag_rows,
                starts=EDGE_STARTS, stops=EDGE_STOPS, n_samp=EDGE_N_SAMP)


def edge_statuses(order):
    """The statuses of group 0 at the eight engineered samples.  Order 0 has one mode: no system can be truncated, and one
    good detector solves it."""
    return [0, 1, 0, 3, 0, 1, 0, 0] if order == 0 else [0, 1, 2, 3, 0, 1, 2, 0]


def edge_fixture_case(name, fixtures=None):
    """-> (case, reference coefficients, excluded, bounds) of ``poly2d_host.fixture_case`` for an ``edges_o*`` case."""
    file = EDGE_FIXTURES[name]
    fix = P.load_fixture(file) if fixtures is None else fixtures.setdefault(file, P.load_fixture(file))
    return P.fixture_case(fix, name, build=build_edge_case)


def nan_free(case):
    """The case with the NaN of the good sample replaced: what the reference's kernel is asked about."""
    clean = dict(case)
    clean["signal"] = case["signal"].copy()
    g0 = np.flatnonzero(case["det_group"] == 0)
    clean["signal"][case["sig_rows"][g0[2]], E_NAN_GOOD] = 1.0
    return clean


# ------------------------------------------------------------------------------------ PolyFilter2D: an empty group
def build_empty_group_case(compact=False):
    """Order 1, 19 detectors in groups 0 and 2 of three (``compact``: the same detectors in groups 0 and 1 of two); one
    view that runs past both ends of the observation."""
    n_det, n_samp, order = 19, 300, 1
    wide = (2 * P.detector_groups(n_det, 2)).astype(np.int32)
    det_group = (wide // 2).astype(np.int32) if compact else wide
    n_group = 2 if compact else 3
    templates, _, quats = P.case_templates(n_det, n_group, order, det_group=det_group)
    signal, det_flags, shared = _random_inputs(7700, 7710, n_det, n_det, n_samp)
    rows = np.arange(n_det, dtype=np.int32)
    return dict(order=order, n_det=n_det, n_group=n_group, n_mode=4, templates=templates, det_group=det_group, quats=quats,
                signal=signal, det_flags=det_flags, shared=shared, sig_rows=rows, flag_rows=rows,
                starts=np.array([-3], dtype=np.int64), stops=np.array([n_samp + 5], dtype=np.int64), n_samp=n_samp)


# ------------------------------------------------------------------------------------ PolyFilter2D: batches
BATCH_N_SAMP = 5001
BATCH_STARTS = np.array([0, 1500, 3400, 4500], dtype=np.int64)        # 6 + 8 + 4 + 2 = 20 sample tiles
BATCH_STOPS = np.array([1500, 3300, 4400, 5000], dtype=np.int64)
BATCH_GROUP_SIZES = (24,) * 4 + (2,) * 60
BATCH_PIECES = (513, 257, 256, 255, 2, 1)      # lengths the views are cut into, in turn: shapes edges_o3 holds to the reference


def batch_tiles():
    """-> first sample tile of every view, and the number of tiles."""
    n = (BATCH_STOPS - BATCH_STARTS + TILE - 1) // TILE
    return np.concatenate([[0], np.cumsum(n)[:-1]]), int(n.sum())


def build_batches_case():
    order, n_group = 3, len(BATCH_GROUP_SIZES)
    n_det = sum(BATCH_GROUP_SIZES)
    labels = np.repeat(np.arange(n_group), BATCH_GROUP_SIZES)
    det_group = labels[np.argsort(H.hashed_uniform(7801, n_det), kind="stable")].astype(np.int32)
    templates, _, quats = P.case_templates(n_det, n_group, order, det_group=det_group)
    n_sig_rows, n_flag_rows = n_det + 2, n_det + 1
    sig_rows = np.argsort(H.hashed_uniform(7802, n_sig_rows))[:n_det].astype(np.int32)
    flag_rows = np.argsort(H.hashed_uniform(7803, n_flag_rows))[:n_det].astype(np.int32)
    signal, det_flags, shared = _random_inputs(7800, 7810, n_sig_rows, n_flag_rows, BATCH_N_SAMP)
    signal[np.setdiff1d(np.arange(n_sig_rows), sig_rows)] = SENTINEL
    return dict(order=order, n_det=n_det, n_group=n_group, n_mode=16, templates=templates, det_group=det_group, quats=quats,
                signal=signal, det_flags=det_flags, shared=shared, sig_rows=sig_rows, flag_rows=flag_rows,
                starts=BATCH_STARTS, stops=BATCH_STOPS, n_samp=BATCH_N_SAMP)


def batch_pieces():
    """[(first, last)]: every view cut into pieces of BATCH_PIECES samples in turn (the last piece of a view is what is
    left), at most three sample tiles each."""
    out, k = [], 0
    for first, last in zip(BATCH_STARTS, BATCH_STOPS):
        at = int(first)
        while at < last:
            n = min(BATCH_PIECES[k % len(BATCH_PIECES)], int(last) - at)
            out.append((at, at + n))
            at += n
            k += 1
    return out
