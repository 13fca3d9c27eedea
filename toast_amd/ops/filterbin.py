"""FilterBin: regress HWP-synchronous harmonics, ground polynomials in azimuth and per-subscan polynomials out of
every detector timestream in ONE least-squares fit, then bin the cleaned signal (reference:
src/toast/ops/filterbin.py:337-2203).

The reference builds the sparse templates of an observation once (`_build_common_templates` :1413-1421), and per
detector masks them (`SparseTemplates.mask` :145-168, twice: `_exec` :895, :940), forms F^T diag(good) F in an
O(n_template^2 n_samp) host loop (`build_template_covariance`, src/toast/_libtoast/ops_filterbin.cpp:276-382), takes
`np.linalg.cond` and `inv` / `pinv` of the full matrix (:193-251) and subtracts template by template (:1569-1577).

Here the templates are split into Nd dense rows in HBM (HWP + ground) and V intervals with K = poly_filter_order + 1
local Legendre polynomials that are never stored (csrc/filterbin.hip).  All detectors of an observation go through
each launch; the device returns the unnormalised blocks of the arrowhead normal matrix
``[[A_d, C_d], [C_d^T, diag(B_dv)]]``, the right-hand sides and the exact counts of good non-zero samples per
template.  The host (``regress``) repeats the reference's two maskings from the counts, normalises the small
matrices with ``D^-1/2 M D^-1/2``, eliminates the interval blocks, and falls back to the reference's own
``cond`` / ``inv`` / ``pinv`` / reject decision on the assembled full matrix whenever a rigorous lower bound of the
full matrix's reciprocal condition number does not clear ``|template_rcond_limit|``.

Not reproduced: observation matrices (`write_obs_matrix`, `noiseweight_obs_matrix`, `cache_dir`, `nskip`;
filterbin.py:1592-2057), deprojection (`deproject_map`, `deproject_nnz`, `deproject_pattern`; :1424-1456),
`precomputed_templates` (:1458-1566), binned-azimuth templates (`ground_filter_bin_width`,
`ground_template_expansion_order`; :1241-1370), `ground_template_time_step` (:1209-1232), `filter_config_file`
(:652-695), `maskfile` (:773-774), the Monte-Carlo mode (`mc_mode`, `mc_index`) and `amplitude_dir` /
`n_save_templates` (:1005-1058).  These traits keep the reference's names and defaults so that the trait audit
(tools/audit_traits.py) stays meaningful for this class, and `exec` raises NotImplementedError for any other value.
The file writers (`write_map`, `write_hits`, `write_cov`, `write_invcov`, `write_rcond`, `write_noiseweighted_map`,
`write_hdf5*`, `output_dir`; :2138-2176) are not declared.  `write_binmap` / `write_noiseweighted_binmap` keep their
effect on the data products: the unfiltered map is binned under the reference's names; nothing goes to disk.
`poly_filter_order` is limited to ``capi.dev.filterbin_max_order()``; the intervals of `poly_filter_view` must be
sorted and disjoint (interval lists are).
"""

import time

import numpy as np

from ..accel import (
    Resident,
    accel_data_create,
    accel_data_delete,
    accel_device_ptr,
    accel_enabled,
    device_scratch,
    make_resident,
    native,
)
from ..data import defaults
from ..traits import Bool, Float, Instance, Int, Unicode
from .mapmaker_ops import CovarianceAndHits
from .operator import Operator
from .pointing import BuildPixelDistribution

ROUTE_INV, ROUTE_PINV, ROUTE_REJECTED, ROUTE_NOFIT = 0, 1, 2, 3


def dense_template_names(hwp_order, ground_order, poly_order, split, leftright, rightleft):
    """Names of the dense templates in the reference's order (filterbin.py:1140-1146, :1173-1197)."""
    names = []
    for order in range(1, (hwp_order or 0) + 1):
        names += [f"HWPSS-cos-{order}", f"HWPSS-sin-{order}"]
    if ground_order is not None:
        min_order = 0 if poly_order is None else poly_order + 1
        for order in range(min_order, ground_order + 1):
            if split:
                names += [f"ground-poly-{order}-{leftright}", f"ground-poly-{order}-{rightleft}"]
            else:
                names.append(f"ground-poly-{order}")
    return names


def trim_intervals(spans, n_samp, bad, n_term):
    """filterbin.py:1383-1402.  ``spans``: (first, last) of the view's intervals, ``bad``: the shared-flagged samples
    BEFORE this call.  Returns (index in the view, start, stop) of the intervals that carry templates and the
    (first, last) of those too short to filter, whose whole length gets ``filter_flag_mask`` in the shared flags."""
    kept, flagged = [], []
    for i, (first, last) in enumerate(spans):
        first, last = max(int(first), 0), min(int(last), n_samp)
        istart, istop = first, last
        while istart < istop and bad[istart]:
            istart += 1
        while istop - 1 > istart and bad[istop - 1]:
            istop -= 1
        if istop - istart < n_term:
            flagged.append((first, last))
            continue
        kept.append((i, istart, istop))
    return kept, flagged


def unpack_symmetric(packed, k):
    """[..., k (k + 1) / 2] upper triangles packed row by row -> [..., k, k]."""
    out = np.zeros(packed.shape[:-1] + (k, k))
    q = 0
    for a in range(k):
        for b in range(a, k):
            out[..., a, b] = packed[..., q]
            out[..., b, a] = packed[..., q]
            q += 1
    return out


def reference_covariance(invcov, rcond_limit):
    """`SparseTemplates.build_template_covariance` after the matrix is formed (filterbin.py:212-251): the template
    covariance and the route taken, or (None, ROUTE_REJECTED)."""
    try:
        cond = np.linalg.cond(invcov)
        rcond = 0 if np.isinf(cond) else 1 / cond
    except np.linalg.LinAlgError:
        return None, ROUTE_REJECTED
    if rcond == 0:
        return None, ROUTE_REJECTED
    if rcond > np.abs(rcond_limit):
        return np.linalg.inv(invcov), ROUTE_INV
    if rcond_limit < 0:
        return None, ROUTE_REJECTED
    return np.linalg.pinv(invcov, rcond=1e-10, hermitian=True), ROUTE_PINV


def solve_blocks(A, r, B, C, p, act_d, act_p, Dd, Dp, rcond_limit):
    """Amplitudes of the unit-norm templates for a stack of detectors.

    A [n, Nd, Nd], r [n, Nd], B [n, V, K, K], C [n, V, Nd, K], p [n, V, K]: the unnormalised blocks under the final
    good samples; act_d [n, Nd], act_p [n, V, K]: the templates that survived the maskings; Dd, Dp: the squared norms
    they were normalised with.  Returns (amp_d [n, Nd], amp_p [n, V, K], route [n], fast [n]); amplitudes of inactive
    templates and of rejected detectors are zero.

    Fast route: with S = A - sum_v C_v B_v^-1 C_v^T the matrix is L diag(S, B_v) L^T, L = [[I, C B^-1], [0, I]], so
    lambda_min(M) >= min(lambda_min(S), lambda_min(B_v)) / (1 + ||B^-1 C^T||_F)^2, and lambda_max(M) <= min(trace,
    ||M||_inf).  Where that lower bound of rcond(M) exceeds 2 |rcond_limit| the reference would invert, and block
    elimination is that inverse applied; every other detector takes the reference's decision on the full matrix."""
    n, nd = r.shape
    n_iv, k = p.shape[1], p.shape[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.where(act_d, 1 / np.sqrt(np.where(act_d, Dd, 1.0)), 0.0)
        sp = np.where(act_p, 1 / np.sqrt(np.where(act_p, Dp, 1.0)), 0.0)
    sd[~np.isfinite(sd)] = 0.0
    sp[~np.isfinite(sp)] = 0.0
    An = A * sd[:, :, None] * sd[:, None, :]
    i = np.arange(nd)
    An[:, i, i] += ~act_d                  # an inactive template: an uncoupled unit entry, zero right-hand side
    Bn = B * sp[..., :, None] * sp[..., None, :]
    j = np.arange(k)
    Bn[:, :, j, j] += ~act_p
    Cn = C * sd[:, None, :, None] * sp[:, :, None, :]
    rn, pn = r * sd, p * sp
    amp_d, amp_p = np.zeros((n, nd)), np.zeros((n, n_iv, k))
    route = np.full(n, ROUTE_INV, dtype=np.int32)
    if n == 0:
        return amp_d, amp_p, route, np.zeros(0, dtype=bool)
    lam = np.full(n, np.inf)
    tau2 = np.zeros(n)
    rowsum = np.zeros(n)
    S, rhs = An.copy(), rn.copy()
    Binv = c_flat = None
    if n_iv > 0:
        # (the blocks are symmetric: their smallest eigenvalue, not positive for a singular or indefinite block)
        ev = np.linalg.eigvalsh(np.where(np.isfinite(Bn), Bn, 0.0))[..., 0]                     # [n, V]
        ok = np.isfinite(Bn).all(axis=(2, 3)) & (ev > 0)
        lam = np.where(ok.all(axis=1), ev.min(axis=1), 0.0)
        Bsafe = np.where(ok[:, :, None, None], Bn, np.eye(k))
        Binv = np.linalg.inv(Bsafe)
        W = np.matmul(Binv, np.swapaxes(Cn, 2, 3))                                             # B^-1 C^T  [n, V, K, Nd]
        c_flat = np.ascontiguousarray(np.transpose(Cn, (0, 2, 1, 3))).reshape(n, nd, n_iv * k)   # C  [n, Nd, V K]
        S -= np.matmul(c_flat, W.reshape(n, n_iv * k, nd))
        rhs -= np.matmul(c_flat, np.matmul(Binv, pn[..., None]).reshape(n, n_iv * k, 1))[..., 0]
        tau2 = np.sum(W * W, axis=(1, 2, 3))
        rowsum = np.max(np.sum(np.abs(Bn), axis=3) + np.sum(np.abs(Cn), axis=2), axis=(1, 2))
    if nd > 0:
        ok_s = np.isfinite(S).all(axis=(1, 2))
        ev = np.linalg.eigvalsh(np.where(ok_s[:, None, None], (S + np.swapaxes(S, 1, 2)) / 2, 0.0))[:, 0]
        lam = np.minimum(lam, np.where(ok_s, ev, 0.0))
        dense_rows = np.sum(np.abs(An), axis=2) + (np.sum(np.abs(Cn), axis=(1, 3)) if n_iv > 0 else 0.0)
        rowsum = np.maximum(rowsum, np.max(dense_rows, axis=1))
    lam_max = np.minimum(rowsum, float(nd + n_iv * k))
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = lam / ((1 + np.sqrt(tau2)) ** 2 * lam_max)
    fast = np.isfinite(bound) & (bound > 2 * np.abs(rcond_limit))
    sel = np.nonzero(fast)[0]
    if sel.size > 0:
        a = np.linalg.solve(S[sel], rhs[sel][..., None])[..., 0] if nd > 0 else np.zeros((sel.size, 0))
        amp_d[sel] = a
        if n_iv > 0:
            ct_a = np.matmul(np.swapaxes(c_flat[sel], 1, 2), a[..., None]).reshape(sel.size, n_iv, k)     # C^T a
            amp_p[sel] = np.matmul(Binv[sel], (pn[sel] - ct_a)[..., None])[..., 0]
    for d in np.nonzero(~fast)[0]:
        # the reference route: the full normalised matrix over the surviving templates, in the reference's order
        id_, ip_ = np.nonzero(act_d[d])[0], np.nonzero(act_p[d].ravel())[0]
        ntot = id_.size + ip_.size
        M = np.zeros((ntot, ntot))
        M[:id_.size, :id_.size] = An[d][np.ix_(id_, id_)]
        if n_iv > 0:
            full_b = np.zeros((n_iv * k, n_iv * k))
            for v in range(n_iv):
                full_b[v * k:(v + 1) * k, v * k:(v + 1) * k] = Bn[d, v]
            M[id_.size:, id_.size:] = full_b[np.ix_(ip_, ip_)]
            cross = np.transpose(Cn[d], (1, 0, 2)).reshape(nd, n_iv * k)[np.ix_(id_, ip_)]
            M[:id_.size, id_.size:] = cross
            M[id_.size:, :id_.size] = cross.T
        cov, route[d] = reference_covariance(M, rcond_limit)
        if cov is None:
            continue
        amps = np.dot(cov, np.concatenate([rn[d][id_], pn[d].ravel()[ip_]]))
        amp_d[d, id_] = amps[:id_.size]
        flat = np.zeros(n_iv * k)
        flat[ip_] = amps[id_.size:]
        amp_p[d] = flat.reshape(n_iv, k)
    return amp_d, amp_p, route, fast


def regress(backend, n_det, n_samp, dense_first, dense_last, starts, stops, n_term, rcond_limit):
    """The detector loop of filterbin.py:854-1003 for all detectors of an observation.

    ``backend.blocks(rows)`` -> dict with, for the detectors ``rows`` under their CURRENT flags: n_good [m], nnz_d [m, Nd],
    nnz_p [m, V, K] (good samples, good non-zero samples per template), A [m, Nd, Nd], r [m, Nd], B [m, V, KP], C [m, V,
    Nd, K], p [m, V, K].  ``backend.flag(spans)`` ORs the filter flag into (row, first, last) stretches of the detector
    flags.  ``backend.subtract(rows, a, b)`` subtracts the fit with coefficients of the UNNORMALISED templates.

    Returns dict(route [n_det], amp_d, amp_p, act_d, act_p, flag_detector [n_det] bool: no good sample before any masking
    (:873-876), fast [n_det] bool)."""
    nd, n_iv, k = len(dense_first), len(starts), n_term
    dense_first, dense_last = np.asarray(dense_first, dtype=np.int64), np.asarray(dense_last, dtype=np.int64)
    starts, stops = np.asarray(starts, dtype=np.int64), np.asarray(stops, dtype=np.int64)
    # a template of one sample is dropped when it is appended (SparseTemplates.append :131-133)
    act_d = np.tile(dense_last > dense_first, (n_det, 1))
    act_p = np.tile((stops - starts > 1)[None, :, None], (n_det, 1, k)) if n_iv > 0 else np.zeros((n_det, 0, k), dtype=bool)
    Dd, Dp = np.zeros((n_det, nd)), np.zeros((n_det, n_iv, k))
    A, r = np.zeros((n_det, nd, nd)), np.zeros((n_det, nd))
    B, C, p = np.zeros((n_det, n_iv, k, k)), np.zeros((n_det, n_iv, nd, k)), np.zeros((n_det, n_iv, k))
    route = np.full(n_det, ROUTE_NOFIT, dtype=np.int32)
    flag_detector = np.zeros(n_det, dtype=bool)
    done = np.zeros(n_det, dtype=bool)
    diag_q = np.cumsum([0] + [k - a for a in range(k - 1)]).astype(np.int64) if k > 0 else np.zeros(0, dtype=np.int64)
    pending = np.arange(n_det)
    for stage in range(3):
        if pending.size == 0:
            break
        blk = backend.blocks(pending)
        spans, again = [], []
        for m, d in enumerate(pending):
            if blk["n_good"][m] == 0:
                spans.append((d, 0, n_samp))
                flag_detector[d] = stage == 0
                continue
            diag_a = np.diagonal(blk["A"][m]).copy() if nd > 0 else np.zeros(0)
            diag_b = blk["B"][m][:, diag_q] if n_iv > 0 else np.zeros((0, k))
            if stage < 2:
                # SparseTemplates.mask: a template without a non-zero good sample is dropped and its span flagged
                null_d = act_d[d] & (blk["nnz_d"][m] == 0)
                null_p = act_p[d] & (blk["nnz_p"][m] == 0)
                act_d[d] &= ~null_d
                act_p[d] &= ~null_p
                Dd[d], Dp[d] = diag_a, diag_b
                if null_d.any() or null_p.any():
                    spans += [(d, int(dense_first[t]), int(dense_last[t]) + 1) for t in np.nonzero(null_d)[0]]
                    spans += [(d, int(starts[v]), int(stops[v])) for v in np.nonzero(null_p.any(axis=1))[0]]
                    again.append(d)
                    continue
            A[d], r[d], C[d], p[d] = blk["A"][m], blk["r"][m], blk["C"][m], blk["p"][m]
            B[d] = unpack_symmetric(blk["B"][m], k)
            done[d] = True
        backend.flag(spans)
        pending = np.array(again, dtype=np.int64)
    fit = np.nonzero(done & (act_d.any(axis=1) | act_p.any(axis=(1, 2))))[0]
    amp_d, amp_p = np.zeros((n_det, nd)), np.zeros((n_det, n_iv, k))
    fast = np.zeros(n_det, dtype=bool)
    if fit.size > 0:
        amp_d[fit], amp_p[fit], route[fit], fast[fit] = solve_blocks(
            A[fit], r[fit], B[fit], C[fit], p[fit], act_d[fit], act_p[fit], Dd[fit], Dp[fit], rcond_limit)
        rejected = fit[route[fit] == ROUTE_REJECTED]
        backend.flag([(d, 0, n_samp) for d in rejected])
        good = fit[route[fit] != ROUTE_REJECTED]
        if good.size > 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                sd = np.where(act_d[good], 1 / np.sqrt(np.where(act_d[good], Dd[good], 1.0)), 0.0)
                sp = np.where(act_p[good], 1 / np.sqrt(np.where(act_p[good], Dp[good], 1.0)), 0.0)
            backend.subtract(good, amp_d[good] * sd, amp_p[good] * sp)
    return dict(route=route, amp_d=amp_d, amp_p=amp_p, act_d=act_d, act_p=act_p, flag_detector=flag_detector, fast=fast)


class _DeviceBackend:
    """``regress`` on the device-resident signal and flags of one observation."""

    def __init__(self, op, D, dense, n_dense, n_samp, dd, dets, fd, shared_ptr, starts, stops):
        self.op, self.D, self.dense, self.nd, self.n = op, D, dense, n_dense, n_samp
        self.dd, self.fd, self.shared_ptr = dd, fd, shared_ptr
        self.sidx = dd.indices(dets)
        self.fidx = fd.indices(dets) if fd is not None else None
        self.starts, self.stops = starts, stops
        self.k = (op.poly_filter_order + 1) if op.poly_filter_order is not None else 1
        self.seconds = dict(dense_fit=0.0, interval_accumulate=0.0, subtract=0.0)

    def _dense_ptr(self):
        return accel_device_ptr(self.dense) if self.nd > 0 else 0

    def _flag_ptr(self):
        return accel_device_ptr(self.fd.buffer) if self.fd is not None else 0

    def blocks(self, rows):
        op, D, nd, n, k = self.op, self.D, self.nd, self.n, self.k
        m, n_iv, kp = len(rows), len(self.starts), self.k * (self.k + 1) // 2
        sidx = self.sidx[rows]
        fidx = self.fidx[rows] if self.fidx is not None else None
        sig_ptr, f_ptr = accel_device_ptr(self.dd.buffer), self._flag_ptr()
        with device_scratch(op.name, owner=op) as s:
            n_good = s.out("n_good", np.zeros(m, dtype=np.int64))
            nnz_d = s.out("nnz_d", np.zeros((m, nd), dtype=np.int64))
            proj = s.out("proj", np.zeros((m, nd)))
            gram = s.out("gram", np.zeros((nd, nd)))
            dgram = s.out("dgram", np.zeros((m, nd, nd)))
            s.work("nflag", np.zeros(m, dtype=np.int64))
            p = s.out("p", np.zeros((m, n_iv, k)))
            nnz_p = s.out("nnz_p", np.zeros((m, n_iv, k), dtype=np.int64))
            bc = s.out("bc", np.zeros((n_iv, kp)))
            cc = s.out("cc", np.zeros((n_iv, nd, k)))
            bf = s.out("bf", np.zeros((m, n_iv, kp)))
            cf = s.out("cf", np.zeros((m, n_iv, nd, k)))
            t0 = self._lap()
            D.filterbin_good_counts(self._dense_ptr(), nd, n, fidx, f_ptr, op.det_flag_mask, self.shared_ptr,
                                    op.shared_flag_mask, m, s.ptr("n_good"), s.ptr("nnz_d"))
            if nd > 0:
                D.template_fit(self._dense_ptr(), nd, n, sidx, sig_ptr, fidx, f_ptr, op.det_flag_mask, self.shared_ptr,
                               op.shared_flag_mask, s.ptr("proj"), s.ptr("gram"), s.ptr("dgram"), s.ptr("nflag"))
            t0 = self._lap("dense_fit", t0)
            if n_iv > 0:
                D.filterbin_accumulate(k - 1, self._dense_ptr(), nd, n, sidx, sig_ptr, fidx, f_ptr, op.det_flag_mask,
                                       self.shared_ptr, op.shared_flag_mask, self.starts, self.stops, s.ptr("p"),
                                       s.ptr("nnz_p"), s.ptr("bc"), s.ptr("cc"), s.ptr("bf"), s.ptr("cf"))
            self._lap("interval_accumulate", t0)
        return dict(n_good=n_good, nnz_d=nnz_d, nnz_p=nnz_p, A=gram[None] - dgram, r=proj, B=bc[None] - bf, C=cc[None] - cf,
                    p=p)

    def _lap(self, key=None, t0=None):
        if not self.op.report_timing:
            return None
        native().accel_synchronize()
        now = time.perf_counter()
        if key is not None:
            self.seconds[key] += now - t0
        return now

    def flag(self, spans):
        if len(spans) == 0:
            return
        if self.fd is None:
            raise RuntimeError("FilterBin: samples cannot be flagged without det_flags")
        rows = self.fidx[[s[0] for s in spans]]
        self.D.filterbin_flag_spans(rows, [s[1] for s in spans], [s[2] for s in spans], self.fd.buffer.shape[0], self.n,
                                    self._flag_ptr(), self.op.filter_flag_mask)

    def subtract(self, rows, a, b):
        t0 = self._lap()
        with device_scratch(self.op.name, owner=self.op) as s:
            s.inp("a", np.ascontiguousarray(a))
            s.inp("b", np.ascontiguousarray(b))
            self.D.filterbin_subtract(self.k - 1, self._dense_ptr(), self.nd, self.n, self.sidx[rows],
                                      accel_device_ptr(self.dd.buffer), s.ptr("a"), self.starts, self.stops, s.ptr("b"))
        self._lap("subtract", t0)


class FilterBin(Operator):
    """FilterBin builds a template matrix and projects out compromised modes.  It then bins the signal.

    ``amplitudes[obs.name][det]``: dict of the fitted amplitudes of the unit-norm templates by the reference's template
    names, or None for a detector that was not fitted; ``routes[obs.name][det]``: ROUTE_INV / ROUTE_PINV /
    ROUTE_REJECTED / ROUTE_NOFIT; ``seconds``: wall time per phase of the last call (with ``report_timing``).
    What the reference operator has and this one leaves out is listed in the module docstring."""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key for the timestream data")
    det_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    filter_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for flagging samples that fail filtering")
    filter_detector_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for detectors that fail filtering")
    det_flag_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for detector sample flagging")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_nonscience, help="Bit mask value for optional telescope flagging")
    hwp_angle = Unicode(defaults.hwp_angle, allow_none=True, help="Observation shared key for HWP angle")
    binning = Instance(klass=Operator, allow_none=True, help="Binning operator for map making.")
    azimuth = Unicode(defaults.azimuth, allow_none=True, help="Observation shared key for Azimuth")
    hwp_filter_order = Int(None, allow_none=True, help="Order of HWP-synchronous signal filter.")
    ground_filter_order = Int(None, allow_none=True,
                              help="Order of a Legendre polynomial to fit as a function of azimuth.")
    split_ground_template = Bool(False, help="Apply a different template for left and right scans")
    leftright_interval = Unicode(defaults.throw_leftright_interval, help="Intervals for left-to-right scans")
    rightleft_interval = Unicode(defaults.throw_rightleft_interval, help="Intervals for right-to-left scans")
    poly_filter_order = Int(1, allow_none=True, help="Polynomial order")
    poly_filter_view = Unicode("throw", allow_none=True, help="Intervals for polynomial filtering")
    write_binmap = Bool(False, help="If True, bin (and keep) the unfiltered map")
    keep_final_products = Bool(False, help="If True, keep the map domain products in data")
    rcond_threshold = Float(1.0e-3, help="Minimum value for inverse pixel condition number cut.")
    reset_pix_dist = Bool(False, help="Clear any existing pixel distribution.  Useful when applying"
                                      "repeatedly to different data objects.")
    template_rcond_limit = Float(1e-6, allow_none=False,
                                 help="Threshold for handling degenerate template covariances.  "
                                      "If the limit is is positive and rcond < limit, use pseudoinverse.  "
                                      "If the limit is negative and rcond < abs(limit), reject detector.")
    report_timing = Bool(False, help="Synchronise around every phase and fill ``seconds`` (costs the overlap)")
    write_noiseweighted_binmap = Bool(False, help="If True, bin (and keep) the noise-weighted unfiltered map")
    # What is left out keeps its name and default, as PolyFilter2D / CommonModeFilter do for theirs: any other value raises.
    write_obs_matrix = Bool(False, help="Not supported: must stay False")
    noiseweight_obs_matrix = Bool(False, help="Not supported: must stay False")
    nskip = Int(1, help="Not supported: must stay 1")
    cache_dir = Unicode(None, allow_none=True, help="Not supported: must stay None")
    deproject_map = Unicode(None, allow_none=True, help="Not supported: must stay None")
    deproject_nnz = Int(1, help="Not supported (deprojection)")
    deproject_pattern = Unicode(".*", help="Not supported (deprojection)")
    precomputed_templates = Unicode(None, allow_none=True, help="Not supported: must stay None")
    precomputed_template_view = Unicode("throw", allow_none=True, help="Not supported (precomputed templates)")
    ground_filter_bin_width = Float(None, allow_none=True, help="Not supported: must stay None")
    ground_template_expansion_order = Int(None, allow_none=True, help="Not supported: must stay None")
    ground_template_time_step = Int(None, allow_none=True, help="Not supported: must stay None")
    filter_config_file = Unicode(None, allow_none=True, help="Not supported: must stay None")
    maskfile = Unicode(None, allow_none=True, help="Not supported: must stay None")
    mc_mode = Bool(False, help="Not supported: must stay False")
    mc_index = Int(None, allow_none=True, help="Not supported (Monte-Carlo mode)")
    amplitude_dir = Unicode(None, allow_none=True, help="Not supported: must stay None")
    n_save_templates = Int(0, help="Not supported (amplitude_dir)")

    UNSUPPORTED = dict(write_obs_matrix=False, noiseweight_obs_matrix=False, nskip=1, cache_dir=None, deproject_map=None,
                       precomputed_templates=None, ground_filter_bin_width=None, ground_template_expansion_order=None,
                       ground_template_time_step=None, filter_config_file=None, maskfile=None, mc_mode=False,
                       amplitude_dir=None)

    def _validate_det_mask(self, value):
        if value < 0:
            raise ValueError("Det mask should be a positive integer")
        return value

    def _validate_det_flag_mask(self, value):
        if value < 0:
            raise ValueError("Det flag mask should be a positive integer")
        return value

    def _validate_shared_flag_mask(self, value):
        if value < 0:
            raise ValueError("Shared flag mask should be a positive integer")
        return value

    def _validate_binning(self, value):
        # filterbin.py:625-650
        if value is not None:
            for trt in ("pixel_dist", "pixel_pointing", "stokes_weights", "binned", "covariance", "det_flags",
                        "det_flag_mask", "shared_flags", "shared_flag_mask", "noise_model", "full_pointing", "sync_type"):
                if not value.has_trait(trt):
                    raise ValueError(f"binning class does not have a {trt} trait")
        return value

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.amplitudes = {}
        self.routes = {}
        self.seconds = {}

    # ------------------------------------------------------------------ common templates
    def _phase(self, obs):
        """filterbin.py:1796-1816."""
        try:
            azmin, azmax = obs["scan_min_az"], obs["scan_max_az"]
            azmin = float(azmin.to_value("rad")) if hasattr(azmin, "to_value") else float(azmin)
            azmax = float(azmax.to_value("rad")) if hasattr(azmax, "to_value") else float(azmax)
            az = np.array(obs.shared[self.azimuth].data, dtype=np.float64)
        except Exception as e:
            raise RuntimeError(f"Failed to get boresight azimuth from TOD.  Perhaps it is not ground TOD? '{e}'")
        return (np.unwrap(az) - azmin) / (azmax - azmin) * 2 - 1

    def _direction_mask(self, obs, name, n):
        mask = np.zeros(n, dtype=np.int32)
        for ival in obs.intervals[name]:
            mask[max(int(ival.first), 0):int(ival.last)] = 1
        return mask

    def build_dense_templates(self, obs):
        """The HWP and ground templates of one observation in HBM (filterbin.py:1120-1238), in the reference's order:
        (host array keying the [Nd, n_samp] device buffer or None, names, first, last non-zero sample per row)."""
        from .. import capi

        D = capi.dev
        n = obs.n_local_samples
        n_hwp = 2 * self.hwp_filter_order if self.hwp_filter_order is not None else 0
        if n_hwp > 0 and (self.hwp_angle is None or self.hwp_angle not in obs.shared):
            raise RuntimeError(f"Cannot apply HWP filtering at order = {self.hwp_filter_order}: "
                               f"no HWP angle found under key = '{self.hwp_angle}'")
        min_order = 0 if self.poly_filter_order is None else self.poly_filter_order + 1
        n_ground = max(self.ground_filter_order - min_order + 1, 0) if self.ground_filter_order is not None else 0
        mult = 2 if self.split_ground_template else 1
        nd = max(n_hwp, 0) + mult * n_ground
        names = dense_template_names(self.hwp_filter_order if n_hwp > 0 else None,
                                     self.ground_filter_order if n_ground > 0 else None, self.poly_filter_order,
                                     self.split_ground_template, self.leftright_interval, self.rightleft_interval)
        assert len(names) == nd
        if nd == 0:
            return None, names, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        dense = np.empty((nd, n), dtype=np.float64)
        accel_data_create(dense, f"{self.name}_templates", owner=self)
        try:
            with device_scratch(self.name, owner=self) as s:
                t_ptr = accel_device_ptr(dense)
                row_ptr = lambda r: t_ptr + 8 * n * r  # noqa: E731
                if n_hwp > 0:
                    s.inp("angle", np.array(obs.shared[self.hwp_angle].data, dtype=np.float64))
                    D.fourier_templates(s.ptr("angle"), n, 1, self.hwp_filter_order + 1, row_ptr(0))
                if n_ground > 0:
                    s.inp("phase", self._phase(obs))
                    if not self.split_ground_template:
                        D.legendre_templates(s.ptr("phase"), n, min_order, self.ground_filter_order + 1, row_ptr(n_hwp))
                    else:
                        s.work("rows", np.empty(n_ground * n, dtype=np.float64))
                        s.inp("lr", self._direction_mask(obs, self.leftright_interval, n))
                        s.inp("rl", self._direction_mask(obs, self.rightleft_interval, n))
                        tmp = s.ptr("rows")
                        D.legendre_templates(s.ptr("phase"), n, min_order, self.ground_filter_order + 1, tmp)
                        for r in range(n_ground):
                            for c, key in enumerate(("lr", "rl")):      # zero inside that direction's intervals
                                D.template_select(tmp + 8 * n * r, s.ptr(key), 1, False, n, row_ptr(n_hwp + 2 * r + c))
                first = s.out("first", np.zeros(nd, dtype=np.int64))
                last = s.out("last", np.zeros(nd, dtype=np.int64))
                D.template_spans(t_ptr, nd, n, s.ptr("first"), s.ptr("last"))
        except BaseException:
            accel_data_delete(dense, f"{self.name}_templates")
            raise
        return dense, names, first, last

    def _poly_intervals(self, obs):
        """The intervals that carry polynomial templates (filterbin.py:1372-1410); too short ones are flagged in the
        SHARED flags, on the host and on the device copy."""
        n = obs.n_local_samples
        if self.poly_filter_order is None:
            return []
        if self.poly_filter_order > _max_order():
            raise RuntimeError(f"FilterBin: poly_filter_order {self.poly_filter_order} exceeds the {_max_order()} of the "
                               "device kernels")
        sf = obs.shared[self.shared_flags] if self.shared_flags is not None else None
        on_device = sf is not None and sf.accel_exists()
        if on_device and sf.accel_in_use():
            sf.accel_update_host()
        bad = (sf.data & self.shared_flag_mask) != 0 if sf is not None else np.zeros(n, dtype=bool)
        spans = [(iv.first, iv.last) for iv in obs.intervals[self.poly_filter_view]]
        kept, flagged = trim_intervals(spans, n, bad, self.poly_filter_order + 1)
        if sf is not None and len(flagged) > 0:
            for first, last in flagged:
                sf.data[first:last] |= sf.data.dtype.type(self.filter_flag_mask)
            if on_device:
                sf.accel_update_device()
        for (_, _, stop), (_, start, _) in zip(kept[:-1], kept[1:]):
            if start < stop:
                raise RuntimeError("FilterBin: the intervals of poly_filter_view must be sorted and disjoint")
        return kept

    # ------------------------------------------------------------------ filtering
    def _filter_observation(self, data, obs, detectors):
        from .. import capi

        D = capi.dev
        dets = obs.select_local_detectors(detectors, flagmask=self.det_mask)
        self.amplitudes[obs.name] = {det: None for det in dets}
        self.routes[obs.name] = {det: ROUTE_NOFIT for det in dets}
        n = obs.n_local_samples
        t0 = time.perf_counter()
        kept = self._poly_intervals(obs)          # first: it may add shared flags
        dense, names, first, last = self.build_dense_templates(obs)
        if self.report_timing:
            native().accel_synchronize()
        self.seconds["template_build"] = self.seconds.get("template_build", 0.0) + time.perf_counter() - t0
        try:
            if len(dets) == 0:
                return
            dd = obs.detdata[self.det_data]
            if dd.dtype != np.dtype(np.float64):
                raise RuntimeError(f"detdata '{self.det_data}' is {dd.dtype}: FilterBin works in place on float64 timestreams")
            signal = Resident(dd, self.det_data)
            fd = make_resident(obs.detdata[self.det_flags], self.det_flags) if self.det_flags is not None else None
            shared_ptr = 0
            if self.shared_flags is not None:
                shared_ptr = accel_device_ptr(make_resident(obs.shared[self.shared_flags], self.shared_flags).data)
            starts = np.array([s[1] for s in kept], dtype=np.int64)
            stops = np.array([s[2] for s in kept], dtype=np.int64)
            k = self.poly_filter_order + 1 if self.poly_filter_order is not None else 1
            backend = _DeviceBackend(self, D, dense, len(names), n, dd, dets, fd, shared_ptr, starts, stops)
            t0 = time.perf_counter()
            res = regress(backend, len(dets), n, first, last, starts, stops, k, self.template_rcond_limit)
            total = time.perf_counter() - t0
            for key, value in backend.seconds.items():
                self.seconds[key] = self.seconds.get(key, 0.0) + value
            self.seconds["host_algebra"] = self.seconds.get("host_algebra", 0.0) + total - sum(backend.seconds.values())
            for i, det in enumerate(dets):
                self.routes[obs.name][det] = int(res["route"][i])
                cur = obs.local_detector_flags.get(det, 0)
                if res["flag_detector"][i]:
                    obs.update_local_detector_flags({det: cur | self.filter_flag_mask})
                if res["route"][i] == ROUTE_REJECTED:
                    obs.update_local_detector_flags({det: cur | self.filter_detector_mask})
                if res["route"][i] in (ROUTE_INV, ROUTE_PINV):
                    amps = {names[t]: float(res["amp_d"][i, t]) for t in np.nonzero(res["act_d"][i])[0]}
                    for v, (index, _, _) in enumerate(kept):
                        for j in np.nonzero(res["act_p"][i, v])[0]:
                            amps[f"poly-{j}-interval-{index}"] = float(res["amp_p"][i, v, j])
                    self.amplitudes[obs.name][det] = amps
            signal.write_back_unless_lazy(data)
        finally:
            if dense is not None:
                accel_data_delete(dense, f"{self.name}_templates")

    def _exec(self, data, detectors=None, **kwargs):
        if len(data.obs) == 0:
            return
        if self.binning is None:
            raise RuntimeError("You must set the 'binning' trait before calling exec()")
        for trait, value in self.UNSUPPORTED.items():
            if getattr(self, trait) != value:
                raise NotImplementedError(f"FilterBin: {trait}={getattr(self, trait)!r} is not supported "
                                          "(see the module docstring for what is left out)")
        # samples that fail filtering must not contribute to maps (filterbin.py:726-744)
        for what, mask in (("det flag mask", self.det_flag_mask), ("shared mask", self.shared_flag_mask),
                           ("det bin mask", self.binning.det_flag_mask), ("shared bin mask", self.binning.shared_flag_mask)):
            if self.filter_flag_mask & mask == 0:
                raise RuntimeError(f"Filter flag mask does not overlap with {what}: {self.filter_flag_mask} & {mask} = 0")
        if not accel_enabled():
            raise RuntimeError("FilterBin needs the HIP library and an assigned device (no host path)")
        binning = self.binning
        if self.reset_pix_dist:
            if binning.pixel_dist in data:
                del data[binning.pixel_dist]
            if binning.covariance in data:
                del data[binning.covariance]        # cannot trust earlier covariance
        if binning.pixel_dist not in data:
            BuildPixelDistribution(pixel_dist=binning.pixel_dist, pixel_pointing=binning.pixel_pointing).apply(data)
        self.amplitudes, self.routes, self.seconds = {}, {}, {}
        self._bin_map(data, detectors, filtered=False)
        for obs in data.obs:
            self._filter_observation(data, obs, detectors)
        self._bin_map(data, detectors, filtered=True)

    def _bin_map(self, data, detectors, filtered):
        """filterbin.py:2059-2176 without the writers."""
        if not filtered and not self.write_binmap and not self.write_noiseweighted_binmap:
            return
        t0 = time.perf_counter()
        tag = "filtered" if filtered else "unfiltered"
        hits_name, invcov_name = f"{self.name}_{tag}_hits", f"{self.name}_{tag}_invcov"
        cov_name, rcond_name = f"{self.name}_{tag}_cov", f"{self.name}_{tag}_rcond"
        map_name, noiseweighted_map_name = f"{self.name}_{tag}_map", f"{self.name}_noiseweighted_{tag}_map"
        binning = self.binning
        binning.noiseweighted = noiseweighted_map_name
        binning.binned = map_name
        binning.det_data = self.det_data
        binning.covariance = cov_name
        # always (re)build the inverse covariance: detector flagging may change during filtering
        for key in (hits_name, invcov_name, cov_name, rcond_name, map_name, noiseweighted_map_name):
            if key in data:
                del data[key]
        CovarianceAndHits(
            pixel_dist=binning.pixel_dist, covariance=binning.covariance, inverse_covariance=invcov_name, hits=hits_name,
            rcond=rcond_name, det_mask=binning.det_mask, det_flags=binning.det_flags, det_flag_mask=binning.det_flag_mask,
            det_data_units=binning.det_data_units, shared_flags=binning.shared_flags,
            shared_flag_mask=binning.shared_flag_mask, pixel_pointing=binning.pixel_pointing,
            stokes_weights=binning.stokes_weights, noise_model=binning.noise_model, rcond_threshold=self.rcond_threshold,
            sync_type=binning.sync_type, save_pointing=binning.full_pointing).apply(data, detectors=detectors)
        binning.apply(data, detectors=detectors)
        if not self.keep_final_products:
            for key in (hits_name, rcond_name, noiseweighted_map_name, map_name, invcov_name, cov_name):
                if key in data:
                    del data[key]
        if self.report_timing:
            native().accel_synchronize()
        self.seconds[f"bin_{tag}"] = time.perf_counter() - t0

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [self.times], "detdata": [self.det_data], "intervals": []}
        for key in (self.shared_flags, self.azimuth, self.hwp_angle):
            if key is not None:
                req["shared"].append(key)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        for key in (self.poly_filter_view, self.leftright_interval, self.rightleft_interval):
            if key is not None:
                req["intervals"].append(key)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": [self.det_data]}


def _max_order():
    from .. import capi

    return capi.dev.filterbin_max_order()
