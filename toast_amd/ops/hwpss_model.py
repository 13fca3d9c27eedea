"""HWPSynchronousModel: fit and remove the half-wave-plate synchronous signal (reference:
src/toast/ops/hwpss_model.py:26-960, src/toast/hwp_utils.py:43-392).

The model of a detector is a comb at the harmonics of the HWP angle,
``sum_h [c_h0 + c_h1 t] sin(h a) + [c_h2 + c_h3 t] cos(h a)`` (the ``t`` terms with ``time_drift``), fitted by least
squares either once per observation or per chunk (``chunk_time``: overlapping chunks; ``chunk_view``: the intervals of a
view) and then interpolated between the chunk centres with a smoothing cubic spline per coefficient.

Two paths, as in ``Demodulate``:

* detector data resident on the device (or ``use_accel=True``): the Gram matrices, the right-hand sides, the model
  subtraction, the flag update and the continuous calibration run in ``csrc/hwpss.hip``; the host sees the Gram
  matrices, the right-hand sides and one sum per detector.  No buffer of sin / cos values is ever written to memory.
* data on the host (and more coefficients per detector than ``toast_hip_hwpss_max_coeff()``): NumPy.

Both share the host work that is small: chunking, the combined shared flags, the ``n_coeff x n_coeff`` solves, the
spline fits (``scipy.interpolate.splrep``), the 2f magnitudes and the outlier cut.

Two quirks of the reference are kept: the Gram matrix of a chunk is built from the shared flags only while the
right-hand sides use the detector's own good samples, and the sample flags receive the uint8 product
``((det_flags & det_flag_mask) | shared) * hwp_flag_mask`` of the flag VALUE.

With ``time_drift`` the basis ``[sin, t sin]`` becomes collinear once ``t`` hardly varies over a chunk relative to its
size: a chunk late in a long observation (rcond ~ 2e-12 for a 3 s chunk 3500 s after the start) fails the reference's
own ``rcond < 1e-8`` test and is flagged, here as there.

Not reproduced: ``fill_gaps`` (the reference draws from NumPy's global, unseeded generator), ``debug`` plots, and the
gather of the magnitudes over the column communicator in the outlier cut: the cut runs over the process's local
detectors."""

import numpy as np
import scipy.interpolate
from scipy.linalg import eigvalsh, lu_factor, lu_solve

from ..accel import Resident, accel_enabled, device_scratch
from ..data import defaults
from ..traits import Bool, Float, Int, TraitError, Unicode
from .operator import Operator


def n_coefficients(harmonics, time_drift):
    return (4 if time_drift else 2) * int(harmonics)


def model_basis(angle, reltime, shared, harmonics, time_drift):
    """[n_samp][n_coeff]: ``[sin_1, cos_1, sin_2, ...]`` or with ``time_drift`` ``[sin_h, t sin_h, cos_h, t cos_h]`` per
    harmonic, zero where ``shared`` is not 0 (hwp_utils.py:61-69 and the coefficient order of :147-222)."""
    good = shared == 0
    n_coeff = n_coefficients(harmonics, time_drift)
    out = np.zeros((len(angle), n_coeff), dtype=np.float64)
    for h in range(harmonics):
        sn = np.sin((h + 1) * angle[good])
        cs = np.cos((h + 1) * angle[good])
        if time_drift:
            out[good, 4 * h + 0] = sn
            out[good, 4 * h + 1] = sn * reltime[good]
            out[good, 4 * h + 2] = cs
            out[good, 4 * h + 3] = cs * reltime[good]
        else:
            out[good, 2 * h + 0] = sn
            out[good, 2 * h + 1] = cs
    return out


def stopped_flags(angle):
    """1 where the HWP does not turn at its nominal rate (hwpss_model.py:930-937)."""
    hdata = np.unwrap(angle, period=2 * np.pi)
    hvel = np.gradient(hdata)
    moving = np.absolute(hvel) > 1.0e-6
    nominal = np.median(hvel[moving])
    unstable = np.absolute(hvel - nominal) > 1.0e-3 * nominal
    return np.array(unstable, dtype=np.uint8)


def solve_chunk(gram_upper, n_good_shared, n_samp, rhs, n_good, n_coeff):
    """Coefficients [n_det][n_coeff] of one chunk from the unscaled upper triangle of its Gram matrix, or None when the
    chunk has no good sample or its matrix fails the condition test (hwp_utils.py:233-252, :311-315,
    hwpss_model.py:796-815).  ``n_samp``: samples of the chunk; ``rhs`` [n_det][n_coeff], ``n_good`` [n_det]."""
    if n_good_shared == 0:
        return None
    cov = np.triu(gram_upper) * (n_samp / n_good_shared)
    cov = cov + np.triu(cov, 1).T
    evals = eigvalsh(cov)
    rcond = np.min(evals) / np.max(evals)
    if not rcond >= 1.0e-8:
        return None
    lu = lu_factor(cov)
    out = np.zeros((len(n_good), n_coeff), dtype=np.float64)
    enough = np.asarray(n_good) >= n_coeff          # not very many good samples: coefficients stay zero
    if np.any(enough):
        # one call for all detectors: every right-hand side is a column of its own
        out[enough] = lu_solve(lu, np.asarray(rhs)[enough].T).T * (n_samp / np.asarray(n_good)[enough])[:, None]
    return out


class HWPSynchronousModel(Operator):
    """Operator that models and removes HWP synchronous signal.

    This fits and optionally subtracts a Maxipol / EBEX style model for the HWPSS.  The time dependent drift term is
    optional.  The 2f component of the model is optionally used to build a relative calibration between detectors,
    either as a fixed table per observation or as continuously varying factors.  The model can be constructed with one
    set of coefficients for the entire observation, or one set per time interval smoothly interpolated across the
    observation.

    ``chunk_time`` is in seconds.  ``fill_gaps=True`` and ``debug`` raise NotImplementedError.  With ``time_drift``,
    chunks late in a long observation are ill conditioned and flagged, as in the reference (see the module docstring).

    Diagnostics of the last call, per observation name (as ``PolyFilter.coefficients``): ``coefficients[obs.name]`` =
    ``{"coeff": [n_det, n_coeff, n_chunk], "coeff_flags": [n_chunk], "detectors": names}`` and ``fit_products[obs.name]``
    = the unscaled upper triangles ``gram`` [n_chunk, n_coeff, n_coeff] with ``n_good_shared`` [n_chunk], and ``rhs``
    [n_det, n_chunk, n_coeff] with ``n_good`` [n_det, n_chunk], as the path that ran produced them."""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key")
    det_mask = Int(defaults.det_mask_invalid, help="Bit mask value for per-detector flagging")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional shared flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for detector sample flagging")
    hwp_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask to use when adding flags based on HWP filter failures.")
    hwp_angle = Unicode(defaults.hwp_angle, allow_none=True, help="Observation shared key for HWP angle")
    harmonics = Int(9, help="Number of harmonics to consider in the expansion")
    subtract_model = Bool(False, help="Subtract the model from the input data")
    save_model = Unicode(None, allow_none=True, help="Save the model to this observation key")
    chunk_view = Unicode(None, allow_none=True,
                         help="The intervals over which to independently compute the HWPSS template")
    chunk_time = Float(None, allow_none=True,
                       help="The overlapping time chunks [s] over which to compute the HWPSS template")
    relcal_fixed = Unicode(None, allow_none=True, help="Build a relative calibration dictionary in this observation key")
    relcal_continuous = Unicode(None, allow_none=True, help="Build interpolated relative calibration timestreams")
    relcal_cut_sigma = Float(5.0, help="Sigma cut for outlier rejection based on relative calibration")
    time_drift = Bool(False, help="If True, include time drift terms in the model")
    fill_gaps = Bool(False, help="If True, fill gaps with a simple noise model (not reproduced: raises)")
    debug = Unicode(None, allow_none=True, help="Path to directory for generating debug plots (not reproduced: raises)")

    def _validate_det_mask(self, check):
        if check < 0:
            raise TraitError("Det mask should be a positive integer")
        return check

    def _validate_det_flag_mask(self, check):
        if check < 0:
            raise TraitError("Flag mask should be a positive integer")
        return check

    def _validate_shared_flag_mask(self, check):
        if check < 0:
            raise TraitError("Flag mask should be a positive integer")
        return check

    def _validate_harmonics(self, check):
        if check < 0:
            raise TraitError("Harmonics should be a non-negative integer")
        return check

    def _validate_fill_gaps(self, check):
        if check:
            raise NotImplementedError("HWPSynchronousModel: fill_gaps draws from an unseeded generator in the reference "
                                      "and is not reproduced")
        return check

    def _validate_debug(self, check):
        if check is not None:
            raise NotImplementedError("HWPSynchronousModel: debug plots are not produced")
        return check

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.coefficients = {}
        self.fit_products = {}

    # ------------------------------------------------------------------------------------------------ driver
    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        if self.relcal_continuous is not None and self.relcal_fixed is not None:
            raise RuntimeError("Only one of continuous and fixed relative calibration can be used")
        if self.chunk_view is not None and self.chunk_time is not None:
            raise RuntimeError("Only one of chunk_view and chunk_time can be used")
        do_cal = self.relcal_continuous or self.relcal_fixed
        if not self.subtract_model and (self.save_model is None) and not do_cal:
            raise RuntimeError("Nothing to do.  You should enable at least one of the options to subtract or save the "
                               "model or to generate calibrations.")
        if use_accel and not accel_enabled():
            raise RuntimeError("HWPSynchronousModel: use_accel=True needs the HIP library and an assigned device")

        self.coefficients, self.fit_products = {}, {}
        for ob in data.obs:
            if not ob.is_distributed_by_detector:
                raise RuntimeError(f"{ob.name} is not distributed by detector")
            if self.hwp_angle is None or self.hwp_angle not in ob.shared:
                # nothing to do, but a requested relative calibration is made: all ones (hwpss_model.py:201-215)
                if self.relcal_fixed is not None:
                    ob[self.relcal_fixed] = {x: 1.0 for x in ob.local_detectors}
                if self.relcal_continuous is not None:
                    self._unit_relcal(ob)
                continue

            local_dets = ob.select_local_detectors(detectors, flagmask=self.det_mask)
            n_coeff = n_coefficients(self.harmonics, self.time_drift)
            reltime = np.array(self._shared_host(ob, self.times), copy=True)
            reltime -= reltime[0]
            angle = np.array(self._shared_host(ob, self.hwp_angle), dtype=np.float64)       # a copy: registered under its own name
            chunks = self._compute_chunking(ob, reltime)
            shared = self._compute_shared_flags(ob, angle)

            dd = ob.detdata[self.det_data]
            on_device = dd.accel_in_use() if use_accel is None else bool(use_accel)
            if on_device:
                from .. import capi

                on_device = 1 <= n_coeff <= capi.dev.hwpss_max_coeff() and len(local_dets) > 0
            path = _DevicePath(self, data, ob, local_dets, angle, reltime, shared) if on_device else \
                _HostPath(self, ob, local_dets, angle, reltime, shared)
            try:
                self._one_observation(ob, local_dets, chunks, reltime, n_coeff, path)
            finally:
                path.close()

    def _one_observation(self, ob, local_dets, chunks, reltime, n_coeff, path):
        n_dets, n_chunk, n_samp = len(local_dets), len(chunks), ob.n_local_samples
        starts = np.array([c["start"] for c in chunks], dtype=np.int64)
        ends = np.array([c["end"] for c in chunks], dtype=np.int64)
        coeff = np.zeros((n_dets, n_coeff, n_chunk), dtype=np.float64)
        coeff_flags = np.zeros(n_chunk, dtype=np.uint8)
        if n_chunk > 0:
            gram, n_good_shared, rhs, n_good = path.fit(starts, ends)
            for ich in range(n_chunk):
                ch_samp = min(int(ends[ich]), n_samp) - int(starts[ich])         # the length of the NumPy slice
                sol = solve_chunk(gram[ich], n_good_shared[ich], ch_samp, rhs[:, ich], n_good[:, ich], n_coeff)
                if sol is None:
                    coeff_flags[ich] = 1
                else:
                    coeff[:, :, ich] = sol
        self.fit_products[ob.name] = {"gram": gram, "rhs": rhs, "n_good": n_good, "n_good_shared": n_good_shared} \
            if n_chunk > 0 else {}
        self.coefficients[ob.name] = {"coeff": coeff, "coeff_flags": coeff_flags, "detectors": list(local_dets)}

        if self.save_model is not None:
            self._store_model(ob, local_dets, chunks, coeff, coeff_flags)

        mag_table = self._average_magnitude(local_dets, coeff, coeff_flags)
        good_dets, cal_center = self._cut_outliers(ob, mag_table)
        relcal_table = {det: cal_center / mag_table[det] for det in good_dets}
        if self.relcal_fixed is not None:
            ob[self.relcal_fixed] = relcal_table
        if self.relcal_continuous is not None:
            self._unit_relcal(ob)
        if not self.subtract_model and not self.relcal_continuous:
            return

        # what every detector gets: its coefficients (fixed or splines) or, when the model cannot be built, only flags
        good_check = set(good_dets)
        listed = [det for det in local_dets if det in good_check]
        rows = [local_dets.index(det) for det in listed]
        active = np.zeros(len(listed), dtype=np.int32)
        fixed = np.zeros((len(listed), n_coeff), dtype=np.float64) if n_chunk == 1 else None
        splines = [None] * len(listed)
        for k, (det, idet) in enumerate(zip(listed, rows)):
            if n_chunk == 1:
                if coeff_flags[0] != 0:
                    self._flag_detector(ob, det)         # only one chunk, which is flagged
                    continue
                fixed[k] = coeff[idet, :, 0]
            else:
                good_chunk = [np.count_nonzero(coeff[idet, :, x]) > 0 and coeff_flags[x] == 0 for x in range(n_chunk)]
                if np.count_nonzero(good_chunk) == 0:
                    self._flag_detector(ob, det)         # all chunks are flagged
                    continue
                ch_times = np.array([x["time"] for y, x in enumerate(chunks) if good_chunk[y]])
                smoothing = max(n_chunk // 16, 4)
                if smoothing >= n_chunk:
                    raise RuntimeError(f"Only {n_chunk} chunks for interpolation. "
                                       "Reduce the split time or use different intervals")
                if len(ch_times) < 4:
                    raise RuntimeError(f"{ob.name}[{det}]: only {len(ch_times)} good chunks, a cubic spline through "
                                       "the model coefficients needs at least 4")
                splines[k] = [scipy.interpolate.splrep(ch_times, coeff[idet, ic, good_chunk], s=smoothing)
                              for ic in range(n_coeff)]
            active[k] = 1
        if len(listed) == 0:
            return
        path.apply(listed, active, fixed, splines, cal_center, mag_table)

    # ------------------------------------------------------------------------------------------------ host pieces
    @staticmethod
    def _shared_host(ob, key):
        obj = ob.shared[key]
        if obj.accel_in_use():
            obj.accel_update_host()
            obj.accel_used(True)            # the download changed nothing: the device copy is still current
        return obj.data

    def _unit_relcal(self, ob):
        ob.detdata.ensure(self.relcal_continuous, dtype=np.float32, create_units=ob.detdata[self.det_data].units)
        ob.detdata[self.relcal_continuous].data[:, :] = 1.0

    def _flag_detector(self, ob, det):
        current = ob.local_detector_flags[det]
        ob.update_local_detector_flags({det: current | self.hwp_flag_mask})

    def _compute_chunking(self, ob, reltime):
        """hwpss_model.py:838-896"""
        chunks = []
        n_samp = ob.n_local_samples
        if self.chunk_view is None:
            if self.chunk_time is None:
                chunks.append({"start": 0, "end": n_samp, "time": reltime[n_samp // 2]})
            else:
                duration = reltime[-1] - reltime[0]
                non_overlap = int(duration / self.chunk_time)
                adjusted_time = duration / non_overlap
                # rounded up so that the final chunk has a few samples less, not a short chunk at the end
                rate = float(ob.telescope.focalplane.sample_rate)
                chunk_samples = int(adjusted_time * rate + 0.5)
                half_chunk = chunk_samples // 2
                ch_start = 0
                for ch in range(non_overlap):
                    chunks.append({"start": ch_start, "end": ch_start + chunk_samples,
                                   "time": reltime[ch_start + half_chunk]})
                    if ch != non_overlap - 1:
                        chunks.append({"start": ch_start + half_chunk, "end": ch_start + half_chunk + chunk_samples,
                                       "time": reltime[ch_start + chunk_samples]})
                    ch_start += chunk_samples
        else:
            for intr in ob.intervals[self.chunk_view].data:
                first, last = int(intr.first), int(intr.last)
                ch_size = last - first
                if ch_size > 10 * self.harmonics:
                    chunks.append({"start": first, "end": last, "time": reltime[first + ch_size // 2]})
        return chunks

    def _compute_shared_flags(self, ob, angle):
        """The combined shared flag byte (hwpss_model.py:898-916)."""
        if self.shared_flags is None:
            shared = np.zeros(ob.n_local_samples, dtype=np.uint8)
        else:
            shared = np.array(self._shared_host(ob, self.shared_flags), dtype=np.uint8)
            shared &= np.uint8(self.shared_flag_mask & 255)
        shared |= stopped_flags(angle)
        if self.chunk_view is not None:
            not_modelled = np.ones_like(shared)
            for intr in ob.intervals[self.chunk_view].data:
                not_modelled[int(intr.first): int(intr.last)] = 0
            shared |= not_modelled
        return shared

    def _store_model(self, ob, dets, chunks, coeff, coeff_flags):
        """hwpss_model.py:656-676"""
        ob_start = ob.shared[self.times].data[0]
        model = []
        for ichk, chk in enumerate(chunks):
            props = {"start": chk["start"], "end": chk["end"], "time": ob_start + chk["time"], "flag": coeff_flags[ichk]}
            props["dets"] = {det: np.array(coeff[idet, :, ichk]) for idet, det in enumerate(dets)}
            model.append(props)
        ob[self.save_model] = model

    def _average_magnitude(self, dets, coeff, coeff_flags):
        """The mean 2f magnitude of every detector over its good chunks (hwpss_model.py:734-760); NaN without one."""
        re_comp, im_comp = (4, 6) if self.time_drift else (2, 3)
        mag = {}
        for idet, det in enumerate(dets):
            ch_mag = []
            for ch in range(coeff.shape[2]):
                if coeff_flags[ch] != 0:
                    continue
                if coeff[idet, re_comp, ch] == 0 and coeff[idet, im_comp, ch] == 0:
                    continue
                ch_mag.append(np.sqrt(coeff[idet, re_comp, ch] ** 2 + coeff[idet, im_comp, ch] ** 2))
            mag[det] = np.mean(ch_mag) if ch_mag else np.nan
        return mag

    def _cut_outliers(self, ob, det_mag):
        """Iterative sigma cut over the local detectors (hwpss_model.py:678-732 without the column gather)."""
        dets = list(det_mag.keys())
        mag = np.array([det_mag[x] for x in dets], dtype=np.float64)
        good = np.ones(len(dets), dtype=bool)
        n_cut = 1
        while n_cut > 0 and np.any(good):
            n_cut = 0
            mn = np.mean(mag[good])
            std = np.std(mag[good])
            for idet in range(len(dets)):
                if good[idet] and np.absolute(mag[idet] - mn) > self.relcal_cut_sigma * std:
                    good[idet] = False
                    n_cut += 1
        central = np.mean(mag[good]) if np.any(good) else np.nan
        local_flags = dict(ob.local_detector_flags)
        for idet, det in enumerate(dets):
            if not good[idet]:
                local_flags[det] |= self.hwp_flag_mask
        ob.update_local_detector_flags(local_flags)
        return [det for idet, det in enumerate(dets) if good[idet]], central

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"shared": [self.times], "detdata": [self.det_data]}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        return req

    def _provides(self):
        prov = {"meta": [], "detdata": [self.det_data]}
        if self.relcal_continuous is not None:
            prov["detdata"].append(self.relcal_continuous)
        if self.save_model is not None:
            prov["meta"].append(self.save_model)
        if self.relcal_fixed is not None:
            prov["meta"].append(self.relcal_fixed)
        return prov

    def _supports_accel(self):
        return True


def pack_splines(splines, n_coeff):
    """(offsets [n_det n_coeff + 1], knots, coefficients) of ``splines[det][coefficient] = (t, c, 3)``; None: no knots."""
    offsets = np.zeros(len(splines) * n_coeff + 1, dtype=np.int64)
    ts, cs = [], []
    for k, per_det in enumerate(splines):
        for ic in range(n_coeff):
            n = 0
            if per_det is not None:
                t, c, degree = per_det[ic]
                if degree != 3 or len(c) != len(t):
                    raise RuntimeError("pack_splines: cubic splines as splrep returns them")
                ts.append(np.asarray(t, dtype=np.float64))
                cs.append(np.asarray(c, dtype=np.float64))
                n = len(t)
            offsets[k * n_coeff + ic + 1] = offsets[k * n_coeff + ic] + n
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(1)     # noqa: E731
    return offsets, np.ascontiguousarray(cat(ts)), np.ascontiguousarray(cat(cs))


class _HostPath:
    """The NumPy path: the formulas of include/toast_hip.h's HWPSS block on host arrays."""

    def __init__(self, op, ob, dets, angle, reltime, shared):
        self.op, self.ob, self.dets = op, ob, dets
        self.angle, self.reltime, self.shared = angle, reltime, shared
        self.basis = model_basis(angle, reltime, shared, op.harmonics, op.time_drift)
        self.signal = ob.detdata[op.det_data].data
        self.sig_rows = ob.detdata[op.det_data].indices(dets)
        self.flags = self.flag_rows = None
        if op.det_flags is not None:
            self.flags = ob.detdata[op.det_flags].data
            self.flag_rows = ob.detdata[op.det_flags].indices(dets)

    def _flag_value(self, det):
        if self.flags is None:
            return self.shared
        row = self.flag_rows[self.dets.index(det)]
        return (self.flags[row] & np.uint8(self.op.det_flag_mask & 255)) | self.shared

    def fit(self, starts, ends):
        n_chunk, n_det, n_coeff = len(starts), len(self.dets), self.basis.shape[1]
        gram = np.zeros((n_chunk, n_coeff, n_coeff))
        n_good_shared = np.zeros(n_chunk, dtype=np.int64)
        rhs = np.zeros((n_det, n_chunk, n_coeff))
        n_good = np.zeros((n_det, n_chunk), dtype=np.int64)
        self.mean = np.zeros((n_det, n_chunk))
        fvs = [self._flag_value(det) for det in self.dets]
        for ich in range(n_chunk):
            slc = slice(int(starts[ich]), int(ends[ich]))
            b = self.basis[slc]
            gram[ich] = np.triu(b.T @ b)
            n_good_shared[ich] = np.count_nonzero(self.shared[slc] == 0)
            for idet in range(n_det):
                good = fvs[idet][slc] == 0
                n_good[idet, ich] = np.count_nonzero(good)
                if n_good[idet, ich] == 0:
                    continue
                sig = self.signal[self.sig_rows[idet], slc][good]
                dc = np.mean(sig)
                sig = sig - dc
                dc2 = np.mean(sig)                       # what is left of a large level (hwp_utils.py:291-292)
                self.mean[idet, ich] = dc + dc2
                rhs[idet, ich] = (sig - dc2) @ b[good]
        return gram, n_good_shared, rhs, n_good

    def apply(self, listed, active, fixed, splines, cal_center, mag_table):
        op = self.op
        n_coeff = self.basis.shape[1]
        re_comp, im_comp = (4, 6) if op.time_drift else (2, 3)
        for k, det in enumerate(listed):
            fv = self._flag_value(det)
            if self.flags is not None:
                row = self.flag_rows[self.dets.index(det)]
                self.flags[row] |= (fv * np.uint8(op.hwp_flag_mask & 255)).astype(np.uint8)
            if not active[k]:
                continue
            good = fv == 0
            model = np.zeros(len(self.angle))
            det_mag = mag_table[det]
            if fixed is not None:
                for ic in range(n_coeff):
                    model += fixed[k, ic] * self.basis[:, ic]
            else:
                det_coeff = np.stack([scipy.interpolate.splev(self.reltime, splines[k][ic], ext=0)
                                      for ic in range(n_coeff)], axis=1)
                for ic in range(n_coeff):
                    model += det_coeff[:, ic] * self.basis[:, ic]
                if op.relcal_continuous is not None:
                    det_mag = np.sqrt(det_coeff[:, re_comp] ** 2 + det_coeff[:, im_comp] ** 2)
                    det_mag[fv != 0] = 1.0
            if op.subtract_model:
                sig = self.signal[self.sig_rows[self.dets.index(det)]]
                sig[good] -= model[good]
                sig[good] -= np.mean(sig[good])
            if op.relcal_continuous is not None:
                self.ob.detdata[op.relcal_continuous][det] = cal_center / det_mag

    def close(self):
        pass


class _DevicePath:
    """The kernels of csrc/hwpss.hip on the resident timestreams."""

    def __init__(self, op, data, ob, dets, angle, reltime, shared):
        from .. import capi

        if not accel_enabled():
            raise RuntimeError("HWPSynchronousModel: the device path needs the HIP library and an assigned device")
        self.D = capi.dev
        self.op, self.data, self.ob, self.dets = op, data, ob, dets
        self.n_samp = ob.n_local_samples
        dd = ob.detdata[op.det_data]
        if dd.dtype != np.dtype(np.float64):
            raise RuntimeError(f"detdata '{op.det_data}' is {dd.dtype}: the device path works in place on float64")
        self.dd = dd
        self.signal = Resident(dd, op.det_data)
        self.sig_rows = dd.indices(dets)
        # the kernels write signal and flags: both get the same release in close()
        self.flags, self.flag_rows, self.flag_ptr = None, None, 0
        if op.det_flags is not None:
            fd = ob.detdata[op.det_flags]
            self.flags = Resident(fd, op.det_flags)
            self.flag_rows = fd.indices(dets)
            self.flag_ptr = self.flags.ptr
        self.scratch = device_scratch(op.name, owner=op)
        self.scratch.__enter__()
        try:
            self.scratch.inp("angle", angle)
            self.scratch.inp("reltime", np.ascontiguousarray(reltime))
            self.scratch.inp("shared", shared)
        except BaseException as err:
            # nobody can call close() on an object whose constructor raised: release what was registered here
            self.scratch.__exit__(type(err), err, err.__traceback__)
            raise
        self.common = (self.n_samp, op.harmonics, op.time_drift, self.scratch.ptr("angle"), self.scratch.ptr("reltime"),
                       self.scratch.ptr("shared"))

    def fit(self, starts, ends):
        n_chunk, n_det = len(starts), len(self.dets)
        n_coeff = n_coefficients(self.op.harmonics, self.op.time_drift)
        gram = np.zeros((n_chunk, n_coeff, n_coeff))
        n_good_shared = np.zeros(n_chunk, dtype=np.int64)
        rhs = np.zeros((n_det, n_chunk, n_coeff))
        n_good = np.zeros((n_det, n_chunk), dtype=np.int64)
        self.mean = np.zeros((n_det, n_chunk))
        with device_scratch(self.op.name + "_fit", owner=self.op) as s:
            for key, arr in (("gram", gram), ("ngs", n_good_shared), ("rhs", rhs), ("ng", n_good), ("mean", self.mean)):
                s.out(key, arr)
            self.D.hwpss_gram(*self.common, starts, ends, s.ptr("gram"), s.ptr("ngs"))
            self.D.hwpss_project(*self.common, self.sig_rows, self.signal.ptr, self.flag_rows, self.flag_ptr,
                                 self.op.det_flag_mask, starts, ends, s.ptr("ng"), s.ptr("mean"), s.ptr("rhs"))
        return gram, n_good_shared, rhs, n_good

    def apply(self, listed, active, fixed, splines, cal_center, mag_table):
        op, ob = self.op, self.ob
        n_coeff = n_coefficients(op.harmonics, op.time_drift)
        pos = {det: k for k, det in enumerate(self.dets)}
        rows = np.array([pos[det] for det in listed], dtype=np.int64)
        sig_rows = self.sig_rows[rows]
        flag_rows = None if self.flag_rows is None else self.flag_rows[rows]
        sums = np.zeros(len(listed))
        counts = np.zeros(len(listed), dtype=np.int64)
        relcal = None
        if op.relcal_continuous is not None:
            rd = ob.detdata[op.relcal_continuous]
            if fixed is not None:
                # one chunk: the fixed table's value over the whole row (hwpss_model.py:347 with a scalar magnitude)
                for k, det in enumerate(listed):
                    if active[k]:
                        rd[det] = cal_center / mag_table[det]
            else:
                relcal = Resident(rd, op.relcal_continuous)
        with device_scratch(op.name + "_apply", owner=op) as s:
            s.work("sum", sums)
            s.work("count", counts)
            kw = {}
            if fixed is not None:
                s.inp("coeff", np.ascontiguousarray(fixed))
                kw["d_coeff"] = s.ptr("coeff")
            else:
                offsets, t, c = pack_splines(splines, n_coeff)
                s.inp("spl_t", t)
                s.inp("spl_c", c)
                kw.update(spl_offset=offsets, d_spl_t=s.ptr("spl_t"), d_spl_c=s.ptr("spl_c"))
                if relcal is not None:
                    kw.update(relcal_index=ob.detdata[op.relcal_continuous].indices(listed), d_relcal=relcal.ptr,
                              cal_center=cal_center)
            self.D.hwpss_subtract(*self.common, sig_rows, self.signal.ptr, flag_rows, self.flag_ptr, op.det_flag_mask,
                                  op.hwp_flag_mask, active, op.subtract_model, s.ptr("sum"), s.ptr("count"), **kw)
            if op.subtract_model:
                self.D.hwpss_remove_mean(self.n_samp, self.scratch.ptr("shared"), sig_rows, self.signal.ptr, flag_rows,
                                         self.flag_ptr, op.det_flag_mask, active, s.ptr("sum"), s.ptr("count"))
        if relcal is not None:
            relcal.write_back_unless_lazy(self.data)

    def close(self):
        self.scratch.__exit__(None, None, None)
        self.signal.write_back_unless_lazy(self.data)
        if self.flags is not None:
            self.flags.write_back_unless_lazy(self.data)
