"""PolyFilter, PolyFilter2D and CommonModeFilter: the timestream filters every ground pipeline runs before GroundFilter
and map-making (reference: src/toast/ops/polyfilter/polyfilter.py:30-431, :433-646 and :648-1015).

* ``PolyFilter`` fits and subtracts a low-order Legendre polynomial per detector and per interval of a view.  The
  reference groups detectors with identical flags and hands each group to ``filter_polynomial`` on the host
  (polyfilter.py:556-602).  Here all detectors and all intervals of an observation go through one call of
  toast_hip_filter_polynomial_dev (csrc/poly_filter.hip); the shared and the detector flags stay separate arrays
  and are combined inside the kernel.
* ``PolyFilter2D`` fits and subtracts, at every time stamp and per detector group (wafer), a low-order 2-D polynomial
  across the focal plane.  The reference redistributes the observation by samples, transposes signal and masks to
  [n_samp][n_det] on the host, calls ``filter_poly2D`` per view and copies everything back (polyfilter.py:132-404).
  Every process holds whole observations with all their detectors in this data model, so nothing is redistributed, and
  one call of toast_hip_filter_poly2d_dev (csrc/poly2d_filter.hip) per observation sweeps the detector-major arrays in
  place over all intervals of the view: moments, a Jacobi eigen-solve truncated at 1e-6 like DGELSS, subtraction and
  the flag update.  Orders above 3, ``use_accel=False`` and a process without a device take a NumPy host path
  (``poly2d_host``: ``np.linalg.lstsq(A, b, rcond=1e-6)`` per system).
* ``CommonModeFilter`` removes the focal-plane common mode at every time stamp: ``sum_detectors`` /
  ``subtract_mean`` of the reference (polyfilter.py:926-977) are toast_hip_sum_detectors_dev /
  toast_hip_subtract_mean_dev, fused into toast_hip_common_mode_subtract_dev.  Every process holds whole observations
  with all their detectors in this data model (there is no column communicator), so no reduction across processes
  sits between the sum and the subtraction and the fused form is the one ``regress=False`` uses.  ``regress=True``
  takes the sum and the mean from the separate kernels and reuses the template-regression kernels of GroundFilter.

Not reproduced: ``CommonModeFilter.redistribute`` and ``.plot``; a ``det_data`` that is not
float64 (the reference converts it to float64 and back, polyfilter.py:561-566; here it raises).  ``PolyFilter2D``: the
reference's summation order (results agree to a bound, not bit for bit), and a NaN or an infinity among the good signals
of a system, which the reference hands to LAPACK: here that system gets zero coefficients and is flagged.
"""

import re

import numpy as np

from ..accel import (
    Resident,
    accel_device_ptr,
    accel_enabled,
    device_scratch,
    make_resident,
    native,
)
from ..data import defaults, detector_direction
from ..traits import Bool, Int, TraitError, Unicode
from .operator import Operator


def view_spans(obs, view, op_name):
    """(starts, stops) of the view's intervals as int64 arrays, stops exclusive; ``view=None`` is the whole
    observation (polyfilter.py:526-543)."""
    if view is not None:
        if view not in obs.intervals:
            raise RuntimeError(f"{op_name} is configured to apply in the '{view}' view "
                               f"but it is not defined for observation '{obs.name}'")
        starts = [int(iv.first) for iv in obs.intervals[view]]
        stops = [int(iv.last) for iv in obs.intervals[view]]
    else:
        starts, stops = [0], [obs.n_local_samples]
    return np.array(starts, dtype=np.int64), np.array(stops, dtype=np.int64)


def flag_unfiltered(shared_flags, starts, stops, poly_flag_mask):
    """Copy of the shared flags with ``poly_flag_mask`` OR-ed into every sample outside all ``[start, stop)``
    (polyfilter.py:612-616)."""
    out = np.array(shared_flags)
    not_filtered = np.ones(out.size, dtype=bool)
    for start, stop in zip(starts, stops):
        not_filtered[start:stop] = False
    out[not_filtered] |= out.dtype.type(poly_flag_mask)
    return out


def _positive(name, value):
    if value < 0:
        raise TraitError(f"{name} should be a positive integer")
    return value


class _Resident:
    """Timestreams, detector flags and shared flags of one observation on the device; ``release`` leaves the
    timestreams there under ``data.lazy_host``, the flags stay in any case."""

    def __init__(self, obs, det_data, det_flags, shared_flags):
        self.dd = obs.detdata[det_data]
        if self.dd.dtype != np.dtype(np.float64):
            raise RuntimeError(f"detdata '{det_data}' is {self.dd.dtype}: the device filters work in place on float64 "
                               "timestreams (the reference converts other types to float64 and back)")
        self.signal = Resident(self.dd, det_data)
        self.sig_ptr = self.signal.ptr
        self.flag_ptr, self.fd = 0, None
        if det_flags is not None:
            self.fd = make_resident(obs.detdata[det_flags], det_flags)
            self.flag_ptr = accel_device_ptr(self.fd.buffer)
        self.shared_ptr = 0
        if shared_flags is not None:
            self.shared_ptr = accel_device_ptr(make_resident(obs.shared[shared_flags], shared_flags).data)

    def flag_index(self, dets):
        return self.fd.indices(dets) if self.fd is not None else None

    def release(self, data):
        self.signal.write_back_unless_lazy(data)


class PolyFilter(Operator):
    """Operator which applies polynomial filtering to the TOD.

    ``coefficients[obs.name]`` ([n_det, n_interval, order + 1], zero beyond the fitted order), ``status[obs.name]``
    (int32 [n_det, n_interval]: 0 fitted, 1 no good sample, 2 order reduced to the number of good samples, 3 a good
    sample is NaN or infinite -- interval left untouched) and ``filtered_detectors[obs.name]`` describe the last call.
    ``det_data`` must be float64 (the reference converts other types; this operator raises).

    The solve: normal equations and Cholesky in fp64 while every pivot keeps at least 5 % of its diagonal entry
    (scattered flags); otherwise -- good samples in a contiguous stretch, e.g. a detector cut for most of a throw --
    the polynomials orthogonal on the good samples by their three-term recurrence, which stays as close to the exact
    least-squares residual as the SVD solve of the reference.  Both give Legendre coefficients and the same status
    values; status 3 does not occur for finite input."""

    API = Int(0, help="Internal interface version for this operator")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to")
    pattern = Unicode(".*", allow_none=True,
                      help="Regex pattern to match against detector names. Only detectors that match the pattern are filtered.")
    order = Int(1, allow_none=False, help="Polynomial order")
    det_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing,
                        help="Bit mask value for detector sample flagging")
    poly_flag_mask = Int(defaults.shared_mask_invalid, help="Shared flag bit mask for samples outside of filtering view")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_nonscience, help="Bit mask value for optional shared flagging")
    view = Unicode("throw", allow_none=True, help="Use this view of the data in all observations")

    def _validate_det_mask(self, value):
        return _positive("Det mask", value)

    def _validate_shared_flag_mask(self, value):
        return _positive("Shared flag mask", value)

    def _validate_det_flag_mask(self, value):
        return _positive("Det flag mask", value)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.coefficients = {}
        self.status = {}
        self.filtered_detectors = {}

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        from .. import capi

        if not accel_enabled():
            raise RuntimeError("PolyFilter needs the HIP library and an assigned device (no host path)")
        D = capi.dev
        pat = re.compile(self.pattern if self.pattern is not None else ".*")
        self.coefficients, self.status, self.filtered_detectors = {}, {}, {}
        for obs in data.obs:
            dets = [d for d in obs.select_local_detectors(detectors, flagmask=self.det_mask) if pat.match(d) is not None]
            starts, stops = view_spans(obs, self.view, "PolyFilter")
            n_term = max(self.order + 1, 0)
            coeff = np.zeros((len(dets), starts.size, n_term))
            status = np.zeros((len(dets), starts.size), dtype=np.int32)
            if len(dets) > 0 and starts.size > 0 and self.order >= 0:
                res = _Resident(obs, self.det_data, self.det_flags, self.shared_flags)
                with device_scratch(self.name, owner=self) as s:
                    s.out("coeff", coeff)
                    s.out("status", status)
                    D.filter_polynomial(self.order, obs.n_local_samples, res.dd.indices(dets), res.sig_ptr,
                                        res.flag_index(dets), res.flag_ptr, self.det_flag_mask, res.shared_ptr,
                                        self.shared_flag_mask, starts, stops, s.ptr("coeff"), s.ptr("status"))
                res.release(data)
            self.coefficients[obs.name] = coeff
            self.status[obs.name] = status
            self.filtered_detectors[obs.name] = dets
            # optionally flag unfiltered data (polyfilter.py:607-617); the device copy follows the host
            if self.shared_flags is not None and self.poly_flag_mask is not None:
                sf = obs.shared[self.shared_flags]
                on_device = sf.accel_exists()
                if on_device and sf.accel_in_use():
                    sf.accel_update_host()
                sf.data[:] = flag_unfiltered(sf.data, starts, stops, self.poly_flag_mask)
                if on_device:
                    sf.accel_update_device()
        data.comm.barrier()

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [], "detdata": [self.det_data], "intervals": [self.view]}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": []}


def poly2d_templates(positions, groups, order):
    """Templates [n_det][(order + 1)^2] of polyfilter.py:227-266.  ``positions`` [n_det][2]: theta, phi of every
    detector; ``groups``: lists of detector indices, in the order the reference walks its ``groups`` dict.  The mean of
    every group is removed (summed detector by detector, like the reference), one scale 0.999 / max(|theta|max, |phi|max)
    over all groups, then theta^xorders * phi^yorders with meshgrid(..., indexing="ij")."""
    pos = np.array(positions, dtype=np.float64)
    for members in groups:
        theta_offset, phi_offset = 0, 0
        for d in members:
            theta_offset += pos[d, 0]
            phi_offset += pos[d, 1]
        theta_offset /= len(members)
        phi_offset /= len(members)
        for d in members:
            pos[d] = [pos[d, 0] - theta_offset, pos[d, 1] - phi_offset]
    scale = 0.999 / max(np.amax(np.abs(pos[:, 0])), np.amax(np.abs(pos[:, 1])))
    orders = np.arange(order + 1)
    xorders, yorders = np.meshgrid(orders, orders, indexing="ij")
    xorders, yorders = xorders.ravel(), yorders.ravel()
    templates = np.zeros((pos.shape[0], (order + 1) ** 2))
    for d in range(pos.shape[0]):
        theta, phi = pos[d, 0] * scale, pos[d, 1] * scale
        templates[d] = theta ** xorders * phi ** yorders
    return templates


def poly2d_host(templates, det_group, n_group, signal, sig_rows, det_flags, flag_rows, det_flag_mask, shared_flags,
                shared_flag_mask, poly_flag_mask, starts, stops):
    """The host path of PolyFilter2D, in place on ``signal`` [rows][n_samp] and ``det_flags`` (may be None).  Per sample
    of every [start, stop) and per group: A = sum_good T T^T, b = sum_good T s, c = lstsq(A, b, rcond=1e-6) -- the
    reference's kernel (kernels_numpy.py:86-97) --; all c == 0 flags the group's detectors with ``poly_flag_mask``;
    otherwise the fit is subtracted from the good detectors.  A system whose b is not finite gets c = 0.
    Returns the coefficients [n_samp][n_group][n_mode] (zero outside the intervals)."""
    n_samp = signal.shape[1]
    n_mode = templates.shape[1]
    det_group = np.asarray(det_group)
    coeff = np.zeros((n_samp, n_group, n_mode))
    members = [np.flatnonzero(det_group == g) for g in range(n_group)]
    for start, stop in zip(starts, stops):
        start, stop = max(int(start), 0), min(int(stop), n_samp)
        for s in range(start, stop):
            shared_ok = shared_flags is None or (int(shared_flags[s]) & shared_flag_mask) == 0
            for g, dets in enumerate(members):
                if dets.size == 0:
                    continue
                if det_flags is not None:
                    good = (det_flags[flag_rows[dets], s] & det_flag_mask) == 0
                else:
                    good = np.ones(dets.size, dtype=bool)
                good &= shared_ok
                used = dets[good]
                if used.size > 0:
                    t = templates[used]
                    values = signal[sig_rows[used], s]
                    proj = t.T @ values
                    if np.all(np.isfinite(proj)):
                        c = np.linalg.lstsq(t.T @ t, proj, rcond=1.0e-6)[0]
                        coeff[s, g] = c
                if np.all(coeff[s, g] == 0):
                    if det_flags is not None:
                        det_flags[flag_rows[dets], s] |= det_flags.dtype.type(poly_flag_mask)
                elif used.size > 0:
                    signal[sig_rows[used], s] -= templates[used] @ coeff[s, g]
    return coeff


class PolyFilter2D(Operator):
    """Operator to regress out 2D polynomials across the focal plane.

    ``coefficients[obs.name]`` ([n_samp, n_group, (order + 1)^2], zero outside the view), ``flagged_samples[obs.name]``
    (per group, the number of samples of the view whose coefficients are all zero: they carry ``poly_flag_mask``) and
    ``filtered_detectors[obs.name]`` / ``groups[obs.name]`` (group keys, sorted) describe the last call.  ``det_data`` must
    be float64.  Orders 0 to 3 run on the device; larger orders, ``use_accel=False`` and a process without a device run
    the NumPy host path.  A system with a NaN or an infinity among its good signals gets zero coefficients (and is
    flagged); the reference passes it to LAPACK."""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to")
    pattern = Unicode(".*", allow_none=True,
                      help="Regex pattern to match against detector names. Only detectors that match the pattern are filtered.")
    order = Int(1, allow_none=False, help="Polynomial order")
    det_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing,
                        help="Bit mask value for detector sample flagging")
    poly_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for samples that fail to filter")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional shared flagging")
    view = Unicode(None, allow_none=True, help="Use this view of the data in all observations")
    focalplane_key = Unicode(None, allow_none=True, help="Which focalplane key to match")

    def _validate_det_mask(self, value):
        return _positive("Det mask", value)

    def _validate_shared_flag_mask(self, value):
        return _positive("Shared flag mask", value)

    def _validate_det_flag_mask(self, value):
        return _positive("Det flag mask", value)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.coefficients = {}
        self.flagged_samples = {}
        self.filtered_detectors = {}
        self.groups = {}

    def _setup(self, obs, pat):
        """-> (detectors, det_group, group keys, templates) of one observation: polyfilter.py:163-266."""
        dets = [d for d in obs.select_local_detectors(None, flagmask=self.det_mask) if pat.match(d) is not None]
        if len(dets) == 0:
            return dets, None, [], None
        focalplane = obs.telescope.focalplane
        positions = []
        for det in dets:
            x, y, z = detector_direction(focalplane[det]["quat"])
            positions.append(np.arcsin([x, y]))
        if self.focalplane_key is None:
            keys, by_key = [None], {None: list(range(len(dets)))}
        else:
            by_key = {}
            for i, det in enumerate(dets):
                if self.focalplane_key not in focalplane[det]:
                    raise RuntimeError(f"Cannot divide detectors by {self.focalplane_key} because it is not defined in "
                                       "the focalplane detector data.")
                by_key.setdefault(focalplane[det][self.focalplane_key], []).append(i)
            keys = sorted(by_key)
        det_group = np.zeros(len(dets), dtype=np.int32)
        for g, key in enumerate(keys):
            det_group[by_key[key]] = g
        # the offsets are taken in the order the groups were met, the group numbers in sorted order (polyfilter.py:211-243)
        templates = poly2d_templates(positions, list(by_key.values()), self.order)
        return dets, det_group, keys, templates

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        from .. import capi

        if detectors is not None:
            raise RuntimeError("PolyFilter2D cannot be run on subsets of detectors")
        if self.order < 0:
            raise TraitError("PolyFilter2D: order should not be negative")
        pat = re.compile(self.pattern if self.pattern is not None else ".*")
        on_device = accel_enabled() and (use_accel is None or use_accel)
        if on_device and self.order > capi.dev.filter_poly2d_max_order():
            on_device = False
        self.coefficients, self.flagged_samples, self.filtered_detectors, self.groups = {}, {}, {}, {}
        n_mode = (self.order + 1) ** 2
        for obs in data.obs:
            # the reference gathers all detectors of a sample on one process first; observations of this data model
            # hold them all already and carry no column communicator
            if getattr(obs, "comm_col", None) is not None:
                raise NotImplementedError("PolyFilter2D: detectors of one observation spread over several processes "
                                          "(obs.comm_col) are not supported")
            dets, det_group, keys, templates = self._setup(obs, pat)
            self.filtered_detectors[obs.name] = dets
            self.groups[obs.name] = keys
            if len(dets) == 0:
                continue
            dd = obs.detdata[self.det_data]
            if dd.dtype != np.dtype(np.float64):
                raise RuntimeError(f"detdata '{self.det_data}' is {dd.dtype}: PolyFilter2D works in place on float64 "
                                   "timestreams (the reference converts other types to float64 and back)")
            starts, stops = view_spans(obs, self.view, "PolyFilter2D")
            n, n_group = obs.n_local_samples, len(keys)
            if starts.size == 0:
                coeff = np.zeros((n, n_group, n_mode))
            elif on_device:
                coeff = self._device(obs, data, capi.dev, dets, det_group, n_group, templates, starts, stops)
            else:
                coeff = self._host(obs, dets, det_group, n_group, templates, starts, stops)
            inside = np.zeros(n, dtype=bool)
            for a, b in zip(starts, stops):
                inside[max(a, 0):min(b, n)] = True
            self.coefficients[obs.name] = coeff
            self.flagged_samples[obs.name] = np.count_nonzero(np.all(coeff == 0, axis=2) & inside[:, None], axis=0)
        data.comm.barrier()

    def _device(self, obs, data, D, dets, det_group, n_group, templates, starts, stops):
        res = _Resident(obs, self.det_data, self.det_flags, self.shared_flags)
        n = obs.n_local_samples
        with device_scratch(self.name, owner=self) as s:
            coeff = s.inout("coeff", np.zeros((n, n_group, templates.shape[1])))
            D.filter_poly2d(self.order, n, res.dd.indices(dets), res.sig_ptr, res.flag_index(dets), res.flag_ptr,
                            self.det_flag_mask, res.shared_ptr, self.shared_flag_mask, self.poly_flag_mask, det_group,
                            n_group, templates, starts, stops, d_coeff=s.ptr("coeff"))
        # the flags changed on the device copy, which is the current one: the host follows lazily through ``.data``
        res.release(data)
        return coeff

    def _host(self, obs, dets, det_group, n_group, templates, starts, stops):
        dd = obs.detdata[self.det_data]
        fd = obs.detdata[self.det_flags] if self.det_flags is not None else None
        sf = obs.shared[self.shared_flags] if self.shared_flags is not None else None
        # ``.data`` makes the host copy of the timestreams and flags the current one
        shared = None
        if sf is not None:
            resident = sf.accel_exists() and sf.accel_in_use()
            if resident:
                sf.accel_update_host()
            shared = np.array(sf.data)
            if resident:
                sf.accel_update_device()
        return poly2d_host(templates, det_group, n_group, dd.data, np.asarray(dd.indices(dets)),
                           fd.data if fd is not None else None, np.asarray(fd.indices(dets)) if fd is not None else None,
                           self.det_flag_mask, shared, self.shared_flag_mask, self.poly_flag_mask, starts, stops)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [], "detdata": [self.det_data], "intervals": []}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        if self.view is not None:
            req["intervals"].append(self.view)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": []}


def regress_coefficients(proj, invcov):
    """coeff[d] = inv(invcov) proj[d] for the two templates [1, mean] (polyfilter.py:951-960); None when the 2 x 2
    matrix is singular."""
    try:
        cov = np.linalg.inv(invcov)
    except np.linalg.LinAlgError:
        return None
    return np.ascontiguousarray(np.dot(proj, cov.T))


class CommonModeFilter(Operator):
    """Operator to regress out common mode at each time stamp.

    ``redistribute`` and ``plot`` must stay False (NotImplementedError otherwise)."""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to")
    pattern = Unicode(".*", allow_none=True,
                      help="Regex pattern to match against detector names. Only detectors that match the pattern are filtered.")
    det_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid | defaults.det_mask_processing,
                        help="Bit mask value for detector sample flagging")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional shared flagging")
    focalplane_key = Unicode(None, allow_none=True, help="Which focalplane key to match")
    redistribute = Bool(False, help="If True, redistribute data before and after filtering for optimal data locality.")
    regress = Bool(False, help="If True, regress the common mode rather than subtract")
    plot = Bool(False, help="If True, plot regression coefficients")

    def _validate_det_mask(self, value):
        return _positive("Det mask", value)

    def _validate_shared_flag_mask(self, value):
        return _positive("Shared flag mask", value)

    def _validate_det_flag_mask(self, value):
        return _positive("Det flag mask", value)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.coefficients = {}

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        from .. import capi

        if detectors is not None:
            raise RuntimeError("CommonModeFilter cannot be run in batch mode")
        if self.redistribute:
            raise NotImplementedError("CommonModeFilter: redistribute=True is not supported (observations are not "
                                      "redistributed by samples in this data model)")
        if self.plot:
            raise NotImplementedError("CommonModeFilter: plot=True is not supported (diagnostics are outside the path)")
        if not accel_enabled():
            raise RuntimeError("CommonModeFilter needs the HIP library and an assigned device (no host path)")
        D = capi.dev
        pat = re.compile(self.pattern if self.pattern is not None else ".*")
        self.coefficients = {}
        for obs in data.obs:
            # The reference all-reduces sum and hits over the observation's column communicator between the sum and the
            # subtraction (polyfilter.py:938-941).  Observations of this data model hold all their detectors on one
            # process and carry no such communicator; one that does would get a wrong (local) mean from the code below.
            if getattr(obs, "comm_col", None) is not None:
                raise NotImplementedError("CommonModeFilter: detectors of one observation spread over several processes "
                                          "(obs.comm_col) are not supported")
            focalplane = obs.telescope.focalplane
            if self.focalplane_key is None:
                values = [None]
            else:
                values = set()
                for det in getattr(obs, "all_detectors", focalplane.detectors):
                    if pat.match(det) is None:
                        continue
                    values.add(focalplane[det][self.focalplane_key])
                values = sorted(values)
            n = obs.n_local_samples
            res = None
            for value in values:
                local_dets = []
                for det in obs.local_detectors:
                    if obs.local_detector_flags[det] & self.det_mask:
                        continue
                    if pat.match(det) is None:
                        continue
                    if value is not None and focalplane[det][self.focalplane_key] != value:
                        continue
                    local_dets.append(det)
                if len(local_dets) == 0:
                    continue
                if res is None:
                    res = _Resident(obs, self.det_data, self.det_flags, self.shared_flags)
                sidx, fidx = res.dd.indices(local_dets), res.flag_index(local_dets)
                if not self.regress:
                    D.common_mode_subtract(n, sidx, res.sig_ptr, fidx, res.flag_ptr, self.det_flag_mask, res.shared_ptr,
                                           self.shared_flag_mask)
                    continue
                # templates [1, sum -> mean] and the hit counts; the sum is row 1
                templates = np.zeros((2, n))
                templates[0] = 1.0
                with device_scratch(self.name, owner=self) as s:
                    s.inp("templates", templates)
                    s.inp("hits", np.zeros(n, dtype=np.int64))
                    D.sum_detectors(n, sidx, res.sig_ptr, fidx, res.flag_ptr, self.det_flag_mask, res.shared_ptr,
                                    self.shared_flag_mask, s.ptr("templates") + 8 * n, s.ptr("hits"))
                    self._regress(obs, D, res, local_dets, sidx, fidx, s, n, value)
            if res is not None:
                native().accel_synchronize()
                res.release(data)

    def _regress(self, obs, D, res, local_dets, sidx, fidx, s, n, value):
        """polyfilter.py:943-970 with the GroundFilter regression kernels: the "shared flags" of the fit are
        ``hits == 0``, the detector flags zero the signal in the projection only, the subtraction covers all samples.
        ``s``: the caller's device scratch with ``templates`` (row 1: the sum) and ``hits``; it releases what is added."""
        nohit = (s.fetch("hits") == 0).astype(np.uint8)
        D.subtract_mean(n, np.zeros(0, dtype=np.int32), res.sig_ptr, s.ptr("templates") + 8 * n,
                        s.ptr("hits"))       # no rows: only sum -> mean where hits != 0 (toast_hip.h)
        n_det = len(local_dets)
        s.inp("nohit", nohit)
        # (the host reads the projection and the common Gram matrix here, and nothing else of the fit)
        s.work("proj", np.zeros((n_det, 2)))
        s.work("gram", np.zeros((2, 2)))
        s.work("dgram", np.zeros((n_det, 2, 2)))
        s.work("nflag", np.zeros(n_det, dtype=np.int64))
        D.template_fit(s.ptr("templates"), 2, n, sidx, res.sig_ptr, fidx, res.flag_ptr, self.det_flag_mask, s.ptr("nohit"), 1,
                       s.ptr("proj"), s.ptr("gram"), s.ptr("dgram"), s.ptr("nflag"))
        coeff = regress_coefficients(s.fetch("proj"), s.fetch("gram"))
        if coeff is None:
            # matrix is singular, flag these dets (polyfilter.py:965-970)
            for det in local_dets:
                obs.update_local_detector_flags({det: defaults.det_mask_invalid})
        else:
            s.inp("coeff", coeff)
            D.template_subtract(s.ptr("templates"), 2, 0, n, sidx, res.sig_ptr, s.ptr("coeff"))
            self.coefficients[(obs.name, value)] = {det: coeff[i] for i, det in enumerate(local_dets)}

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [], "detdata": [self.det_data]}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": []}
