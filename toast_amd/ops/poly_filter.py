"""PolyFilter and CommonModeFilter: the two timestream filters every ground pipeline runs before
GroundFilter and map-making (reference: src/toast/ops/polyfilter/polyfilter.py:433-646 and :648-1015).

* ``PolyFilter`` fits and subtracts a low-order Legendre polynomial per detector and per interval of a view.  The
  reference groups detectors with identical flags and hands each group to ``filter_polynomial`` on the host
  (polyfilter.py:556-602).  Here all detectors and all intervals of an observation go through one call of
  toast_hip_filter_polynomial_dev (csrc/poly_filter.hip); the shared and the detector flags stay separate arrays
  and are combined inside the kernel.
* ``CommonModeFilter`` removes the focal-plane common mode at every time stamp: ``sum_detectors`` /
  ``subtract_mean`` of the reference (polyfilter.py:926-977) are toast_hip_sum_detectors_dev /
  toast_hip_subtract_mean_dev, fused into toast_hip_common_mode_subtract_dev.  Every process holds whole observations
  with all their detectors in this data model (there is no column communicator), so no reduction across processes
  sits between the sum and the subtraction and the fused form is the one ``regress=False`` uses.  ``regress=True``
  takes the sum and the mean from the separate kernels and reuses the template-regression kernels of GroundFilter.

Not reproduced: ``PolyFilter2D``; ``CommonModeFilter.redistribute`` and ``.plot``; a
``det_data`` that is not float64 (the reference converts it to float64 and back, polyfilter.py:561-566; here it
raises).
"""

import re

import numpy as np

from ..accel import (
    accel_data_create,
    accel_data_delete,
    accel_data_update_device,
    accel_data_update_host,
    accel_device_ptr,
    accel_enabled,
    native,
)
from ..data import defaults
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
    """Timestreams, detector flags and shared flags of one observation on the device, the way GroundFilter._exec
    makes them resident; ``release`` leaves the timestreams there under ``data.lazy_host``."""

    def __init__(self, obs, det_data, det_flags, shared_flags):
        self.dd = obs.detdata[det_data]
        if self.dd.dtype != np.dtype(np.float64):
            raise RuntimeError(f"detdata '{det_data}' is {self.dd.dtype}: the device filters work in place on float64 "
                               "timestreams (the reference converts other types to float64 and back)")
        self.made_resident = False
        if not self.dd.accel_in_use():
            if not self.dd.accel_exists():
                self.dd.accel_create(det_data)
            self.dd.accel_update_device()
            self.made_resident = True
        self.sig_ptr = accel_device_ptr(self.dd.buffer)
        self.flag_ptr, self.fd = 0, None
        if det_flags is not None:
            self.fd = obs.detdata[det_flags]
            if not self.fd.accel_in_use():
                if not self.fd.accel_exists():
                    self.fd.accel_create(det_flags)
                self.fd.accel_update_device()
            self.flag_ptr = accel_device_ptr(self.fd.buffer)
        self.shared_ptr, self.sf = 0, None
        if shared_flags is not None:
            self.sf = obs.shared[shared_flags]
            if not self.sf.accel_in_use():
                if not self.sf.accel_exists():
                    self.sf.accel_create(shared_flags)
                self.sf.accel_update_device()
            self.shared_ptr = accel_device_ptr(self.sf.data)

    def flag_index(self, dets):
        return self.fd.indices(dets) if self.fd is not None else None

    def release(self, data):
        if self.made_resident and not getattr(data, "lazy_host", False):
            self.dd.accel_update_host()
            self.dd.accel_delete()
        else:
            self.dd.accel_used(True)


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
                outs = {"coeff": coeff, "status": status}
                for key, arr in outs.items():
                    accel_data_create(arr, f"{self.name}_{key}", owner=self)
                D.filter_polynomial(self.order, obs.n_local_samples, res.dd.indices(dets), res.sig_ptr,
                                    res.flag_index(dets), res.flag_ptr, self.det_flag_mask, res.shared_ptr,
                                    self.shared_flag_mask, starts, stops, accel_device_ptr(coeff),
                                    accel_device_ptr(status))
                native().accel_synchronize()
                for key, arr in outs.items():
                    accel_data_update_host(arr, f"{self.name}_{key}")
                    accel_data_delete(arr, f"{self.name}_{key}")
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
                hits = np.zeros(n, dtype=np.int64)
                work = {"templates": templates, "hits": hits}
                for key, arr in work.items():
                    accel_data_create(arr, f"{self.name}_{key}", owner=self)
                    accel_data_update_device(arr, f"{self.name}_{key}")
                t_ptr, h_ptr = accel_device_ptr(templates), accel_device_ptr(hits)
                sum_ptr = t_ptr + 8 * n
                D.sum_detectors(n, sidx, res.sig_ptr, fidx, res.flag_ptr, self.det_flag_mask, res.shared_ptr,
                                self.shared_flag_mask, sum_ptr, h_ptr)
                self._regress(obs, D, res, local_dets, sidx, fidx, templates, hits, value)
                native().accel_synchronize()
                for key, arr in work.items():
                    accel_data_delete(arr, f"{self.name}_{key}")
            if res is not None:
                native().accel_synchronize()
                res.release(data)

    def _regress(self, obs, D, res, local_dets, sidx, fidx, templates, hits, value):
        """polyfilter.py:943-970 with the GroundFilter regression kernels: the "shared flags" of the fit are
        ``hits == 0``, the detector flags zero the signal in the projection only, the subtraction covers all samples."""
        n = hits.size
        native().accel_synchronize()
        accel_data_update_host(hits, f"{self.name}_hits")
        nohit = (hits == 0).astype(np.uint8)
        D.subtract_mean(n, np.zeros(0, dtype=np.int32), res.sig_ptr, accel_device_ptr(templates) + 8 * n,
                        accel_device_ptr(hits))       # no rows: only sum -> mean where hits != 0 (toast_hip.h)
        n_det = len(local_dets)
        proj = np.zeros((n_det, 2))
        gram = np.zeros((2, 2))
        dgram = np.zeros((n_det, 2, 2))
        nflag = np.zeros(n_det, dtype=np.int64)
        outs = {"nohit": nohit, "proj": proj, "gram": gram, "dgram": dgram, "nflag": nflag}
        for key, arr in outs.items():
            accel_data_create(arr, f"{self.name}_{key}", owner=self)
        accel_data_update_device(nohit, f"{self.name}_nohit")
        D.template_fit(accel_device_ptr(templates), 2, n, sidx, res.sig_ptr, fidx, res.flag_ptr, self.det_flag_mask,
                       accel_device_ptr(nohit), 1, accel_device_ptr(proj), accel_device_ptr(gram), accel_device_ptr(dgram),
                       accel_device_ptr(nflag))
        native().accel_synchronize()
        for key in ("proj", "gram"):
            accel_data_update_host(outs[key], f"{self.name}_{key}")
        coeff = regress_coefficients(proj, gram)
        if coeff is None:
            # matrix is singular, flag these dets (polyfilter.py:965-970)
            for det in local_dets:
                obs.update_local_detector_flags({det: defaults.det_mask_invalid})
        else:
            accel_data_create(coeff, f"{self.name}_coeff", owner=self)
            accel_data_update_device(coeff, f"{self.name}_coeff")
            D.template_subtract(accel_device_ptr(templates), 2, 0, n, sidx, res.sig_ptr, accel_device_ptr(coeff))
            native().accel_synchronize()
            accel_data_delete(coeff, f"{self.name}_coeff")
            self.coefficients[(obs.name, value)] = {det: coeff[i] for i, det in enumerate(local_dets)}
        for key, arr in outs.items():
            accel_data_delete(arr, f"{self.name}_{key}")

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
