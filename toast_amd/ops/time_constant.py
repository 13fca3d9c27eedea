"""TimeConstant: convolve each detector timestream with (or deconvolve from it) the detector's single-pole time
constant, K(f) = 1 + i 2 pi tau f, on the device (reference: src/toast/ops/time_constant.py:22-232 ->
toast.fft.convolve(kernel_func=...); here toast_amd.fft.SinglePole -> toast_hip_fft_convolve_pole)."""

import numpy as np

from .. import fft as hipfft
from .. import rng
from ..accel import Resident, accel_enabled
from ..data import defaults
from ..noise import name_UID
from ..traits import Bool, Float, Int, Unicode
from .operator import Operator


class TimeConstant(Operator):
    """Simple time constant filtering without flag checks."""

    API = Int(0, help="Internal interface version for this operator")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to")
    det_mask = Int(defaults.det_mask_invalid, help="Bit mask value for per-detector flagging")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional shared flagging.  Flagged "
                           "shared samples will be propagated to detector sample flags")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for detector sample flagging")
    tau = Float(None, allow_none=True, help="Time constant [s] to apply to all detectors.  Overrides `tau_name`")
    tau_sigma = Float(None, allow_none=True, help="Randomized fractional error to add to each time constant.")
    tau_name = Unicode(None, allow_none=True, help="Key to use to find time constants [s] in the Focalplane.")
    tau_flag_mask = Int(defaults.det_mask_invalid, help="Detector flag mask for cutting detectors with invalid Tau values.")
    batch = Bool(False, help="Accepted for compatibility: all detectors always go through one batched device call")
    deconvolve = Bool(False, help="Deconvolve the time constant instead.")
    realization = Int(0, help="Realization ID, only used if tau_sigma is nonzero")
    debug = Unicode(None, allow_none=True, help="Path to directory for generating debug plots (not produced here)")

    def _get_tau(self, obs, det):
        """time_constant.py:101-126, tau as a float in seconds."""
        focalplane = obs.telescope.focalplane
        tau = float(focalplane[det][self.tau_name]) if self.tau is None else self.tau
        if self.tau_sigma:
            # randomize tau in a reproducible manner
            row = focalplane[det]
            key1 = int(row["uid"]) if "uid" in row else name_UID(det)
            x = rng.random(1, sampler="gaussian", key=(key1, 123456), counter=(obs.session.uid, self.realization))[0]
            tau = tau * (1 + x * self.tau_sigma)
        return tau

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        if self.tau is None and self.tau_name is None:
            raise RuntimeError("Either tau or tau_name must be set.")
        for obs in data.obs:
            dets = obs.select_local_detectors(detectors, flagmask=self.det_mask)
            if len(dets) == 0:
                continue
            rate = obs.telescope.focalplane.sample_rate
            # the time constants of all detectors; a tau that is not finite flags its detector, which is then processed
            # with tau = 0 (time_constant.py:144-153)
            taus = np.zeros(len(dets), dtype=np.float64)
            for idet, det in enumerate(dets):
                tau = self._get_tau(obs, det)
                if np.isfinite(tau):
                    taus[idet] = tau
                else:
                    obs.local_detector_flags[det] |= defaults.det_mask_invalid
            # the kernel function of time_constant.py:155-168; convolve(deconvolve=False) multiplies by what it describes
            invert = not self.deconvolve
            dd = obs.detdata[self.det_data]
            idx = dd.indices(dets)
            n_samp = dd.shape[1]
            extend = None
            shflg = None
            if self.det_flags is not None:
                if self.shared_flags is not None:
                    # propagated to the detector flags as the reference writes it (time_constant.py:182-190), by the
                    # device pass that extends them
                    shflg = (self.det_flag_mask * np.array(
                        obs.shared[self.shared_flags].data & self.shared_flag_mask, dtype=np.uint8)).astype(np.uint8)
                # impulse response spread (fft.py:836-872) through the same GPU pipeline, measured on the device
                extend = hipfft.impulse_extents_pole(len(dets), n_samp, rate, taus, invert)
                if np.any(extend == n_samp):
                    raise RuntimeError("Impulse response spreads to all samples")
            on_dev = dd.accel_in_use() or accel_enabled()
            if on_dev:
                # one page-locked upload instead of pageable staging; with lazy host coherence the filtered
                # timestream stays resident for the operators that follow
                signal = Resident(dd, self.det_data)
            hipfft.convolve_buffer_pole(dd.arg(on_dev), idx, rate, taus, invert, use_accel=on_dev)
            if on_dev:
                signal.write_back_unless_lazy(data)
            if extend is not None:
                # shared flags + extend_flags + first / last samples (fft.py:935-945) in one device pass
                fdata = obs.detdata[self.det_flags]
                if accel_enabled():
                    flags = Resident(fdata, self.det_flags)
                    hipfft.extend_flags_buffer(fdata.buffer, fdata.indices(dets), self.det_flag_mask, extend,
                                               or_row=shflg, use_accel=True)
                    flags.write_back_unless_lazy(data)
                else:
                    hipfft.extend_flags_buffer(fdata.data, fdata.indices(dets), self.det_flag_mask, extend, or_row=shflg)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"shared": [], "detdata": [self.det_data]}
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
            if self.shared_flags is not None:
                req["shared"].append(self.shared_flags)
        return req

    def _provides(self):
        return dict()
