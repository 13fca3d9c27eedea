"""Demodulate and StokesWeightsDemod: half-wave-plate demodulation (reference: src/toast/ops/demodulation.py:30-1130).

``Demodulate`` turns every HWP-modulated detector into pseudo-detectors: ``demod0_<det>`` is the low-passed signal (I),
``demod4r_<det>`` / ``demod4i_<det>`` are the signal band-passed around 4 f_HWP, multiplied by twice the Q / U pointing
weight with the polarization efficiency divided out, and low-passed; ``do_2f`` adds ``demod2r_`` / ``demod2i_`` from the
2 f_HWP band.  Everything is decimated by ``nskip``.  The filters are ``scipy.signal.firwin`` windows with the
reference's automatic length, so the taps are the reference's.  The result is a new ``Data`` (or replaces the
observations with ``in_place``) with a demodulated telescope, decimated shared data, flags, intervals and noise model.

Two paths, chosen per observation by where ``det_data`` lives:

* resident on the device (or ``use_accel=True``): ``stokes_weights`` runs for a batch of detectors at a time (bounded
  by the free device memory; ``max_batch`` attribute, 0 = automatic), the filters are the direct-form kernel of
  csrc/demod.hip -- the band-passed stream lives in a scratch block of the arena, the modulation is computed while it
  is staged -- and the flags are decimated on the device.  The outputs are created on the device and stay there; no
  timestream is downloaded;
* on the host: the reference's own ``scipy.signal.fftconvolve`` calls.

Both give the same numbers to rounding: the direct sum is no further from the exact convolution than the transform.
Flagged samples are not masked in the convolution (the reference does not mask them either).

``do_2f`` is not the fast path: the half-angle factors and their sign bookkeeping are sequential per detector, they are
computed on the host with the reference's statements (the weights of the batch are downloaded for it) and fed to the
kernel as an explicit modulation array.

Shared fields: this data model has no communicator types, the rule is by shape -- a field whose first dimension is the
observation's sample count is decimated with ``[offset % nskip :: nskip]``, any other field is copied.

``StokesWeightsDemod`` gives the pseudo-detectors their constant pointing weights.  The rotation of Q / U between two
pointing frames (``detector_pointing_in`` / ``detector_pointing_out``) is not built: both must be ``None``.
"""

import numpy as np
from scipy.signal import fftconvolve, firwin

from .. import capi
from ..accel import Resident, accel_device_ptr, accel_enabled, device_scratch, make_resident
from ..data import Data, Focalplane, IntervalList, Observation, Telescope, defaults
from ..noise import Noise, name_UID
from ..traits import Bool, Float, Instance, Int, TraitError, Unicode
from .operator import Operator


class Lowpass:
    """A callable class that applies the low pass filter (demodulation.py:30-61; frequencies in Hz)"""

    def __init__(self, fmax, fsample, wkernel=None, offset=0, nskip=1, window="hamming"):
        if wkernel is None:
            # set kernel size longer than low-pass filter time scale
            wkernel = (1 << int(np.ceil(np.log(fsample / fmax * 10) / np.log(2)))) - 1
        self.wkernel = wkernel
        self.lpf = firwin(wkernel, fmax, window=window, pass_zero=True, fs=fsample)
        self._offset = offset
        self._nskip = nskip

    def __call__(self, signal):
        lowpassed = fftconvolve(signal, self.lpf, mode="same").real
        downsampled = lowpassed[self._offset % self._nskip:: self._nskip]
        return downsampled


class Bandpass:
    """A callable class that applies the bandpass filter (demodulation.py:64-89; frequencies in Hz)"""

    def __init__(self, fmin, fmax, fsample, wkernel=None, window="hamming"):
        if wkernel is None:
            # set kernel size longer than low-pass filter time scale
            wkernel = (1 << int(np.ceil(np.log(fsample / fmin * 10) / np.log(2)))) - 1
        self.wkernel = wkernel
        self.bpf = firwin(wkernel, [fmin, fmax], window=window, pass_zero=False, fs=fsample)

    def __call__(self, signal, downsample=True):
        bandpassed = fftconvolve(signal, self.bpf, mode="same").real
        return bandpassed


def half_angle_factors(qweights):
    """The 2f demodulation factors |cos(psi / 2)|, |sin(psi / 2)| of normalised Q weights with the sign of every
    second mode inverted (demodulation.py:742-761)."""
    signal_demod2r = np.sqrt(0.5 * (1 + qweights))
    signal_demod2i = np.sqrt(0.5 * (1 - qweights))
    for sig in signal_demod2r, signal_demod2i:
        dsig = np.diff(sig)
        dsig[sig[1:] > 0.5] = 0
        starts = np.where(dsig[:-1] * dsig[1:] < 0)[0]
        for start, stop in zip(starts[::2], starts[1::2]):
            sig[start + 1: stop + 2] *= -1
        # handle some corner cases
        dsig = np.diff(sig)
        dstep = np.median(np.abs(dsig[sig[1:] < 0.5]))
        bad = np.abs(dsig) > 2 * dstep
        bad = np.hstack([bad, False])
        sig[bad] *= -1
    return signal_demod2r, signal_demod2i


def _clear_observation(obs):
    """What the reference's ``Observation.clear`` does here: drop detector data, shared data and metadata."""
    for key in list(obs.detdata.keys()):
        del obs.detdata[key]
    for key in list(obs.shared.keys()):
        if obs.shared[key].accel_exists():
            obs.shared[key].accel_delete()
        del obs.shared[key]
    for key in list(obs.keys()):
        del obs[key]


class Demodulate(Operator):
    """Demodulate and downsample HWP-modulated data"""

    allowed_modes = ("", "I", "QU", "IQU")

    API = Int(0, help="Internal interface version for this operator")
    stokes_weights = Instance(klass=Operator, allow_none=True,
                              help="This must be an instance of a Stokes weights operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    hwp_angle = Unicode(defaults.hwp_angle, help="Observation shared key for HWP angle")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to.  Use ';' if multiple "
                                               "signal flavors should be demodulated.")
    det_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for detector sample flagging")
    demod_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for demod & downsample flagging")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True,
                           help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional shared flagging")
    noise_model = Unicode("noise_model", allow_none=True, help="Observation key containing the noise model")
    wkernel = Int(None, allow_none=True, help="Override automatic filter kernel size")
    fcut = Float(0.95, help="Low pass cut-off frequency in units of HWP frequency")
    fmin_2f = Float(1.05, help="Low frequency end of the 2f-bandpass filter in units of HWP frequency")
    fmax_2f = Float(2.95, help="High frequency end of the 2f-bandpass filter in units of HWP frequency")
    fmin_4f = Float(3.05, help="Low frequency end of the 4f-bandpass filter in units of HWP frequency")
    fmax_4f = Float(4.95, help="High frequency end of the 4fbandpass filter in units of HWP frequency")
    nskip = Int(3, help="Downsampling factor")
    window = Unicode("hamming", help="Window function name recognized by scipy.signal.firwin")
    keep_dets_frac = Float(0, help="If less than this fraction of detectors are good, cut the observation")
    purge = Bool(False, help="Remove inputs after demodulation")
    in_place = Bool(False, help="Modify the data object in-place.  Implies purge=True.")
    do_2f = Bool(False, help="also cache the 2f-demodulated signal")
    mode = Unicode("IQU", help="Return I, QU or IQU timestreams.")

    def _validate_det_mask(self, check):
        if check < 0:
            raise TraitError("Det mask should be a positive integer")
        return check

    def _validate_det_flag_mask(self, check):
        if check < 0:
            raise TraitError("Det flag mask should be a positive integer")
        return check

    def _validate_shared_flag_mask(self, check):
        if check < 0:
            raise TraitError("Shared flag mask should be a positive integer")
        return check

    def _validate_stokes_weights(self, weights):
        if weights is not None:
            if not isinstance(weights, Operator):
                raise TraitError("stokes_weights should be an Operator instance")
            # Check that this operator has the traits we expect
            for trt in ["weights", "view", "mode"]:
                if not weights.has_trait(trt):
                    raise TraitError(f"stokes_weights operator should have a '{trt}' trait")
            # Check that weights are supported
            supported = ("I", "QU", "IQU")
            if weights.mode not in supported:
                raise TraitError(f"Stokes weights mode not in {supported}")
        return weights

    def _validate_mode(self, mode):
        if mode not in self.allowed_modes:
            raise TraitError(f"mode must be one of {self.allowed_modes}")
        return mode

    def _validate_nskip(self, check):
        if check < 1:
            raise TraitError("nskip must be at least one")
        return check

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.max_batch = 0
        self.demod_data = None

    # ------------------------------------------------------------------------------------------------ exec
    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        for trait in ["stokes_weights"]:
            if getattr(self, trait) is None:
                raise RuntimeError(f"You must set the '{trait}' trait before calling exec()")
        if "QU" in self.mode and "QU" not in self.stokes_weights.mode:
            raise RuntimeError("Cannot produce demodulated QU without QU Stokes weights")
        if self.stokes_weights.hwp_angle is None:
            raise RuntimeError("The Stokes weights operator (self.stokes_weights) does not have HWP angle")
        if self.do_2f and "QU" not in self.stokes_weights.mode:
            raise RuntimeError("Cannot produce the 2f signal without QU Stokes weights")

        if self.in_place:
            self.demod_data = None
        else:
            self.demod_data = Data(comm=data.comm)

        # Demodulation only applies to observations with HWP.  We also cut all observations where no more than
        # keep_dets_frac of the detectors are good.
        demodulate_input_obs = []
        for obs in data.obs:
            if self.hwp_angle not in obs.shared:
                if self.in_place or self.purge:
                    # Un-demodulated observations will be deleted
                    _clear_observation(obs)
                continue
            hwp_angle = obs.shared[self.hwp_angle].data
            if np.abs(np.median(np.diff(hwp_angle))) < 1e-6:
                # Stepped or stationary HWP
                if self.in_place:
                    _clear_observation(obs)
                continue
            n_dets = len(obs.local_detectors)
            n_good = np.sum([1 for x, y in obs.local_detector_flags.items() if y & self.det_mask == 0])
            if n_good / n_dets <= self.keep_dets_frac:
                if self.in_place:
                    _clear_observation(obs)
                continue
            demodulate_input_obs.append(obs)

        # Each modulated detector demodulates into one or more pseudo detectors
        self.prefixes = []
        if "I" in self.mode:
            self.prefixes.append("demod0")
        if "QU" in self.mode:
            self.prefixes.extend(["demod4r", "demod4i"])
        if self.do_2f:
            self.prefixes.extend(["demod2r", "demod2i"])
        if len(self.prefixes) == 0:
            raise RuntimeError("There are no pseudo detectors to modulate to")

        demodulate_obs = []
        for obs in demodulate_input_obs:
            # Get the detectors which are not cut with per-detector flags
            local_dets = obs.select_local_detectors(detectors, flagmask=self.det_mask)
            all_dets = local_dets
            offset = obs.local_index_offset
            flavors = self.det_data.split(";")
            for flavor in flavors:
                if obs.detdata[flavor].dtype != np.dtype(np.float64) or obs.detdata[flavor].sample_shape != ():
                    raise RuntimeError(f"detdata '{flavor}' must hold one float64 per sample to be demodulated")

            resident = any(obs.detdata[flavor].accel_in_use() for flavor in flavors)
            on_device = resident if use_accel is None else bool(use_accel)
            if on_device and not accel_enabled():
                raise RuntimeError("Demodulate: use_accel=True needs the HIP library and an assigned device")

            fsample = float(obs.telescope.focalplane.sample_rate)
            # fmod is the HWP spin frequency.  Polarization signal is at 4 x fmod
            fmod = self._get_fmod(obs)
            lowpass = Lowpass(self.fcut * fmod, fsample, wkernel=self.wkernel, offset=offset, nskip=self.nskip,
                              window=self.window)
            bandpass2f = Bandpass(self.fmin_2f * fmod, self.fmax_2f * fmod, fsample, wkernel=self.wkernel,
                                  window=self.window)
            bandpass4f = Bandpass(self.fmin_4f * fmod, self.fmax_4f * fmod, fsample, wkernel=self.wkernel,
                                  window=self.window)

            # Create a new observation to hold the demodulated and downsampled data
            demod_telescope = self._demodulate_telescope(obs, all_dets)
            demod_all_samples = self._demodulated_samples(obs)
            demod_name = f"demod_{obs.name}"
            demod_obs = Observation(obs.comm, demod_telescope, demod_all_samples, name=demod_name,
                                    uid=name_UID(demod_name), session=obs.session)
            sample_sets = self._demodulate_sample_sets(obs)
            if sample_sets is not None:
                demod_obs.all_sample_sets = sample_sets

            # Allocate storage
            demod_dets = []
            for det in local_dets:
                for prefix in self.prefixes:
                    demod_dets.append(f"{prefix}_{det}")

            self._demodulate_shared_data(obs, demod_obs)
            for flavor in flavors:
                demod_obs.detdata.ensure(flavor, detectors=demod_dets, dtype=np.float64,
                                         create_units=obs.detdata[flavor].units, accel=on_device, zero_new=False)
            if self.det_flags is not None:
                demod_obs.detdata.ensure(self.det_flags, detectors=demod_dets, dtype=np.uint8, accel=on_device,
                                         zero_new=False)

            self._demodulate_flags(obs, demod_obs, local_dets, lowpass.wkernel, offset, on_device)
            if on_device:
                self._demodulate_signal_device(data, obs, demod_obs, local_dets, lowpass, bandpass2f, bandpass4f, offset)
            else:
                self._demodulate_signal(data, obs, demod_obs, local_dets, lowpass, bandpass2f, bandpass4f)
            self._demodulate_noise(obs, demod_obs, local_dets, fsample, fmod, lowpass, bandpass2f, bandpass4f)
            self._demodulate_intervals(obs, demod_obs)
            self._demodulate_metadata(obs, demod_obs)
            demodulate_obs.append(demod_obs)

            if self.in_place or self.purge:
                # Input observations are not saved
                _clear_observation(obs)

        if self.in_place:
            data.obs.clear()
            data.obs.extend(demodulate_obs)
        else:
            self.demod_data.obs = demodulate_obs

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def _get_fmod(self, obs):
        """Return the modulation frequency [Hz]"""
        times = obs.shared[self.times].data
        hwp_angle = np.unwrap(obs.shared[self.hwp_angle].data)
        hwp_rate = np.absolute(np.mean(np.diff(hwp_angle) / np.diff(times)) / (2 * np.pi))
        return hwp_rate

    def _demodulate_telescope(self, obs, all_dets):
        """Every focalplane row is repeated once per prefix; the sample rate is divided by nskip."""
        focalplane = obs.telescope.focalplane
        all_set = set(all_dets)
        names, rows = [], []
        for det in focalplane.detectors:
            if det not in all_set:
                continue
            # Each detector translates into one or more
            for prefix in self.prefixes:
                names.append(f"{prefix}_{det}")
                rows.append(focalplane[det])
        basic = ("quat", "gamma", "pol_leakage", "cal")
        extra = []
        for row in rows:
            for key in row:
                if key not in basic and key not in extra:
                    extra.append(key)
        quats = [row["quat"] for row in rows] if rows else np.zeros((0, 4))
        demod_focalplane = Focalplane(names, quats, gamma=[row["gamma"] for row in rows],
                                      epsilon=[row["pol_leakage"] for row in rows], cal=[row["cal"] for row in rows],
                                      sample_rate=focalplane.sample_rate / self.nskip,
                                      columns={key: [row.get(key) for row in rows] for key in extra})
        demod_name = f"demod_{obs.telescope.name}"
        return Telescope(demod_name, demod_focalplane, uid=name_UID(demod_name))

    def _demodulated_samples(self, obs):
        """Compute number of samples in the demodulated observation."""
        off = obs.local_index_offset % self.nskip
        return len(obs.shared[self.times].data[off:: self.nskip])

    def _demodulate_shared_data(self, obs, demod_obs):
        """Downsample shared data: fields along the samples are decimated, the others copied."""
        off = obs.local_index_offset % self.nskip
        for field in obs.shared.keys():
            shobj = obs.shared[field]
            if shobj.accel_in_use():
                # a field the device holds the current copy of (tables built there): refresh the host side, leave it resident
                shobj.accel_update_host()
                shobj.accel_used(True)
            values = shobj.data
            if values.ndim >= 1 and values.shape[0] == obs.n_local_samples:
                values = np.ascontiguousarray(values[off:: self.nskip])
            else:
                values = values.copy()
            demod_obs.shared.create(field, values)
        times = demod_obs.shared[self.times].data
        demod_obs.intervals._times = times
        demod_obs.intervals[None] = IntervalList(times, samplespans=[(0, demod_obs.n_local_samples)])

    def _demodulate_metadata(self, obs, demod_obs):
        """Copy over and optionally downsample metadata"""
        demod_times = demod_obs.shared[self.times].data
        for key, value in obs.items():
            if key in demod_obs:
                # Already demodulated
                continue
            if hasattr(value, "downsample"):
                demod_obs[key] = value.downsample(demod_times)
            else:
                demod_obs[key] = value
        # Other observation attributes
        for key, value in vars(obs).items():
            if key.startswith("_"):
                continue
            if hasattr(demod_obs, key):
                # Already demodulated
                continue
            if hasattr(value, "downsample"):
                setattr(demod_obs, key, value.downsample(demod_times))
            else:
                setattr(demod_obs, key, value)

    def _demodulate_sample_sets(self, obs):
        sample_sets = getattr(obs, "all_sample_sets", None)
        if sample_sets is None:
            return None
        demod_sample_sets = []
        offset = 0
        for sample_set in sample_sets:
            demod_sample_set = []
            for chunksize in sample_set:
                first_sample = offset
                last_sample = offset + chunksize
                demod_first_sample = int(np.ceil(first_sample / self.nskip))
                demod_last_sample = int(np.ceil(last_sample / self.nskip))
                demod_chunksize = demod_last_sample - demod_first_sample
                demod_sample_set.append(demod_chunksize)
                offset += chunksize
            demod_sample_sets.append(demod_sample_set)
        return demod_sample_sets

    def _demodulate_intervals(self, obs, demod_obs):
        if self.nskip == 1:
            demod_obs.intervals = obs.intervals
            return
        times = demod_obs.shared[self.times].data
        for name, ivals in obs.intervals.items():
            if name is None:
                continue
            timespans = [[ival.start, ival.stop] for ival in ivals]
            demod_obs.intervals[name] = IntervalList(times, timespans=timespans)
        # Force the creation of new "all" interval
        demod_obs.intervals[None] = IntervalList(times, samplespans=[(0, demod_obs.n_local_samples)])

    # ------------------------------------------------------------------------------------------------ flags
    def _demodulate_flag(self, flags, wkernel, offset):
        """Collapse flags inside the filter window and downsample"""
        # FIXME (reference): for now, just downsample the flags
        flags = flags.copy()
        # flag invalid samples in both ends
        flags[:wkernel] |= self.demod_flag_mask
        flags[-wkernel:] |= self.demod_flag_mask
        new_flags = np.array(flags[offset % self.nskip:: self.nskip])
        return new_flags

    def _shared_flags_device(self, sin, sout, n, wkernel, offset):
        """The shared flags as a batch of one row through the flags kernel; the small result is brought back, the
        demodulated observation's shared data lives on the host like every other shared field."""
        if sout.data.size == 0:
            return
        flags_in = Resident(sin, self.shared_flags)
        sout.accel_create(self.shared_flags)
        try:
            capi.dev.demod_flags(n, wkernel, self.demod_flag_mask, self.nskip, offset, flags_in.ptr, 1, n,
                                 [0], accel_device_ptr(sout.data), 1, sout.data.size, [0])
            sout.accel_used(True)
            sout.accel_update_host()
        finally:
            sout.accel_delete()
            flags_in.drop_if_created()

    def _demodulate_flags(self, obs, demod_obs, dets, wkernel, offset, on_device=False):
        """Demodulate and downsample flags"""
        if self.shared_flags is not None:
            sin, sout = obs.shared[self.shared_flags], demod_obs.shared[self.shared_flags]
            if on_device and sin.data.dtype == np.dtype(np.uint8):
                self._shared_flags_device(sin, sout, obs.n_local_samples, wkernel, offset)
            else:
                sout.data[:] = self._demodulate_flag(sin.data, wkernel, offset)

        input_det_flags = obs.local_detector_flags
        output_det_flags = dict()
        for det in dets:
            for prefix in self.prefixes:
                output_det_flags[f"{prefix}_{det}"] = input_det_flags[det]
        demod_obs.update_local_detector_flags(output_det_flags)
        if self.det_flags is None or len(dets) == 0:
            return
        fin, fout = obs.detdata[self.det_flags], demod_obs.detdata[self.det_flags]
        if on_device and fin.dtype == np.dtype(np.uint8):
            flags_in = Resident(fin, self.det_flags)
            try:
                in_row, out_row = [], []
                for det in dets:
                    for prefix in self.prefixes:
                        in_row.append(int(fin.indices([det])[0]))
                        out_row.append(int(fout.indices([f"{prefix}_{det}"])[0]))
                capi.dev.demod_flags(obs.n_local_samples, wkernel, self.demod_flag_mask, self.nskip, offset,
                                     flags_in.ptr, fin.buffer.shape[0], fin.buffer.shape[1], in_row,
                                     accel_device_ptr(fout.buffer), fout.buffer.shape[0], fout.buffer.shape[1], out_row)
                fout.accel_used(True)
            finally:
                if flags_in.created:
                    capi.synchronize()
                    flags_in.drop_if_created()
            return
        if fout.accel_in_use():
            fout.accel_update_host()
        for det in dets:
            demod_flags = self._demodulate_flag(fin[det], wkernel, offset)
            for prefix in self.prefixes:
                fout[f"{prefix}_{det}"] = demod_flags
        if on_device:
            fout.accel_update_device()

    # ------------------------------------------------------------------------------------------------ host path
    def _one_observation(self, data, obs):
        """A Data that holds only ``obs`` (the reference's ``data.select(obs_uid=...)``)."""
        sub = Data(comm=data.comm)
        sub.obs.append(obs)
        return sub

    def _demodulate_signal(self, data, obs, demod_obs, dets, lowpass, bandpass2f, bandpass4f):
        """demodulate signal TOD"""
        obs_data = self._one_observation(data, obs)
        for det in dets:
            # Get weights
            self.stokes_weights.apply(obs_data, detectors=[det])
            weights = obs.detdata[self.stokes_weights.weights][det]
            # iweights = 1
            # qweights = eta * cos(2 * psi_det + 4 * psi_hwp)
            # uweights = eta * sin(2 * psi_det + 4 * psi_hwp)
            qweights = uweights = None
            if self.stokes_weights.mode == "IQU":
                iweights, qweights, uweights = weights.T
            elif self.stokes_weights.mode == "QU":
                qweights, uweights = weights.T
            if "QU" in self.mode:
                # remove polarization efficiency from the Q/U weights
                etainv = 1 / np.sqrt(qweights**2 + uweights**2)
                qweights = qweights * etainv
                uweights = uweights * etainv

            for flavor in self.det_data.split(";"):
                signal = obs.detdata[flavor][det]
                det_data = demod_obs.detdata[flavor]
                if "I" in self.mode:
                    det_data[f"demod0_{det}"] = lowpass(signal)
                if "QU" in self.mode:
                    bandpassed = bandpass4f(signal)
                    det_data[f"demod4r_{det}"] = lowpass(bandpassed * 2 * qweights)
                    det_data[f"demod4i_{det}"] = lowpass(bandpassed * 2 * uweights)
                if self.do_2f:
                    signal_demod2r, signal_demod2i = half_angle_factors(qweights)
                    # Demodulate and lowpass for 2f
                    highpassed = bandpass2f(signal)
                    det_data[f"demod2r_{det}"] = lowpass(highpassed * signal_demod2r)
                    det_data[f"demod2i_{det}"] = lowpass(highpassed * signal_demod2i)

    # ------------------------------------------------------------------------------------------------ device path
    def _demodulate_signal_device(self, data, obs, demod_obs, dets, lowpass, bandpass2f, bandpass4f, offset):
        """The same on resident data: batches of detectors through csrc/demod.hip."""
        if len(dets) == 0:
            return
        dev = capi.dev
        n = obs.n_local_samples
        flavors = self.det_data.split(";")
        for flavor in flavors:
            make_resident(obs.detdata[flavor], flavor)
            demod_obs.detdata[flavor].accel_used(True)

        def fir(in_rows, d_in, n_in_rows, taps, nskip, off, dd_out, out_names, **mod):
            dev.demod_fir(n, taps, nskip, off, d_in, n_in_rows, n, in_rows, accel_device_ptr(dd_out.buffer),
                          dd_out.buffer.shape[0], dd_out.buffer.shape[1], dd_out.indices(out_names), **mod)

        if "I" in self.mode:
            for flavor in flavors:
                dd, out = obs.detdata[flavor], demod_obs.detdata[flavor]
                fir(dd.indices(dets), accel_device_ptr(dd.buffer), dd.buffer.shape[0], lowpass.lpf, self.nskip,
                    offset, out, [f"demod0_{d}" for d in dets])
        if "QU" not in self.mode and not self.do_2f:
            return

        nnz = len(self.stokes_weights.mode)
        comp_q = nnz - 2
        per_det = 8 * n * (nnz + 4 + 1 + (2 if self.do_2f else 0))
        batch = int(self.max_batch)
        if batch <= 0:
            free, _ = capi.accel_mem_info()
            batch = max(1, (free // 2) // per_det)
        batch = max(1, min(batch, len(dets), 16384))
        obs_data = self._one_observation(data, obs)
        wname = self.stokes_weights.weights
        for b0 in range(0, len(dets), batch):
            part = dets[b0:b0 + batch]
            nb = len(part)
            self.stokes_weights.apply(obs_data, detectors=part, use_accel=True)
            wd = obs.detdata[wname]
            if wd.dtype != np.dtype(np.float64) or wd.sample_shape != (nnz,):
                raise RuntimeError("Demodulate: the device path reads float64 Stokes weights")
            make_resident(wd, wname)
            wrows = [int(r) for r in wd.indices(part)]
            with device_scratch() as s:
                scratch = capi.device_malloc(nb * n * 8)
                try:
                    if self.do_2f:
                        # sequential per detector: on the host, with the reference's statements
                        factors = np.empty((2 * nb, n), dtype=np.float64)
                        host_w = np.array(wd.data)
                        wd.accel_used(True)             # the download changed nothing: the device copy is still current
                        for b, det in enumerate(part):
                            qw, uw = host_w[wd.indices([det])[0]].T[comp_q:comp_q + 2]
                            if "QU" in self.mode:
                                # remove polarization efficiency from the Q/U weights
                                qw = qw * (1 / np.sqrt(qw**2 + uw**2))
                            factors[b], factors[nb + b] = half_angle_factors(qw)
                        s.inp("demod_2f_factors", factors)
                    for flavor in flavors:
                        dd, out = obs.detdata[flavor], demod_obs.detdata[flavor]
                        d_in = accel_device_ptr(dd.buffer)
                        rows = list(range(nb))
                        if "QU" in self.mode:
                            dev.demod_fir(n, bandpass4f.bpf, 1, 0, d_in, dd.buffer.shape[0], n, dd.indices(part), scratch,
                                          nb, n, rows)
                            fir(rows + rows, scratch, nb, lowpass.lpf, self.nskip, offset, out,
                                [f"demod4r_{d}" for d in part] + [f"demod4i_{d}" for d in part],
                                mod_mode=capi.DEMOD_MOD_WEIGHTS, d_mod=accel_device_ptr(wd.buffer),
                                n_mod_rows=wd.buffer.shape[0], mod_stride=n * nnz, mod_row=wrows + wrows,
                                mod_comp=[comp_q] * nb + [comp_q + 1] * nb, nnz=nnz, comp_q=comp_q)
                        if self.do_2f:
                            dev.demod_fir(n, bandpass2f.bpf, 1, 0, d_in, dd.buffer.shape[0], n, dd.indices(part), scratch,
                                          nb, n, rows)
                            fir(rows + rows, scratch, nb, lowpass.lpf, self.nskip, offset, out,
                                [f"demod2r_{d}" for d in part] + [f"demod2i_{d}" for d in part],
                                mod_mode=capi.DEMOD_MOD_ARRAY, d_mod=s.ptr("demod_2f_factors"), n_mod_rows=2 * nb,
                                mod_stride=n, mod_row=list(range(2 * nb)))
                finally:
                    capi.synchronize()
                    capi.device_free(scratch)

    # ------------------------------------------------------------------------------------------------ noise
    def _demodulate_noise(self, obs, demod_obs, dets, fsample, hwp_rate, lowpass, bandpass2f, bandpass4f):
        """Add Noise objects for the new detectors"""
        if self.noise_model is None:
            return
        noise = obs[self.noise_model]

        demod_detectors = []
        demod_freqs = {}
        demod_psds = {}
        demod_indices = {}
        demod_weights = {}

        lpf = lowpass.lpf
        lpf_freq = np.fft.rfftfreq(lpf.size, 1 / fsample)
        lpf_value = np.abs(np.fft.rfft(lpf)) ** 2
        for det in dets:
            # weight -- ignored
            # index  - ignored
            # rate
            rate_in = noise.rate(det)
            # freq
            freq_in = noise.freq(det)
            # Lowpass transfer function
            tf = np.interp(freq_in, lpf_freq, lpf_value)
            # Find the highest frequency without significant suppression
            # to measure noise weights at
            iweight = tf.size - 1
            while iweight > 0 and tf[iweight] < 0.99:
                iweight -= 1
            # psd
            psd_in = noise.psd(det)
            n_mode = len(self.prefixes)
            for indexoff, prefix in enumerate(self.prefixes):
                demod_det = f"{prefix}_{det}"
                # Get the demodulated PSD
                if prefix == "demod0":
                    # this PSD does not change
                    psd_out = psd_in.copy()
                elif prefix.startswith("demod2"):
                    # get noise at 2f
                    psd_out = np.zeros_like(psd_in)
                    psd_out[:] = np.interp(2 * hwp_rate, freq_in, psd_in)
                else:
                    # get noise at 4f
                    psd_out = np.zeros_like(psd_in)
                    psd_out[:] = np.interp(4 * hwp_rate, freq_in, psd_in)
                # Lowpass
                psd_out *= tf
                # Downsample
                rate_out = rate_in / self.nskip
                ind = freq_in <= rate_out / 2
                freq_out = freq_in[ind]
                # Last bin must equal the new Nyquist frequency
                freq_out[-1] = rate_out / 2
                psd_out = psd_out[ind] / self.nskip
                # Calculate noise weight
                noisevar = psd_out[iweight]
                invvar = 1.0 / noisevar / rate_out
                # Insert
                demod_detectors.append(demod_det)
                demod_freqs[demod_det] = freq_out
                demod_psds[demod_det] = psd_out
                demod_indices[demod_det] = noise.index(det) * n_mode + indexoff
                demod_weights[demod_det] = invvar
        demod_obs[self.noise_model] = Noise(detectors=demod_detectors, freqs=demod_freqs, psds=demod_psds,
                                            indices=demod_indices, detweights=demod_weights)

    def _finalize(self, data, **kwargs):
        return self.demod_data

    def _requires(self):
        req = {"shared": [self.times], "detdata": [self.det_data]}
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        return req

    def _provides(self):
        return dict()


class StokesWeightsDemod(Operator):
    """Compute the Stokes pointing weights for demodulated data"""

    allowed_modes = ("I", "QU", "IQU")

    API = Int(0, help="Internal interface version for this operator")
    mode = Unicode("IQU", help="The Stokes weights to generate")
    view = Unicode(None, allow_none=True, help="Use this view of the data in all observations")
    weights = Unicode(defaults.weights, help="Observation detdata key for output weights")
    single_precision = Bool(False, help="If True, use 32bit float in output")
    detector_pointing_in = Instance(klass=Operator, allow_none=True,
                                    help="Pointing operator in the native Q/U frame, typically az/el.  "
                                         "Must be set if `detector_pointing_out` is set.  Has no effect if "
                                         " `detector_pointing_out` is not set.")
    detector_pointing_out = Instance(klass=Operator, allow_none=True,
                                     help="Pointing operator for the desired frame, typically RA/Dec.  "
                                          "Requires `detector_pointing_in` to be set.")
    det_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for per-detector flagging")

    def _validate_mode(self, mode):
        if mode not in self.allowed_modes:
            raise TraitError(f"Invalid mode (must be one of {self.allowed_modes})")
        return mode

    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    @staticmethod
    def pseudo_weights(det, mode, eta):
        """The weights of every sample of pseudo-detector ``det`` (demodulation.py:1063-1114 without rotation)."""
        nnz = len(mode)
        out = np.zeros(nnz, dtype=np.float64)
        if det.startswith("demod0"):
            # Stokes I only
            if "I" in mode:
                out[0] = 1.0
        elif det.startswith("demod4r"):
            # Stokes Q only
            if "QU" in mode:
                out[nnz - 2] = 1.0 * eta
        elif det.startswith("demod4i"):
            # Stokes U only
            if "QU" in mode:
                out[nnz - 1] = 1.0 * eta
        # anything else is not an I/Q/U pseudo detector
        return out

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        nnz = len(self.mode)
        if self.detector_pointing_in is not None or self.detector_pointing_out is not None:
            raise NotImplementedError("StokesWeightsDemod: the rotation of Q / U between the frames of "
                                      "detector_pointing_in and detector_pointing_out is not built; leave both None")
        dtype = np.float32 if self.single_precision else np.float64
        if use_accel and not accel_enabled():
            raise RuntimeError("StokesWeightsDemod: use_accel=True needs the HIP library and an assigned device")

        for obs in data.obs:
            dets = obs.select_local_detectors(detectors, flagmask=self.det_mask)
            on_device = bool(use_accel)
            if use_accel is None:
                # follow the data: resident timestreams get resident weights
                on_device = accel_enabled() and any(dd.accel_in_use() for dd in obs.detdata.values()
                                                    if dd.sample_shape == () and dd.dtype == np.dtype(np.float64))
            obs.detdata.ensure(self.weights, sample_shape=(nnz,), dtype=dtype, detectors=dets, accel=on_device,
                               zero_new=False)
            if len(dets) == 0:
                continue
            weights = obs.detdata[self.weights]
            values = np.zeros((len(dets), nnz), dtype=np.float64)
            for idet, det in enumerate(dets):
                props = obs.telescope.focalplane[det]
                eta = props["pol_efficiency"] if "pol_efficiency" in props else 1.0
                values[idet] = self.pseudo_weights(det, self.mode, eta)
            if on_device:
                capi.dev.stokes_weights_demod(obs.n_local_samples, values, weights.indices(dets),
                                              accel_device_ptr(weights.buffer), weights.buffer.shape[0],
                                              single_precision=self.single_precision)
                weights.accel_used(True)
            else:
                for idet, det in enumerate(dets):
                    weights[det] = values[idet].astype(dtype)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        return {"shared": list(), "detdata": list()}

    def _provides(self):
        return {"detdata": [self.weights]}

    def _implementations(self):
        from ..traits import ImplementationType

        return [ImplementationType.DEFAULT, ImplementationType.COMPILED]

    def _supports_accel(self):
        return True
