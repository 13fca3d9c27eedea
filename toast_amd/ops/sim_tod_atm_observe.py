"""ObserveAtmosphere: detector pointing observes simulated atmosphere slabs (reference:
src/toast/ops/sim_tod_atm_observe.py:27-628).

``data[sim][session_name][wind_index]`` is a list of ``toast_amd.atm.AtmSim`` slabs, as in the reference; every view of
the data picks the wind interval it lies in (:214-236) and accumulates the line-of-sight integrals of all its slabs.
On the device all detectors of a view go through each slab in ONE launch (csrc/atm_observe.hip): the good-sample mask
and the extent of every detector's times, az and el come from one reduction kernel, the integrals accumulate in a
scratch row per detector, failed samples are flagged after a slab that reported a failure (:379-399) and a finish
kernel applies gain, absorption, polarization, loading and the unit scale (:424-483).  Without a device the same steps
run through ``AtmSim.observe`` on NumPy.

Not part of this operator: the interpolated path (``sample_rate``), the fade at wind breaks (``fade_time`` with more
than one view) and the bandpass convolution of absorption and loading -- ``ob[absorption][det]`` and
``ob[loading][det]`` hold band-averaged values.

The reference's flagging statement ``det_flags[vw][det][good][bad] |= mask`` (:396-398) writes into the copy that the
boolean index ``[good]`` makes and so leaves the flags as they were; this operator raises the mask, which is what the
statement is there to do."""

import numpy as np

from .. import capi
from ..accel import Resident, accel_data_update_host, accel_enabled, device_scratch
from ..data import KELVIN_TO, defaults
from ..traits import Bool, Float, Int, TraitError, Unicode
from .operator import Operator

TWOPI = 2 * np.pi


def quats_to_azel(quats):
    """az, el of detector quaternions [n][4]: qa_to_angles (src/libtoast/src/toast_math_qarray.cpp:1166-1188) --
    normalise, rotate the z axis, theta = pi / 2 - asin(dir.z), phi = atan2(dir.y, dir.x) wrapped to [0, 2 pi) -- then
    az = 2 pi - phi, el = pi / 2 - theta (sim_tod_atm_observe.py:287-288)."""
    q = np.asarray(quats, dtype=np.float64)
    norm = 0.0
    for k in range(4):
        norm = norm + q[:, k] * q[:, k]
    q = q * (1.0 / np.sqrt(norm))[:, None]
    n2 = 0.0
    for k in range(4):
        n2 = n2 + q[:, k] * q[:, k]
    u = q * (1.0 / np.sqrt(n2))[:, None]
    xw, yw = u[:, 3] * u[:, 0], u[:, 3] * u[:, 1]
    x2, xz, y2, yz = -u[:, 0] * u[:, 0], u[:, 0] * u[:, 2], -u[:, 1] * u[:, 1], u[:, 1] * u[:, 2]
    d0 = 2 * (yw + xz) + 0.0
    d1 = 2 * (yz - xw) + 0.0
    d2 = 2 * (x2 + y2) + 1.0
    theta = np.pi / 2 - np.arcsin(d2)
    phi = np.arctan2(d1, d0)
    phi = np.where(phi < 0.0, phi + TWOPI, phi)
    return TWOPI - phi, np.pi / 2 - theta


class ObserveAtmosphere(Operator):
    """Operator which uses detector pointing to observe a simulated atmosphere slab."""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key for accumulating dipole timestreams")
    det_data_units = Unicode(defaults.det_data_units, help="Output units if creating detector data")
    quats_azel = Unicode(defaults.quats_azel, allow_none=True, help="Observation detdata key for detector quaternions")
    weights = Unicode(None, allow_none=True, help="Observation detdata key for detector Stokes weights")
    weights_mode = Unicode("IQU", help="Stokes weights mode (eg. 'I', 'IQU', 'QU')")
    polarization_fraction = Float(0, help="Polarization fraction (only Q polarization).")
    view = Unicode(None, allow_none=True, help="Use this view of valid data in all observations")
    wind_view = Unicode("wind", help="The view of times matching individual simulated atmosphere slabs")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional flagging")
    det_mask = Int(defaults.det_mask_invalid, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for detector sample flagging")
    sim = Unicode("atm_sim", help="Data key with the dictionary of sims per session")
    absorption = Unicode(None, allow_none=True, help="The observation key for the absorption")
    loading = Unicode(None, allow_none=True, help="The observation key for the loading")
    n_bandpass_freqs = Int(100, help="The number of sampling frequencies used when convolving the bandpass with "
                           "atmosphere absorption and loading (accepted; the values are band averages already)")
    sample_rate = Float(None, allow_none=True, help="Rate [Hz] at which to sample atmospheric TOD before interpolation.  "
                        "Default is no interpolation; the interpolated path is not implemented")
    fade_time = Float(None, allow_none=True, help="Fade in/out time [s] to avoid a step at wind break (not implemented "
                      "for more than one view)")
    gain = Float(1.0, help="Scaling applied to the simulated TOD")
    debug_tod = Bool(False, help="If True, dump TOD to pickle files (ignored)")

    def _validate_det_mask(self, value):
        if value < 0:
            raise TraitError("Det mask should be a positive integer")
        return value

    def _validate_det_flag_mask(self, value):
        if value < 0:
            raise TraitError("Flag mask should be a positive integer")
        return value

    def _validate_shared_flag_mask(self, value):
        if value < 0:
            raise TraitError("Flag mask should be a positive integer")
        return value

    # ------------------------------------------------------------------ pieces of the reference's _exec
    @staticmethod
    def _std_range(x):
        """A 'standard' range for an array of angles, ie. [lo, hi] with 0 <= lo < 2pi and 0 <= hi - lo (:507-519)."""
        y = np.unwrap(x)
        return ObserveAtmosphere._std_range_of(y.min(), y.max())

    @staticmethod
    def _std_range_of(lo, hi):
        a, b = np.divmod(lo, TWOPI)
        return b, hi - TWOPI * a

    def _detector_absorption_and_loading(self, obs, absorption_key, loading_key, dets):
        """Per-detector absorption and loading (:521-550).  The Focalplane has no bandpass: the values under
        ``obs[key][det]`` are band averages already."""
        absorption_det = None if absorption_key is None else {d: float(obs[absorption_key][d]) for d in dets}
        loading_det = None if loading_key is None else {d: float(obs[loading_key][d]) for d in dets}
        return absorption_det, loading_det

    def _wind_index(self, ob, cur_wind, n_views, t_first):
        """(:220-226)"""
        wind = ob.intervals[self.wind_view]
        times = ob.shared[self.times].data
        if n_views > 1:
            while cur_wind < len(wind) - 1 and t_first > times[wind[cur_wind].last - 1]:
                cur_wind += 1
        return cur_wind

    def _check_slab(self, prefix, det, sim, tmin_det, tmax_det, az_range, el_range):
        """The reference's two errors (:319-339)."""
        if sim.tmin > tmin_det or sim.tmax < tmax_det:
            raise RuntimeError(f"{prefix} : {det} Detector time: [{tmin_det:.1f}, {tmax_det:.1f}], is not contained in "
                               f"[{sim.tmin:.1f}, {sim.tmax:.1f}]")
        (azmin_det, azmax_det), (elmin_det, elmax_det) = az_range, el_range
        if not (sim.azmin <= azmin_det and azmax_det <= sim.azmax) or not (
                sim.elmin <= elmin_det and elmin_det <= sim.elmax):
            raise RuntimeError(f"{prefix} : {det} Detector Az/El: [{azmin_det:.5f}, {azmax_det:.5f}], "
                               f"[{elmin_det:.5f}, {elmax_det:.5f}] is not contained in [{sim.azmin:.5f}, "
                               f"{sim.azmax:.5f}], [{sim.elmin:.5f} {sim.elmax:.5f}]")

    def _components(self):
        comp_i = self.weights_mode.index("I") if "I" in self.weights_mode else -1
        comp_q = self.weights_mode.index("Q") if "Q" in self.weights_mode else -1
        return comp_i, comp_q

    # ------------------------------------------------------------------ exec
    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        if self.absorption is None:
            raise RuntimeError("You must set the 'absorption' trait before calling exec()")
        if self.sample_rate is not None:
            raise NotImplementedError("ObserveAtmosphere: the interpolated path (sample_rate) is not implemented")
        on_dev = accel_enabled() if use_accel is None else bool(use_accel)
        for ob in data.obs:
            dets = ob.select_local_detectors(detectors, flagmask=self.det_mask)
            absorption, loading = self._detector_absorption_and_loading(ob, self.absorption, self.loading, dets)
            ob.detdata.ensure(self.det_data, detectors=dets, create_units=self.det_data_units)
            if len(dets) == 0:
                continue
            units = ob.detdata[self.det_data].units
            if units not in KELVIN_TO:
                raise RuntimeError(f"ObserveAtmosphere: no conversion from K to '{units}'")
            scale = KELVIN_TO[units]
            views = ob.intervals[self.view]
            if len(views) > 1 and self.fade_time is not None:
                raise NotImplementedError("ObserveAtmosphere: fading between wind views (fade_time) is not implemented")
            prefix = f"{data.comm.group if hasattr(data.comm, 'group') else 0} : {ob.name}"
            run = self._observe_device if on_dev else self._observe_host
            run(data, ob, dets, views, absorption, loading, scale, prefix)

    def _observe_host(self, data, ob, dets, views, absorption, loading, scale, prefix):
        times_all = ob.shared[self.times].data
        sh_all = None if self.shared_flags is None else ob.shared[self.shared_flags].data
        signal = ob.detdata[self.det_data].data
        quats = ob.detdata[self.quats_azel].data
        flags = None if self.det_flags is None else ob.detdata[self.det_flags].data
        weights = None if self.weights is None else ob.detdata[self.weights].data
        rows = {name: ob.detdata[name].indices(dets) for name in (self.det_data, self.quats_azel)}
        if flags is not None:
            rows[self.det_flags] = ob.detdata[self.det_flags].indices(dets)
        if weights is not None:
            rows[self.weights] = ob.detdata[self.weights].indices(dets)
        comp_i, comp_q = self._components()
        cur_wind = 0
        for iv in views:
            first, last = int(iv.first), int(iv.last)
            times = times_all[first:last]
            if times.size == 0:
                continue
            cur_wind = self._wind_index(ob, cur_wind, len(views), times[0])
            sh = None if sh_all is None else sh_all[first:last] & self.shared_flag_mask
            sim_list = data[self.sim][ob.session.name][cur_wind]
            for k, det in enumerate(dets):
                bits = np.zeros(times.size, dtype=np.uint8)
                if flags is not None:
                    bits |= flags[rows[self.det_flags][k], first:last] & self.det_flag_mask
                if sh is not None:
                    bits |= sh
                good = bits == 0
                if not np.any(good):
                    continue
                az, el = quats_to_azel(quats[rows[self.quats_azel][k], first:last][good])
                t_good = np.ascontiguousarray(times[good])
                atm = np.zeros(t_good.size)
                az_range, el_range = self._std_range(az), self._std_range(el)
                for sim in sim_list:
                    self._check_slab(prefix, det, sim, t_good[0], t_good[-1], az_range, el_range)
                    err = sim.observe(t_good, az, el, atm, -1.0, use_accel=False)
                    if err != 0 and flags is not None:
                        bad = np.abs(atm) < 1e-30
                        idx = first + np.nonzero(good)[0][bad]
                        flags[rows[self.det_flags][k], idx] |= np.uint8(self.det_flag_mask)
                atm *= self.gain * absorption[det]
                if weights is None:
                    w_i, w_q = 1, 0
                else:
                    w = weights[rows[self.weights][k], first:last][good]
                    w_i = w[:, comp_i].copy() if comp_i >= 0 else 0
                    w_q = w[:, comp_q].copy() if comp_q >= 0 else 0
                atm *= w_i + w_q * self.polarization_fraction
                if loading is not None:
                    atm += loading[det] / np.sin(el)
                signal[rows[self.det_data][k], first + np.nonzero(good)[0]] += scale * atm

    def _observe_device(self, data, ob, dets, views, absorption, loading, scale, prefix):
        dd, qd = ob.detdata[self.det_data], ob.detdata[self.quats_azel]
        fd = None if self.det_flags is None else ob.detdata[self.det_flags]
        wd = None if self.weights is None else ob.detdata[self.weights]
        td = ob.shared[self.times]
        sd = None if self.shared_flags is None else ob.shared[self.shared_flags]
        n_all = ob.n_local_samples
        signal, quats, times_dev = Resident(dd, self.det_data), Resident(qd, self.quats_azel), Resident(td, self.times)
        flags = None if fd is None else Resident(fd, self.det_flags)
        wts = None if wd is None else Resident(wd, self.weights)
        shared = None if sd is None else Resident(sd, self.shared_flags)
        row_d, row_q = dd.indices(dets), qd.indices(dets)
        row_f = None if fd is None else fd.indices(dets)
        row_w = None if wd is None else wd.indices(dets)
        nnz = 0 if wd is None else int(np.prod(wd.detector_shape[1:], dtype=np.int64))
        comp_i, comp_q = self._components()
        ga = np.array([self.gain * absorption[d] for d in dets], dtype=np.float64)
        ld = None if loading is None else np.array([loading[d] for d in dets], dtype=np.float64)
        times_host = td.data
        cur_wind = 0
        wrote_flags = False
        for iv in views:
            first, last = int(iv.first), int(iv.last)
            n = last - first
            if n <= 0:
                continue
            cur_wind = self._wind_index(ob, cur_wind, len(views), times_host[first])
            sim_list = data[self.sim][ob.session.name][cur_wind]
            p_quats = quats.ptr + first * 32
            p_flags = 0 if flags is None else flags.ptr + first
            p_shared = 0 if shared is None else shared.ptr + first
            p_times = times_dev.ptr + first * 8
            with device_scratch("atm_observe", owner=self) as s:
                s.work("good", np.zeros((len(dets), n), dtype=np.uint8))
                s.work("atm", np.zeros((len(dets), n), dtype=np.float64))
                d_good, d_atm = s.ptr("good"), s.ptr("atm")
                capi.dev.memset(d_atm, 0, len(dets) * n * 8)
                ranges = capi.dev.atm_good_ranges(n, n_all, row_q, p_quats, qd.shape[0], row_f, p_flags,
                                                  0 if fd is None else fd.shape[0], self.det_flag_mask, p_shared,
                                                  self.shared_flag_mask, d_good)
                seen = [k for k in range(len(dets)) if ranges[k, 0] >= 0]
                extent = {}
                for k in seen:
                    r = ranges[k]
                    if r[6] - r[5] < np.pi:
                        az_range = self._std_range_of(r[4] + r[5], r[4] + r[6])
                    else:
                        # the scan wanders more than pi from its first good sample: np.unwrap on the host
                        az_range = self._std_range(self._host_az(qd, row_q[k], first, last, s.fetch("good")[k]))
                    extent[k] = (times_host[first + int(r[0])], times_host[first + int(r[1])], az_range,
                                 self._std_range_of(r[2], r[3]))
                for sim in sim_list:
                    for k in seen:
                        self._check_slab(prefix, dets[k], sim, *extent[k])
                    status = sim.observe_quats(n, n_all, p_times, row_q, p_quats, qd.shape[0], d_good, d_atm)
                    if np.any(status != 0) and flags is not None:
                        capi.dev.atm_flag_failed(n, n_all, d_good, d_atm, row_f, status, p_flags, fd.shape[0],
                                                 self.det_flag_mask)
                        wrote_flags = True
                capi.dev.atm_finish(n, n_all, d_good, d_atm, ga, ld, row_q, p_quats, qd.shape[0], row_w,
                                    0 if wts is None else wts.ptr + first * nnz * 8, 0 if wd is None else wd.shape[0],
                                    nnz, comp_i, comp_q, self.polarization_fraction, scale, row_d,
                                    signal.ptr + first * 8, dd.shape[0])
        signal.write_back_unless_lazy(data)
        if flags is not None:
            if wrote_flags:
                flags.write_back_unless_lazy(data)
            else:
                flags.host_stays_current()
                flags.drop_if_created()
        for res in (quats, times_dev, wts, shared):
            if res is not None:
                res.host_stays_current()
                res.drop_if_created()

    def _host_az(self, qd, row, first, last, good):
        if qd.accel_in_use():
            accel_data_update_host(qd.buffer, self.quats_azel)
        az, _ = quats_to_azel(qd.buffer[row, first:last][good != 0])
        return az

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"global": [self.sim], "shared": [self.times], "detdata": [self.det_data, self.quats_azel],
               "intervals": [self.wind_view]}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        if self.weights is not None:
            req["detdata"].append(self.weights)
        if self.view is not None:
            req["intervals"].append(self.view)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": [self.det_data], "intervals": []}

    def _supports_accel(self):
        return True
