"""SimDipole: the CMB dipole, solar and orbital, accumulated into detector timestreams (reference:
src/toast/ops/sim_tod_dipole.py:19-244 over src/toast/dipole.py).

Trait names, defaults and validators are the reference's; its ``Quantity`` traits are ``Float`` here: ``solar_speed`` in
km/s, ``solar_gal_lat`` / ``solar_gal_lon`` in degrees, ``cmb`` in K, ``freq`` in Hz.  The telescope velocity under
``ob.shared[velocity]`` is [n_samp, 3] in km/s, in the coordinate system of the boresight (``coord``).

On the device one launch per observation covers all views and all selected detectors (csrc/sim_dipole.hip): the
boresight, the flags and the velocity are read once per sample, detector quaternions are never written.  Without a device
``toast_amd.dipole.dipole`` runs per view and detector, as the reference does.

``shared_flags=None`` works here and means no flagging; the reference indexes ``views.shared[None]`` and fails."""

import numpy as np

from .. import capi, dipole
from ..accel import Resident, accel_enabled
from ..data import KELVIN_TO, defaults
from ..synth import quat_mult
from ..traits import Bool, Float, Int, TraitError, Unicode
from .operator import Operator


class SimDipole(Operator):
    """Operator which generates dipole signal for detectors."""

    API = Int(0, help="Internal interface version for this operator")
    det_data = Unicode(defaults.det_data, help="Observation detdata key for accumulating dipole timestreams")
    det_data_units = Unicode(defaults.det_data_units, help="Output units if creating detector data")
    view = Unicode(None, allow_none=True, help="Use this view of the data in all observations")
    boresight = Unicode(defaults.boresight_radec, help="Observation shared key for boresight")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_invalid, help="Bit mask value for optional flagging")
    velocity = Unicode(defaults.velocity, help="Observation shared key for velocity")
    subtract = Bool(False, help="If True, subtract the dipole timestream instead of accumulating")
    mode = Unicode("total", help="Valid options are solar, orbital, and total")
    coord = Unicode("E", help="Valid options are 'C' (Equatorial), 'E' (Ecliptic), and 'G' (Galactic)")
    solar_speed = Float(dipole.solar_speed,
                        help="Amplitude of the solarsystem barycenter velocity with respect to the CMB [km/s]")
    solar_gal_lat = Float(dipole.solar_gal_lat, help="Galactic latitude of direction of solarsystem motion [degrees]")
    solar_gal_lon = Float(dipole.solar_gal_lon, help="Galactic longitude of direction of solarsystem motion [degrees]")
    cmb = Float(dipole.t_cmb, help="CMB monopole value [K]")
    freq = Float(0.0, help="Optional observing frequency [Hz]")

    def _validate_mode(self, value):
        if value not in ["solar", "orbital", "total"]:
            raise TraitError("Invalid mode (must be 'solar', 'orbital' or 'total')")
        return value

    def _validate_coord(self, value):
        if value is not None:
            if value not in ["E", "C", "G"]:
                raise TraitError("coordinate system must be 'E', 'C', or 'G'")
        return value

    def _validate_shared_flag_mask(self, value):
        if value < 0:
            raise TraitError("Flag mask should be a positive integer")
        return value

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        on_dev = accel_enabled() if use_accel is None else bool(use_accel)
        solar_vel = dipole.solar_velocity(self.coord, self.solar_speed, self.solar_gal_lat, self.solar_gal_lon)
        sol = solar_vel if self.mode in ("solar", "total") else None
        for ob in data.obs:
            dets = ob.select_local_detectors(detectors)
            ob.detdata.ensure(self.det_data, detectors=dets, create_units=self.det_data_units)
            if len(dets) == 0:
                continue
            units = ob.detdata[self.det_data].units
            if units not in KELVIN_TO:
                raise RuntimeError(f"SimDipole: no conversion from K to '{units}'")
            scale = -KELVIN_TO[units] if self.subtract else KELVIN_TO[units]
            views = ob.intervals[self.view]
            vel = ob.shared[self.velocity] if self.mode in ("orbital", "total") else None
            if vel is not None and vel.data.shape != (ob.n_local_samples, 3):
                raise RuntimeError(f"SimDipole: '{self.velocity}' should hold [n_samp, 3] velocities")
            run = self._dipole_device if on_dev else self._dipole_host
            run(data, ob, dets, views, vel, sol, scale)

    def _dipole_host(self, data, ob, dets, views, vel, sol, scale):
        nullquat = np.array([0, 0, 0, 1], dtype=np.float64)
        bore_all = ob.shared[self.boresight].data
        flags_all = None if self.shared_flags is None else ob.shared[self.shared_flags].data
        signal = ob.detdata[self.det_data].data
        rows = ob.detdata[self.det_data].indices(dets)
        focalplane = ob.telescope.focalplane
        for iv in views:
            first, last = int(iv.first), int(iv.last)
            if last <= first:
                continue
            boresight = np.array(bore_all[first:last])
            if flags_all is not None:
                bad = (flags_all[first:last] & self.shared_flag_mask) != 0
                boresight[bad, :] = nullquat
            v = None if vel is None else vel.data[first:last]
            for row, det in zip(rows, dets):
                quats = quat_mult(boresight, focalplane[det]["quat"])
                dipole_tod = dipole.dipole(quats, vel=v, solar=sol, cmb=self.cmb, freq=self.freq)
                signal[row, first:last] += scale * dipole_tod

    def _dipole_device(self, data, ob, dets, views, vel, sol, scale):
        dd, bd = ob.detdata[self.det_data], ob.shared[self.boresight]
        sd = None if self.shared_flags is None else ob.shared[self.shared_flags]
        n_all = ob.n_local_samples
        signal, bore = Resident(dd, self.det_data), Resident(bd, self.boresight)
        flags = None if sd is None else Resident(sd, self.shared_flags)
        velocity = None if vel is None else Resident(vel, self.velocity)
        focalplane = ob.telescope.focalplane
        fp = np.array([focalplane[d]["quat"] for d in dets], dtype=np.float64).reshape((-1, 4))
        capi.dev.sim_dipole(fp, bore.ptr, dd.indices(dets), signal.ptr, dd.shape[0], n_all, views.data,
                            0 if flags is None else flags.ptr, 0 if flags is None else n_all, self.shared_flag_mask,
                            0 if velocity is None else velocity.ptr, sol, self.cmb, self.freq, scale)
        signal.write_back_unless_lazy(data)
        for res in (bore, flags, velocity):
            if res is not None:
                res.host_stays_current()
                res.drop_if_created()

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [self.boresight, self.shared_flags], "detdata": [self.det_data], "intervals": []}
        if self.view is not None:
            req["intervals"].append(self.view)
        return req

    def _provides(self):
        return {"meta": [], "shared": [], "detdata": [self.det_data]}

    def _supports_accel(self):
        return True
