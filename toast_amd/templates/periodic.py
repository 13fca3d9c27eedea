"""Periodic template: one amplitude per detector and observation for every bin of a shared (or per-detector) quantity.

Reference: src/toast/templates/periodic.py (pure NumPy, one detector and one view at a time).  With ``key="azimuth"``
this is the ground template solved inside the map-maker.  The amplitude layout is the reference's: detector-major;
within a detector by observation, then by bin.

Two paths.  The host path (``use_accel`` false) is NumPy with the reference's own expressions.  The device path
(``add_to_signal_multi`` / ``project_signal_multi`` and ``_apply_precond`` on resident vectors) runs the kernels of
csrc/template_basis.hip on a cached int32 row of bin indices per observation.

Reproduced from the reference, on both paths:

* the bin of a sample is ``int32((v - obs_min) / incr)``, truncated, clamped to ``nbins - 1``;
* ``add_to_signal`` applies the key's own flags only, ``project_signal`` and the hit counts also the detector flags;
* ``hits < minimum_bin_hits`` is evaluated after EVERY view and a flag is never cleared (periodic.py:251-271), so a bin
  that reaches the minimum only in a later view stays flagged;
* ``apply_precond`` leaves the output untouched where the amplitude is flagged.

Not reproduced: with ``is_detdata_key=True`` the reference slices the FIRST axis of the detector data with the sample
range of a view (``ob.detdata[key].data[vw_slc]``, periodic.py:124, 254, 293), i.e. it selects detector rows by sample
numbers.  Here a per-detector key means what its help string says: every detector is binned by its own row of the key
(and flagged by its own row of ``flags``); ``obs_min`` / ``obs_max`` run over the good samples of all rows.  An
observation without the key has no amplitudes; the reference indexes its per-observation lists by position and
misplaces the later observations in that case.
"""

import numpy as np

from ..accel import accel_device_ptr
from ..traits import Bool, Float, Int, Unicode
from . import Amplitudes, DeviceMirror, Template, make_resident, release_borrowed


class Periodic(Template):
    """Amplitudes which are periodic in time: a value per detector, observation and bin of the ``key`` data."""

    is_detdata_key = Bool(False, help="If True, the periodic data and flags are detector fields, not shared")
    key = Unicode(None, allow_none=True, help="Observation data key for the periodic quantity")
    flags = Unicode(None, allow_none=True, help="Observation data key for flags to use")
    flag_mask = Int(0, help="Bit mask value for flags")
    bins = Int(10, allow_none=True, help="Number of bins between min / max values of data key")
    increment = Float(None, allow_none=True, help="The increment of the data key for each bin")
    minimum_bin_hits = Int(3, help="Minimum number of samples per amplitude bin")

    def __init__(self, **kwargs):
        self._index = {}        # per observation: the mirror of its int32 rows of bin indices
        super().__init__(**kwargs)

    _amp_hits = property(lambda self: self._mirrors["hits"].host)

    # ------------------------------------------------------------------ set-up
    def _key_field(self, ob):
        return ob.detdata if self.is_detdata_key else ob.shared

    def _has_key(self, ob):
        return self.key in self._key_field(ob)

    def _key_rows(self, ob):
        """(key values, flag values or None) as [n_row][n_samp] host arrays; one row for a shared key."""
        field = self._key_field(ob)
        vals = np.asarray(field[self.key].data, dtype=np.float64)
        flg = None if self.flags is None else np.asarray(field[self.flags].data)
        if not self.is_detdata_key:
            vals = vals.reshape(1, -1)
            flg = None if flg is None else flg.reshape(1, -1)
        return vals, flg

    def _initialize(self, new_data):
        from ..accel import accel_enabled

        self.clear()
        if self.key is None:
            raise RuntimeError("You must set key before initializing")
        if self.bins is not None and self.increment is not None:
            raise RuntimeError("Only one of bins and increment can be specified")
        if self.bins is None and self.increment is None:
            raise RuntimeError("One of bins and increment must be specified")
        all_dets = {}
        self._obs_dets = {}
        self._obs_min, self._obs_max, self._obs_incr, self._obs_nbins = {}, {}, {}, {}
        total_bins = 0
        for iob, ob in enumerate(new_data.obs):
            self._obs_dets[iob] = set()
            if not self._has_key(ob):
                continue
            vals, flg = self._key_rows(ob)
            omin = omax = None
            for vw in ob.intervals[self.view]:
                vw_data = vals[:, vw.first:vw.last]
                if flg is not None:
                    vw_data = vw_data[np.logical_not(flg[:, vw.first:vw.last] & self.flag_mask)]
                if vw_data.size == 0:
                    continue
                vmin, vmax = np.amin(vw_data), np.amax(vw_data)
                omin = vmin if omin is None else min(omin, vmin)
                omax = vmax if omax is None else max(omax, vmax)
            if omin is None or omin == omax:
                raise RuntimeError(f"Periodic data {self.key} is constant for observation {ob.name}")
            if self.bins is not None:
                obins = int(self.bins)
                oincr = (omax - omin) / obins if obins > 0 else 0.0
            else:
                oincr = float(self.increment)
                obins = int((omax - omin) / oincr)
            self._obs_min[iob], self._obs_max[iob] = float(omin), float(omax)
            self._obs_nbins[iob], self._obs_incr[iob] = obins, float(oincr)
            total_bins += obins
            dets = self._obs_detectors(ob, also_in=(self.key,) if self.is_detdata_key else ())
            self._obs_dets[iob] = set(dets)
            all_dets.update(dict.fromkeys(dets))
        self._all_dets = list(all_dets.keys())
        if total_bins == 0:
            raise RuntimeError(f"Template {self.name} has zero amplitude bins- change the binning size.")
        self._layout_detector_major(new_data.comm, self._obs_nbins)
        self._mirrors["hits"] = DeviceMirror(np.zeros(self._n_local, dtype=np.int32), f"{self.name}_hits")
        self._amp_flags = np.zeros(self._n_local, dtype=bool)
        if self._n_local == 0:
            return
        # (set-up runs on the device for a template that will be swept there; what it reads is handed back)
        if accel_enabled() and self.supports_accel():
            self._init_hits_device(new_data)
        else:
            self._init_hits_host(new_data)

    def _host_index(self, iob, ob):
        """int32 [n_row][n_samp]: the bin of every sample in view whose key flags are clear (periodic.py:311-317),
        -1 elsewhere; computed once per observation."""
        if iob not in self._index:
            vals, flg = self._key_rows(ob)
            index = np.full(vals.shape, -1, dtype=np.int32)
            nbins = self._obs_nbins[iob]
            for vw in ob.intervals[self.view]:
                sl = slice(vw.first, vw.last)
                for row in range(vals.shape[0]):
                    if flg is not None:
                        good = np.logical_not(flg[row, sl] & self.flag_mask)
                    else:
                        good = np.ones(vw.last - vw.first, dtype=bool)
                    amp_indx = np.array((vals[row, sl][good] - self._obs_min[iob]) / self._obs_incr[iob], dtype=np.int32)
                    amp_indx[amp_indx >= nbins] = nbins - 1
                    index[row, sl][good] = amp_indx
            self._index[iob] = DeviceMirror(index, f"{self.name}_index")
        return self._index[iob].host

    def _index_row(self, ob, det):
        return int(ob.detdata[self.key].indices([det])[0]) if self.is_detdata_key else 0

    def _init_hits_host(self, new_data):
        """periodic.py:232-272, view after view."""
        for det in self._all_dets:
            amp_offset = self._det_start[det]
            for iob, ob in enumerate(new_data.obs):
                if det not in self._obs_dets[iob]:
                    continue
                nbins = self._obs_nbins[iob]
                irow = self._host_index(iob, ob)[self._index_row(ob, det)]
                amp_hits = self._amp_hits[amp_offset:amp_offset + nbins]
                amp_flags = self._amp_flags[amp_offset:amp_offset + nbins]
                for vw in ob.intervals[self.view]:
                    sl = slice(vw.first, vw.last)
                    good = irow[sl] >= 0
                    if self.det_flags is not None:
                        good &= (ob.detdata[self.det_flags][det, sl] & self.det_flag_mask) == 0
                    np.add.at(amp_hits, irow[sl][good], 1)
                    amp_flags[amp_hits < self.minimum_bin_hits] = True
                amp_offset += nbins

    def _device_index(self, iob, ob, borrowed=None):
        """Device pointer of the cached index of one observation (toast_hip_periodic_index_dev on first use)."""
        from .. import capi

        index = self._index.get(iob)
        if index is None or not index.on_device:
            field = self._key_field(ob)
            key = make_resident(field[self.key], self.key, borrowed)
            kbuf = key.buffer if self.is_detdata_key else key.data
            if kbuf.dtype != np.float64:
                raise RuntimeError(f"Periodic template {self.name}: the key {self.key} must be float64 on the device")
            f_ptr = 0
            if self.flags is not None:
                fl = make_resident(field[self.flags], self.flags, borrowed)
                fbuf = fl.buffer if self.is_detdata_key else fl.data
                if fbuf.dtype != np.uint8 or fbuf.shape != kbuf.shape:
                    raise RuntimeError(f"Periodic template {self.name}: the flags {self.flags} must be uint8 with the "
                                       f"shape of the key")
                f_ptr = accel_device_ptr(fbuf)
            n_row = kbuf.shape[0] if self.is_detdata_key else 1
            host_valid = index is not None
            if not host_valid:
                index = self._index[iob] = DeviceMirror(np.empty((n_row, ob.n_local_samples), dtype=np.int32),
                                                        f"{self.name}_index")
            capi.dev.periodic_index(accel_device_ptr(kbuf), f_ptr, self.flag_mask, n_row, ob.n_local_samples,
                                    self._obs_min[iob], self._obs_incr[iob], self._obs_nbins[iob],
                                    ob.intervals[self.view].data, index.create().ptr)
            if not host_valid:
                index.written()      # (rows that _host_index computed are the same ones: both sides current)
        return index.ptr

    def _index_rows(self, ob, dets):
        return ob.detdata[self.key].indices(dets) if self.is_detdata_key else None

    def _init_hits_device(self, new_data):
        """Hits of the first view, then of all views (toast_hip_periodic_hits_dev).  The hit counts only grow, so an
        amplitude is below the minimum after SOME view exactly when it is below it after the FIRST view: the flags of
        periodic.py:270-271 are ``hits_after_first_view < minimum_bin_hits``.  The first view is the sample range up to
        its end, which needs the views sorted and disjoint: checked."""
        from .. import capi

        hits = self._mirrors["hits"].create(zero_out=True)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            views = ob.intervals[self.view]
            if len(dets) == 0 or len(views) == 0 or self._obs_nbins[iob] == 0:
                continue
            borrowed = []
            f_idx, f_ptr = self._det_flag_args(ob, dets, borrowed)
            args = (self._device_index(iob, ob, borrowed), self._index_rows(ob, dets), f_idx, f_ptr, self.det_flag_mask,
                    self.det_amp_offsets(iob, dets), ob.n_local_samples, self._obs_nbins[iob])
            # [0, views[0].last) holds exactly the first view: interval lists are sorted and disjoint (IntervalList)
            firsts = np.array([int(v.first) for v in views])
            lasts = np.array([int(v.last) for v in views])
            if np.any(firsts[1:] < lasts[:-1]):
                raise RuntimeError(f"Periodic template {self.name}: the intervals of view {self.view} of observation "
                                   f"{ob.name} are not sorted and disjoint")
            split = int(views[0].last)
            capi.dev.periodic_hits(*args, 0, split, hits.ptr)
            hits.written()
            for off in self.det_amp_offsets(iob, dets):
                sl = slice(int(off), int(off) + self._obs_nbins[iob])
                self._amp_flags[sl] = self._amp_hits[sl] < self.minimum_bin_hits
            capi.dev.periodic_hits(*args, split, ob.n_local_samples, hits.ptr)
            hits.written()
            _ = hits.host      # (fetched now: the kernels are done with what was borrowed)
            release_borrowed(borrowed)

    # ------------------------------------------------------------------ Template interface
    def _detectors(self):
        return self._all_dets

    def _zeros(self):
        z = Amplitudes(self.data.comm, self._n_global, self._n_local)
        z.local_flags[:] = np.where(self._amp_flags, 1, 0)
        return z

    def add_to_signal_multi(self, detectors, amplitudes, **kwargs):
        """All detectors of an observation in one launch (device-resident buffers only)."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            if self._obs_nbins[iob] == 0:
                continue
            capi.dev.periodic_add_to_signal(self._device_index(iob, ob), self._index_rows(ob, dets),
                                            self.det_amp_offsets(iob, dets), accel_device_ptr(amplitudes.buffer),
                                            dd.indices(dets), accel_device_ptr(dd.buffer), ob.n_local_samples,
                                            self._obs_nbins[iob])

    def project_signal_multi(self, detectors, amplitudes, path=0, **kwargs):
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            if self._obs_nbins[iob] == 0:
                continue
            f_idx, f_ptr = self._det_flag_args(ob, dets)
            capi.dev.periodic_project_signal(self._device_index(iob, ob), self._index_rows(ob, dets), dd.indices(dets),
                                             accel_device_ptr(dd.buffer), f_idx, f_ptr, self.det_flag_mask,
                                             self.det_amp_offsets(iob, dets), accel_device_ptr(amplitudes.buffer),
                                             ob.n_local_samples, self._obs_nbins[iob], path=path)

    def _add_to_signal_host(self, detector, amplitudes):
        amp_offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            nbins = self._obs_nbins[iob]
            amps = local[amp_offset:amp_offset + nbins]
            irow = self._host_index(iob, ob)[self._index_row(ob, detector)]
            row = ob.detdata[self.det_data][detector]
            for vw in ob.intervals[self.view]:
                sl = slice(vw.first, vw.last)
                good = irow[sl] >= 0
                row[sl][good] += amps[irow[sl][good]]
            amp_offset += nbins

    def _project_signal_host(self, detector, amplitudes):
        amp_offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            nbins = self._obs_nbins[iob]
            amps = local[amp_offset:amp_offset + nbins]
            irow = self._host_index(iob, ob)[self._index_row(ob, detector)]
            row = ob.detdata[self.det_data][detector]
            for vw in ob.intervals[self.view]:
                sl = slice(vw.first, vw.last)
                good = irow[sl] >= 0
                if self.det_flags is not None:
                    good &= (ob.detdata[self.det_flags][detector, sl] & self.det_flag_mask) == 0
                np.add.at(amps, irow[sl][good], row[sl][good])
            amp_offset += nbins

    def _add_prior(self, amplitudes_in, amplitudes_out, **kwargs):
        return      # no prior for this template (periodic.py:392-394)

    def _apply_precond(self, amplitudes_in, amplitudes_out, use_accel=None, **kwargs):
        if self._n_local == 0:
            return
        if amplitudes_in.accel_in_use() or amplitudes_out.accel_in_use():
            from .. import capi

            amplitudes_in.accel_resident()
            amplitudes_out.accel_resident()
            capi.dev.periodic_apply_precond(self._n_local, self._mirrors["hits"].upload().ptr,
                                            accel_device_ptr(amplitudes_in.local_flags),
                                            accel_device_ptr(amplitudes_in.buffer), accel_device_ptr(amplitudes_out.buffer))
            return
        # periodic.py:396-419
        amp_good = amplitudes_in.local_flags == 0
        amplitudes_out.local[amp_good] = amplitudes_in.local[amp_good] * self._amp_hits[amp_good]

    def write(self, amplitudes, out):
        raise NotImplementedError("Periodic.write (an HDF5 dump of the amplitudes) is not part of this project")

    def plot(self, amp_file, out_root=None):
        raise NotImplementedError("Periodic.plot (diagnostic figures from an HDF5 dump) is not part of this project")

    def clear(self):
        """Release the device copies of the index rows and of the hit counts; forget the cached indices."""
        for index in self._index.values():
            index.drop(fetch=False)
        self._index = {}
        super().clear()
