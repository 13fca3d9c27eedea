"""SubHarmonic template: Legendre polynomials per detector and view, solved with the map.

Reference: src/toast/templates/subharmonic.py (pure NumPy, one detector and one view at a time).  The amplitude layout
is the reference's: detector-major; within a detector by observation, then by view, ``order + 1`` values per view.

Two paths.  The host path (``use_accel`` false) is NumPy with the reference's own expressions.  The device path
(``add_to_signal_multi`` / ``project_signal_multi``, what ``TemplateMatrix`` looks for, and ``_apply_precond`` on
resident vectors) runs the kernels of csrc/template_basis.hip, which evaluate the basis per sample and never store it.

Two properties of the reference are reproduced on both paths and matter to callers:

* ``project_signal`` applies NO flags and ASSIGNS the amplitudes instead of accumulating (subharmonic.py:205-218);
* the preconditioner is the inverse of ``detweight * sum_good T_r T_c`` with the detector flags applied (:157-179).

A (detector, view) without a single good sample makes the reference fail inside ``np.linalg.inv``; here both paths raise
``numpy.linalg.LinAlgError`` with the detector, observation and view in the message.
"""

import numpy as np

from ..accel import accel_device_ptr, device_scratch
from ..data import defaults
from ..traits import Int, Unicode
from . import release_borrowed
from .legendre import LegendreBlocks, legendre_basis  # noqa: F401  (legendre_basis: imported from here by its users)


class SubHarmonic(LegendreBlocks):
    """Noise fluctuations slower than the length of a view: ``order + 1`` Legendre amplitudes per detector and view."""

    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    order = Int(1, help="The filter order")
    noise_model = Unicode(None, allow_none=True, help="Observation key containing the optional noise model")

    _label = "SubHarmonic template"

    # ------------------------------------------------------------------ set-up
    def _initialize(self, new_data):
        from ..accel import accel_enabled

        self.clear()
        if self.order < 0:
            raise RuntimeError("SubHarmonic: the order must not be negative")
        if not self._layout_blocks(new_data):
            return
        # (set-up runs on the device for a template that will be swept there; the flags it reads are handed back)
        if accel_enabled() and self.supports_accel():
            gram, ngood = self._gram_device(new_data)
        else:
            gram, ngood = self._gram_host(new_data)
        self._invert(new_data, gram, ngood)

    def _gram_host(self, new_data):
        """subharmonic.py:157-178 for every block -> ([n_block][norder][norder], good samples per block)."""
        norder = self.order + 1
        gram = np.zeros_like(self._precond)
        ngood = np.zeros(gram.shape[0], dtype=np.int64)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            if len(dets) == 0:
                continue
            weights = self._det_weights(ob, dets)
            blocks = self._blocks(iob, dets)
            for ivw, vw in enumerate(ob.intervals[self.view]):
                templates = self._view_templates(iob, ob)[ivw]
                for det, detweight, blk in zip(dets, weights, blocks):
                    good = slice(0, templates.shape[1], 1)
                    n_good = templates.shape[1]
                    if self.det_flags is not None:
                        flags = ob.detdata[self.det_flags][det, vw.first:vw.last]
                        good = (flags & self.det_flag_mask) == 0
                        n_good = int(np.count_nonzero(good))
                    prec = gram[blk + ivw]
                    for row in range(norder):
                        for col in range(row, norder):
                            prec[row, col] = np.dot(templates[row][good], templates[col][good])
                            prec[row, col] *= detweight
                            if row != col:
                                prec[col, row] = prec[row, col]
                    ngood[blk + ivw] = n_good
        return gram, ngood

    def _gram_device(self, new_data):
        """The same sums by toast_hip_subharmonic_precond_build_dev: one call per observation."""
        from .. import capi

        norder = self.order + 1
        gram = np.zeros_like(self._precond)
        ngood = np.zeros(gram.shape[0], dtype=np.int64)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            n_view = self._obs_nview[iob]
            if len(dets) == 0 or n_view == 0:
                continue
            borrowed = []
            f_idx, f_ptr = self._det_flag_args(ob, dets, borrowed)
            try:
                with device_scratch(self.name) as s:
                    g = s.out("gram", np.zeros((len(dets), n_view, norder, norder), dtype=np.float64))
                    n = s.out("ngood", np.zeros((len(dets), n_view), dtype=np.int64))
                    capi.dev.subharmonic_precond_build(norder, f_idx, f_ptr, self.det_flag_mask, self._det_weights(ob, dets),
                                                       ob.n_local_samples, ob.intervals[self.view].data, s.ptr("gram"),
                                                       s.ptr("ngood"))
            finally:
                release_borrowed(borrowed)
            self._scatter_blocks(iob, dets, g, gram)
            self._scatter_blocks(iob, dets, n, ngood)
        return gram, ngood

    def _invert(self, new_data, gram, ngood):
        """subharmonic.py:179 for every block; a block without good samples has no inverse."""
        empty = np.flatnonzero(ngood == 0)
        if empty.size > 0:
            raise np.linalg.LinAlgError(f"SubHarmonic template {self.name}: {self._describe_block(new_data, int(empty[0]))} has "
                                        f"no unflagged sample ({empty.size} such blocks): its preconditioner is singular")
        self._invert_blocks(new_data, gram, lambda blk: f" ({int(ngood[blk])} unflagged samples)")

    # ------------------------------------------------------------------ Template interface
    def add_to_signal_multi(self, detectors, amplitudes, **kwargs):
        """All detectors and all views of an observation in one launch (device-resident buffers only)."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            capi.dev.subharmonic_add_to_signal(self.order + 1, self.det_amp_offsets(iob, dets),
                                               accel_device_ptr(amplitudes.buffer), dd.indices(dets),
                                               accel_device_ptr(dd.buffer), ob.n_local_samples, ob.intervals[self.view].data)

    def project_signal_multi(self, detectors, amplitudes, **kwargs):
        """No flags, and the amplitudes are assigned: see the module docstring."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            capi.dev.subharmonic_project_signal(self.order + 1, self.det_amp_offsets(iob, dets),
                                                accel_device_ptr(amplitudes.buffer), dd.indices(dets),
                                                accel_device_ptr(dd.buffer), ob.n_local_samples, ob.intervals[self.view].data)

    def _add_to_signal_host(self, detector, amplitudes):
        norder = self.order + 1
        offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            for ivw, vw in enumerate(ob.intervals[self.view]):
                templates = self._view_templates(iob, ob)[ivw]
                amp_view = local[offset:offset + norder]
                for order in range(norder):
                    row[vw.first:vw.last] += templates[order] * amp_view[order]
                offset += norder

    def _project_signal_host(self, detector, amplitudes):
        norder = self.order + 1
        offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            for ivw, vw in enumerate(ob.intervals[self.view]):
                amp_view = local[offset:offset + norder]
                for order, template in enumerate(self._view_templates(iob, ob)[ivw]):
                    amp_view[order] = np.dot(row[vw.first:vw.last], template)
                offset += norder
