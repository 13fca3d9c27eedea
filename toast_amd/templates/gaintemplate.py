"""GainTemplate: slow gain fluctuations of a detector, solved with the map.

Reference: src/toast/templates/gaintemplate.py (pure NumPy, one detector and one view at a time).  The model is a Legendre
series in time multiplied by a per-detector *signal estimate* timestream (the detdata key ``template_name``):
``signal += estimate * (L @ a)``.  The amplitude layout is the reference's, and SubHarmonic's: detector-major; within a
detector by observation, then by view, ``order + 1`` values per view.  No amplitude flags, no prior.

Two paths.  The host path is NumPy.  The device path (``add_to_signal_multi`` / ``project_signal_multi``, what
``TemplateMatrix`` looks for, ``_apply_precond`` on resident vectors, and the Gram matrices at set-up when the accelerator
is on) runs the Legendre sweeps of csrc/template_basis.hip, which evaluate the basis per sample and never store it.

What the reference does, reproduced on both paths -- each the opposite of SubHarmonic:

* ``project_signal`` ACCUMULATES onto the amplitudes and APPLIES ``det_flags & det_flag_mask`` (gaintemplate.py:199-220);
* ``add_to_signal`` applies no flags (:182-197);
* the preconditioner is the inverse of ``detweight * sum_i L_r L_c estimate_i^2`` over ALL samples of the view: the
  reference computes ``good`` there and never uses it (:159-171).

Where this template deviates from the reference, on purpose:

* The basis.  The reference evaluates ``scipy.special.legendre(k)`` as monomials; here ``legendre_basis()`` and the device
  evaluate the three-term recurrence, like SubHarmonic.  The two agree bit for bit up to order 1 and differ by up to
  7e-15 absolute at order 8, so from order 2 on nothing can be bit-identical to the reference; the tests bound it.
* More than one observation, and views.  The reference multiplies a view-length basis by the whole-observation estimate
  row (it raises for any view but the whole observation), and its two sweeps never advance the amplitude offset past the
  detector's first block, so with two observations both use the first block -- while its own layout and
  ``_apply_precond`` do advance.  Here the estimate is sliced to the view and the offset advances by ``order + 1`` per view
  and per observation in every method: the reference's layout, consistently.  The two agree for one observation and
  ``view=None``, which the fixture pins; the rest is pinned to exact sums by the tests.
* A (detector, observation, view) whose Gram matrix has no inverse (an estimate that is identically zero, fewer samples
  than terms) fails inside ``np.linalg.inv`` in the reference; here both paths raise ``numpy.linalg.LinAlgError`` naming
  the detector, observation and view.
* The detector weight multiplies the finished sums; the reference scales the rows by its square root before the product.

``order + 1`` may be at most ``toast_hip_subharmonic_max_terms()`` on the device; above it ``supports_accel()`` answers no
and the host path runs.
"""

import numpy as np

from ..accel import accel_device_ptr, device_scratch
from ..traits import Int, Unicode
from . import make_resident, release_borrowed
from .legendre import LegendreBlocks


class GainTemplate(LegendreBlocks):
    """Gain drifts: ``order + 1`` Legendre amplitudes per detector and view, multiplying the signal estimate."""

    order = Int(1, help="The order of Legendre polynomials to fit the gain amplitudes")
    template_name = Unicode(None, allow_none=True, help="detdata key encoding the signal estimate to fit the gain amplitudes")
    noise_model = Unicode(None, allow_none=True, help="Observation key containing the noise model")

    _label = "GainTemplate"

    def __init__(self, **kwargs):
        self._borrowed = []      # estimates the sweeps uploaded, and those of them they had to register
        self._created = []
        super().__init__(**kwargs)

    # ------------------------------------------------------------------ set-up
    def _initialize(self, new_data):
        from ..accel import accel_enabled

        self.clear()
        if self.order < 0:
            raise RuntimeError("GainTemplate: the order must not be negative")
        if self.template_name is None:
            raise RuntimeError(f"GainTemplate {self.name}: template_name (the detdata key of the signal estimate) is not set")
        for ob in new_data.obs:
            if self.template_name not in ob.detdata:
                raise RuntimeError(f"GainTemplate {self.name}: observation {ob.name} has no detdata '{self.template_name}' "
                                   f"(the signal estimate)")
            self._check_float64(ob, self.template_name)
            if self.det_data in ob.detdata:
                self._check_float64(ob, self.det_data)
        if not self._layout_blocks(new_data, also_in=(self.template_name,)):
            return
        if accel_enabled() and self.supports_accel():
            gram = self._gram_device(new_data)
        else:
            gram = self._gram_host(new_data)
        self._invert(new_data, gram)

    def _check_float64(self, ob, key):
        if ob.detdata[key].buffer.dtype != np.float64:
            raise RuntimeError(f"GainTemplate {self.name}: detdata '{key}' of observation {ob.name} must be float64, "
                               f"it is {ob.detdata[key].buffer.dtype}")

    def _gram_host(self, new_data):
        """gaintemplate.py:159-170 for every block, the estimate sliced to the view -> [n_block][norder][norder]."""
        gram = np.zeros_like(self._precond)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            if len(dets) == 0:
                continue
            weights = self._det_weights(ob, dets)
            blocks = self._blocks(iob, dets)
            est = ob.detdata[self.template_name]
            for ivw, vw in enumerate(ob.intervals[self.view]):
                templates = self._view_templates(iob, ob)[ivw]
                for det, detweight, blk in zip(dets, weights, blocks):
                    lt = templates * est[det, vw.first:vw.last]
                    gram[blk + ivw] = lt.dot(lt.T) * detweight
        return gram

    def _gram_device(self, new_data):
        """The same sums by toast_hip_gain_precond_build_dev: one call per observation."""
        from .. import capi

        norder = self.order + 1
        gram = np.zeros_like(self._precond)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            n_view = self._obs_nview[iob]
            if len(dets) == 0 or n_view == 0:
                continue
            borrowed = []
            try:
                est = self._resident_estimate(ob, borrowed)
                with device_scratch(self.name) as s:
                    g = s.out("gram", np.zeros((len(dets), n_view, norder, norder), dtype=np.float64))
                    capi.dev.gain_precond_build(norder, est.indices(dets), accel_device_ptr(est.buffer),
                                                self._det_weights(ob, dets), ob.n_local_samples,
                                                ob.intervals[self.view].data, s.ptr("gram"))
            finally:
                release_borrowed(borrowed)
            self._scatter_blocks(iob, dets, g, gram)
        return gram

    def _block_samples(self, new_data):
        """Number of samples of every block's view, in amplitude order."""
        n = np.zeros(self._precond.shape[0], dtype=np.int64)
        for iob, ob in enumerate(new_data.obs):
            dets = [d for d in self._all_dets if d in self._obs_dets[iob]]
            lens = np.array([int(vw.last - vw.first) for vw in ob.intervals[self.view]], dtype=np.int64)
            for blk in (self._blocks(iob, dets) if len(dets) > 0 else ()):
                n[blk:blk + lens.size] = lens
        return n

    def _invert(self, new_data, gram):
        """gaintemplate.py:171 for every block; a block with fewer samples than terms or a zero estimate has no inverse."""
        norder = self.order + 1
        n_samp = self._block_samples(new_data)
        short = np.flatnonzero(n_samp < norder)
        if short.size > 0:
            blk = int(short[0])
            raise np.linalg.LinAlgError(f"GainTemplate {self.name}: {self._describe_block(new_data, blk)} has "
                                        f"{int(n_samp[blk])} samples for {norder} terms ({short.size} such blocks): its "
                                        f"preconditioner is singular")
        null = np.flatnonzero(~np.any(gram.reshape(gram.shape[0], -1) != 0, axis=1))
        if null.size > 0:
            raise np.linalg.LinAlgError(f"GainTemplate {self.name}: {self._describe_block(new_data, int(null[0]))} has a "
                                        f"signal estimate that is zero everywhere ({null.size} such blocks): its "
                                        f"preconditioner is singular")
        self._invert_blocks(new_data, gram)

    # ------------------------------------------------------------------ Template interface
    def _estimate_args(self, ob, dets):
        """(rows of ``dets`` in the estimate, its device pointer); resident from the first sweep until ``clear()``."""
        est = self._resident_estimate(ob, self._borrowed)
        return est.indices(dets), accel_device_ptr(est.buffer)

    def _resident_estimate(self, ob, borrowed):
        est = ob.detdata[self.template_name]
        if not est.accel_in_use() and not est.accel_exists() and est.buffer.size > 0:
            self._created.append(est)       # (nobody else asked for a device copy: ``clear()`` frees it)
        return make_resident(est, self.template_name, borrowed)

    def add_to_signal_multi(self, detectors, amplitudes, **kwargs):
        """All detectors and all views of an observation in one launch (device-resident buffers only)."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            e_idx, e_ptr = self._estimate_args(ob, dets)
            capi.dev.gain_add_to_signal(self.order + 1, self.det_amp_offsets(iob, dets), accel_device_ptr(amplitudes.buffer),
                                        dd.indices(dets), accel_device_ptr(dd.buffer), e_idx, e_ptr, ob.n_local_samples,
                                        ob.intervals[self.view].data)

    def project_signal_multi(self, detectors, amplitudes, **kwargs):
        """With the solver flags, onto the amplitudes already there: see the module docstring."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            e_idx, e_ptr = self._estimate_args(ob, dets)
            f_idx, f_ptr = self._det_flag_args(ob, dets)
            capi.dev.gain_project_signal(self.order + 1, self.det_amp_offsets(iob, dets), accel_device_ptr(amplitudes.buffer),
                                         dd.indices(dets), accel_device_ptr(dd.buffer), e_idx, e_ptr, f_idx, f_ptr,
                                         self.det_flag_mask, ob.n_local_samples, ob.intervals[self.view].data)

    def _add_to_signal_host(self, detector, amplitudes):
        """gaintemplate.py:182-197 with an explicit ascending-k sum: the statement of k_legendre_add, bit for bit."""
        norder = self.order + 1
        offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            est = ob.detdata[self.template_name][detector]
            for ivw, vw in enumerate(ob.intervals[self.view]):
                templates = self._view_templates(iob, ob)[ivw]
                amp_view = local[offset:offset + norder]
                delta_gain = np.zeros(templates.shape[1], dtype=np.float64)
                for order in range(norder):
                    delta_gain += templates[order] * amp_view[order]
                row[vw.first:vw.last] += est[vw.first:vw.last] * delta_gain
                offset += norder

    def _project_signal_host(self, detector, amplitudes):
        """gaintemplate.py:199-220."""
        norder = self.order + 1
        offset = self._det_start[detector]
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            est = ob.detdata[self.template_name][detector]
            for ivw, vw in enumerate(ob.intervals[self.view]):
                mask = 1
                if self.det_flags is not None:
                    mask = (ob.detdata[self.det_flags][detector, vw.first:vw.last] & self.det_flag_mask) == 0
                lt = self._view_templates(iob, ob)[ivw] * est[vw.first:vw.last]
                local[offset:offset + norder] += np.dot(lt, row[vw.first:vw.last] * mask)
                offset += norder

    def clear(self):
        """Release the device copy of the preconditioner, hand back what the sweeps made resident, drop the host basis."""
        super().clear()
        release_borrowed(self._borrowed)
        for est in self._created:
            if est.accel_exists():
                est.accel_delete()          # (only read: the host copy is the current one)
        self._created = []
