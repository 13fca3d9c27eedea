"""What the two Legendre-series templates share: SubHarmonic (templates/subharmonic.py) and GainTemplate
(templates/gaintemplate.py) both solve ``order + 1`` Legendre amplitudes per detector and view, in the same layout --
detector-major; within a detector by observation, then by view -- with a dense ``norder x norder`` preconditioner block
per (detector, observation, view), and both run the Legendre sweeps of csrc/template_basis.hip on the device.

The subclasses keep what is theirs: traits, what makes a block singular, their Gram sums and their sweeps.
"""

import numpy as np

from ..accel import accel_device_ptr
from . import Amplitudes, DeviceMirror, Template


def legendre_basis(norder, view_len):
    """[norder][view_len] templates of one view: subharmonic.py:143-155, the same array expressions."""
    templates = np.zeros((norder, view_len), dtype=np.float64)
    r = np.linspace(-1.0, 1.0, view_len)
    for order in range(norder):
        if order == 0:
            templates[order] = 1.0
        elif order == 1:
            templates[order] = r
        else:
            templates[order] = ((2 * order - 1) * r * templates[order - 1] - (order - 1) * templates[order - 2]) / order
    return templates


class LegendreBlocks(Template):
    """``order + 1`` Legendre amplitudes per detector and view.  A subclass has an ``order`` trait and sets ``_label``,
    the start of its error messages."""

    _label = None

    # inverse of the weighted Gram matrix of every (detector, observation, view) block, in amplitude order
    _precond = property(lambda self: self._mirrors["precond"].host)

    def __init__(self, **kwargs):
        self._templates = {}
        super().__init__(**kwargs)

    # ------------------------------------------------------------------ set-up
    def _layout_blocks(self, new_data, also_in=()):
        """The detectors, the amplitude layout and a zeroed preconditioner; False when nothing is local."""
        norder = self.order + 1
        all_dets = {}
        self._obs_dets = {}
        for iob, ob in enumerate(new_data.obs):
            dets = self._obs_detectors(ob, also_in=also_in)
            self._obs_dets[iob] = set(dets)
            all_dets.update(dict.fromkeys(dets))
        self._all_dets = list(all_dets.keys())
        self._obs_nview = {iob: len(ob.intervals[self.view]) for iob, ob in enumerate(new_data.obs)}
        self._layout_detector_major(new_data.comm, {iob: n * norder for iob, n in self._obs_nview.items()})
        self._templates = {}
        self._mirrors["precond"] = DeviceMirror(np.zeros((self._n_local // norder, norder, norder), dtype=np.float64),
                                                f"{self.name}_precond")
        return self._n_local > 0

    @staticmethod
    def _max_terms():
        from .. import capi

        return capi.dev.subharmonic_max_terms()

    def _view_templates(self, iob, ob):
        """The basis of every view of one observation, built on first use by the host path."""
        if iob not in self._templates:
            self._templates[iob] = [legendre_basis(self.order + 1, int(vw.last - vw.first)) for vw in ob.intervals[self.view]]
        return self._templates[iob]

    def _blocks(self, iob, dets):
        """First block (amplitude index / norder) of each detector for observation ``iob``."""
        return self.det_amp_offsets(iob, dets) // (self.order + 1)

    def _scatter_blocks(self, iob, dets, result, out):
        """``result[detector of dets][view]...`` of observation ``iob`` into ``out[block]...``."""
        n_view = self._obs_nview[iob]
        for k, blk in enumerate(self._blocks(iob, dets)):
            out[blk:blk + n_view] = result[k]

    def _invert_blocks(self, new_data, gram, detail=lambda blk: ""):
        """The preconditioner is the inverse of every block of ``gram``; a block without one is named, with ``detail(blk)``
        after the message."""
        try:
            self._precond[:] = np.linalg.inv(gram)
        except np.linalg.LinAlgError:
            for blk in range(gram.shape[0]):
                try:
                    np.linalg.inv(gram[blk])
                except np.linalg.LinAlgError as err:
                    raise np.linalg.LinAlgError(f"{self._label} {self.name}: {self._describe_block(new_data, blk)} has a "
                                                f"singular preconditioner{detail(blk)}") from err
            raise
        if not np.all(np.isfinite(self._precond)):
            bad = int(np.flatnonzero(~np.isfinite(self._precond).all(axis=(1, 2)))[0])
            raise np.linalg.LinAlgError(f"{self._label} {self.name}: {self._describe_block(new_data, bad)} has a "
                                        f"preconditioner that is not finite")

    def _describe_block(self, new_data, blk):
        norder = self.order + 1
        for det in self._all_dets:
            off = self._det_start[det] // norder
            for iob, ob in enumerate(new_data.obs):
                if det not in self._obs_dets[iob]:
                    continue
                if blk < off + self._obs_nview[iob]:
                    return f"detector {det}, observation {ob.name}, view {blk - off}"
                off += self._obs_nview[iob]
        return f"block {blk}"

    # ------------------------------------------------------------------ Template interface
    def _detectors(self):
        return self._all_dets

    def _zeros(self):
        # no explicit flagging of amplitudes in these templates (subharmonic.py:184-188, gaintemplate.py:176-180)
        return Amplitudes(self.data.comm, self._n_global, self._n_local)

    def _supports_accel(self):
        return self.order + 1 <= self._max_terms()

    def _add_prior(self, amplitudes_in, amplitudes_out, **kwargs):
        return      # no prior for these templates (subharmonic.py:220-222, gaintemplate.py:222-224)

    def _apply_precond(self, amplitudes_in, amplitudes_out, use_accel=None, **kwargs):
        if self._n_local == 0:
            return
        norder = self.order + 1
        if amplitudes_in.accel_in_use() or amplitudes_out.accel_in_use():
            from .. import capi

            amplitudes_in.accel_resident()
            amplitudes_out.accel_resident()
            capi.dev.subharmonic_apply_precond(norder, self._n_local // norder, self._mirrors["precond"].upload().ptr,
                                               accel_device_ptr(amplitudes_in.buffer), accel_device_ptr(amplitudes_out.buffer))
            return
        # subharmonic.py:224-236, gaintemplate.py:226-238: one small dense product per block
        a_in = amplitudes_in.local.reshape(-1, norder)
        amplitudes_out.local.reshape(-1, norder)[:] = np.einsum("brc,bc->br", self._precond, a_in)

    def clear(self):
        """Release the device copy of the preconditioner and the host basis."""
        super().clear()
        self._templates = {}
