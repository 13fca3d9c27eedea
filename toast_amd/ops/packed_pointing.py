"""The fused offset solver's launch context (``FusedContext`` / ``ObsPass``: the route of each sweep written once) and
its packed pointing cache (``PackedPointing`` / ``PackCache``: one frame that builds, keeps and gives back the packed copy
of an observation's pointing, ``packed_pointing.hip``).  Every device call and allocator query is looked up on ``capi``
when it is made."""

import os

import numpy as np

from .. import capi

# expanded pointing (32 B per detector-sample) that the on-the-fly fill holds at a time
PACK_EXPAND_BYTES = 4 << 30


def _switched_on(name):
    return os.environ.get(name, "1") != "0"


def room_for_pack(nbytes):
    """The packed cache is an extra: it is built only while at least a fifth of the device stays free afterwards (a
    data set of many observations keeps the on-the-fly / unpacked sweeps for those that do not fit)."""
    free, total = capi.accel_mem_info()
    return free - nbytes >= total // 5


class DeviceBlocks:
    """Raw device blocks that go back together."""

    def __init__(self):
        self.blocks = []

    def take(self, nbytes):
        ptr = capi.device_malloc(nbytes, -2)
        self.blocks.append((ptr, nbytes))
        return ptr

    def release(self):
        """Every block goes back, once: a released (or partially built) holder owns nothing."""
        while self.blocks:
            capi.device_release(*self.blocks.pop(0))     # (kept by the manager for the next solve's copy of the same size)


class PackedPointing(DeviceBlocks):
    """One observation's packed pointing on the device: ``key`` (local pixel offset and flag bits, one word per
    detector-sample, or per pair-sample with ``pair``), ``qu`` (the Q / U weights), ``cal`` (the intensity weight per
    detector), ``corr`` (the pair weight sums, or 0), and the device blocks behind them."""

    def __init__(self):
        super().__init__()
        self.key = self.qu = self.cal = self.corr = 0
        self.pair = False

    @property
    def bytes_per_sample(self):
        """Per detector-sample and sweep: 20, 18 (pair words) or 14 (+ pair weight sums)."""
        return 14 if self.corr else (18 if self.pair else 20)

    def add_pair_weights(self, n_det, n_samp, ivl):
        """With pair words: the partner's Q / U weights as float sums q_a + q_b, u_a + u_b when that is exact for every
        sample in view (orthogonal pairs of equal calibration and efficiency; toast_hip_offset_pack_pair_weights_dev) --
        14 instead of 18 B per detector-sample in both sweeps.  Anything else leaves the pack as it is."""
        if not self.pair or not _switched_on("TOAST_HIP_PACKED_PAIR_WEIGHTS"):
            return
        nbytes = max(8 * ((n_det + 1) // 2) * n_samp, 16)
        try:
            ptr = self.take(nbytes)
        except RuntimeError:
            return
        if capi.dev.offset_pack_pair_weights(self.qu, ptr, n_det, n_samp, ivl):
            self.corr = ptr
        else:
            capi.device_release(*self.blocks.pop())


class PackCache:
    """``iob -> (identity, PackedPointing)``: one packed copy per observation for the whole solve.  The launch plan is
    rebuilt when the amplitude vectors change (starting guess, then the proposal); the pointing behind it is the same --
    same arrays at the same device addresses, same flags and masks, same views."""

    def __init__(self):
        self.entries = {}

    def release(self):
        for _ident, pk in self.entries.values():
            pk.release()
        self.entries = {}

    def cached(self, c, ps, in_solve):
        """The packed copy of one observation's cached pointing (toast_hip_offset_pack_pointing_dev), or None when it
        cannot be had: switched off, rows of an odd length, an intensity weight that varies along a row, no memory."""
        if not self._wanted(c, ps, in_solve):
            return None
        ident = (tuple(ps.dets), int(ps.n_samp), c.g2l_ptr, c.nps, ps.pp, tuple(int(i) for i in ps.pi), ps.wp,
                 tuple(int(i) for i in ps.wi)) + self._flags_ident(c, ps)

        def fill(pk, corr):
            """One sweep over the arrays: with a block for the pair sums the one-sweep form, else pack + pair check."""
            args = (c.g2l_ptr, c.nps, ps.pi, ps.pp, ps.wi, ps.wp, ps.f_idx, ps.f_ptr, ps.f_ns, c.det_flag_mask, ps.s_ptr,
                    ps.s_n, c.shared_flag_mask, ps.pf_idx, ps.pf_ptr, ps.pf_n, c.tmpl_flag_mask, int(ps.n_samp), ps.ivl,
                    pk.key, pk.qu, pk.cal)
            if corr:
                return capi.dev.offset_pack_pointing_onepass(*args, corr)
            return capi.dev.offset_pack_pointing(*args) + (False,)

        return self._get(c, ps, ident, fill, pair_sums_need_room=False, redo_without_pair_words=False)

    def on_the_fly(self, c, ps, in_solve, source, descriptor, n_submap):
        """The packed cache of an observation whose pointing is NOT cached (full_pointing=False, packed_cache=True):
        pixels and weights of a batch of detectors are expanded from the boresight into a bounded temporary
        (toast_hip_otf_pixels_healpix_dev / _stokes_weights_dev), packed into the batch's rows, and the temporary goes to
        the next batch; co-pointing pairs are merged at the end.  ``source``: what identifies the pointing model,
        ``descriptor(dets)``: the on-the-fly pointing descriptor of a batch's detectors.  None as for ``cached``."""
        if not self._wanted(c, ps, in_solve):
            return None
        dets, n_det, n_samp = ps.dets, len(ps.dets), int(ps.n_samp)
        ident = ("otf", tuple(dets), n_samp, c.g2l_ptr, c.nps) + tuple(source) + self._flags_ident(c, ps)
        batch = max(2, int(PACK_EXPAND_BYTES // (32 * n_samp)) // 2 * 2)       # whole pairs
        batch = min(batch, n_det + (n_det & 1))

        def fill(pk, corr, pix_ptr, w_ptr, hsub_ptr):
            """Batch by batch: with a block for the pair sums the pair words and sums straight from each batch's expanded
            pointing (one sweep per batch; batches are whole pairs), else plain words per batch, then pair check and
            merge over all rows.  -> (ok, every batch in pair words, every batch's sums usable)"""
            D = capi.dev
            pairs, sums = True, True
            for b0 in range(0, n_det, batch):
                rows = np.arange(len(dets[b0:b0 + batch]), dtype=np.int32)
                pt = descriptor(dets[b0:b0 + batch])
                D.otf_pixels_healpix(pt, rows, pix_ptr, n_samp, ps.ivl, hsub_ptr, n_submap, c.nps)
                D.otf_stokes_weights(pt, rows, w_ptr, n_samp, ps.ivl)
                pf_idx = None if ps.pf_idx is None else ps.pf_idx[b0:b0 + batch]
                args = (c.g2l_ptr, c.nps, rows, pix_ptr, rows, w_ptr, ps.f_idx[b0:b0 + batch], ps.f_ptr, ps.f_ns,
                        c.det_flag_mask, ps.s_ptr, ps.s_n, c.shared_flag_mask, pf_idx, ps.pf_ptr, ps.pf_n,
                        c.tmpl_flag_mask, n_samp, ps.ivl, pk.key + 4 * b0 * n_samp, pk.qu + 16 * b0 * n_samp,
                        pk.cal + 8 * b0)
                if corr:
                    good, pair_b, sums_b = D.offset_pack_pointing_onepass(*args, corr + 8 * (b0 // 2) * n_samp)
                    pairs, sums = pairs and pair_b, sums and sums_b
                    if good and not pair_b:
                        return True, False, False
                else:
                    good, _ = D.offset_pack_pointing(*args, pair_words=False)
                if not good:
                    return False, False, False
            if corr:
                return True, pairs, sums
            return True, bool(D.offset_pack_pairs(pk.key, n_det, n_samp, ps.ivl)), False

        return self._get(c, ps, ident, fill, temps=(8 * batch * n_samp, 24 * batch * n_samp, max(int(n_submap), 16)),
                         temps_room=32 * batch * n_samp, pair_sums_need_room=True, redo_without_pair_words=True)

    @staticmethod
    def _wanted(c, ps, in_solve):
        """The guards of both paths.  ``in_solve``: the pack is a SNAPSHOT of pixels, weights and flags, keyed by their
        device addresses, so it lives inside a solve (solve() sets keep_on_device and gives the pack back in its finally
        block).  A stand-alone apply() sweeps the live arrays -- an in-place edit followed by accel_update_device keeps
        the address."""
        return (_switched_on("TOAST_HIP_PACKED_POINTING") and in_solve and c.nnz == 3 and int(ps.n_samp) % 2 == 0
                and len(ps.dets) > 0)

    @staticmethod
    def _flags_ident(c, ps):
        return (ps.f_ptr, ps.f_ns, c.det_flag_mask, ps.s_ptr, ps.s_n, c.shared_flag_mask, ps.pf_ptr, ps.pf_n,
                c.tmpl_flag_mask, np.ascontiguousarray(ps.ivl).tobytes())

    def _get(self, c, ps, ident, fill, temps=(), temps_room=0, *, pair_sums_need_room, redo_without_pair_words):
        """The frame both paths share.  ``fill(pack, corr, *temporaries) -> (ok, pair words, pair sums usable)`` writes
        the rows: with ``corr`` (the block for the pair sums) in the one-sweep form, with 0 in the separate form.  The
        two switches are where the two paths differ today (DESIGN.md lists them):
          pair_sums_need_room      the pair-sum block counts in the room check (on the fly), or not (cached)
          redo_without_pair_words  a one-sweep fill without pair words is redone here in the separate form and the pair
                                   weights are then tried separately (on the fly), or the C entry's own fall-back is
                                   trusted and nothing follows (cached)
        On both paths a one-sweep fill WITH pair words counts as used whatever it says about the sums: no separate
        pair weights follow it (``onepass`` below)."""
        n_det, n_samp = len(ps.dets), int(ps.n_samp)
        have = self.entries.get(ps.iob)
        if have is not None:
            if have[0] == ident:
                return have[1]
            del self.entries[ps.iob]
            have[1].release()
        need = 20 * n_det * n_samp + temps_room
        if not room_for_pack(need):
            return None
        pk, scratch = PackedPointing(), DeviceBlocks()
        try:
            pk.key, pk.qu, pk.cal = (pk.take(max(n, 16)) for n in (4 * n_det * n_samp, 16 * n_det * n_samp, 8 * n_det))
            temp_ptrs = [scratch.take(nbytes) for nbytes in temps]
        except RuntimeError:
            pk.release()
            scratch.release()
            return None
        # the pair weight sums are written by the same sweep (toast_hip_offset_pack_pointing_onepass_dev): their block
        # is taken first and given back when the pairs turn out not to qualify
        corr, corr_bytes = 0, max(8 * ((n_det + 1) // 2) * n_samp, 16)
        if (_switched_on("TOAST_HIP_PACKED_PAIR_WEIGHTS") and _switched_on("TOAST_HIP_PACK_ONEPASS")
                and (not pair_sums_need_room or room_for_pack(need + corr_bytes))):
            try:
                corr = pk.take(corr_bytes)
            except RuntimeError:
                corr = 0
        onepass = bool(corr)
        try:
            ok, pk.pair, sums = fill(pk, corr, *temp_ptrs)
            if onepass and ok and not pk.pair and redo_without_pair_words:
                onepass = False
                ok, pk.pair, sums = fill(pk, 0, *temp_ptrs)
        finally:
            scratch.release()
        if corr and not (ok and onepass and sums):
            capi.device_release(*pk.blocks.pop())
            corr = 0
        if not ok:
            pk.release()
            return None
        pk.corr = corr
        if not onepass:
            pk.add_pair_weights(n_det, n_samp, ps.ivl)
        self.entries[ps.iob] = (ident, pk)
        return pk


class _Record:
    """The fields named in ``__slots__``, by keyword; None where not given."""

    __slots__ = ()

    def __init__(self, **given):
        for name in self.__slots__:
            setattr(self, name, None)
        for name, value in given.items():
            setattr(self, name, value)      # (AttributeError for a name that is not a field)


class ObsPass(_Record):
    """One observation of the fused sweeps.  ``step``: baseline length in samples, ``ao`` / ``nav``: first amplitude per
    detector / amplitudes per view, ``detw``: detector weights; rows, device pointer and row length of the detector flags
    (``f_*``), the shared flags (``s_*``) and the template's solver flags (``pf_*``); the pointing as rows of the cached
    pixels and weights (``pi``, ``pp``, ``wi``, ``wp``) or as the on-the-fly descriptor ``pt``; ``pk``: its
    PackedPointing when the solve has one."""

    __slots__ = ("iob", "dets", "step", "ao", "nav", "n_samp", "ivl", "detw", "f_idx", "f_ptr", "f_ns", "s_ptr", "s_n",
                 "pf_idx", "pf_ptr", "pf_n", "pi", "pp", "wi", "wp", "pt", "pk")

    @property
    def route(self):
        """Which sweeps: "packed" (the solver's packed pointing cache), "fused" (the cached pixels / weights as they
        are) or "fused-otf" (pointing evaluated in the kernels)"""
        return "packed" if self.pk is not None else ("fused" if self.pt is None else "fused-otf")


class FusedContext(_Record):
    """The launch context of one solve: raw device pointers (valid for one generation of the memory manager), masks
    and sizes, and one ``ObsPass`` per observation in ``passes``."""

    __slots__ = ("on_the_fly", "nnz", "nps", "n_local", "zmap", "amps_in", "amps_out", "zmap_ptr", "zmap_bytes", "cov_ptr",
                 "g2l_ptr", "in_ptr", "in_flags_ptr", "out_ptr", "out_bytes", "det_flag_mask", "shared_flag_mask",
                 "tmpl_flag_mask", "owner_computes", "prior", "passes")

    def accumulate(self, ps):
        """zmap += A^T N^-1 M a  over one observation"""
        D, pk = capi.dev, ps.pk
        if pk is not None:
            D.offset_accumulate_packed(ps.step, ps.ao, ps.nav, self.in_ptr, self.in_flags_ptr, self.zmap_ptr, pk.key, pk.qu,
                                       pk.cal, ps.detw, ps.n_samp, ps.ivl, pair_words=pk.pair, pair_corr=pk.corr)
        elif ps.pt is not None:
            D.otf_offset_accumulate(ps.pt, ps.step, ps.ao, ps.nav, self.in_ptr, self.in_flags_ptr, self.g2l_ptr,
                                    self.zmap_ptr, self.nps, ps.f_idx, ps.f_ptr, ps.f_ns, ps.detw, self.det_flag_mask,
                                    ps.n_samp, ps.ivl, ps.s_ptr, ps.s_n, self.shared_flag_mask)
        else:
            D.offset_accumulate(ps.step, ps.ao, ps.nav, self.in_ptr, self.in_flags_ptr, self.g2l_ptr, self.zmap_ptr,
                                self.nps, self.nnz, ps.pi, ps.pp, ps.wi, ps.wp, ps.f_idx, ps.f_ptr, ps.f_ns, ps.detw,
                                self.det_flag_mask, ps.n_samp, ps.ivl, ps.s_ptr, ps.s_n, self.shared_flag_mask)

    def scan_project(self, ps):
        """a_out += M^T N^-1 (M a - A zmap)  over one observation"""
        D, pk = capi.dev, ps.pk
        if pk is not None:
            D.offset_scan_project_packed(ps.step, ps.ao, ps.nav, self.in_ptr, self.out_ptr, self.in_flags_ptr,
                                         self.zmap_ptr, pk.key, pk.qu, pk.cal, ps.detw, ps.n_samp, ps.ivl,
                                         pair_words=pk.pair, pair_corr=pk.corr)
        elif ps.pt is not None:
            D.otf_offset_scan_project(ps.pt, ps.step, ps.ao, ps.nav, self.in_ptr, self.out_ptr, self.in_flags_ptr,
                                      self.g2l_ptr, self.zmap_ptr, self.nps, ps.pf_idx, ps.pf_ptr, ps.pf_n,
                                      self.tmpl_flag_mask, ps.detw, ps.n_samp, ps.ivl)
        else:
            D.offset_scan_project(ps.step, ps.ao, ps.nav, self.in_ptr, self.out_ptr, self.in_flags_ptr, self.g2l_ptr,
                                  self.zmap_ptr, self.nps, self.nnz, ps.pi, ps.pp, ps.wi, ps.wp, ps.pf_idx, ps.pf_ptr,
                                  self.tmpl_flag_mask, ps.detw, ps.n_samp, ps.ivl)

    def scan_project_signal(self, ps, sig_idx, sig_ptr):
        """a_out += M^T N^-1 (d - A zmap)  over one observation, d the rows ``sig_idx`` at ``sig_ptr`` (the right-hand
        side: it never sweeps a packed copy)"""
        D = capi.dev
        if ps.pt is not None:
            D.otf_offset_scan_project_signal(ps.pt, ps.step, ps.ao, ps.nav, sig_idx, sig_ptr, self.out_ptr,
                                             self.in_flags_ptr, self.g2l_ptr, self.zmap_ptr, self.nps, ps.pf_idx,
                                             ps.pf_ptr, ps.pf_n, self.tmpl_flag_mask, ps.detw, ps.n_samp, ps.ivl)
        else:
            D.offset_scan_project_signal(ps.step, ps.ao, ps.nav, sig_idx, sig_ptr, self.out_ptr, self.in_flags_ptr,
                                         self.g2l_ptr, self.zmap_ptr, self.nps, self.nnz, ps.pi, ps.pp, ps.wi, ps.wp,
                                         ps.pf_idx, ps.pf_ptr, self.tmpl_flag_mask, ps.detw, ps.n_samp, ps.ivl)
