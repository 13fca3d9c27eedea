"""Template regression: TemplateMatrix, SolverRHS, SolverLHS and the PCG ``solve`` loop.

Reference: src/toast/ops/mapmaker_templates.py:32-420 (TemplateMatrix),
src/toast/ops/mapmaker_solve.py:27-229 (SolverRHS), :232-521 (SolverLHS), :524-755 (solve).

    RHS:  b  = M^T N^-1 Z d          LHS:  a' = M^T N^-1 Z M a (+ prior)
    Z = I - P (P^T N^-1 P)^-1 P^T N^-1
"""

import numpy as np

from .. import capi
from ..accel import accel_data_create, accel_data_delete, accel_device_ptr, accel_enabled, make_resident, native
from ..data import defaults
from ..pixels import PixelData
from ..templates import AmplitudesMap, Offset
from ..traits import Bool, ImplementationType, Instance, Int, List, Unicode
from .mapmaker_ops import Copy, Delete, NoiseWeight, ScanMap, device_det_flags, device_g2l, device_shared_flags
from .operator import Operator
from .packed_pointing import FusedContext, ObsPass, PackCache
from .pipeline import Pipeline, uncached_detector_sets
from .pointing import compact_pixel_cache, otf_descriptor, otf_supported


class TemplateMatrix(Operator):
    """Projects amplitudes to timestreams (``transpose=False``: tod = M a, after zeroing) or
    accumulates timestreams into amplitudes (``transpose=True``: a += M^T tod)."""

    API = Int(0, help="Internal interface version for this operator")
    templates = List([], help="This should be a list of Template-derived objects")
    amplitudes = Unicode(None, allow_none=True, help="Data key for template amplitudes")
    transpose = Bool(False, help="If True, apply the transpose.")
    accumulate = Bool(False, help="transpose=False: add M a to the existing timestreams instead of zeroing them first "
                      "(not a reference trait; lets ApplyAmplitudes work without a second timestream buffer)")
    view = Unicode(None, allow_none=True, help="Use this view of the data in all observations")
    det_data = Unicode(None, allow_none=True, help="Observation detdata key for the timestream data")
    det_data_units = Unicode(defaults.det_data_units, allow_none=True, help="Desired units of detector data")
    det_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for per-detector flagging")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for solver flags to use")
    det_flag_mask = Int(defaults.det_mask_nonscience, help="Bit mask value for solver flags")

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._initialized = False

    def duplicate(self):
        """Same templates, independent traits (mapmaker_templates.py:181-196)."""
        ret = TemplateMatrix(API=self.API, templates=list(self.templates), amplitudes=self.amplitudes,
                             transpose=self.transpose, view=self.view, det_data=self.det_data,
                             det_data_units=self.det_data_units, det_mask=self.det_mask, det_flags=self.det_flags,
                             det_flag_mask=self.det_flag_mask)
        ret._initialized = self._initialized
        return ret

    def reset(self):
        self._initialized = False
        for tmpl in self.templates:
            if hasattr(tmpl, "clear"):
                tmpl.clear()

    def reset_templates(self):
        self.reset()

    def initialize(self, data):
        if not self._initialized:
            for tmpl in self.templates:
                tmpl.view = self.view
                tmpl.det_data_units = self.det_data_units
                tmpl.det_mask = self.det_mask
                tmpl.det_flags = self.det_flags
                tmpl.det_flag_mask = self.det_flag_mask
                # the data trait triggers template initialisation
                tmpl.det_data = self.det_data
                tmpl.data = data
            self._initialized = True

    def apply_precond(self, amps_in, amps_out, use_accel=None, **kwargs):
        if not self._initialized:
            raise RuntimeError("You must call exec() once before applying preconditioners")
        for tmpl in self.templates:
            if tmpl.enabled:
                tmpl.apply_precond(amps_in[tmpl.name], amps_out[tmpl.name], use_accel=use_accel, **kwargs)

    def add_prior(self, amps_in, amps_out, use_accel=None, **kwargs):
        if not self._initialized:
            raise RuntimeError("You must call exec() once before adding the prior")
        for tmpl in self.templates:
            if tmpl.enabled:
                tmpl.add_prior(amps_in[tmpl.name], amps_out[tmpl.name], use_accel=use_accel, **kwargs)

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        implementation, use_accel = self.select_kernels(use_accel=use_accel)
        if self.det_data is None:
            raise RuntimeError("You must set the det_data trait before calling exec()")
        if self.amplitudes is None:
            raise RuntimeError("You must set the amplitudes trait before calling exec()")
        if len(self.templates) == 0:
            raise RuntimeError("No templates in use")
        for tmpl in self.templates:
            tmpl.det_data = self.det_data
        self.initialize(data)
        all_dets = data.all_local_detectors(selection=detectors, flagmask=self.det_mask)
        if self.transpose:
            if self.amplitudes not in data:
                data[self.amplitudes] = AmplitudesMap()
                for tmpl in self.templates:
                    if tmpl.enabled:
                        data[self.amplitudes][tmpl.name] = tmpl.zeros()
            for tmpl in self.templates:
                if not tmpl.enabled:
                    continue
                if use_accel and hasattr(tmpl, "project_signal_multi"):
                    tmpl.project_signal_multi(all_dets, data[self.amplitudes][tmpl.name], **kwargs)
                else:
                    for d in all_dets:
                        tmpl.project_signal(d, data[self.amplitudes][tmpl.name], use_accel=use_accel, **kwargs)
        else:
            if self.amplitudes not in data:
                raise RuntimeError(f"Template amplitudes '{self.amplitudes}' do not exist in data")
            for ob in data.obs:
                dets = ob.select_local_detectors(selection=detectors, flagmask=self.det_mask)
                exists = ob.detdata.ensure(self.det_data, detectors=dets, accel=use_accel,
                                           create_units=self.det_data_units)
                if exists and not self.accumulate:
                    ob.detdata[self.det_data].reset(dets=dets)
            for tmpl in self.templates:
                if not tmpl.enabled:
                    continue
                if use_accel and hasattr(tmpl, "add_to_signal_multi"):
                    tmpl.add_to_signal_multi(all_dets, data[self.amplitudes][tmpl.name], **kwargs)
                else:
                    for d in all_dets:
                        tmpl.add_to_signal(d, data[self.amplitudes][tmpl.name], use_accel=use_accel, **kwargs)

    def _finalize(self, data, use_accel=None, **kwargs):
        if self.transpose and self.amplitudes in data:
            # make the accumulated amplitudes current on the host for the PCG algebra -- unless the host side is brought up
            # to date on access anyway (Data.lazy_host; Amplitudes.local): the solver's algebra runs on the device
            if not getattr(data, "lazy_host", False):
                data[self.amplitudes].accel_update_host()
            for v in data[self.amplitudes].values():
                v.sync()

    def _requires(self):
        req = {"global": [], "meta": [], "shared": [], "detdata": [], "intervals": []}
        if self.view is not None:
            req["intervals"].append(self.view)
        if self.transpose:
            req["detdata"].append(self.det_data)
            if self.det_flags is not None:
                req["detdata"].append(self.det_flags)
        else:
            req["global"].append(self.amplitudes)
            if self.accumulate:
                req["detdata"].append(self.det_data)   # added to, not overwritten
        return req

    def _provides(self):
        prov = {"global": [], "detdata": []}
        if self.transpose:
            prov["global"].append(self.amplitudes)
        else:
            prov["detdata"].append(self.det_data)
        return prov

    def _implementations(self):
        return [ImplementationType.DEFAULT, ImplementationType.COMPILED]

    def _supports_accel(self):
        return all(t.supports_accel() for t in self.templates)


def _sequence_pipe(binning, det_data, units, first, last):
    """The tail of both sides as the reference's operators on the timestream ``det_data``: ``first``, [the pointing when
    it is not cached,] subtract the scanned binned map, noise-weight, ``last``."""
    pixels, weights = binning.pixel_pointing, binning.stokes_weights
    scan_map = ScanMap(pixels=pixels.pixels, weights=weights.weights, view=pixels.view, map_key=binning.binned,
                       det_data=det_data, det_data_units=units, det_mask=binning.det_mask,
                       det_flag_mask=binning.det_flag_mask, subtract=True)
    noise_weight = NoiseWeight(noise_model=binning.noise_model, det_data=det_data, det_mask=binning.det_mask,
                               det_flag_mask=binning.det_flag_mask, view=pixels.view)
    if binning.full_pointing:
        return Pipeline(detector_sets=["ALL"], operators=[first, scan_map, noise_weight, last])
    return Pipeline(detector_sets=uncached_detector_sets(),
                    operators=[first, pixels, weights, scan_map, noise_weight, last])


def collect_stable(collect, error):
    """``collect()`` gathers raw device pointers.  An allocation made meanwhile can fail and trigger the eviction handler
    (Data.accel_evict), which may free a buffer whose pointer was already taken.  Every create / delete bumps the memory
    manager's generation, so: collect again until one whole pass ran without any (the second pass normally finds
    everything resident and allocates nothing)."""
    for _attempt in range(4):
        gen0 = capi.accel_generation()
        out = collect()
        if capi.accel_generation() == gen0:
            return out
    raise RuntimeError(error)


def can_fuse(binning, template_matrix):
    """Whether the fused offset kernels can stand in for the operator sequence of this binning and these templates."""
    if not accel_enabled():
        return False
    if capi.get_deterministic():
        # debug mode: only build_noise_weighted has an order-deterministic form (deterministic.hip)
        return False
    if not binning.full_pointing:
        # uncached pointing: only through the on-the-fly kernels
        if not (getattr(binning, "on_the_fly", False)
                and otf_supported(binning.pixel_pointing, binning.stokes_weights)):
            return False
    tmpls = [t for t in template_matrix.templates if t.enabled]
    if len(tmpls) != 1 or not isinstance(tmpls[0], Offset):
        return False
    if tmpls[0].use_noise_prior and binning.pixel_pointing.view is not None:
        # with a noise prior the baselines ignore the view (offset.py:135-140); the fused
        # kernels take the baseline boundaries from the pointing view
        return False
    if binning.stokes_weights.mode not in ("I", "IQU"):
        return False
    return True


def fused_prepare(binning, tm, out, data, detectors, cache=None, in_solve=False):
    """Everything of the fused sweeps that is not a kernel launch: residency of the operands, device pointers,
    per-observation index arrays.  ``out``: the Data key of the output amplitudes; ``cache``: the PackCache that may hold
    packed copies of the pointing (``in_solve``: a solve is running, the only time it does).  Returns the FusedContext."""
    pixels_op, weights_op = binning.pixel_pointing, binning.stokes_weights
    tmpl = [t for t in tm.templates if t.enabled][0]
    amps_in = data[tm.amplitudes][tmpl.name]
    amps_out = data[out][tmpl.name]
    # full_pointing: cached pointing, resident on the device (computed once, reused by every
    # iteration); otherwise the kernels evaluate the pointing on the fly from the boresight
    pixels_op.detector_pointing.det_mask = binning.det_mask
    on_the_fly = not binning.full_pointing
    if not on_the_fly:
        cached = True
        for ob in data.obs:
            dets = ob.select_local_detectors(detectors, flagmask=binning.det_mask)
            for key in (pixels_op.pixels, weights_op.weights):
                if key not in ob.detdata or not set(dets) <= set(ob.detdata[key].detectors):
                    cached = False
        if cached:
            # do not drag the detector quaternions (4x the pixel volume) to the device again
            for ob in data.obs:
                make_resident(ob.detdata[pixels_op.pixels], pixels_op.pixels)
                make_resident(ob.detdata[weights_op.weights], weights_op.weights)
        else:
            pixels_op.apply(data, detectors=detectors, use_accel=True)
            weights_op.apply(data, detectors=detectors, use_accel=True)
    dist = data[binning.pixel_dist]
    nnz = len(weights_op.mode)
    if binning.binned not in data:
        data[binning.binned] = PixelData(dist, np.float64, n_value=nnz)
    zmap = data[binning.binned]
    if not zmap.accel_exists():
        zmap.accel_create(binning.binned, zero_out=True)
    cov = make_resident(data[binning.covariance], binning.covariance)
    g2l = device_g2l(data, binning.pixel_dist, dist)
    make_resident(amps_in, f"{tmpl.name}_in")
    if not amps_out.accel_exists():
        amps_out.accel_create(f"{tmpl.name}_out", zero_out=True)
    world = dist._world()
    ctx = FusedContext(
        on_the_fly=on_the_fly, nnz=nnz, nps=dist.n_pix_submap, n_local=dist.n_local_submap, zmap=zmap, amps_in=amps_in,
        amps_out=amps_out, zmap_ptr=accel_device_ptr(zmap.buffer), zmap_bytes=zmap.buffer.nbytes,
        cov_ptr=accel_device_ptr(cov.buffer), g2l_ptr=accel_device_ptr(g2l.data), in_ptr=accel_device_ptr(amps_in.buffer),
        in_flags_ptr=accel_device_ptr(amps_in.local_flags), out_ptr=accel_device_ptr(amps_out.buffer),
        out_bytes=amps_out.buffer.nbytes, det_flag_mask=binning.det_flag_mask, shared_flag_mask=binning.shared_flag_mask,
        tmpl_flag_mask=tmpl.det_flag_mask, passes=[],
        # several processes, one GPU each: sum over processes and covariance in one owner-computes pass on the stream
        owner_computes=bool(world is not None and binning.sync_type == "alltoallv" and world.device_comm()
                            and dist.replicated))
    if tmpl.use_noise_prior and tmpl._prior is not None:
        tmpl._prior.to_device()
        ctx.prior = tmpl._prior
    for iob, ob in enumerate(data.obs):
        dets = [d for d in ob.select_local_detectors(detectors, flagmask=binning.det_mask)
                if d in tmpl._obs_dets[iob]]
        if len(dets) == 0:
            continue
        noise = ob[binning.noise_model]
        n_samp = ob.n_local_samples
        f_idx, f_ptr, f_ns = device_det_flags(ob, binning.det_flags, dets, resident=True)
        s_ptr, s_n = device_shared_flags(ob, binning.shared_flags, resident=True)
        pf_idx, pf_ptr, pf_n = None, 0, 0
        if tmpl.det_flags is not None:
            pflags = tmpl._solver_flags(iob, ob, True)
            pf_idx, pf_ptr, pf_n = ob.detdata[tmpl.det_flags].indices(dets), accel_device_ptr(pflags), n_samp
        ps = ObsPass(iob=iob, dets=dets, step=tmpl._step_length(tmpl.step_time, tmpl._obs_rate[iob]),
                     ao=tmpl.det_amp_offsets(iob, dets), nav=tmpl._obs_views[iob], n_samp=n_samp,
                     ivl=ob.intervals[pixels_op.view].data,
                     detw=np.array([noise.detector_weight(d) for d in dets], dtype=np.float64),
                     f_idx=f_idx, f_ptr=f_ptr, f_ns=f_ns, s_ptr=s_ptr, s_n=s_n, pf_idx=pf_idx, pf_ptr=pf_ptr, pf_n=pf_n)
        if on_the_fly:
            compact = None
            if getattr(binning, "compact_cache", False):
                compact = compact_pixel_cache(ob, dets, pixels_op, weights_op, dist, ctx.g2l_ptr)
            ps.pt = otf_descriptor(ob, dets, pixels_op, weights_op, compact=compact)
        else:
            pd, wd = ob.detdata[pixels_op.pixels], ob.detdata[weights_op.weights]
            ps.pi, ps.pp = pd.indices(dets), accel_device_ptr(pd.buffer)
            ps.wi, ps.wp = wd.indices(dets), accel_device_ptr(wd.buffer)
        ctx.passes.append(ps)
    # (last: the packed copies are read from the arrays whose pointers were just collected)
    if cache is not None and not on_the_fly:
        for ps in ctx.passes:
            ps.pk = cache.cached(ctx, ps, in_solve)
    elif cache is not None and getattr(binning, "packed_cache", False) and not getattr(binning, "compact_cache", False):
        for ps in ctx.passes:
            ob = data.obs[ps.iob]
            ps.pk = cache.on_the_fly(ctx, ps, in_solve, (id(ob), pixels_op.nside, pixels_op.nest),
                                     lambda dets, ob=ob: otf_descriptor(ob, dets, pixels_op, weights_op), dist.n_submap)
    return ctx


class SolverRHS(Operator):
    """Right-hand side ``b = M^T N^-1 Z d`` (mapmaker_solve.py:27-229)."""

    API = Int(0, help="Internal interface version for this operator")
    det_data = Unicode(None, allow_none=True, help="Observation detdata key for the timestream data")
    det_data_units = Unicode(defaults.det_data_units, allow_none=True, help="Desired units of detector data")
    binning = Instance(klass=Operator, help="Binning operator for solving")
    template_matrix = Instance(klass=Operator, help="This must be an instance of a template matrix operator")
    fused = Bool(True, help="With one Offset template on the accelerator (pointing cached, compact-cached or on the fly): "
                            "project the timestreams in one pass that leaves them untouched instead of copy / scan / "
                            "weight / project "
                            "(not a reference trait; False = the reference operator sequence)")

    def _can_fuse(self, data):
        """Whether the fused tail runs, or the sequence has to."""
        if not (self.fused and can_fuse(self.binning, self.template_matrix)):
            return False
        tmpl = [t for t in self.template_matrix.templates if t.enabled][0]
        if tmpl.use_noise_prior:
            return False     # (the prior's baselines ignore the view; keep the reference sequence there)
        for ob in data.obs:
            if self.det_data in ob.detdata and ob.detdata[self.det_data].dtype != np.float64:
                return False
        return True

    def _exec_fused(self, data, detectors):
        """b = M^T N^-1 (d - A C A^T N^-1 d): the binning pass, then ONE pass over the cached pointing that reads d
        (toast_hip_offset_scan_project_signal_dev) -- no copy of the timestreams, no scan_map / noise_weight /
        project_signal passes over it.  It sweeps the arrays as they are: no packed cache."""
        tm = self.template_matrix
        tm.transpose = True
        tm.det_data = self.det_data
        tm.det_data_units = self.det_data_units
        for t in tm.templates:
            t.det_data = self.det_data
        tm.initialize(data)
        tmpl = [t for t in tm.templates if t.enabled][0]
        if tm.amplitudes not in data:
            data[tm.amplitudes] = AmplitudesMap()
            data[tm.amplitudes][tmpl.name] = tmpl.zeros()

        def collect():
            # the binned map of the pass above is an INPUT here (the left-hand side only uses that buffer as scratch)
            make_resident(data[self.binning.binned], self.binning.binned)
            for ob in data.obs:
                if self.det_data in ob.detdata:
                    make_resident(ob.detdata[self.det_data], self.det_data)
            return fused_prepare(self.binning, tm, tm.amplitudes, data, detectors)

        ctx = collect_stable(collect, "SolverRHS: device buffers keep being evicted while the right-hand side is prepared "
                                      "(device memory too small for its working set)")
        # (like TemplateMatrix(transpose): amplitudes that already exist are added to, not reset)
        for ps in ctx.passes:
            dd = data.obs[ps.iob].detdata[self.det_data]
            ctx.scan_project_signal(ps, dd.indices(ps.dets), accel_device_ptr(dd.buffer))
        ctx.amps_out.accel_used(True)
        tm._finalize(data)

    def _exec(self, data, detectors=None, **kwargs):
        for trait in ("det_data", "binning", "template_matrix"):
            if getattr(self, trait) is None:
                raise RuntimeError(f"You must set the '{trait}' trait before calling exec()")
        self.binning.det_data = self.det_data
        self.binning.det_data_units = self.det_data_units
        self.binning.apply(data, detectors=detectors)
        if self._can_fuse(data):
            self._exec_fused(data, detectors)
            return
        det_temp = "temp_RHS"
        self.template_matrix.transpose = True
        self.template_matrix.det_data = det_temp
        self.template_matrix.det_data_units = self.det_data_units
        _sequence_pipe(self.binning, det_temp, self.det_data_units, Copy(detdata=[(self.det_data, det_temp)]),
                       self.template_matrix).apply(data, detectors=detectors)
        Delete(detdata=[det_temp]).apply(data)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = self.binning.requires()
        req["detdata"].append(self.det_data)
        return req

    def _provides(self):
        return {"global": [self.template_matrix.amplitudes]}


class SolverLHS(Operator):
    """Left-hand side ``a' = M^T N^-1 Z M a + M_p a`` for the current proposal
    (mapmaker_solve.py:232-521).  This is the per-iteration hot loop."""

    API = Int(0, help="Internal interface version for this operator")
    det_temp = Unicode("temp_LHS", help="Observation detdata key for temporary timestream data")
    det_data_units = Unicode(defaults.det_data_units, allow_none=True, help="Desired units of detector data")
    binning = Instance(klass=Operator, help="Binning operator for solving")
    template_matrix = Instance(klass=Operator, help="This must be an instance of a template matrix operator")
    out = Unicode(None, allow_none=True, help="Output Data key for resulting amplitudes")
    fused = Bool(True, help="Use the fused device-resident kernels when the template is an Offset template "
                            "(pointing cached, compact-cached or evaluated on the fly)")
    packed_pointing = Bool(True, help="With cached IQU pointing: let the fused kernels sweep a packed copy of it "
                                      "(20 instead of 33 bytes per detector-sample: local pixel offset and flag bits in "
                                      "one word, the Q / U weights, the intensity weight once per detector), built on "
                                      "the device at the first iteration and released at the end of the solve")

    # -- fused path ---------------------------------------------------------------------------
    def _can_fuse(self, data):
        return bool(self.fused and can_fuse(self.binning, self.template_matrix))

    def __del__(self):
        try:
            self.release_packed()
        except Exception:     # noqa: BLE001 -- interpreter shutdown: the library may be gone already
            pass

    def release_packed(self):
        """Give the packed pointing cache back (and forget the recorded launches that point into it)."""
        cache = self.__dict__.pop("_packed", None)
        if cache is not None and cache.entries:
            self.__dict__.pop("_fused_plan", None)
            cache.release()

    def _pack_cache(self):
        """The packed pointing cache of this operator; None when the trait switches it off."""
        if not self.packed_pointing:
            return None
        return self.__dict__.setdefault("_packed", PackCache())

    @staticmethod
    def _fused_first_half(c):
        """zmap = 0;  a_out = 0;  zmap += A^T N^-1 M a   (launches only, ``capi.dev``)"""
        capi.dev.memset(c.zmap_ptr, 0, c.zmap_bytes)
        capi.dev.memset(c.out_ptr, 0, c.out_bytes)
        if c.prior is not None:
            # a_out = C_a^-1 a: the noise prior term of the left-hand side (mapmaker_solve.py:409-411)
            c.prior.add_prior(c.amps_in, c.amps_out)
        for ps in c.passes:
            c.accumulate(ps)

    @staticmethod
    def _fused_second_half(c):
        """zmap = C zmap;  a_out += M^T N^-1 (M a - A zmap)"""
        if c.owner_computes:
            # zmap = C . (sum over processes of zmap) in one owner-computes pass on this stream: RCCL reduce-scatter,
            # covariance on the owned pixel shard, all-gather (toast_hip_comm_map_reduce_apply_dev)
            capi.dev.comm_map_reduce_apply(c.n_local * c.nps, c.nnz, c.cov_ptr, c.zmap_ptr, reduce=True)
        else:
            capi.dev.cov_apply_diag(c.n_local, c.nps, c.nnz, c.cov_ptr, c.zmap_ptr)
        for ps in c.passes:
            c.scan_project(ps)

    def _exec_fused(self, data, detectors):
        """a' = M^T N^-1 (M a - A C A^T N^-1 M a) with two passes over the pointing and no
        timestream buffer: offset_accumulate -> [all-reduce] -> cov_apply_diag ->
        offset_scan_project (toast_amd/csrc/kernels.hip, otf_kernels.hip).

        The launch sequence of an iteration is recorded once (``capi.capture``: the C-ABI calls
        with their converted arguments) and replayed while the operands and the memory manager's
        generation are unchanged: the host then spends ~0.1 ms per iteration instead of
        re-deriving ~100 arguments, and the GPU does not idle between iterations."""
        binning, tm = self.binning, self.template_matrix
        tmpl = [t for t in tm.templates if t.enabled][0]
        tm.det_data = self.det_temp
        for t in tm.templates:
            t.det_data = None  # no timestream needed
        tm.initialize(data)
        amps_in = data[tm.amplitudes][tmpl.name]
        amps_out = data[self.out][tmpl.name]
        key = (id(data), None if detectors is None else tuple(detectors), id(amps_in), id(amps_out),
               id(data.get(binning.binned)), id(data.get(binning.covariance)), id(data.get(binning.pixel_dist)),
               binning.full_pointing, bool(getattr(binning, "compact_cache", False)),
               bool(getattr(binning, "packed_cache", False)), binning.det_flags,
               binning.det_flag_mask, binning.shared_flags, binning.shared_flag_mask, binning.det_mask,
               tmpl.det_flags, tmpl.det_flag_mask, tmpl.step_time, tmpl.use_noise_prior, tmpl.precond_width,
               amps_in.accel_in_use())
        plan = self.__dict__.get("_fused_plan")
        if plan is None or plan["key"] != key or plan["generation"] != capi.accel_generation():
            ctx = collect_stable(
                lambda: fused_prepare(binning, tm, self.out, data, detectors, cache=self._pack_cache(),
                                      in_solve=getattr(self, "keep_on_device", False)),
                "SolverLHS: device buffers keep being evicted while the fused left-hand side is prepared "
                "(device memory too small for its working set)")
            with capi.capture() as first:
                self._fused_first_half(ctx)
            with capi.capture() as second:
                self._fused_second_half(ctx)
            key = key[:4] + (id(data.get(binning.binned)),) + key[5:-1] + (True,)
            plan = dict(key=key, generation=capi.accel_generation(), ctx=ctx, first=first, second=second)
            self._fused_plan = plan
            # which sweeps the plan holds and the bytes per detector-sample of a packed one, one entry per observation
            self.last_route = tuple(ps.route for ps in ctx.passes)
            self.last_pack_bytes = tuple(None if ps.pk is None else ps.pk.bytes_per_sample for ps in ctx.passes)
        ctx = plan["ctx"]
        zmap = ctx.zmap
        zmap.accel_used(True)
        amps_out.accel_used(True)
        plan["first"].replay()
        if not ctx.owner_computes:
            zmap.sync_allreduce()      # (device-resident: an RCCL all-reduce on the same stream; no-op for one process)
        plan["second"].replay()
        if not getattr(self, "keep_on_device", False):
            native().accel_synchronize()
            amps_out.accel_update_host()
            amps_in.accel_used(False)  # host copy is current again (never modified on the device)
        for t in tm.templates:
            t.det_data = self.det_temp

    def _zero_temp(self, data):
        for ob in data.obs:
            if self.det_temp in ob.detdata:
                ob.detdata[self.det_temp].reset()

    def _exec(self, data, detectors=None, **kwargs):
        for trait in ("binning", "template_matrix", "out"):
            if getattr(self, trait) is None:
                raise RuntimeError(f"You must set the '{trait}' trait before calling exec()")
        if self._can_fuse(data):
            if self.out in data and not data[self.out].accel_in_use():
                data[self.out].reset()      # (device-current output: the first fused pass zeroes it itself)
            self._exec_fused(data, detectors)
            return
        self.last_route = ("sequence",)
        self._zero_temp(data)
        self.template_matrix.transpose = False
        self.template_matrix.det_data = self.det_temp
        self.template_matrix.det_data_units = self.det_data_units
        self.binning.det_data = self.det_temp
        self.binning.det_data_units = self.det_data_units
        self.binning.pre_process = self.template_matrix
        self.binning.apply(data, detectors=detectors)
        self.binning.pre_process = None
        if self.out in data:
            data[self.out].reset()
        self.template_matrix.add_prior(data[self.template_matrix.amplitudes], data[self.out])
        template_transpose = self.template_matrix.duplicate()
        template_transpose.amplitudes = self.out
        template_transpose.transpose = True
        self._zero_temp(data)
        _sequence_pipe(self.binning, self.det_temp, self.det_data_units, self.template_matrix,
                       template_transpose).apply(data, detectors=detectors)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = self.binning.requires()
        req["global"].append(self.template_matrix.amplitudes)
        return req

    def _provides(self):
        return {"global": [self.out]}


def _device_scalars(rhs, vectors):
    """The PCG can keep its scalars on the device when every amplitude vector is in use there and the dot products can
    be summed over the processes on the stream (one process, or the library's own communicator)."""
    import os

    if os.environ.get("TOAST_HIP_PCG_SCALARS", "device") == "host":
        return False
    mine = all(v.n_local > 0 and v.accel_in_use() for amps in (rhs,) + tuple(vectors) for v in amps.values())
    comm = next(iter(rhs.values()))._comm
    if comm is not None and comm.comm_world is not None:
        # a collective decision (the communicator is created collectively, and every rank must take the same loop)
        return bool(comm.device_comm()) and bool(int(comm.allreduce_scalar(1 if mine else 0, op="min")))
    return mine


def _pcg_device_scalars(data, detectors, lhs_op, result, residual, precond, proposal, lhs_out, sqsum_init, delta,
                        convergence, n_iter_min, n_iter_max, log, iteration_seconds):
    """The PCG loop of ``solve`` with alpha, beta, delta and the residual norms on the device (toast_hip_pcg_*,
    csrc/pcg.hip): same recurrence, same convergence / stall / iteration-limit tests as the reference
    (mapmaker_solve.py:660-755), evaluated by one-thread kernels between the vector kernels.  The host enqueues
    iteration k + 1 while the device works on iteration k and reads the status one iteration late; an iteration
    enqueued after the end is a no-op for the solution (alpha = 0)."""
    import time as _time

    D = capi.dev
    state_host = np.zeros(D.pcg_state_bytes(n_iter_max), dtype=np.uint8)   # host key of the device-side state block
    accel_data_create(state_host, "pcg_state")
    try:
        d_state = accel_device_ptr(state_host)
        D.pcg_init(d_state, sqsum_init, delta, convergence, n_iter_min, n_iter_max)
        names = list(result.keys())
        first = result[names[0]]
        comm = first._comm
        reduce_dots = bool(comm is not None and comm.comm_world is not None and not first._full)

        def dot(a, b, stage):
            for i, k in enumerate(names):
                x, y = a[k], b[k]
                # one process: the stage runs in the same launch, right behind the last template's reduction
                inline = stage if (i == len(names) - 1 and not reduce_dots) else 0
                D.pcg_dot(d_state, x.n_local, x._dptr(), y._dptr(), accel_device_ptr(x.local_flags),
                          accel_device_ptr(y.local_flags), accumulate=(i > 0), stage=inline)
            if reduce_dots:
                D.pcg_stage(d_state, stage, allreduce=True)     # sum over the ranks on the stream, then the stage

        def axpby(y, a_sel, x, b_sel):
            for k in names:
                D.pcg_axpby(d_state, y[k].n_local, a_sel, x[k]._dptr(), b_sel, y[k]._dptr())

        # The two updates whose output a dot product reads run inside that dot product's launch (same bits as the
        # separate launches; TOAST_HIP_PCG_FUSE=0 keeps them apart): result / residual update + r . r, and -- for
        # templates whose preconditioner is a diagonal -- z = M^-1 r + z . r.
        import os

        fuse = os.environ.get("TOAST_HIP_PCG_FUSE", "1") != "0"
        templates = {t.name: t for t in lhs_op.template_matrix.templates if t.enabled}

        def step_and_norm():
            if not fuse:
                for k in names:       # result += alpha * proposal;  residual -= alpha * lhs_out
                    D.pcg_step(d_state, result[k].n_local, proposal[k]._dptr(), result[k]._dptr(),
                               lhs_out[k]._dptr(), residual[k]._dptr())
                dot(residual, residual, 2)
                return
            for i, k in enumerate(names):
                inline = 2 if (i == len(names) - 1 and not reduce_dots) else 0
                D.pcg_step_dot(d_state, result[k].n_local, proposal[k]._dptr(), result[k]._dptr(), lhs_out[k]._dptr(),
                               residual[k]._dptr(), accel_device_ptr(residual[k].local_flags), accumulate=(i > 0),
                               stage=inline)
            if reduce_dots:
                D.pcg_stage(d_state, 2, allreduce=True)

        def precondition_and_project():
            diag = {k: (templates[k].precond_diag_device() if (fuse and k in templates and
                                                                hasattr(templates[k], "precond_diag_device")) else None)
                    for k in names}
            if not any(v is not None for v in diag.values()):
                lhs_op.template_matrix.apply_precond(residual, precond)
                dot(precond, residual, 3)
                return
            for i, k in enumerate(names):
                inline = 3 if (i == len(names) - 1 and not reduce_dots) else 0
                r, z = residual[k], precond[k]
                if diag[k] is not None:
                    D.pcg_precond_diag_dot(d_state, r.n_local, diag[k], r._dptr(), accel_device_ptr(r.local_flags),
                                           z._dptr(), accel_device_ptr(z.local_flags), accumulate=(i > 0), stage=inline)
                else:
                    if k in templates:
                        templates[k].apply_precond(r, z)
                    D.pcg_dot(d_state, z.n_local, z._dptr(), r._dptr(), accel_device_ptr(z.local_flags),
                              accel_device_ptr(r.local_flags), accumulate=(i > 0), stage=inline)
            if reduce_dots:
                D.pcg_stage(d_state, 3, allreduce=True)

        seen = 0       # relative residuals reported so far (the log lags one iteration behind the device)
        for it in range(n_iter_max + 1):
            if iteration_seconds is not None:
                iteration_seconds.append(_time.perf_counter())
            lhs_op.apply(data, detectors=detectors)
            dot(proposal, lhs_out, 1)
            step_and_norm()
            precondition_and_project()
            axpby(proposal, D.PCG_LIVE, precond, D.PCG_BETA)         # proposal = precond + beta * proposal
            st = D.pcg_status(d_state, lag=1)                        # the status after the PREVIOUS iteration
            if log is not None and st.n_history > seen:
                log(f"MapMaker iteration {st.n_history - 1:4d}, relative residual = {st.relative:0.6e}")
            seen = int(st.n_history)
            if st.done != 0:
                break
        history, final = D.pcg_history(d_state, n_iter_max)
        if final.done == 3:
            raise RuntimeError("Residual is not finite")
        if log is not None:
            log(f"MapMaker PCG finished after {len(history)} iterations ({D.PCG_DONE.get(int(final.done), '?')}), "
                f"relative residual = {final.relative:0.6e}")
        if iteration_seconds is not None and len(iteration_seconds) > len(history):
            del iteration_seconds[len(history):]     # the speculative iteration after the end
        return [float(x) for x in history]
    finally:
        accel_data_delete(state_host, "pcg_state")


def solve(data, detectors, lhs_op, rhs_key, result_key, convergence=1.0e-12, n_iter_min=3, n_iter_max=100,
          log=None, iteration_seconds=None):
    """Preconditioned conjugate gradient for the template amplitudes
    (mapmaker_solve.py:524-755; same recurrence, same convergence / stall tests).

    Returns the list of relative residuals, one per iteration."""
    if rhs_key not in data:
        raise RuntimeError(f"rhs_key '{rhs_key}' does not exist in data")
    rhs = data[rhs_key]
    if not isinstance(rhs, AmplitudesMap):
        raise RuntimeError("rhs_key does not point to an AmplitudesMap")
    if result_key not in data:
        data[result_key] = rhs.duplicate()
        data[result_key].reset()
    result = data[result_key]
    if not isinstance(result, AmplitudesMap):
        raise RuntimeError("result_key does not point to an AmplitudesMap")

    # With the fused device path every PCG vector stays resident on the GPU: the per-iteration
    # algebra (3 dots, 3 axpby, the preconditioner) runs in device kernels and only the three
    # scalars cross PCIe.  Otherwise the vectors live on the host as in the reference.
    on_device = bool(getattr(lhs_op, "_can_fuse", lambda d: False)(data))

    def place(amps, name):
        if on_device:
            amps.accel_resident(name)
        return amps

    place(rhs, rhs_key)
    place(result, result_key)
    lhs_out_key = f"{lhs_op.name}_out"
    if lhs_out_key in data:
        data[lhs_out_key].clear()
        del data[lhs_out_key]
    data[lhs_out_key] = rhs.duplicate()
    lhs_out = data[lhs_out_key]
    proposal_key = f"{lhs_op.name}_in"
    if proposal_key in data:
        data[proposal_key].clear()
        del data[proposal_key]
    data[proposal_key] = rhs.duplicate()
    data[proposal_key].reset()
    proposal = data[proposal_key]

    try:
        # residual of the starting guess
        lhs_op.template_matrix.amplitudes = result_key
        lhs_op.out = lhs_out_key
        lhs_op.keep_on_device = on_device
        lhs_op.apply(data, detectors=detectors)
        residual = rhs.duplicate()
        residual -= lhs_out
        precond = rhs.duplicate()
        precond.reset()
        lhs_op.template_matrix.apply_precond(residual, precond)
        proposal.copy_from(precond)
        lhs_op.template_matrix.amplitudes = proposal_key

        sqsum = rhs.dot(rhs)
        sqsum_init = sqsum
        sqsum_best = sqsum
        last_best = sqsum
        delta = proposal.dot(residual)
        history = []
        import time as _time

        if on_device and _device_scalars(rhs, (result, residual, precond, proposal, lhs_out)):
            if not np.isfinite(sqsum):
                raise RuntimeError("Residual is not finite")
            history = _pcg_device_scalars(data, detectors, lhs_op, result, residual, precond, proposal, lhs_out, sqsum_init,
                                          delta, convergence, n_iter_min, n_iter_max, log, iteration_seconds)
            n_iter_max = 0       # the host-scalar loop below does not run

        for it in range(n_iter_max):
            if iteration_seconds is not None:
                # every iteration ends in a dot product (a device synchronisation): wall time per
                # iteration is the time between those points
                iteration_seconds.append(_time.perf_counter())
            if not np.isfinite(sqsum):
                raise RuntimeError("Residual is not finite")
            lhs_op.apply(data, detectors=detectors)
            alpha = delta / proposal.dot(lhs_out)
            # result += alpha * proposal ; residual -= alpha * lhs_out  (mapmaker_solve.py:683-701,
            # same roundings as the reference's scaled temporary)
            result.axpby(alpha, proposal)
            residual.axpby(-alpha, lhs_out)
            sqsum = residual.dot(residual)
            relative = sqsum / sqsum_init if sqsum_init != 0 else 0.0
            history.append(relative)
            if log is not None:
                log(f"MapMaker iteration {it:4d}, relative residual = {relative:0.6e}")
            if relative < convergence or sqsum < 1e-30:
                break
            sqsum_best = min(sqsum, sqsum_best)
            if it % 10 == 0 and it >= n_iter_min:
                if last_best < sqsum_best * 2:
                    break
                last_best = sqsum_best
            lhs_op.template_matrix.apply_precond(residual, precond)
            delta_last = delta
            delta = precond.dot(residual)
            beta = delta / delta_last
            # proposal = beta * proposal + precond
            proposal.axpby(1.0, precond, beta)
        if iteration_seconds is not None and len(iteration_seconds) > 0:
            iteration_seconds.append(_time.perf_counter())
            stamps = list(iteration_seconds)
            iteration_seconds[:] = [b - a for a, b in zip(stamps[:-1], stamps[1:])]
    finally:
        # The packed pointing cache is a snapshot of pixels, weights and flags that belongs to THIS solve: whatever ends
        # it -- convergence, the iteration limit, a non-finite residual, an error in a kernel -- gives it back, so that a
        # later use of the operator packs the arrays as they are then.
        lhs_op.keep_on_device = False
        if hasattr(lhs_op, "release_packed"):
            lhs_op.release_packed()
    # hand the solution back on the host (AmplitudesMap.accel_update_host skips host-current ones); with lazy host
    # coherence the vectors stay device-current -- ApplyAmplitudes reads them there -- and ``Amplitudes.local`` copies back
    # when the host asks
    if not getattr(data, "lazy_host", False):
        result.accel_update_host()
        rhs.accel_update_host()
    for tmp in (residual, precond):
        tmp.clear()
    proposal.clear()
    del data[proposal_key]
    lhs_out.clear()
    del data[lhs_out_key]
    return history
