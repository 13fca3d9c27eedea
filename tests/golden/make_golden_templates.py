#!/usr/bin/env python3
"""Generate tests/golden/templates_basis.npz: the SubHarmonic and Periodic templates, produced by the reference's own
methods.

The reference implements both templates in NumPy (src/toast/templates/subharmonic.py, periodic.py).  Their methods
``_initialize``, ``_view_flags_and_index``, ``_add_to_signal``, ``_project_signal`` and ``_apply_precond`` are compiled
from the syntax tree of those files where they lie (as tests/golden/make_golden_mapmaker.py does with ``solve()``) and
run against small stand-ins for ``data`` / ``obs`` / ``view`` that wrap the observations of tests/templates_case.py.
Nothing of the reference's text is copied; the fixture stores only numbers: amplitude layout, hit counts, flags, bin
indices, preconditioners and the results of the three operations.

One end-to-end case (``run_e2e``): amplitudes and residual history of the reference's ``solve()`` over [Offset, SubHarmonic,
Periodic], built like tests/golden/mapmaker_e2e.npz from the pieces of tests/golden/make_golden_mapmaker.py.

Build container only.      python tests/golden/make_golden_templates.py
"""
import ast
import os
import re
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import templates_case as tc  # noqa: E402

REF_DIR = "/root/reference/src/toast/templates"
METHODS = ("_initialize", "_view_flags_and_index", "_add_to_signal", "_project_signal", "_apply_precond")


class _Quiet:
    @staticmethod
    def get():
        return _Quiet()

    def __getattr__(self, name):
        return lambda *a, **k: None


def load_reference_class(filename, classname):
    """A bare class holding the reference's methods of ``classname``, compiled from its source file."""
    path = os.path.join(REF_DIR, filename)
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == classname]
    assert len(cls) == 1
    fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    for fn in fns:
        fn.decorator_list = []
    holder = ast.ClassDef(name=classname, bases=[], keywords=[], body=fns, decorator_list=[])
    mod = ast.Module(body=[holder], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "re": re, "OrderedDict": OrderedDict, "Logger": _Quiet, "MPI": None}
    exec(compile(mod, path, "exec"), ns)
    return ns[classname]


# ------------------------------------------------------------------ stand-ins for what the methods touch
class Amp:
    def __init__(self, n, flags=None):
        self.local = np.zeros(n)
        self.local_flags = np.zeros(n, dtype=np.uint8) if flags is None else flags


class _Weight:
    def __init__(self, value):
        self.value = value

    def to_value(self, units):
        return self.value


class _Noise:
    def __init__(self, model):
        self.model = model

    def detector_weight(self, det):
        return _Weight(self.model.detector_weight(det))


class _ViewRows:
    """``ob.view[name].detdata[key][ivw]``: detector -> the samples of one view (a NumPy view of the row)."""

    def __init__(self, dd, first, last):
        self.dd, self.first, self.last = dd, first, last

    def __getitem__(self, det):
        return self.dd[det][self.first:self.last]

    def __setitem__(self, det, value):
        self.dd[det][self.first:self.last] = value


class _ViewDetdata:
    def __init__(self, ob, ivl):
        self.ob, self.ivl = ob, ivl

    def __getitem__(self, key):
        return [_ViewRows(self.ob.detdata[key], int(v.first), int(v.last)) for v in self.ivl]


class _View:
    def __init__(self, ob, name):
        self.ivl = ob.intervals[name].data
        self.detdata = _ViewDetdata(ob, self.ivl)

    def __len__(self):
        return len(self.ivl)

    def __iter__(self):
        return iter([slice(int(v.first), int(v.last), 1) for v in self.ivl])


class _Views:
    def __init__(self, ob):
        self.ob = ob

    def __getitem__(self, name):
        return _View(self.ob, name)


class Obs:
    class comm:
        group_rank = 0

    def __init__(self, ob):
        self._ob = ob
        self.name, self.detdata, self.shared, self.intervals = ob.name, ob.detdata, ob.shared, ob.intervals
        self.local_detectors, self.n_local_samples = ob.local_detectors, ob.n_local_samples
        self.view = _Views(ob)

    def select_local_detectors(self, selection=None, flagmask=0):
        return self._ob.select_local_detectors(selection=selection, flagmask=flagmask)

    def __contains__(self, key):
        return key is not None and key in self._ob

    def __getitem__(self, key):
        return _Noise(self._ob[key])


class RefData:
    class comm:
        comm_world = None
        group = 0
        world_size = 1
        world_rank = 0

    def __init__(self, data):
        self.obs = [Obs(ob) for ob in data.obs]


def instance(cls, data, **traits):
    t = cls()
    t.name, t.pattern, t.view, t.det_data, t.det_data_units = cls.__name__, None, tc.VIEW, tc.DET_DATA, 1.0
    t.det_mask, t.det_flags, t.det_flag_mask = 1, tc.DET_FLAGS, tc.DET_FLAG_MASK
    for k, v in traits.items():
        setattr(t, k, v)
    t.data = RefData(data)
    t._initialize(t.data)
    return t


def signals(data):
    return {f"obs{i}": ob.detdata[tc.DET_DATA].data.copy() for i, ob in enumerate(data.obs)}


def run_subharmonic(name, cls, blob):
    layout, traits = tc.SUBHARMONIC_CASES[name]
    data = tc.build(layout)
    t = instance(cls, data, times="times", **traits)
    norder = t.order + 1
    blob[f"{name}_n_local"] = np.array(t._n_local)
    blob[f"{name}_det_start"] = np.array([t._det_start[d] for d in t._all_dets], dtype=np.int64)
    # preconditioner blocks in amplitude order
    prec = np.zeros((t._n_local // norder, norder, norder))
    for det in t._all_dets:
        blk = t._det_start[det] // norder
        for iob, ob in enumerate(t.data.obs):
            if det not in t._obs_dets[iob]:
                continue
            for ivw in range(len(ob.view[t.view])):
                prec[blk] = t._precond[iob][ivw][det]
                blk += 1
    blob[f"{name}_precond"] = prec
    # M^T d first (the signal is still the seeded one), then d + M a
    proj = Amp(t._n_local)
    proj.local[:] = 123.0          # assigned, not accumulated
    for det in t._all_dets:
        t._project_signal(det, proj)
    blob[f"{name}_project"] = proj.local.copy()
    amps = Amp(t._n_local)
    amps.local[:] = tc.amplitudes(t._n_local, 1)
    for det in t._all_dets:
        t._add_to_signal(det, amps)
    for k, v in signals(data).items():
        blob[f"{name}_add_{k}"] = v
    out = Amp(t._n_local)
    t._apply_precond(amps, out)
    blob[f"{name}_precond_out"] = out.local.copy()
    print(f"{name}: order {t.order}, {t._n_local} amplitudes, cond(Gram) up to "
          f"{max(np.linalg.cond(np.linalg.inv(p)) for p in prec):.1f}")


def run_periodic(name, cls, blob):
    layout, traits = tc.PERIODIC_CASES[name]
    data = tc.build(layout)
    t = instance(cls, data, is_detdata_key=False, **traits)
    blob[f"{name}_n_local"] = np.array(t._n_local)
    blob[f"{name}_det_offset"] = np.array([t._det_offset[d] for d in t._all_dets], dtype=np.int64)
    blob[f"{name}_obs_min"] = np.array(t._obs_min)
    blob[f"{name}_obs_max"] = np.array(t._obs_max)
    blob[f"{name}_obs_incr"] = np.array(t._obs_incr)
    blob[f"{name}_obs_nbins"] = np.array(t._obs_nbins, dtype=np.int64)
    blob[f"{name}_hits"] = t._amp_hits.copy()
    blob[f"{name}_flags"] = t._amp_flags.astype(np.uint8)
    # the bin of every sample as add_to_signal sees it (key flags only), -1 where it has none
    for iob, ob in enumerate(t.data.obs):
        index = np.full(ob.n_local_samples, -1, dtype=np.int32)
        for vw in ob.intervals[t.view].data:
            good, amp_indx = t._view_flags_and_index(0, iob, ob, vw, det_flags=False)
            index[vw.first:vw.last][good] = amp_indx
        blob[f"{name}_index_obs{iob}"] = index
    flags = t._amp_flags.astype(np.uint8)
    proj = Amp(t._n_local, flags)
    proj.local[:] = 0.5            # accumulated on top
    for det in t._all_dets:
        t._project_signal(det, proj)
    blob[f"{name}_project"] = proj.local.copy()
    amps = Amp(t._n_local, flags)
    amps.local[:] = tc.amplitudes(t._n_local, 2)
    for det in t._all_dets:
        t._add_to_signal(det, amps)
    for k, v in signals(data).items():
        blob[f"{name}_add_{k}"] = v
    out = Amp(t._n_local, flags)
    out.local[:] = -3.0            # untouched where flagged
    t._apply_precond(amps, out)
    blob[f"{name}_precond_out"] = out.local.copy()
    late = int(np.count_nonzero(t._amp_flags & (t._amp_hits >= t.minimum_bin_hits)))
    print(f"{name}: bins {t._obs_nbins}, {t._n_local} amplitudes, {int(t._amp_flags.sum())} flagged, "
          f"{late} of them reach the minimum in a later view")
    assert late > 0


def run_e2e(sub_cls, per_cls, blob):
    """``solve()`` of the reference over [Offset, SubHarmonic, Periodic], built like tests/golden/mapmaker_e2e.npz: the
    pieces of tests/golden/make_golden_mapmaker.py (the reference's compiled kernels in oracle/_ref, its ``solve()``, the
    operator order of SolveAmplitudes / SolverRHS / SolverLHS) with the two NumPy templates next to the offset kernels.
    One whole-observation view; solver flags with mask 255 for the binning and for all three templates."""
    import make_golden_mapmaker as mg
    from toast_amd import synth
    from toast_amd.data import defaults

    ref = mg.ref
    data, cfg = tc.build_e2e()
    ob = data.obs[0]
    n_det, n_samp, rate, nside = cfg["n_det"], cfg["n_samp"], cfg["rate"], cfg["nside"]
    dets = list(ob.local_detectors)
    idx = np.arange(n_det, dtype=np.int32)
    fpl = ob.telescope.focalplane
    fp = np.ascontiguousarray(np.array([fpl[d]["quat"] for d in dets]))
    gamma = np.array([float(fpl[d]["gamma"]) for d in dets])
    eps = np.array([float(fpl[d]["pol_leakage"]) for d in dets])
    cal = np.array([float(fpl[d]["cal"]) for d in dets])
    bore = ob.shared[defaults.boresight_radec].data
    sflags = ob.shared[defaults.shared_flags].data
    hwp = np.ascontiguousarray(ob.shared[defaults.hwp_angle].data)
    dflags = ob.detdata[defaults.det_flags].data
    signal = ob.detdata[defaults.det_data].data
    ivl = ob.intervals[None].data
    detw = np.array([float(ob[defaults.noise_model].detector_weight(d)) for d in dets])
    nps = 3072 if nside >= 16 else 12 * nside * nside
    n_submap = 12 * nside * nside // nps
    nnz = 3
    quats = np.zeros((n_det, n_samp, 4))
    ref.pointing_detector(fp, bore, idx, quats, ivl, sflags, defaults.shared_mask_invalid, False)
    pixels = np.zeros((n_det, n_samp), dtype=np.int64)
    hsub = np.zeros(n_submap, dtype=np.uint8)
    ref.pixels_healpix(idx, quats, sflags, defaults.shared_mask_invalid, idx, pixels, ivl, hsub, nps, nside, True, False)
    weights = np.zeros((n_det, n_samp, nnz))
    ref.stokes_weights_IQU(idx, quats, idx, weights, hwp, ivl, eps, gamma, cal, False, False)
    g2l, hit = synth.global_to_local(hsub)
    n_local = int(hit.size)
    # solver flags (bit 1), solver covariance, rcond cut (bit 4): SolveAmplitudes, as in make_golden_mapmaker.run_case
    sflag1 = ((sflags & defaults.shared_mask_nonscience) > 0).astype(np.uint8)
    solver_flags = np.empty((n_det, n_samp), dtype=np.uint8)
    for d in range(n_det):
        solver_flags[d] = sflag1 | ((dflags[d] & defaults.det_mask_nonscience) > 0).astype(np.uint8)
    hits = np.zeros(n_local * nps, dtype=np.int64)
    invcov = np.zeros(n_local * nps * 6)
    for d in range(n_det):
        sm, lp = mg.global_pixel_to_submap(pixels[d], g2l, nps)
        lp[(solver_flags[d] & 255) != 0] = -1
        lp[(sflags & defaults.shared_mask_nonscience) != 0] = -1
        ref.cov_accum_diag_hits(n_local, nps, 1, sm, lp, hits, False)
        ref.cov_accum_diag_invnpp(n_local, nps, nnz, sm, lp, np.ascontiguousarray(weights[d]).reshape(-1), float(detw[d]),
                                  invcov, False)
    s_cov = invcov.copy()
    s_rcond = np.zeros(n_local * nps)
    mg.cov_eigendecompose_diag(n_local, nps, nnz, s_cov, s_rcond, 1.0e-8)
    rcond_mask = (s_rcond < 1.0e-8).astype(np.uint8)
    for d in range(n_det):
        sm, lp = mg.global_pixel_to_submap(pixels[d], g2l, nps)
        solver_flags[d][(rcond_mask.reshape(n_local, nps)[sm, lp] & 255) != 0] |= 4
    # the timestream the templates work on and their flags live in the observation, where the NumPy templates look
    ob.detdata.create("temp", dtype=np.float64)
    ob.detdata.create("solver_flags", dtype=np.uint8)
    ob.detdata["solver_flags"].data[:] = solver_flags
    tod = ob.detdata["temp"].data
    # Offset: layout, variances, flags (offset.py:250-330), as in make_golden_mapmaker.run_case
    step = int(np.rint(cfg["step_time"] * rate))
    n_amp_views = np.array([(int(v["last"] - v["first"]) + step - 1) // step for v in ivl], dtype=np.int64)
    per_det = int(n_amp_views.sum())
    n_amp = n_det * per_det
    amp_flags = np.zeros(n_amp, dtype=np.uint8)
    offset_var = np.zeros(n_amp)
    off = 0
    for d in range(n_det):
        for ivw, vw in enumerate(ivl):
            first, last = int(vw["first"]), int(vw["last"])
            fl = (solver_flags[d, first:last] & 255).astype(np.uint8)
            voff = 0
            for amp in range(int(n_amp_views[ivw])):
                amplen = step if amp < n_amp_views[ivw] - 1 else (last - first) - voff
                n_good = amplen - int(np.count_nonzero(fl[voff:voff + amplen]))
                if (n_good / amplen) <= 0.5:
                    amp_flags[off + amp] = 1
                else:
                    offset_var[off + amp] = 1.0 / (detw[d] * n_good)
                voff += step
            off += int(n_amp_views[ivw])
    common = dict(view=None, det_data="temp", det_flags="solver_flags", det_flag_mask=255)
    sub = instance(sub_cls, data, times="times", order=cfg["order"], noise_model=defaults.noise_model, **common)
    per = instance(per_cls, data, is_detdata_key=False, key=tc.KEY, flags=None, flag_mask=0, bins=cfg["bins"],
                   increment=None, minimum_bin_hits=cfg["minimum_bin_hits"], **common)
    numpy_templates = {"subharmonic": sub, "ground": per}

    def new_amps():
        return mg.AmpMap(baselines=mg.Amp(n_amp, amp_flags), subharmonic=mg.Amp(sub._n_local, np.zeros(sub._n_local, np.uint8)),
                         ground=mg.Amp(per._n_local, per._amp_flags.astype(np.uint8)))

    def template_add(amps):          # TemplateMatrix: template after template, detector after detector
        for d in range(n_det):
            ref.template_offset_add_to_signal(step, d * per_det, n_amp_views, amps["baselines"].local,
                                              amps["baselines"].local_flags, d, tod, ivl, False)
        for name, t in numpy_templates.items():
            for det in dets:
                t._add_to_signal(det, amps[name])

    def template_project(amps):
        for d in range(n_det):
            ref.template_offset_project_signal(d, tod, d, solver_flags, 255, step, d * per_det, n_amp_views,
                                               amps["baselines"].local, amps["baselines"].local_flags, ivl, False)
        for name, t in numpy_templates.items():
            for det in dets:
                t._project_signal(det, amps[name])

    def bin_map(cov):
        z = np.zeros((n_local, nps, nnz))
        ref.build_noise_weighted(g2l, z, idx, pixels, idx, weights, idx, tod, idx, solver_flags, detw, 255, ivl, sflags, 0, False)
        ref.cov_apply_diag(n_local, nps, nnz, cov, z.reshape(-1))
        return z

    def scan_subtract_weight(binned):
        ref.ops_scan_map_float64(g2l, nps, binned, tod, idx, pixels, idx, weights, idx, ivl, 1.0, False, True, False, False)
        ref.noise_weight(tod, idx, ivl, detw, False)

    # right-hand side (SolverRHS._exec)
    tod[:] = signal
    binned = bin_map(s_cov)
    scan_subtract_weight(binned)
    rhs = new_amps()
    template_project(rhs)

    class TemplateMatrix:
        amplitudes = None

        def apply_precond(self, amps_in, amps_out):
            ref.template_offset_apply_diag_precond(offset_var, amps_in["baselines"].local, amps_in["baselines"].local_flags,
                                                   amps_out["baselines"].local, False)
            for name, t in numpy_templates.items():
                t._apply_precond(amps_in[name], amps_out[name])

    class LHS:
        name = "mm_lhs"
        out = None
        template_matrix = TemplateMatrix()

        def apply(self, d, detectors=None):
            a_in = d[self.template_matrix.amplitudes]
            tod[:] = 0.0
            template_add(a_in)
            b = bin_map(s_cov)
            d[self.out].reset()
            tod[:] = 0.0
            template_add(a_in)
            scan_subtract_weight(b)
            template_project(d[self.out])

    store = mg.Data()
    store["rhs"] = rhs
    mg.AmpMap.dots = []
    mg.load_reference_solve()(store, None, LHS(), "rhs", "amplitudes", convergence=1.0e-30, n_iter_max=cfg["iters"],
                              n_iter_min=cfg["iters"])
    dots = np.array(mg.AmpMap.dots)
    history = dots[3::3] / dots[0]
    for name in tc.E2E_NAMES:
        blob[f"e2e_amplitudes_{name}"] = store["amplitudes"][name].local.copy()
        blob[f"e2e_rhs_{name}"] = rhs[name].local.copy()
        blob[f"e2e_flags_{name}"] = np.asarray(rhs[name].local_flags, dtype=np.uint8).copy()
    blob["e2e_history"] = history
    blob["e2e_dots"] = dots
    blob["e2e_solver_flag_counts"] = np.array([int(np.count_nonzero(solver_flags & b)) for b in (1, 4)])
    print(f"e2e: {n_det} x {n_samp}, nside {nside}: amplitudes {[store['amplitudes'][k].local.size for k in tc.E2E_NAMES]}, "
          f"residual {history[0]:.3e} -> {history[-1]:.3e}")


def main():
    sub = load_reference_class("subharmonic.py", "SubHarmonic")
    per = load_reference_class("periodic.py", "Periodic")
    blob = {}
    for name in tc.SUBHARMONIC_CASES:
        run_subharmonic(name, sub, blob)
    for name in tc.PERIODIC_CASES:
        run_periodic(name, per, blob)
    run_e2e(sub, per, blob)
    path = os.path.join(HERE, "templates_basis.npz")
    np.savez_compressed(path, **blob)
    assert all(v.dtype != object for v in blob.values())
    print("templates_basis.npz: %.3f MB" % (os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
