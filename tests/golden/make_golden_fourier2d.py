#!/usr/bin/env python3
"""Generate tests/golden/fourier2d.npz: the Fourier2D template, produced by the reference's own methods.

The reference implements the template in NumPy and SciPy (src/toast/templates/fourier2d.py).  Its methods ``_initialize``,
``_add_to_signal``, ``_project_signal``, ``_add_prior`` and ``_apply_precond`` are compiled from the syntax tree of that
file where it lies (as tests/golden/make_golden_templates.py does for SubHarmonic and Periodic) and run against small
stand-ins: ``u`` (units are plain floats), ``qa.rotate`` (the reference kernel's formula in NumPy), ``AlignedF64``,
``ob.view[...]`` with ``.shared`` and ``.detdata``, and ``comm_row = comm_col = None``.  Nothing of the reference's text is
copied; the fixture stores only numbers, on the sample subset of tests/fourier2d_case.py:

* the amplitude layout, the basis ``T``, the filters ``invcorr``, the norms and the results of the four operations;
* the yardsticks the GPU tests scale their bounds from (``yard_*``), measured here:
    add / project / norms   the reference's own deviation from the exactly summed value (``math.fsum`` of the rounded
                            products), in units of eps * sum|terms| per output: the largest over the outputs;
    prior                   the reference's distance from the same convolution taken in ``longdouble`` by direct summation,
                            in units of max|out| of the case: the largest over the modes and views;
* one end-to-end case (``run_e2e``): amplitudes and residual history of the reference's ``solve()`` over
  [Offset, Fourier2D] with the prior inside the left-hand side, built like the end-to-end case of
  tests/golden/make_golden_templates.py.

Build container only.      python tests/golden/make_golden_fourier2d.py
"""
import ast
import math
import os
import re
import sys
from collections import OrderedDict

import numpy as np
import scipy
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fourier2d_case as fc  # noqa: E402
import make_golden_templates as mt  # noqa: E402

REF_FILE = "/root/reference/src/toast/templates/fourier2d.py"
METHODS = ("_initialize", "_add_to_signal", "_project_signal", "_add_prior", "_apply_precond", "clear")
EPS = np.finfo(np.float64).eps
SIZE_LIMIT = 1 << 20


# ------------------------------------------------------------------ stand-ins for what the methods touch
class _Units:
    second = 1.0
    radian = 1.0


class _Value:
    def __init__(self, value):
        self.value = value

    def to_value(self, units):
        return self.value


class _Aligned:
    def __init__(self, n):
        self._a = np.zeros(n, dtype=np.float64)

    @staticmethod
    def zeros(n):
        return _Aligned(int(n))

    def array(self):
        return self._a

    def clear(self):
        pass


class _Qa:
    @staticmethod
    def rotate(q, v):
        """One quaternion (x, y, z, w), one vector: normalise, then 2 * (R - 1) v + v
        (src/libtoast/src/toast_math_qarray.cpp, the formula of every qa_rotate variant)."""
        q = np.asarray(q, dtype=np.float64)
        v = np.asarray(v, dtype=np.float64)
        norm = 0.0
        for c in q:
            norm += c * c
        x, y, z, w = q / np.sqrt(norm)
        xw, yw, zw = w * x, w * y, w * z
        x2, xy, xz = -x * x, x * y, x * z
        y2, yz, z2 = -y * y, y * z, -z * z
        return np.array([2 * ((y2 + z2) * v[0] + (xy - zw) * v[1] + (yw + xz) * v[2]) + v[0],
                         2 * ((zw + xy) * v[0] + (x2 + z2) * v[1] + (yz - xw) * v[2]) + v[1],
                         2 * ((xz - yw) * v[0] + (xw + yz) * v[1] + (x2 + y2) * v[2]) + v[2]])


def load_reference_class():
    """A bare class holding the reference's methods of Fourier2D, compiled from its source file."""
    tree = ast.parse(open(REF_FILE).read(), REF_FILE)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Fourier2D"]
    assert len(cls) == 1
    fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert len(fns) == len(METHODS)
    for fn in fns:
        fn.decorator_list = []
    holder = ast.ClassDef(name="Fourier2D", bases=[], keywords=[], body=fns, decorator_list=[])
    mod = ast.Module(body=[holder], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "re": re, "os": os, "OrderedDict": OrderedDict, "scipy": scipy, "u": _Units, "qa": _Qa,
          "AlignedF64": _Aligned, "MPI": None, "Logger": mt._Quiet}
    exec(compile(mod, REF_FILE, "exec"), ns)
    return ns["Fourier2D"]


class _ViewShared:
    def __init__(self, ob, ivl):
        self.ob, self.ivl = ob, ivl

    def __getitem__(self, key):
        return [self.ob.shared[key].data[int(v.first):int(v.last)] for v in self.ivl]


class _View(mt._View):
    def __init__(self, ob, name):
        super().__init__(ob, name)
        self.shared = _ViewShared(ob, self.ivl)


class _Views:
    def __init__(self, ob):
        self.ob = ob

    def __getitem__(self, name):
        return _View(self.ob, name)


class _Focalplane:
    def __init__(self, fp):
        self._fp = fp
        self.field_of_view = _Value(fp.field_of_view)

    def __getitem__(self, det):
        return self._fp[det]


class _Telescope:
    def __init__(self, fp):
        self.focalplane = _Focalplane(fp)


class Obs(mt.Obs):
    comm_row = None
    comm_col = None
    local_index_offset = 0

    def __init__(self, ob):
        super().__init__(ob)
        self.view = _Views(ob)
        self.telescope = _Telescope(ob.telescope.focalplane)


class RefData(mt.RefData):
    def __init__(self, data):
        self.obs = [Obs(ob) for ob in data.obs]


def instance(cls, data, view=fc.VIEW, det_data=fc.DET_DATA, det_flags=fc.DET_FLAGS, det_flag_mask=fc.DET_FLAG_MASK, **traits):
    t = cls()
    t.name, t.pattern, t.view, t.det_data, t.det_data_units = "Fourier2D", None, view, det_data, 1.0
    t.det_mask, t.det_flags, t.det_flag_mask = 1, det_flags, det_flag_mask
    t.times, t.correlation_length, t.correlation_amplitude = "times", _Value(10.0), 10.0
    t.order, t.fit_subharmonics, t.noise_model, t.debug_plots = 1, True, None, None
    for k, v in traits.items():
        setattr(t, k, _Value(float(v)) if k == "correlation_length" else v)
    t.data = RefData(data)
    t._initialize(t.data)
    return t


# ------------------------------------------------------------------ yardsticks
def fsum_deviation(value, terms):
    """|value - exact sum of terms| in units of eps * sum|terms|."""
    scale = EPS * math.fsum(abs(x) for x in terms)
    return abs(value - math.fsum(terms)) / scale if scale > 0 else 0.0


def floored_frequencies(times, corr_len, amp):
    """How many frequencies the reference's floor replaces for one view (fourier2d.py:268-280, NumPy's complex order)."""
    corr = np.exp((times[0] - times) / corr_len) * amp
    ihalf = times.size // 2
    if times.size % 2 == 0:
        corr[ihalf:] = corr[ihalf - 1:: -1]
    else:
        corr[ihalf + 1:] = corr[ihalf - 1:: -1]
    fcorr = np.fft.rfft(corr)
    return int(np.count_nonzero(fcorr < (1.0e-6 * amp))), fcorr.size


def run_case(name, cls, blob):
    layout, traits = fc.CASES[name]
    data = fc.build(layout)
    t = instance(cls, data, **traits)
    nmode = t._nmode
    rows, cols = fc.sample_subset(layout)
    blob[f"{name}_n_local"] = np.array(t._n_local)
    blob[f"{name}_nmode"] = np.array(nmode)
    blob[f"{name}_view_offset"] = np.array([o for iob in range(len(data.obs)) for o in t._obs_view_local_offset[iob]],
                                           dtype=np.int64)
    blob[f"{name}_local_ranges"] = np.array(t._local_ranges, dtype=np.int64)
    blob[f"{name}_rows"] = rows
    for iob, ob in enumerate(data.obs):
        dets = [d for d in ob.local_detectors if d in t._obs_dets[iob]]
        tm = np.array([t._templates[iob][0][d] for d in dets])
        for ivw in range(1, len(t._templates[iob])):
            assert all(np.array_equal(t._templates[iob][ivw][d], t._templates[iob][0][d]) for d in dets)
        fc.check_rank(tm)
        blob[f"{name}_T_obs{iob}"] = tm
        blob[f"{name}_cols_obs{iob}"] = cols[iob]
        for ivw, filt in enumerate(t._filters[iob]):
            blob[f"{name}_invcorr_{iob}_{ivw}"] = filt
    blob[f"{name}_filter_scale"] = t._filter_scale.copy()
    norms = t._norms.reshape(-1, nmode)
    blob[f"{name}_norms"] = norms[rows].copy()
    zero_row = fc.all_flagged_row(layout)
    if zero_row is not None:
        assert np.all(norms[zero_row] == 0.0)
    floored = []
    for iob, ob in enumerate(data.obs):
        for first, last in fc.view_samples(layout)[iob]:
            floored.append(floored_frequencies(ob.shared["times"].data[first:last].copy(), t.correlation_length.value,
                                               t.correlation_amplitude))
    blob[f"{name}_floored"] = np.array(floored, dtype=np.int64)
    yard = {}

    # norms: the sum before the inversion, against the exact sum
    worst = 0.0
    for iob, ob in enumerate(data.obs):
        dets = [d for d in ob.local_detectors if d in t._obs_dets[iob]]
        w = [1.0 if t.noise_model is None else ob[t.noise_model].detector_weight(d) for d in dets]
        off = 0
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            base = t._obs_view_local_offset[iob][ivw] // nmode
            good = (ob.detdata[fc.DET_FLAGS].data[:, first:last] & fc.DET_FLAG_MASK) == 0
            for i in range(0, last - first, 7):
                for m in range(0, nmode, 3):
                    rowidx = ob.detdata[fc.DET_FLAGS].indices(dets)
                    terms = [float(t._templates[iob][ivw][d][m] ** 2 * wd) for d, wd, r in zip(dets, w, rowidx) if good[r, i]]
                    if terms:
                        worst = max(worst, fsum_deviation(1.0 / norms[base + i, m], terms))
    yard["norms"] = worst

    # M^T d first (the signal is still the seeded one), on top of amplitudes that are not zero
    start = fc.amplitudes(t._n_local, 2)
    proj = mt.Amp(t._n_local)
    proj.local[:] = start
    for det in t._all_dets:
        t._project_signal(det, proj)
    pv = proj.local.reshape(-1, nmode)
    blob[f"{name}_project"] = pv[rows].copy()
    worst = 0.0
    for iob, ob in enumerate(data.obs):
        dets = [d for d in t._all_dets if d in t._obs_dets[iob]]
        sig = ob.detdata[fc.DET_DATA]
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            base = t._obs_view_local_offset[iob][ivw] // nmode
            for i in range(0, last - first, 7):
                for m in range(0, nmode, 3):
                    terms = [float(start[(base + i) * nmode + m])]
                    terms += [float(sig[d][first + i] * t._templates[iob][ivw][d][m]) for d in dets]
                    worst = max(worst, fsum_deviation(pv[base + i, m], terms))
    yard["project"] = worst

    # d + M a
    amps = mt.Amp(t._n_local)
    amps.local[:] = fc.amplitudes(t._n_local, 1)
    before = {iob: ob.detdata[fc.DET_DATA].data.copy() for iob, ob in enumerate(data.obs)}
    for det in t._all_dets:
        t._add_to_signal(det, amps)
    av = amps.local.reshape(-1, nmode)
    worst = 0.0
    for iob, ob in enumerate(data.obs):
        after = ob.detdata[fc.DET_DATA].data
        blob[f"{name}_add_obs{iob}"] = after[:, cols[iob]].copy()
        dets = [d for d in t._all_dets if d in t._obs_dets[iob]]
        rowidx = ob.detdata[fc.DET_DATA].indices(dets)
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            base = t._obs_view_local_offset[iob][ivw] // nmode
            for d, r in list(zip(dets, rowidx))[::3]:
                tm = t._templates[iob][ivw][d]
                for i in range(0, last - first, 7):
                    terms = [float(before[iob][r, first + i])] + [float(x) for x in av[base + i] * tm]
                    worst = max(worst, fsum_deviation(after[r, first + i], terms))
        # outside the views nothing changes
        outside = np.ones(after.shape[1], dtype=bool)
        for first, last in fc.view_samples(layout)[iob]:
            outside[first:last] = False
        assert np.array_equal(after[:, outside], before[iob][:, outside])
    yard["add"] = worst

    out = mt.Amp(t._n_local)
    t._apply_precond(amps, out)
    assert np.array_equal(out.local, amps.local * t._norms)      # (the tests take this product as the expectation)

    # prior, on top of an output that is not zero
    out = mt.Amp(t._n_local)
    out.local[:] = 0.5
    t._add_prior(amps, out)
    ov = out.local.reshape(-1, nmode)
    blob[f"{name}_prior"] = ov[rows].copy()
    blob[f"{name}_prior_max"] = np.array(np.max(np.abs(ov - 0.5)))
    worst = 0.0
    scale_of_case = float(np.max(np.abs(ov - 0.5)))
    for iob, ob in enumerate(data.obs):
        for ivw, (first, last) in enumerate(fc.view_samples(layout)[iob]):
            base = t._obs_view_local_offset[iob][ivw] // nmode
            n = last - first
            filt = t._filters[iob][ivw]
            shift = (filt.size - 1) // 2
            for m in sorted(set([0, 1, nmode // 2, nmode - 1])):
                full = np.convolve(av[base:base + n, m].astype(np.longdouble),
                                   (filt * t._filter_scale[m]).astype(np.longdouble))
                exact = full[shift:shift + n]
                got = (ov[base:base + n, m] - 0.5).astype(np.longdouble)
                # (the 0.5 the prior was added to costs the reference one rounding of its own: eps / 2 of the sum)
                worst = max(worst, float(np.max(np.abs(got - exact))) / scale_of_case)
    yard["prior"] = worst
    for k, v in yard.items():
        blob[f"{name}_yard_{k}"] = np.array(v)
    print(f"{name}: {layout}, nmode {nmode}, {t._n_local} amplitudes, floored {[f[0] for f in floored]} of "
          f"{[f[1] for f in floored]}; yardsticks " + ", ".join(f"{k} {v:.3g}" for k, v in yard.items()))
    return floored


def run_e2e(cls, blob):
    """``solve()`` of the reference over [Offset, Fourier2D], built like the end-to-end case of
    tests/golden/make_golden_templates.py from the pieces of tests/golden/make_golden_mapmaker.py (the reference's compiled
    kernels in oracle/_ref, its ``solve()``, the operator order of SolveAmplitudes / SolverRHS / SolverLHS) with the NumPy
    template next to the offset kernels and its prior added inside the left-hand side, where the reference adds it
    (src/toast/ops/mapmaker_solve.py:399-411: the output is reset, then the prior, then the projection accumulates).
    One whole-observation view; solver flags with mask 255 for the binning and for both templates."""
    import make_golden_mapmaker as mg
    from toast_amd import synth
    from toast_amd.data import defaults

    ref = mg.ref
    data, cfg = fc.build_e2e()
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
    # solver flags (bit 1), solver covariance, rcond cut (bit 4): SolveAmplitudes
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
    # the timestream the templates work on and their flags live in the observation, where the NumPy template looks
    ob.detdata.create("temp", dtype=np.float64)
    ob.detdata.create("solver_flags", dtype=np.uint8)
    ob.detdata["solver_flags"].data[:] = solver_flags
    tod = ob.detdata["temp"].data
    # Offset: layout, variances, flags (offset.py:250-330)
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
    f2d = instance(cls, data, view=None, det_data="temp", det_flags="solver_flags", det_flag_mask=255, order=cfg["order"],
                   fit_subharmonics=cfg["fit_subharmonics"], noise_model=defaults.noise_model,
                   correlation_length=cfg["correlation_length"], correlation_amplitude=cfg["correlation_amplitude"])

    def new_amps():
        return mg.AmpMap(baselines=mg.Amp(n_amp, amp_flags), fourier2d=mg.Amp(f2d._n_local, np.zeros(f2d._n_local, np.uint8)))

    def template_add(amps):          # TemplateMatrix: template after template, detector after detector
        for d in range(n_det):
            ref.template_offset_add_to_signal(step, d * per_det, n_amp_views, amps["baselines"].local,
                                              amps["baselines"].local_flags, d, tod, ivl, False)
        for det in dets:
            f2d._add_to_signal(det, amps["fourier2d"])

    def template_project(amps):
        for d in range(n_det):
            ref.template_offset_project_signal(d, tod, d, solver_flags, 255, step, d * per_det, n_amp_views,
                                               amps["baselines"].local, amps["baselines"].local_flags, ivl, False)
        for det in dets:
            f2d._project_signal(det, amps["fourier2d"])

    def bin_map(cov):
        z = np.zeros((n_local, nps, nnz))
        ref.build_noise_weighted(g2l, z, idx, pixels, idx, weights, idx, tod, idx, solver_flags, detw, 255, ivl, sflags, 0, False)
        ref.cov_apply_diag(n_local, nps, nnz, cov, z.reshape(-1))
        return z

    def scan_subtract_weight(binned):
        ref.ops_scan_map_float64(g2l, nps, binned, tod, idx, pixels, idx, weights, idx, ivl, 1.0, False, True, False, False)
        ref.noise_weight(tod, idx, ivl, detw, False)

    # right-hand side (SolverRHS._exec): no prior
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
            f2d._apply_precond(amps_in["fourier2d"], amps_out["fourier2d"])

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
            f2d._add_prior(a_in["fourier2d"], d[self.out]["fourier2d"])     # (the Offset template has no prior here)
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
    for name in fc.E2E_NAMES:
        blob[f"e2e_amplitudes_{name}"] = store["amplitudes"][name].local.copy()
        blob[f"e2e_rhs_{name}"] = rhs[name].local.copy()
        blob[f"e2e_flags_{name}"] = np.asarray(rhs[name].local_flags, dtype=np.uint8).copy()
    blob["e2e_history"] = history
    print(f"e2e: {n_det} x {n_samp}, nside {nside}: amplitudes {[store['amplitudes'][k].local.size for k in fc.E2E_NAMES]}, "
          f"residual {history[0]:.3e} -> {history[-1]:.3e}")


def main():
    cls = load_reference_class()
    blob = {}
    for name in fc.CASES:
        floored = run_case(name, cls, blob)
        if name == "floor":
            assert max(f[0] for f in floored) > 100, floored      # the floor is active, and by hundreds of frequencies
        if name == "m7":
            assert any(f[0] > 0 for f in floored), floored        # ... and at the default traits too
    blob["yard_prior_max"] = np.array(max(float(blob[f"{c}_yard_prior"]) for c in fc.CASES))
    if "--no-e2e" not in sys.argv:
        run_e2e(cls, blob)
    path = os.path.join(HERE, "fourier2d.npz")
    np.savez_compressed(path, **blob)
    assert all(v.dtype != object for v in blob.values())
    size = os.path.getsize(path)
    print("fourier2d.npz: %.3f MB" % (size / 1e6))
    assert size < SIZE_LIMIT, size


if __name__ == "__main__":
    main()
