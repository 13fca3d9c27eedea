#!/usr/bin/env python3
"""Generate tests/golden/gain_template.npz: the GainTemplate, produced by the reference's own methods.

The reference implements the template in NumPy and SciPy (src/toast/templates/gaintemplate.py).  Its methods
``_initialize``, ``_get_polynomials``, ``_add_to_signal``, ``_project_signal`` and ``_apply_precond`` are compiled from the
syntax tree of that file where it lies and run against the stand-ins of tests/golden/make_golden_templates.py, which wrap
the observations of tests/gain_template_case.py.  Nothing of the reference's text is copied; the fixture stores only
numbers: amplitude layout, preconditioners, the results of the three operations, and -- for the bounds of the tests -- the
exactly summed projection with the magnitude of its terms.

Every case is ONE observation with ``view=None``: the only configuration in which the reference is consistent with itself
(see toast_amd/templates/gaintemplate.py).

Per case the generator prints how far the reference's own results lie from exactly summed values, with the basis taken
from the three-term recurrence (``legendre_basis``; the reference's monomial evaluation of scipy.special.legendre differs
from it from order 2 on, and that difference is part of these figures):

    project   | ref - (PRESET + fsum_good fl(fl(est_i sig_i) T_k(r_i))) |  in  eps (PRESET + sum|terms|)
    inverse   | ref - G^-1 |, G = w sum_i fl(T_r est_i) fl(T_c est_i) and its inverse in exact rational arithmetic,
              in  eps cond(G) max|G^-1|
    add       | ref - (s_i + est_i sum_k T_k a_k) | in exact rational arithmetic,  in  eps (|s_i| + |est_i| sum_k |T_k a_k|)

One end-to-end case (``run_e2e``): amplitudes, right-hand side, flags and residual history of the reference's ``solve()``
over [Offset, GainTemplate], built like the end-to-end case of tests/golden/make_golden_templates.py.

Build container only.      python tests/golden/make_golden_gain_template.py
"""
import ast
import math
import os
import re
import sys
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import scipy
import scipy.special  # noqa: F401  (the reference asks for scipy.special.legendre)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gain_template_case as gc  # noqa: E402
import make_golden_templates as mt  # noqa: E402
import templates_case as tc  # noqa: E402
from toast_amd.templates.subharmonic import legendre_basis  # noqa: E402

METHODS = ("_initialize", "_get_polynomials", "_add_to_signal", "_project_signal", "_apply_precond")
EPS = np.finfo(np.float64).eps


def load_reference_gain():
    """A bare class holding the reference's methods of GainTemplate (the approach of mt.load_reference_class, with
    ``scipy`` in the namespace)."""
    path = os.path.join(mt.REF_DIR, "gaintemplate.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GainTemplate"]
    assert len(cls) == 1
    fns = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert len(fns) == len(METHODS)
    for fn in fns:
        fn.decorator_list = []
    holder = ast.ClassDef(name="GainTemplate", bases=[], keywords=[], body=fns, decorator_list=[])
    mod = ast.Module(body=[holder], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "re": re, "scipy": scipy, "OrderedDict": OrderedDict, "MPI": None}
    exec(compile(mod, path, "exec"), ns)
    return ns["GainTemplate"]


def invert_exact(g):
    """Inverse of a square matrix of Fractions by Gauss-Jordan elimination."""
    n = len(g)
    a = [list(row) + [Fraction(int(r == c)) for c in range(n)] for r, row in enumerate(g)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col] != 0)
        a[col], a[piv] = a[piv], a[col]
        p = a[col][col]
        a[col] = [x / p for x in a[col]]
        for r in range(n):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [x - f * y for x, y in zip(a[r], a[col])]
    return [row[n:] for row in a]


def exact_project(sig, est, good, basis):
    """-> (PRESET + exact sums, PRESET + sums of magnitudes) of fl(fl(est sig) T_k) over the good samples."""
    w = (est * sig)[good]
    exact, scale = [], []
    for k in range(basis.shape[0]):
        terms = w * basis[k][good]
        exact.append(math.fsum([gc.PRESET] + list(terms)))
        scale.append(gc.PRESET + np.abs(terms).sum())
    return exact, scale


def exact_inverse(est, basis, weight):
    u = [[Fraction(float(x)) for x in basis[k] * est] for k in range(basis.shape[0])]
    n = len(u)
    g = [[None] * n for _ in range(n)]
    for r in range(n):
        for c in range(r, n):
            g[r][c] = g[c][r] = Fraction(float(weight)) * sum(x * y for x, y in zip(u[r], u[c]))
    inv = invert_exact(g)
    return np.array([[float(x) for x in row] for row in g]), np.array([[float(x) for x in row] for row in inv])


def add_deviation(got, s0, est, basis, amp):
    """Largest | got - exact | / (eps (|s| + |est| sum|T_k a_k|)) over the samples, the exact value in rationals."""
    worst = 0.0
    fa = [Fraction(float(a)) for a in amp]
    for i in range(s0.size):
        gain = sum(Fraction(float(basis[k, i])) * fa[k] for k in range(len(fa)))
        exact = Fraction(float(s0[i])) + Fraction(float(est[i])) * gain
        scale = abs(s0[i]) + abs(est[i]) * sum(abs(basis[k, i] * amp[k]) for k in range(len(fa)))
        worst = max(worst, abs(float(Fraction(float(got[i])) - exact)) / (EPS * scale))
    return worst


def run_case(name, cls, blob):
    traits, det_flags = gc.template_traits(name)
    data = gc.build()
    t = mt.instance(cls, data, view=None, det_flags=det_flags, **traits)
    ob = data.obs[0]
    norder = t.order + 1
    dets = list(t._all_dets)
    blob[f"{name}_n_local"] = np.array(t._n_local)
    blob[f"{name}_det_start"] = np.array([t._det_start[d] for d in dets], dtype=np.int64)
    prec = np.array([t._precond[0][0][d] for d in dets])
    blob[f"{name}_precond"] = prec
    sig0 = ob.detdata[tc.DET_DATA].data.copy()
    est = ob.detdata[gc.ESTIMATE].data
    basis = legendre_basis(norder, ob.n_local_samples)
    # M^T d first (the signal is still the seeded one), accumulated onto PRESET; then d + M a
    proj = mt.Amp(t._n_local)
    proj.local[:] = gc.PRESET
    for det in dets:
        t._project_signal(det, proj)
    blob[f"{name}_project"] = proj.local.copy()
    exact, scale, f_proj, f_inv, cond_max = [], [], 0.0, 0.0, 0.0
    for k, det in enumerate(dets):
        good = np.ones(ob.n_local_samples, dtype=bool)
        if det_flags is not None:
            good = (ob.detdata[det_flags][det] & tc.DET_FLAG_MASK) == 0
        e, s = exact_project(sig0[k], est[k], good, basis)
        exact += e
        scale += s
        weight = 1.0 if t.noise_model is None else ob[t.noise_model].detector_weight(det)
        g, inv = exact_inverse(est[k], basis, weight)
        cond = np.linalg.cond(g)
        cond_max = max(cond_max, cond)
        f_inv = max(f_inv, np.abs(prec[k] - inv).max() / (EPS * cond * np.abs(inv).max()))
    exact, scale = np.array(exact), np.array(scale)
    f_proj = float((np.abs(proj.local - exact) / (EPS * scale)).max())
    blob[f"{name}_project_exact"] = exact
    blob[f"{name}_project_scale"] = scale
    amps = mt.Amp(t._n_local)
    amps.local[:] = tc.amplitudes(t._n_local, 1)
    for det in dets:
        t._add_to_signal(det, amps)
    added = ob.detdata[tc.DET_DATA].data.copy()
    blob[f"{name}_add_obs0"] = added
    f_add = max(add_deviation(added[k], sig0[k], est[k], basis, amps.local[k * norder:(k + 1) * norder])
                for k in range(len(dets)))
    out = mt.Amp(t._n_local)
    t._apply_precond(amps, out)
    blob[f"{name}_precond_out"] = out.local.copy()
    blob[f"{name}_figures"] = np.array([f_proj, f_inv, f_add, cond_max])
    print(f"{name}: order {t.order}, {t._n_local} amplitudes; the reference's deviation from the exact values: "
          f"project {f_proj:.2f} eps sum|terms|, inverse {f_inv:.2f} eps cond max|G^-1| (cond up to {cond_max:.1f}), "
          f"add {f_add:.2f} eps (|s| + |est| sum|T a|)")


def run_e2e(cls, blob):
    """``solve()`` of the reference over [Offset, GainTemplate]: the pieces of tests/golden/make_golden_mapmaker.py (the
    reference's compiled kernels in oracle/_ref, its ``solve()``, the operator order of SolveAmplitudes / SolverRHS /
    SolverLHS) with the NumPy template next to the offset kernels.  One whole-observation view; solver flags with mask
    255 for the binning and for both templates."""
    import make_golden_mapmaker as mg
    from toast_amd import synth
    from toast_amd.data import defaults

    ref = mg.ref
    data, cfg = gc.build_e2e()
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
    gain = mt.instance(cls, data, view=None, det_data="temp", det_flags="solver_flags", det_flag_mask=255,
                       order=cfg["order"], template_name=gc.ESTIMATE, noise_model=defaults.noise_model)

    def new_amps():
        return mg.AmpMap(baselines=mg.Amp(n_amp, amp_flags), gain=mg.Amp(gain._n_local, np.zeros(gain._n_local, np.uint8)))

    def template_add(amps):          # TemplateMatrix: template after template, detector after detector
        for d in range(n_det):
            ref.template_offset_add_to_signal(step, d * per_det, n_amp_views, amps["baselines"].local,
                                              amps["baselines"].local_flags, d, tod, ivl, False)
        for det in dets:
            gain._add_to_signal(det, amps["gain"])

    def template_project(amps):
        for d in range(n_det):
            ref.template_offset_project_signal(d, tod, d, solver_flags, 255, step, d * per_det, n_amp_views,
                                               amps["baselines"].local, amps["baselines"].local_flags, ivl, False)
        for det in dets:
            gain._project_signal(det, amps["gain"])

    def bin_map(cov):
        z = np.zeros((n_local, nps, nnz))
        ref.build_noise_weighted(g2l, z, idx, pixels, idx, weights, idx, tod, idx, solver_flags, detw, 255, ivl, sflags, 0, False)
        ref.cov_apply_diag(n_local, nps, nnz, cov, z.reshape(-1))
        return z

    def scan_subtract_weight(binned):
        ref.ops_scan_map_float64(g2l, nps, binned, tod, idx, pixels, idx, weights, idx, ivl, 1.0, False, True, False, False)
        ref.noise_weight(tod, idx, ivl, detw, False)

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
            gain._apply_precond(amps_in["gain"], amps_out["gain"])

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
    for name in gc.E2E_NAMES:
        blob[f"e2e_amplitudes_{name}"] = store["amplitudes"][name].local.copy()
        blob[f"e2e_rhs_{name}"] = rhs[name].local.copy()
        blob[f"e2e_flags_{name}"] = np.asarray(rhs[name].local_flags, dtype=np.uint8).copy()
    blob["e2e_history"] = history
    blob["e2e_injected"] = gc.e2e_injected(cfg)
    print(f"e2e: {n_det} x {n_samp}, nside {nside}: amplitudes {[store['amplitudes'][k].local.size for k in gc.E2E_NAMES]}, "
          f"residual {history[0]:.3e} -> {history[-1]:.3e}")
    print("e2e: injected gain amplitudes\n", gc.e2e_injected(cfg), "\n     recovered\n",
          store["amplitudes"]["gain"].local.reshape(n_det, -1))


def main():
    cls = load_reference_gain()
    blob = {}
    for name in gc.CASES:
        run_case(name, cls, blob)
    run_e2e(cls, blob)
    path = os.path.join(HERE, "gain_template.npz")
    np.savez_compressed(path, **blob)
    assert all(v.dtype != object for v in blob.values())
    print("gain_template.npz: %.3f MB" % (os.path.getsize(path) / 1e6))


if __name__ == "__main__":
    main()
