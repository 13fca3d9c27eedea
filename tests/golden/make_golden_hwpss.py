#!/usr/bin/env python3
"""Generate tests/golden/hwpss.npz from THE REFERENCE'S OWN code.  Build container only.

The functions hwpss_samples, hwpss_sincos_buffer, hwpss_compute_coeff_covariance, hwpss_compute_coeff and
hwpss_build_model of the reference's src/toast/hwp_utils.py and the methods of HWPSynchronousModel
(src/toast/ops/hwpss_model.py) are taken out of their files with ``ast`` and executed here on stand-in containers: units
equal to 1, no communicators, a logger and a timer that do nothing.  Nothing of the reference is copied into the
repository, and the fixture stores outputs only (the inputs come from the seeds of tests/hwpss_case.py).

Per case the file stores

* the reference's integer outputs, compared bit for bit: good counts, coeff_flags, sample flags, detector flags, the cut;
* long-double evaluations (tests/hwpss_case.py) of the Gram matrices, right-hand sides, coefficients, cleaned signal and
  relative calibrations, rounded to double: what both paths of the operator are compared with;
* ``ref_err_*``: how far the reference's own doubles are from those, in units of eps * scale, scale = sum |terms| (for the
  coefficients: cond * max |coefficient| of the chunk);
* the conditions that keep the comparison honest: every chunk's rcond and condition number, the knot count of every
  spline, the smallest distance of a good-sample count from n_coeff.

For the chunked cases the long-double model uses the reference's own splines (FITPACK runs in double only); ``lebesgue``
is the largest sum of |cardinal functions| of the least-squares spline on the knots FITPACK chose, over the observation:
the factor by which a coefficient error of the chunks can grow in the interpolated coefficients.

    python tests/golden/make_golden_hwpss.py
"""
import ast
import os
import sys
import types

import numpy as np
import scipy
import scipy.interpolate
from scipy.linalg import eigvalsh, lu_factor, lu_solve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF_OP = "/root/reference/src/toast/ops/hwpss_model.py"
REF_UTIL = "/root/reference/src/toast/hwp_utils.py"

import hwpss_case as hc  # noqa: E402

L = np.longdouble


class Q(float):
    """A quantity whose unit is 1."""

    def to_value(self, unit=None):
        return float(self)


class Quiet:
    """Logger, timer and environment: every method does nothing."""

    @classmethod
    def get(cls):
        return cls()

    def __getattr__(self, name):
        return lambda *a, **k: None


class DetData:
    """detdata[name]: rows by detector name, ``[det, slice]``, ``[:, :]``."""

    def __init__(self, dets, n, dtype):
        self.dets = list(dets)
        self.arr = np.zeros((len(dets), n), dtype=dtype)
        self.units = 1.0

    def _key(self, key):
        if isinstance(key, tuple):
            first = key[0] if isinstance(key[0], slice) else self.dets.index(key[0])
            return (first,) + tuple(key[1:])
        return self.dets.index(key)

    def __getitem__(self, key):
        return self.arr[self._key(key)]

    def __setitem__(self, key, value):
        self.arr[self._key(key)] = value


class DetDataManager(dict):
    def ensure(self, name, dtype=np.float64, create_units=None, **kw):
        if name not in self:
            self[name] = DetData(self.dets, self.n, dtype)


class Obs(dict):
    is_distributed_by_detector = True
    comm_col = None
    comm_col_rank = 0

    def __init__(self, case, G):
        super().__init__()
        spec = hc.CASES[case]
        n_det = spec["n_det"]
        self.name = "obs_" + case
        self.local_detectors = hc.det_names(n_det)
        self.local_detector_flags = {d: 0 for d in self.local_detectors}
        self.n_local_samples = hc.N
        self.comm = types.SimpleNamespace(comm_group=None)
        self.telescope = types.SimpleNamespace(focalplane=types.SimpleNamespace(sample_rate=Q(hc.RATE)))
        self.shared = {"times": types.SimpleNamespace(data=G["times"]), "hwp_angle": types.SimpleNamespace(data=G["angle"]),
                       "flags": types.SimpleNamespace(data=np.array(G["shared_flags"]))}
        self.detdata = DetDataManager()
        self.detdata.dets, self.detdata.n = self.local_detectors, hc.N
        self.detdata["signal"] = DetData(self.local_detectors, hc.N, np.float64)
        self.detdata["signal"].arr[:] = G["signal"]
        self.detdata["flags"] = DetData(self.local_detectors, hc.N, np.uint8)
        self.detdata["flags"].arr[:] = G["det_flags"]
        # det_flags=None: the reference still ORs into detdata[None]; a row set nobody reads
        self.detdata[None] = DetData(self.local_detectors, hc.N, np.uint8)
        self.intervals = {}
        if "view" in spec:
            self.intervals["chunks"] = [types.SimpleNamespace(first=a, last=b) for a, b in spec["view"]]

    def update_local_detector_flags(self, flags):
        self.local_detector_flags.update(flags)

    def select_local_detectors(self, flagmask=0):
        return [d for d in self.local_detectors if not (self.local_detector_flags[d] & flagmask)]


def reference(record):
    """Namespace with the reference's functions and the operator's methods; ``record`` collects what the solves see."""
    def rec_lu_factor(cov):
        record["cov"].append(np.array(cov))
        return lu_factor(cov)

    def rec_lu_solve(lu, rhs):
        record["rhs"].append(np.array(rhs))
        return lu_solve(lu, rhs)

    def rec_eigvalsh(cov):
        ev = eigvalsh(cov)
        record["evals"].append((float(np.min(ev)), float(np.max(ev))))
        return ev

    def rec_splrep(x, y, s=None):
        tck = scipy.interpolate.splrep(x, y, s=s)
        record["tck"].append(tck)
        record["spl_x"].append(np.array(x))
        return tck

    fake_scipy = types.SimpleNamespace(interpolate=types.SimpleNamespace(splrep=rec_splrep, splev=scipy.interpolate.splev))
    unit = types.SimpleNamespace(Hz=1.0, second=1.0)
    ns = {"np": np, "scipy": fake_scipy, "u": unit, "os": os, "eigvalsh": rec_eigvalsh, "lu_factor": rec_lu_factor,
          "lu_solve": rec_lu_solve, "MPI": None, "Logger": Quiet, "Timer": Quiet, "Environment": Quiet,
          "flatten": lambda x: x}
    util = ast.parse(open(REF_UTIL).read())
    for node in util.body:
        if isinstance(node, ast.FunctionDef) and node.name in (
                "hwpss_samples", "hwpss_sincos_buffer", "hwpss_compute_coeff_covariance", "hwpss_compute_coeff",
                "hwpss_build_model"):
            node.decorator_list = []
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), REF_UTIL, "exec"), ns)
    methods = []
    for node in ast.parse(open(REF_OP).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == "HWPSynchronousModel":
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and not fn.name.startswith("_check") and fn.name != "__init__":
                    fn.decorator_list = []
                    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), REF_OP, "exec"), ns)
                    methods.append(fn.name)
    return ns, methods


def holder(ns, methods, traits):
    base = dict(times="times", det_data="signal", det_mask=1, shared_flags="flags", shared_flag_mask=1, det_flags="flags",
                det_flag_mask=1, hwp_flag_mask=1, hwp_angle="hwp_angle", harmonics=9, subtract_model=False, save_model=None,
                chunk_view=None, chunk_time=None, relcal_fixed=None, relcal_continuous=None, relcal_cut_sigma=5.0,
                time_drift=False, fill_gaps=False, debug=None)
    base.update(traits)
    if base["chunk_time"] is not None:
        base["chunk_time"] = Q(base["chunk_time"])
    h = types.SimpleNamespace(**base)
    for name in methods:
        setattr(h, name, types.MethodType(ns[name], h))
    return h


def lebesgue(x, t, reltime):
    """max over the observation of sum_j |l_j|: l_j the least-squares cubic spline on the knots t through the unit
    vector e_j at x."""
    total = np.zeros(len(reltime))
    for j in range(len(x)):
        e = np.zeros(len(x))
        e[j] = 1.0
        if len(t) == len(x) + 4:
            spl = scipy.interpolate.make_interp_spline(x, e, k=3, t=t)
        else:
            spl = scipy.interpolate.make_lsq_spline(x, e, t, k=3)
        total += np.abs(spl(reltime, extrapolate=True))
    return float(np.max(total))


def main():
    record = {"cov": [], "rhs": [], "evals": [], "tck": [], "spl_x": []}
    ns, methods = reference(record)
    out = {}
    for case, spec in hc.CASES.items():
        for v in record.values():
            del v[:]
        G = hc.make_inputs(case)
        ob = Obs(case, G)
        op = holder(ns, methods, spec["op"])
        data = types.SimpleNamespace(obs=[ob], comm=types.SimpleNamespace(comm_group=None, world_rank=0, comm_world=None))
        with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
            __import__("warnings").simplefilter("ignore")
            op._exec(data)
        H, drift = op.harmonics, op.time_drift
        n_coeff = (4 if drift else 2) * H
        n_det = spec["n_det"]
        dets = ob.local_detectors

        # what the reference worked with
        reltime = G["times"] - G["times"][0]
        chunks = op._compute_chunking(ob, reltime)
        starts = np.array([c["start"] for c in chunks], dtype=np.int64)
        ends = np.array([c["end"] for c in chunks], dtype=np.int64)
        ob0 = Obs(case, G)                  # the flags before the run
        shared, det_fv = op._compute_flags(ob0, dets)
        fv = np.array([det_fv[d] for d in dets])
        P = f"{case}_"
        out[P + "starts"], out[P + "ends"] = starts, ends
        out[P + "chunk_times"] = np.array([c["time"] for c in chunks])
        out[P + "shared"] = shared

        basis = hc.basis_ld(G["angle"], reltime, shared, H, drift)
        fit = hc.fit_ld(basis, shared, fv, G["signal"], starts, ends)

        # chunk flags, conditions; the recorded matrices belong to the chunks that reached eigvalsh / lu_factor
        coeff_flags = np.zeros(len(chunks), dtype=np.uint8)
        rcond = np.full(len(chunks), np.nan)
        cond = np.full(len(chunks), np.nan)
        ev = iter(record["evals"])
        cov = iter(record["cov"])
        rhs = iter(record["rhs"])
        err_gram = err_rhs = 0.0
        min_count_distance = 10 ** 9
        for c in range(len(chunks)):
            n = hc.chunk_length(starts[c], ends[c])
            if fit["n_good_shared"][c] == 0:
                coeff_flags[c] = 1
                continue
            lo, hi = next(ev)
            rcond[c] = lo / hi
            assert rcond[c] >= 1e-6 or rcond[c] <= 1e-10, (case, c, rcond[c])
            if rcond[c] < 1e-8:
                coeff_flags[c] = 1
                continue
            cond[c] = hi / lo
            scale = float(n) / float(fit["n_good_shared"][c])
            got = next(cov)
            err_gram = max(err_gram, hc.units(np.triu(got) - np.triu(fit["gram"][c]) * L(scale),
                                              np.triu(fit["gram_scale"][c]) * L(scale)))
            for d in range(n_det):
                cnt = int(fit["n_good"][d, c])
                if case != "chunks" or (d, c) != (1, 0):
                    min_count_distance = min(min_count_distance, abs(cnt - n_coeff), abs(cnt - (n_coeff - 1)))
                if cnt < n_coeff:
                    continue
                err_rhs = max(err_rhs, hc.units(next(rhs) - fit["rhs"][d, c], fit["rhs_scale"][d, c]))
        assert next(cov, None) is None and next(rhs, None) is None and next(ev, None) is None
        assert min_count_distance > 0, case
        out[P + "coeff_flags"], out[P + "rcond"], out[P + "cond"] = coeff_flags, rcond, cond
        out[P + "min_count_distance"] = min_count_distance
        out[P + "n_good"], out[P + "n_good_shared"] = fit["n_good"], fit["n_good_shared"]
        out[P + "gram"] = np.array([np.triu(g) for g in fit["gram"]], dtype=np.float64).reshape(len(chunks), n_coeff, n_coeff)
        out[P + "rhs"] = fit["rhs"].astype(np.float64)
        out[P + "mean"] = fit["mean"].astype(np.float64)
        out[P + "ref_err_gram"], out[P + "ref_err_rhs"] = err_gram, err_rhs

        # coefficients: the reference's (through save_model or recomputed) against extended precision
        exact = hc.coeff_ld(fit, starts, ends, coeff_flags)
        out[P + "coeff"] = exact.astype(np.float64)
        if op.save_model is not None:
            ref_coeff = np.array([[ob[op.save_model][c]["dets"][d] for c in range(len(chunks))] for d in dets])
            ref_coeff = np.transpose(ref_coeff, (0, 2, 1))
            assert [int(m["flag"]) for m in ob[op.save_model]] == list(coeff_flags)
            err = 0.0
            for c in range(len(chunks)):
                if not coeff_flags[c]:
                    for d in range(n_det):
                        err = max(err, hc.units(ref_coeff[d, :, c] - exact[d, :, c],
                                                np.full(n_coeff, cond[c] * float(np.max(np.abs(exact[d, :, c]))))))
            out[P + "ref_err_coeff"] = err

        # detector flags and the cut
        out[P + "detector_flags"] = np.array([ob.local_detector_flags[d] for d in dets], dtype=np.int64)
        out[P + "sample_flags"] = ob.detdata["flags"].arr if op.det_flags is not None else np.zeros(0, dtype=np.uint8)
        if case == "cut":
            assert list(out[P + "detector_flags"]) == [0, 0, 0, 0, 0, 1], out[P + "detector_flags"]

        # cleaned signal
        active = [d for d in range(n_det) if ob.local_detector_flags[dets[d]] == 0]
        err_clean = 0.0
        clean = np.array(G["signal"])
        knots = []
        leb = 1.0
        tck = iter(record["tck"])
        spx = iter(record["spl_x"])
        for d in active:
            if len(chunks) == 1:
                cts = exact[d, :, 0]
            else:
                cts = np.zeros((hc.N, n_coeff))
                for k in range(n_coeff):
                    spl, x = next(tck), next(spx)
                    knots.append(len(spl[0]))
                    assert len(spl[0]) in (8, len(x) + 4), (case, d, k, len(spl[0]))
                    cts[:, k] = scipy.interpolate.splev(reltime, spl, ext=0)
                    if k == 0:
                        leb = max(leb, lebesgue(x, spl[0], reltime))
            y, scale = hc.cleaned_ld(G["signal"][d], fv[d], basis, cts)
            good = fv[d] == 0
            err_clean = max(err_clean, hc.units(ob.detdata["signal"].arr[d][good] - y[good], scale[good]))
            clean[d] = y.astype(np.float64)
        out[P + "cleaned"] = clean
        out[P + "ref_err_clean"] = err_clean
        out[P + "knots"] = np.array(knots, dtype=np.int64)
        out[P + "lebesgue"] = leb
        for d in range(n_det):
            if d not in active:           # a flagged detector's data is untouched
                assert np.array_equal(ob.detdata["signal"].arr[d], G["signal"][d], equal_nan=True)

        # relative calibrations: the reference's own values (their error follows the coefficients')
        if op.relcal_fixed is not None:
            out[P + "relcal"] = np.array([ob[op.relcal_fixed].get(d, np.nan) for d in dets])
        if op.relcal_continuous is not None and "compare" not in spec:
            out[P + "relcal_ts"] = ob.detdata[op.relcal_continuous].arr
        if case == "chunks":
            out[P + "last_end_past_n_samp"] = bool(ends[-1] > hc.N)
        print(f"{case:11s} chunks {len(chunks)} flagged {list(np.flatnonzero(coeff_flags))} rcond {np.nanmin(rcond):.1e} "
              f"cond {np.nanmax(cond):.1e} ref_err gram {err_gram:.1f} rhs {err_rhs:.1f} coeff "
              f"{out.get(P + 'ref_err_coeff', float('nan')):.2f} clean {err_clean:.1f} knots {sorted(set(knots))} "
              f"lebesgue {leb:.2f} detflags {list(out[P + 'detector_flags'])}")

    np.savez_compressed(hc.GOLD_PATH, **out)
    print(f"{hc.GOLD_PATH}: {os.path.getsize(hc.GOLD_PATH)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
