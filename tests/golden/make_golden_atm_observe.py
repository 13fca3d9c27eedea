#!/usr/bin/env python3
"""Generate tests/golden/atm_observe.npz from THE REFERENCE'S OWN code.  Build container only.

toast::atm_sim_observe: the reference's toast_atm_observe.cpp, toast_atm.cpp, toast_sys_utils.cpp,
toast_sys_environment.cpp and its generated version.cpp are compiled IN PLACE from the reference tree with
``g++ -O2 -fopenmp -DHAVE_CHOLMOD`` into a temporary directory outside the repository, together with
toast_math_qarray.cpp / toast_math_sf.cpp for qa_to_angles.  This script writes into that directory a stand-in
``cholmod.h`` (two structs, CHOLMOD_INT, no-op cholmod_start / cholmod_finish: observation never calls CHOLMOD) and an
``extern "C"`` shim around the two functions, called through ctypes.  Nothing compiled and no reference text enters
the repository.

ObserveAtmosphere: ``_exec`` and ``_std_range`` are taken out of src/toast/ops/sim_tod_atm_observe.py with ``ast`` and
run on plain stand-in containers whose ``cur_sim.observe`` calls the shim and whose ``qa.to_iso_angles`` calls the
reference's qa_to_angles.

Inputs come from tests/atm_observe_case.py and are regenerated from seeds there; the fixture stores outputs only.
Next to the reference's outputs it stores, per case,

* ``ld_hi / ld_lo``  a long-double evaluation of the same chain (two doubles per sample), ``scale``
  (xstep T0 sum_steps max|corner values| |1 - z / zatm|, plus |tod before| where tod was pre-filled),
* ``ref_dev``        the reference's own deviation from it, max over samples, in units of eps * scale_i,

and the conditions that keep the comparison honest, checked here and asserted by the host test:

* ``face``    every step point of every ray, evaluated in long double, lies at least 1e-9 cell widths from every cell
              face (a point on a grid plane makes the reference's fractional-step check fire on rounding alone);
* ``cell0``   no ray enters cell (0, 0, 0): the reference's per-thread cache (last_ind, last_nodes) starts as that cell
              with ZERO node values and would return 0 there, the device reads the real values;
* ``failed``  in the cases with holes at least one sample and at most a quarter of the samples fail.

The flags of the operator case: the reference's statement ``det_flags[vw][det][good][bad] |= mask``
(sim_tod_atm_observe.py:396-398) writes into the COPY that the boolean index ``[good]`` makes, so the flag bytes it
leaves are the ones it found (stored as ``op_flags_asrun``; the host test asserts that they equal the input).  What the
statement is there to do -- raise the mask on the good samples whose atmosphere is still zero after a failed slab -- is
stored as ``op_flags``: computed from the reference's own per-slab ``atmdata`` (recorded by the stand-in
``cur_sim.observe``) with the reference's threshold, and checked against the count ``nbad`` that the reference logs.

    python tests/golden/make_golden_atm_observe.py
"""
import ast
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
REF_OP = REF + "/src/toast/ops/sim_tod_atm_observe.py"

import atm_observe_case as ac  # noqa: E402

L = np.longdouble

CHOLMOD_H = """#pragma once
typedef struct cholmod_common_struct { int itype, print, final_ll; } cholmod_common;
typedef struct cholmod_sparse_struct { int n; } cholmod_sparse;
#define CHOLMOD_INT 0
static inline int cholmod_start(cholmod_common * c) { (void)c; return 1; }
static inline int cholmod_finish(cholmod_common * c) { (void)c; return 1; }
"""

SHIM = """#include <cstddef>
#include <cstdint>
#include <toast/sys_utils.hpp>
#include <toast/atm.hpp>
#include <toast/math_qarray.hpp>
extern "C" int shim_atm_sim_observe(
    long nsamp, double * times, double * az, double * el, double * tod, double * g, long * n,
    long * compressed_index, long * full_index, double * realization) {
    return toast::atm_sim_observe(
        (size_t)nsamp, times, az, el, tod, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11],
        g[12], g[13], g[14], g[15], g[16], g[17], g[18], g[19], g[20], g[21], g[22], g[23], g[24],
        n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], (int64_t *)compressed_index, (int64_t *)full_index, realization);
}
extern "C" void shim_qa_to_angles(long n, double const * quat, double * theta, double * phi, double * pa) {
    toast::qa_to_angles((size_t)n, quat, theta, phi, pa, false);
}
"""

GEOM_ORDER = ("T0", "azmin", "azmax", "elmin", "elmax", "tmin", "tmax", "rmin", "rmax", "fixed_r", "zatm", "zmax", "wx",
              "wy", "wz", "xstep", "ystep", "zstep", "xstart", "delta_x", "ystart", "delta_y", "zstart", "delta_z",
              "maxdist")


def build_reference(tmp):
    src = REF + "/src/libtoast"
    open(os.path.join(tmp, "cholmod.h"), "w").write(CHOLMOD_H)
    open(os.path.join(tmp, "shim.cpp"), "w").write(SHIM)
    subprocess.check_call(["sh", src + "/generate_version_cpp.sh", "golden-atm"], cwd=tmp, stdout=subprocess.DEVNULL)
    lib = os.path.join(tmp, "libatmref.so")
    files = [src + "/src/" + f for f in ("toast_atm_observe.cpp", "toast_atm.cpp", "toast_sys_utils.cpp",
                                         "toast_sys_environment.cpp", "toast_math_qarray.cpp", "toast_math_sf.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-fopenmp", "-fPIC", "-shared", "-DHAVE_CHOLMOD", "-I" + tmp,
                           "-I" + src + "/include", os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "version.cpp")]
                          + files + ["-o", lib])
    return C.CDLL(lib)


def ref_observe(lib, vol, times, az, el, tod, fixed_r):
    geom, ci, fi, rz = vol
    g = np.array([dict(geom, fixed_r=fixed_r)[k] for k in GEOM_ORDER], dtype=np.float64)
    n = np.array([ci.size, geom["nx"], geom["ny"], geom["nz"], geom["ny"] * geom["nz"], geom["nz"], 1, rz.size],
                 dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for a in (times, az, el, tod):
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return int(lib.shim_atm_sim_observe(C.c_long(times.size), p(times), p(az), p(el), p(tod), p(g), p(n), p(ci), p(fi),
                                        p(rz)))


def kernel_cases(lib, out):
    for name, spec in ac.CASES.items():
        fixed_r = spec.get("fixed_r", -1.0)
        times, az, el, tod0 = ac.pointing(name)
        tod = tod0.copy()
        want = tod0.astype(L)
        scale = np.abs(tod0) if spec.get("prefill") else np.zeros(times.size)
        statuses, failed_any, face, cell0 = [], np.zeros(times.size, dtype=bool), np.inf, False
        vols = ac.case_volumes(name)
        for k, vol in enumerate(vols):
            before = tod.copy()
            statuses.append(ref_observe(lib, vol, times, az, el, tod, fixed_r))
            ld = ac.longdouble_observe(vol, times, az, el, fixed_r)
            want = want + ld["val"]
            scale = scale + ld["scale"]
            face, cell0 = min(face, ld["face"]), cell0 or ld["cell0"]
            untouched = tod.view(np.uint64) == before.view(np.uint64)
            # the reference leaves exactly the skipped and the failed samples as they were
            assert np.array_equal(untouched, ld["skip"] | ld["failed"]), name
            out[f"{name}_failed{k}"] = ld["failed"]
            out[f"{name}_skip{k}"] = ld["skip"]
            failed_any |= ld["failed"]
        assert face >= 1e-9, (name, face)
        assert not cell0, name
        if name in ac.HOLE_CASES:
            assert 1 <= failed_any.sum() <= times.size // 4, (name, failed_any.sum())
        else:
            assert failed_any.sum() == 0, name
        hi, lo = ac.split(want)
        dev = ac.deviation(tod, want, scale)
        out[f"{name}_tod"], out[f"{name}_status"] = tod, np.array(statuses, dtype=np.int64)
        out[f"{name}_ld_hi"], out[f"{name}_ld_lo"], out[f"{name}_scale"] = hi, lo, scale
        out[f"{name}_ref_dev"], out[f"{name}_face"], out[f"{name}_cell0"] = dev, face, cell0
        print(f"{name:12s} status {statuses} failed {int(failed_any.sum()):3d} / {times.size:3d}  face {face:.2e}  "
              f"ref_dev {dev:.3f}")


# ------------------------------------------------------------------------------------------------ operator
class Recorder:
    def __init__(self):
        self.errors = []

    def error(self, msg):
        self.errors.append(msg)

    def warning(self, msg):
        pass


def reference_operator(lib, log):
    """A holder with the reference's _exec and _std_range as methods."""
    tree = ast.parse(open(REF_OP).read())
    timers = types.SimpleNamespace(start=lambda *a: None, stop=lambda *a: None)

    def to_iso_angles(q):
        q = np.ascontiguousarray(q, dtype=np.float64)
        n = q.shape[0]
        theta, phi, pa = np.zeros(n), np.zeros(n), np.zeros(n)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        lib.shim_qa_to_angles(C.c_long(n), p(q), p(theta), p(phi), p(pa))
        return theta, phi, pa

    ns = {"np": np, "u": types.SimpleNamespace(K=1.0, Hz=1.0, s=1.0),
          "qa": types.SimpleNamespace(to_iso_angles=to_iso_angles),
          "Environment": types.SimpleNamespace(get=lambda: None),
          "Logger": types.SimpleNamespace(get=lambda: log),
          "GlobalTimers": types.SimpleNamespace(get=lambda: timers),
          "unit_conversion": lambda a, b: ac.OP["scale"]}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == "ObserveAtmosphere":
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name in ("_exec", "_std_range"):
                    fn.decorator_list = []
                    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), REF_OP, "exec"), ns)
    return ns


class Views:
    """``ob.view[name]``: per-view slices of the shared and detector arrays."""

    def __init__(self, spans, shared, detdata):
        self._spans = spans
        self.shared = {k: [v[a:b] for a, b in spans] for k, v in shared.items()}
        self.detdata = {k: [{d: v[i, a:b] for i, d in enumerate(ac.OP_DETS)} for a, b in spans]
                        for k, v in detdata.items()}
        for k, v in detdata.items():
            if k == "signal":
                # det_data[vw][det, good]
                self.detdata[k] = [DetView(v[:, a:b]) for a, b in spans]

    def __len__(self):
        return len(self._spans)


class DetView:
    def __init__(self, arr):
        self.arr = arr

    def __getitem__(self, key):
        if isinstance(key, tuple):
            return self.arr[(ac.OP_DETS.index(key[0]),) + key[1:]]
        return self.arr[ac.OP_DETS.index(key)]

    def __setitem__(self, key, value):
        self.arr[(ac.OP_DETS.index(key[0]),) + key[1:]] = value


def operator_case(lib, out):
    log = Recorder()
    ns = reference_operator(lib, log)
    inp = ac.operator_inputs()
    signal, flags = inp["signal"].copy(), inp["det_flags"].copy()
    shared = {"times": inp["times"], "flags": inp["shared_flags"]}
    detdata = {"signal": signal, "flags": flags, "quats_azel": inp["quats"], "weights": inp["weights"]}
    views = Views(ac.OP_VIEWS, shared, detdata)
    record = []      # (view, atmdata after the slab, status) in call order

    class Sim:
        def __init__(self, vol, view):
            self.vol, self.view = vol, view
            g = vol[0]
            self.azmin, self.azmax, self.elmin, self.elmax, self.tmin, self.tmax = (
                g["azmin"], g["azmax"], g["elmin"], g["elmax"], g["tmin"], g["tmax"])

        def observe(self, times, az, el, tod, fixed_r):
            t, a, e = (np.ascontiguousarray(x, dtype=np.float64) for x in (times, az, el))
            st = ref_observe(lib, self.vol, t, a, e, tod, fixed_r)
            record.append((self.view, tod.copy(), st))
            return st

    sims = [[Sim(ac.volume(kind), v) for kind in kinds] for v, kinds in enumerate(ac.OP_SLABS)]
    class DetData(dict):
        def ensure(self, *a, **k):
            return True

    ob = types.SimpleNamespace(
        name="obs", session=types.SimpleNamespace(name="session"),
        select_local_detectors=lambda sel, flagmask=0: list(ac.OP_DETS),
        detdata=DetData(signal=types.SimpleNamespace(units=1.0)), view={None: views, "wind": views})
    data = {"atm_sim": {"session": sims}}

    class Data(dict):
        pass

    data = Data(data)
    data.obs = [ob]
    data.comm = types.SimpleNamespace(comm_group=None, group=0, group_rank=0)
    holder = types.SimpleNamespace(
        absorption="absorption", loading="loading", det_mask=1, det_data="signal", det_data_units=1.0, view=None,
        wind_view="wind", det_flags="flags", quats_azel="quats_azel", weights="weights", weights_mode="IQU",
        times="times", shared_flags="flags", shared_flag_mask=ac.OP["shared_flag_mask"],
        det_flag_mask=ac.OP["det_flag_mask"], sim="atm_sim", sample_rate=None, debug_tod=False, gain=ac.OP["gain"],
        fade_time=None, polarization_fraction=ac.OP["polarization_fraction"],
        _detector_absorption_and_loading=lambda ob_, a, l, dets: (ac.OP["absorption"], ac.OP["loading"]),
        _std_range=ns["_std_range"])
    ns["_exec"](holder, data)

    # what :379-399 is there to do, from the reference's own per-slab atmdata (module docstring)
    expected = inp["det_flags"].copy()
    calls = iter(record)
    n_bad = []
    for v, (a, b) in enumerate(ac.OP_VIEWS):
        sh = inp["shared_flags"][a:b] & ac.OP["shared_flag_mask"]
        for d in range(len(ac.OP_DETS)):
            good = ((inp["det_flags"][d, a:b] & ac.OP["det_flag_mask"]) | sh) == 0
            for _ in ac.OP_SLABS[v]:
                view, atm, st = next(calls)
                assert view == v and atm.size == good.sum()
                if st != 0:
                    bad = np.abs(atm) < 1e-30
                    n_bad.append(int(bad.sum()))
                    row = expected[d, a:b]
                    idx = np.nonzero(good)[0][bad]
                    row[idx] |= ac.OP["det_flag_mask"]
    logged = [int(re.search(r"failed for (\d+) ", m).group(1)) for m in log.errors if "ObserveAtmosphere failed for" in m]
    assert logged == n_bad, (logged, n_bad)
    assert sum(n_bad) > 0, "the operator case raises no flag"
    assert np.array_equal(flags, inp["det_flags"]), "the reference changed flag bytes after all: store those"
    out["op_signal"] = signal
    out["op_flags_asrun"] = flags
    out["op_flags"] = expected
    out["op_status"] = np.array([st for _, _, st in record], dtype=np.int64)
    out["op_nbad"] = np.array(n_bad, dtype=np.int64)

    # the long-double value of the chain for the tolerance of the values: atm from the kernel cases' evaluation with the
    # reference's az / el (the angles are inputs of the chain here), then :424-483 in long double
    want = inp["signal"].astype(L)
    scale = np.abs(inp["signal"]).astype(L)
    to_iso = ns["qa"].to_iso_angles
    for v, (a, b) in enumerate(ac.OP_VIEWS):
        sh = inp["shared_flags"][a:b] & ac.OP["shared_flag_mask"]
        for d, det in enumerate(ac.OP_DETS):
            good = ((inp["det_flags"][d, a:b] & ac.OP["det_flag_mask"]) | sh) == 0
            theta, phi, _ = to_iso(inp["quats"][d, a:b][good])
            az, el = 2 * np.pi - phi, np.pi / 2 - theta
            atm, sc = np.zeros(good.sum(), dtype=L), np.zeros(good.sum(), dtype=L)
            for kind in ac.OP_SLABS[v]:
                ld = ac.longdouble_observe(ac.volume(kind), inp["times"][a:b][good], az, el)
                assert ld["face"] >= 1e-9 and not ld["cell0"]
                atm, sc = atm + ld["val"], sc + ld["scale"].astype(L)
            w = inp["weights"][d, a:b][good].astype(L)
            pol = w[:, 0] + w[:, 1] * L(ac.OP["polarization_fraction"])
            ga = L(ac.OP["gain"]) * L(ac.OP["absorption"][det])
            load = L(ac.OP["loading"][det]) / np.sin(el.astype(L))
            idx = a + np.nonzero(good)[0]
            want[d, idx] += L(ac.OP["scale"]) * (atm * ga * pol + load)
            scale[d, idx] += L(ac.OP["scale"]) * (sc * abs(ga) * np.abs(pol) + np.abs(load))
    hi, lo = ac.split(want.reshape(-1))
    out["op_ld_hi"], out["op_ld_lo"] = hi.reshape(want.shape), lo.reshape(want.shape)
    out["op_scale"] = scale.astype(np.float64)
    out["op_ref_dev"] = ac.deviation(signal.reshape(-1), want.reshape(-1), out["op_scale"].reshape(-1))
    print(f"operator: statuses {out['op_status'].tolist()} nbad {n_bad} ref_dev {out['op_ref_dev']:.3f}")


def main():
    out = {}
    with tempfile.TemporaryDirectory(prefix="golden_atm_") as tmp:
        lib = build_reference(tmp)
        kernel_cases(lib, out)
        operator_case(lib, out)
    np.savez_compressed(ac.GOLD_PATH, **out)
    print(f"{ac.GOLD_PATH}: {os.path.getsize(ac.GOLD_PATH)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
