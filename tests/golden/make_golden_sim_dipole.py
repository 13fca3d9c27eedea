#!/usr/bin/env python3
"""Generate tests/golden/sim_dipole.npz from THE REFERENCE'S OWN code.  Build container only.

The reference's ``dipole`` (src/toast/dipole.py) and ``array_dot`` (src/toast/utils.py) are taken out of their files with
``ast`` and executed here.  astropy and healpy are absent: a stand-in units namespace in which every unit is 1 replaces
the first (quantities are floats whose ``to_value`` returns themselves), ``scipy.constants`` is the real one, and
``qa.rotate`` / ``qa.mult`` are this repository's NumPy restatements of toast_math_qarray.cpp (tests/sim_dipole_case.py
``rotate``, ``synth.quat_mult``).  Nothing of the reference is copied into the repository.

The inputs come from tests/sim_dipole_case.py and are stored, so that the fixture also pins them.  Next to the
reference's outputs the file stores ``err_<case>``: how far they are from a long-double evaluation of the same formulas,
in units eps * scale (scale = cmb for freq 0, cmb * max(beta) otherwise) -- the reference's own error, which sets the
tests' allowance.

    python tests/golden/make_golden_sim_dipole.py
"""
import ast
import os
import sys
import types

import numpy as np
import scipy.constants

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF_DIPOLE = "/root/reference/src/toast/dipole.py"
REF_UTILS = "/root/reference/src/toast/utils.py"

import sim_dipole_case as sc  # noqa: E402
from toast_amd import synth  # noqa: E402


class Q(float):
    """A quantity whose unit is 1."""

    def to_value(self, unit=None):
        return float(self)

    def __mul__(self, other):
        return Q(float(self) * other)

    __rmul__ = __mul__


def function(path, name, ns):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            node.decorator_list = []
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), path, "exec"), ns)
            return ns[name]
    raise RuntimeError(f"{path} has no function {name}")


def reference():
    unit = types.SimpleNamespace(Kelvin=Q(1.0), Hz=Q(1.0), K=Q(1.0))
    ns = {"np": np, "constants": scipy.constants, "u": unit, "t_cmb": Q(sc.dp.t_cmb),
          "qa": types.SimpleNamespace(rotate=sc.rotate, mult=synth.quat_mult)}
    function(REF_UTILS, "array_dot", ns)
    return function(REF_DIPOLE, "dipole", ns)


def main():
    ref_dipole = reference()
    inp = sc.inputs()
    out = {k: inp[k] for k in ("bore", "fp", "vel", "solar", "flags", "noise")}
    out["cmb"] = np.float64(inp["cmb"])
    assert scipy.constants.h == sc.dp.PLANCK_H and scipy.constants.k == sc.dp.BOLTZMANN_K
    assert scipy.constants.speed_of_light == sc.dp.SPEED_OF_LIGHT
    for case in sc.CASES:
        mode, freq = sc.case_parts(case)
        vel, solar = sc.velocities(inp, mode)
        scale = sc.case_scale(inp, case)
        worst = 0.0
        for mask, n_det, key in ((1, sc.case_dets(case), "ref_"), (0, sc.N_SMALL, "ref0_")):
            rows = np.zeros((n_det, sc.N))
            for d in range(n_det):
                quats = sc.pointing(inp, d, mask)
                rows[d] = ref_dipole(quats, vel=None if vel is None else vel.copy(), solar=solar, cmb=Q(inp["cmb"]),
                                     freq=Q(freq))
                exact, _ = sc.longdouble_dipole(quats, vel, solar, inp["cmb"], freq)
                worst = max(worst, float(np.max(np.abs(rows[d].astype(sc.L) - exact))) / (sc.EPS * scale))
            out[key + case] = rows
        out["err_" + case] = np.float64(worst)
        raw = worst * scale / inp["cmb"]
        print(f"{case:13s} rms {np.sqrt(np.mean(out['ref_' + case] ** 2)):.4e} K  peak "
              f"{np.max(np.abs(out['ref_' + case])):.4e} K  ref_err {worst:.3f} eps*scale (scale {scale:.4e} K; "
              f"{raw:.4f} eps*cmb)")
    np.savez_compressed(sc.GOLD_PATH, **out)
    print(f"wrote {sc.GOLD_PATH}: {os.path.getsize(sc.GOLD_PATH)} bytes")


if __name__ == "__main__":
    main()
