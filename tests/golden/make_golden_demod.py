#!/usr/bin/env python3
"""Generate tests/golden/demod.npz from THE REFERENCE'S OWN code.  Build container only.

The reference's classes Lowpass and Bandpass and the methods _demodulate_flag, _demodulate_signal, _demodulate_noise,
_get_fmod and _demodulate_sample_sets of Demodulate (src/toast/ops/demodulation.py) are taken out of their file with
``ast`` and executed here; astropy is absent, a stand-in units namespace in which every unit is 1 replaces it
(quantities are floats / arrays whose ``to_value`` returns themselves).  Nothing of the reference is copied into the
repository.

The inputs (signals, Stokes weights, flags) come from tests/demod_case.py and are stored, so the fixture pins
demodulation alone.  Next to the reference's outputs the file stores how far they are from a long-double direct
evaluation of the same chain, as a fraction of the chain's scale (sum |h_lp| max |x| for demod0, 2 sum |h_bp| sum |h_lp|
max |x| for demod4*):

* fft_ref_err     the reference's ``fftconvolve`` results;
* direct_ref_err  a double-precision direct sum in tap order;

and ``recovery_leak``: how far the reference's method is from the constants I0, eta Q0, eta U0 on the unflagged interior
of a signal built from them (a property of the filters).

    python tests/golden/make_golden_demod.py
"""
import ast
import os
import sys
import types

import numpy as np
import scipy.signal
from scipy.signal import fftconvolve, firwin

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/src/toast/ops/demodulation.py"

import demod_case as dc  # noqa: E402

L = np.longdouble


class Q(float):
    """A quantity whose unit is 1."""

    def to_value(self, unit=None):
        return float(self)

    def __truediv__(self, other):
        return Q(float(self) / other)

    def __mul__(self, other):
        return Q(float(self) * other)

    __rmul__ = __mul__


class Plain(np.ndarray):
    def to_value(self, unit=None):
        return np.asarray(self)

    def __getitem__(self, key):
        out = super().__getitem__(key)
        return Q(out) if np.ndim(out) == 0 else out


def plain(a):
    return np.array(a, dtype=np.float64).view(Plain)


class NoiseOut:
    def __init__(self, detectors, freqs, psds, indices, detweights):
        self.detectors, self.freqs, self.psds, self.indices, self.detweights = detectors, freqs, psds, indices, detweights


def reference():
    """(namespace with Lowpass / Bandpass, holder with the methods)."""
    tree = ast.parse(open(REF).read())
    unit = types.SimpleNamespace(Hz=1.0, second=1.0, K=1.0)
    ns = {"np": np, "scipy": scipy, "u": unit, "fftconvolve": fftconvolve, "firwin": firwin, "Noise": NoiseOut}
    wanted = {"_demodulate_flag", "_demodulate_signal", "_demodulate_noise", "_get_fmod", "_demodulate_sample_sets"}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in ("Lowpass", "Bandpass"):
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), REF, "exec"), ns)
        if isinstance(node, ast.ClassDef) and node.name == "Demodulate":
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name in wanted:
                    fn.decorator_list = []
                    exec(compile(ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[])), REF, "exec"), ns)
    return ns, wanted


def holder(ns, wanted, **attrs):
    h = types.SimpleNamespace(**attrs)
    for name in wanted:
        setattr(h, name, types.MethodType(ns[name], h))
    return h


def filters(ns, fmod, wkernel, offset=0):
    fs = Q(dc.RATE)
    low = ns["Lowpass"](Q(0.95 * fmod), fs, wkernel=wkernel, offset=offset, nskip=dc.NSKIP, window="hamming")
    bp2 = ns["Bandpass"](Q(1.05 * fmod), Q(2.95 * fmod), fs, wkernel=wkernel, window="hamming")
    bp4 = ns["Bandpass"](Q(3.05 * fmod), Q(4.95 * fmod), fs, wkernel=wkernel, window="hamming")
    return low, bp2, bp4


def run_signal(ns, wanted, dets, signal, weights, low, bp2, bp4, do_2f):
    """The reference's _demodulate_signal on plain containers: {pseudo detector: timestream}."""
    sw = types.SimpleNamespace(apply=lambda *a, **k: None, weights="weights", mode="IQU")
    h = holder(ns, wanted, stokes_weights=sw, mode="IQU", det_data="signal", do_2f=do_2f)
    obs = types.SimpleNamespace(uid=0, detdata={"weights": {d: weights[d] for d in dets},
                                                "signal": {d: signal[d] for d in dets}})
    demod_obs = types.SimpleNamespace(detdata={"signal": {}})
    data = types.SimpleNamespace(select=lambda **k: None)
    h._demodulate_signal(data, obs, demod_obs, list(dets), low, bp2, bp4)
    return demod_obs.detdata["signal"]


def main():
    ns, wanted = reference()
    inp = dc.make_inputs()
    out = dict(inp)
    table = dc.weight_table(inp)
    signal = {d: inp["signal"][i] for i, d in enumerate(dc.DETS)}

    obs = types.SimpleNamespace(shared={"times": types.SimpleNamespace(data=dc.times()),
                                        "hwp_angle": types.SimpleNamespace(data=dc.hwp_angle())})
    h0 = holder(ns, wanted, times="times", hwp_angle="hwp_angle", nskip=dc.NSKIP, demod_flag_mask=1, noise_model="noise",
                prefixes=["demod0", "demod4r", "demod4i"])
    fmod = float(h0._get_fmod(obs))
    out["fmod"] = fmod

    fft_err = direct_err = 0.0
    for case, spec in dc.CASES.items():
        wk = spec["op"].get("wkernel")
        do_2f = bool(spec["op"].get("do_2f"))
        low, bp2, bp4 = filters(ns, fmod, wk)
        out[f"{case}_lpf"], out[f"{case}_bpf4"], out[f"{case}_bpf2"] = low.lpf, bp4.bpf, bp2.bpf
        res = run_signal(ns, wanted, spec["dets"], signal, table, low, bp2, bp4, do_2f)
        for name, tod in res.items():
            out[f"{case}_tod_{name}"] = np.array(tod, dtype=np.float64)
        for d in spec["dets"]:
            x = signal[d]
            w_qu = table[d][:, 1:]
            s0, s4 = dc.chain_scales(x, low.lpf, bp4.bpf)
            ld = dc.chain(x, w_qu, low.lpf, bp4.bpf, 0, dc.NSKIP, dc.same_longdouble)
            dbl = dc.chain(x, w_qu, low.lpf, bp4.bpf, 0, dc.NSKIP, dc.same_double_direct)
            for prefix, want, got, scale in zip(("demod0", "demod4r", "demod4i"), ld, dbl, (s0, s4, s4)):
                ref = res[f"{prefix}_{d}"]
                fft_err = max(fft_err, float(np.max(np.abs(ref.astype(L) - want)) / scale))
                direct_err = max(direct_err, float(np.max(np.abs(got.astype(L) - want)) / scale))
    out["fft_ref_err"], out["direct_ref_err"] = fft_err, direct_err

    # flags and sample counts for every offset
    low, bp2, bp4 = filters(ns, fmod, None)
    out["wkernel"] = low.wkernel
    for off in range(dc.NSKIP):
        out[f"flags_shared_off{off}"] = h0._demodulate_flag(inp["shared_flags"], low.wkernel, off)
        out[f"flags_D0_off{off}"] = h0._demodulate_flag(inp["det_flags"][0], low.wkernel, off)
    out["flags_short"] = h0._demodulate_flag(inp["det_flags"][0][:700], low.wkernel, 1)
    sets = h0._demodulate_sample_sets(types.SimpleNamespace(all_sample_sets=dc.SAMPLE_SETS))
    out["sample_sets"] = np.array([c for s in sets for c in s], dtype=np.int64)

    # noise model
    f, psds = dc.noise_inputs()
    noise = types.SimpleNamespace(rate=lambda det: Q(2 * f[-1]), freq=lambda det: plain(f), psd=lambda det: plain(psds[det]),
                                  index=lambda det: dc.NOISE_INDEX[det])
    for case, prefixes in (("default", ["demod0", "demod4r", "demod4i"]),
                           ("2f", ["demod0", "demod4r", "demod4i", "demod2r", "demod2i"])):
        h0.prefixes = prefixes
        dets = list(dc.CASES[case]["dets"])
        demod_obs = {}
        h0._demodulate_noise({"noise": noise}, demod_obs, dets, Q(dc.RATE), fmod, low, bp2, bp4)
        model = demod_obs["noise"]
        out[f"noise_{case}_dets"] = np.array(model.detectors)
        for k, name in enumerate(model.detectors):
            out[f"noise_{case}_freq_{k}"] = np.asarray(model.freqs[name], dtype=np.float64)
            out[f"noise_{case}_psd_{k}"] = np.asarray(model.psds[name], dtype=np.float64)
        out[f"noise_{case}_index"] = np.array([model.indices[n] for n in model.detectors], dtype=np.int64)
        out[f"noise_{case}_weight"] = np.array([float(model.detweights[n]) for n in model.detectors])

    # recovery: what the reference's method leaves of constant I0, Q0, U0
    rec = dc.recovery_signal(inp)
    res = run_signal(ns, wanted, dc.DETS, {d: rec[i] for i, d in enumerate(dc.DETS)}, table, low, bp2, bp4, False)
    flags = {}
    for i, d in enumerate(dc.DETS):
        fl = h0._demodulate_flag(np.zeros(dc.N, dtype=np.uint8), low.wkernel, 0)
        for prefix in ("demod0", "demod4r", "demod4i"):
            flags[f"{prefix}_{d}"] = fl
    out["recovery_leak"] = dc.recovery_leak(res, flags, dc.DETS)

    np.savez(dc.GOLD_PATH, **out)
    size = os.path.getsize(dc.GOLD_PATH)
    print(f"fmod {fmod!r}  wkernel {low.wkernel} / {bp4.wkernel}")
    print(f"fft_ref_err {fft_err:.3e}  direct_ref_err {direct_err:.3e}  recovery_leak {out['recovery_leak']:.3e}")
    print(f"{dc.GOLD_PATH}: {size} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
