#!/usr/bin/env python3
"""Generate tests/golden/noise_estim.npz from THE REFERENCE'S OWN code.  Build container only.

The reference's toast_fod_psd.cpp and the two toast_sys_* files are compiled where they lie into a temporary directory
outside the repository, behind a few lines of ``extern "C"`` glue written by this script.  The reference's Python
functions flagged_running_average, highpass_flagged_signal, crosscov_psd (noise_estimation_utils.py) and log_bin,
bin_psds, discard_outliers (noise_estimation.py) are taken out of their files with ``ast`` and executed with the
compiled sums bound in; the few lines of process_noise_estimate between them (the second, decimated estimate, the merge
at fcut, the mean over the periods) are restated here.  Nothing of the reference is copied into the repository.

Inputs come from ``toast_amd.rng`` streams (tests/noise_estim_case.py), so the file holds outputs only.  Next to them
it stores how far the reference itself is from a more precise evaluation:

* sums_ref_err   max over cases and lags of |reference - long double sum| / sum |products at that lag|;
* trend_ref_err  the ``fftconvolve`` running average against a long double window sum, relative to the row's rms;
* psd_ref_err    the whole chain in double against the same chain fed with long double sums and trend, relative to
                 max |PSD| of the row.

    python tests/golden/make_golden_noise_estim.py
"""
import ast
import copy
import ctypes as C
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import scipy.signal
from scipy.signal import fftconvolve

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/src"

import noise_estim_case as nc  # noqa: E402

L = np.longdouble

GLUE = r"""
#include <cstdint>
#include <toast/sys_utils.hpp>
#include <toast/fod_psd.hpp>
extern "C" {
void g_autosums(int64_t n, const double * x, const uint8_t * good, int64_t lagmax, double * sums, int64_t * hits,
                int64_t all_sums) { toast::fod_autosums(n, x, good, lagmax, sums, hits, all_sums); }
void g_crosssums(int64_t n, const double * x, const double * y, const uint8_t * good, int64_t lagmax, double * sums,
                 int64_t * hits, int64_t all_sums, int64_t symmetric) {
    toast::fod_crosssums(n, x, y, good, lagmax, sums, hits, all_sums, symmetric);
}
}
"""


def build_reference(tmp):
    glue = os.path.join(tmp, "glue.cpp")
    open(glue, "w").write(GLUE)
    subprocess.check_call(["sh", REF + "/libtoast/generate_version_cpp.sh", "golden"], cwd=tmp, stdout=subprocess.DEVNULL)
    srcs = [REF + "/libtoast/src/" + f for f in ("toast_fod_psd.cpp", "toast_sys_utils.cpp", "toast_sys_environment.cpp")]
    out = os.path.join(tmp, "libref_fod.so")
    # -O2, no -march: no FMA contraction, the numerical ground truth (as oracle/ref_build.sh)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-I" + REF + "/libtoast/include",
                           "-I" + REF + "/libtoast/src", glue, os.path.join(tmp, "version.cpp")] + srcs + ["-o", out])
    return C.CDLL(out)


def bind_sums(lib):
    P = C.c_void_p

    def ptr(a):
        return P(a.ctypes.data)

    def fod_autosums(x, good, lagmax, sums, hits, all_sums):
        x, good = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(good, dtype=np.uint8)
        assert sums.flags.c_contiguous and hits.flags.c_contiguous and sums.size == lagmax and hits.size == lagmax
        lib.g_autosums(C.c_int64(x.size), ptr(x), ptr(good), C.c_int64(lagmax), ptr(sums), ptr(hits),
                       C.c_int64(int(all_sums)))

    def fod_crosssums(x, y, good, lagmax, sums, hits, all_sums, symmetric):
        x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
        good = np.ascontiguousarray(good, dtype=np.uint8)
        assert sums.flags.c_contiguous and hits.flags.c_contiguous and sums.size == lagmax and hits.size == lagmax
        lib.g_crosssums(C.c_int64(x.size), ptr(x), ptr(y), ptr(good), C.c_int64(lagmax), ptr(sums), ptr(hits),
                        C.c_int64(int(all_sums)), C.c_int64(int(symmetric)))

    return fod_autosums, fod_crosssums


# ------------------------------------------------------------------------------ the reference's Python, by ast
class _Log:
    @staticmethod
    def get():
        return _Log()

    def debug(self, *a, **k):
        pass


def reference_functions(fod_autosums, fod_crosssums):
    ns = {"np": np, "fftconvolve": fftconvolve, "fod_autosums": fod_autosums, "fod_crosssums": fod_crosssums,
          "MPI": None, "copy": copy, "scipy": scipy, "Logger": _Log}

    def take(path, names, klass=None):
        tree = ast.parse(open(path).read())
        body = tree.body
        if klass is not None:
            body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == klass).body
        for node in body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                node.decorator_list = []
                mod = ast.Module(body=[node], type_ignores=[])
                exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)

    take(REF + "/toast/ops/noise_estimation_utils.py", {"flagged_running_average", "highpass_flagged_signal", "crosscov_psd"})
    take(REF + "/toast/ops/noise_estimation.py", {"log_bin", "bin_psds", "discard_outliers"}, klass="NoiseEstim")
    return ns


def precise_functions(ns):
    """The same chain fed with long double sums and a long double running average."""
    def autosums(x, good, lagmax, sums, hits, all_sums):
        s, _, h = nc.sums_longdouble(np.asarray(x), None, np.asarray(good), lagmax, all_sums, 0)
        sums += s.astype(np.float64)
        hits += h

    def crosssums(x, y, good, lagmax, sums, hits, all_sums, symmetric):
        s, _, h = nc.sums_longdouble(np.asarray(x), np.asarray(y), np.asarray(good), lagmax, all_sums, symmetric)
        sums += s.astype(np.float64)
        hits += h

    def highpass(sig, good, naverage):
        if np.sum(good) == 0:
            return np.zeros_like(sig)
        trend, _ = nc.trend_longdouble(sig, good, naverage)
        return (sig.astype(L) - trend).astype(np.float64)

    exec_ns = reference_functions(autosums, crosssums)
    exec_ns["highpass_flagged_signal"] = highpass
    return exec_ns


def reference_estimate(ns, op, obs, det1, det2, flags, global_intervals, fsample):
    """process_noise_estimate (noise_estimation.py:926-1231) for one process: the reference's functions, with the
    lines between them restated."""
    from toast_amd.data import defaults

    me = types.SimpleNamespace(nbin_psd=op.nbin_psd, save_cov=False)
    me.log_bin = types.MethodType(ns["log_bin"], me)
    bin_psds = types.MethodType(ns["bin_psds"], me)
    discard = types.MethodType(ns["discard_outliers"], me)
    times = np.array(obs.shared[defaults.times].data)
    lagmax, period = op.lagmax, float(op.stationary_period)
    good = flags == 0
    sig1 = ns["highpass_flagged_signal"](np.array(obs.detdata[op.det_data][det1]), good, lagmax)
    sig2 = None if det1 == det2 else ns["highpass_flagged_signal"](np.array(obs.detdata[op.det_data][det2]), good, lagmax)
    my_psds1 = ns["crosscov_psd"](times, times, global_intervals, sig1, sig2, flags, lagmax, lagmax, period, fsample,
                                  None, False, op.symmetric)
    if op.nsum > 1:
        times2 = times[::op.nsum]
        flags2 = flags[::op.nsum].copy()
        dec1 = sig1[::op.nsum].copy()
        dec2 = None if sig2 is None else sig2[::op.nsum].copy()
        lagmax2 = min(lagmax, times2.size)
        dec1 = ns["highpass_flagged_signal"](dec1, flags2 == 0, lagmax2)
        if dec2 is not None:
            dec2 = ns["highpass_flagged_signal"](dec2, flags2 == 0, lagmax2)
        my_psds2 = ns["crosscov_psd"](times2, times2, global_intervals, dec1, dec2, flags2, lagmax2, lagmax2, period,
                                      fsample / op.nsum, None, False, op.symmetric)
        keep = min(len(my_psds1), len(my_psds2))
        my_psds1, my_psds2 = my_psds1[:keep], my_psds2[:keep]
    fmin, fmax = 1 / period, fsample / 2
    binned1, my_times, binfreq1 = bin_psds(my_psds1, fmin, fmax)
    if op.nsum > 1:
        binned2, _, binfreq2 = bin_psds(my_psds2, fmin, fmax)
        fcut = fsample / 2 / op.naverage / 100
        ind1, ind2 = binfreq1 > fcut, binfreq2 <= fcut
        binfreq = np.hstack([binfreq2[ind2], binfreq1[ind1]])
        binned = [np.hstack([p2[ind2], p1[ind1]]) for p1, p2 in zip(binned1, binned2)]
    else:
        binfreq, binned = binfreq1, binned1
    good_psds, _, _, _ = discard(binfreq, list(binned), list(my_times), None)
    return binfreq, np.mean(np.array(good_psds), axis=0)


def operator_params(given):
    """The traits of the reference operator that matter here, with its defaults (noise_estimation.py:38-182; the masks
    are defaults.det_mask_invalid = 1 and defaults.shared_mask_nonscience = 15, observation.py:87-111)."""
    p = dict(det_data="signal", det_flags="flags", shared_flags="flags", det_mask=1, det_flag_mask=1, shared_flag_mask=15,
             symmetric=False, nbin_psd=1000, lagmax=10000, stationary_period=86400, nosingle=False, nocross=True, nsum=1,
             naverage=100, view=None, pairs=[], focalplane_key=None, remove_common_mode=False)
    assert set(given) <= set(p), given
    p.update(given)
    return types.SimpleNamespace(**p)


def reference_pairs(obs, op, local_dets):
    """(det_names, pairs) of noise_estimation.py:394-438."""
    if op.focalplane_key is not None:
        fp = obs.telescope.focalplane
        det_names, key2det = [], {}
        for det in local_dets:
            key = fp[det][op.focalplane_key]
            if key not in key2det:
                det_names.append(det)
                key2det[key] = det
        pairs = []
        for det1 in key2det.values():
            for det2 in key2det.values():
                if det1 == det2 and op.nosingle:
                    continue
                if det1 != det2 and op.nocross:
                    continue
                pairs.append([det1, det2])
    else:
        det_names = list(obs.local_detectors)
        if len(op.pairs) > 0:
            pairs = op.pairs
        else:
            pairs = []
            for idet1 in range(len(det_names)):
                for idet2 in range(idet1, len(det_names)):
                    det1, det2 = det_names[idet1], det_names[idet2]
                    if det1 == det2 and op.nosingle:
                        continue
                    if det1 != det2 and op.nocross:
                        continue
                    pairs.append([det1, det2])
    if op.symmetric:
        pairs = sorted({tuple(sorted(pair)) for pair in pairs})
    return det_names, pairs


def reference_flags(obs, op, det1, det2):
    """The sample flags of a pair (noise_estimation.py:443-447, :482-494)."""
    flags = np.zeros(obs.n_local_samples, dtype=bool)
    if op.shared_flags is not None:
        flags[:] = (np.asarray(obs.shared[op.shared_flags].data) & op.shared_flag_mask) != 0
    if op.det_flags is not None:
        flags |= (np.asarray(obs.detdata[op.det_flags][det1]) & op.det_flag_mask) != 0
        if det1 != det2:
            flags |= (np.asarray(obs.detdata[op.det_flags][det2]) & op.det_flag_mask) != 0
    return flags


def remove_common_mode(obs, op):
    """noise_estimation.py:340-356 on the host: a copy of the signal loses the mean of the unflagged samples over the
    detectors of every focalplane key value (CommonModeFilter, polyfilter.py:880-960, with its default shared mask
    defaults.shared_mask_invalid = 1) and is then subtracted from the signal."""
    import poly_filter_host as ph

    sig = obs.detdata[op.det_data].data
    temp = sig.copy()
    fl = obs.detdata[op.det_flags].data
    shared = np.asarray(obs.shared["flags"].data)
    fp = obs.telescope.focalplane
    dets = [d for d in obs.local_detectors if not (obs.local_detector_flags[d] & op.det_mask)]
    for value in sorted({fp[d][op.focalplane_key] for d in obs.local_detectors}):
        rows = [obs.local_detectors.index(d) for d in dets if fp[d][op.focalplane_key] == value]
        total, hits = np.zeros(sig.shape[1]), np.zeros(sig.shape[1], dtype=np.int64)
        ph.sum_detectors(rows, rows, shared, 1, temp, fl, op.det_flag_mask, total, hits)
        ph.subtract_mean(rows, temp, total, hits)
    sig[:] = sig - temp


def main():
    tmp = tempfile.mkdtemp(prefix="golden_noise_estim_")
    fod_autosums, fod_crosssums = bind_sums(build_reference(tmp))
    ns = reference_functions(fod_autosums, fod_crosssums)
    pns = precise_functions(ns)
    out = {}

    # ---- lagged sums
    serr = 0.0
    for name, n, lagmax, fk, kind, all_sums, sym, seed in nc.sums_cases():
        x, y, good = nc.sums_inputs(n, lagmax, fk, kind, seed)
        sums = np.full(lagmax, 0.25)                     # accumulated into
        hits = np.full(lagmax, 3, dtype=np.int64)
        if kind == "auto":
            fod_autosums(x, good, lagmax, sums, hits, all_sums)
        else:
            fod_crosssums(x, y, good, lagmax, sums, hits, all_sums, sym)
        ld, norm, h = nc.sums_longdouble(x, y, good, lagmax, all_sums, sym)
        assert np.array_equal(h + 3, hits), name
        # the error of the sums themselves: a fresh accumulation from zero
        s0, h0 = np.zeros(lagmax), np.zeros(lagmax, dtype=np.int64)
        if kind == "auto":
            fod_autosums(x, good, lagmax, s0, h0, all_sums)
        else:
            fod_crosssums(x, y, good, lagmax, s0, h0, all_sums, sym)
        serr = max(serr, nc.sums_distance(s0, ld, norm))
        out[f"sums_{name}"] = sums
        out[f"hits_{name}"] = hits
        hi = ld.astype(np.float64)
        out[f"ld_{name}"] = np.stack([hi, (ld - hi.astype(L)).astype(np.float64)])
    out["sums_ref_err"] = np.array(serr)

    # ---- running average
    terr = 0.0
    flagged_running_average = ns["flagged_running_average"]
    stored = {(n, w, fk, off): name for name, n, w, fk, off in nc.TREND_ROWS}
    rows = [(n, w, fk, 0.0) for n in (1000,) for w in nc.TREND_WINDOWS for fk in nc.FLAG_KINDS] + [(4099, 100, "random", 1.0e6)]
    for n, w, fk, off in rows:
        name = stored.get((n, w, fk, off), f"{n}_{w}_{fk}")
        x, good = nc.trend_inputs(name, n, w, fk, off)
        trend = flagged_running_average(x, good == 0, w)
        ld, cnt = nc.trend_longdouble(x, good, w)
        terr = max(terr, float(np.max(np.abs(trend.astype(L) - ld))) / nc.row_rms(x))
        if (n, w, fk, off) in stored:
            out[f"trend_{name}"] = trend
            out[f"trend_hit_{name}"] = (cnt > 0)
    out["trend_ref_err"] = np.array(terr)

    # ---- operator cases: pairs, keys and flags are built here from the observation with plain NumPy
    perr = 0.0
    for name, case in nc.OP_CASES.items():
        op = operator_params(case["op"])
        obs = nc.make_obs(name).obs[0]
        if op.focalplane_key is not None and op.remove_common_mode:
            remove_common_mode(obs, op)
        fsample = obs.telescope.focalplane.sample_rate
        local = [d for d in obs.local_detectors if not (obs.local_detector_flags[d] & op.det_mask)]
        det_names, pairs = reference_pairs(obs, op, local)
        ivals = [(None, None)] if op.view is None else [(iv.start, iv.stop) for iv in obs.intervals[op.view]]
        keys = []
        for det1, det2 in pairs:
            if det1 not in det_names or det2 not in det_names:
                continue
            key = det1 if det1 == det2 else f"{det1} x {det2}"
            if det1 in local and det2 in local:
                flags = reference_flags(obs, op, det1, det2)
                freq, psd = reference_estimate(ns, op, obs, det1, det2, flags.copy(), ivals, fsample)
                _, psd_ld = reference_estimate(pns, op, obs, det1, det2, flags.copy(), ivals, fsample)
                perr = max(perr, float(np.max(np.abs(psd - psd_ld)) / np.max(np.abs(psd))))
            else:
                freq = np.array([0.0, 1.0e-5, fsample / 4, fsample / 2])
                psd = np.zeros(4)
            out[f"op_{name}_freq_{len(keys)}"] = freq[1:]
            out[f"op_{name}_psd_{len(keys)}"] = psd[1:]
            keys.append(key)
        out[f"op_{name}_keys"] = np.array(keys)
    out["psd_ref_err"] = np.array(perr)

    path = os.path.join(HERE, "noise_estim.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;",
          {k: float(out[k]) for k in ("sums_ref_err", "trend_ref_err", "psd_ref_err")})


if __name__ == "__main__":
    main()
