#!/usr/bin/env python3
"""Generate tests/golden/filterbin.npz by RUNNING THE REFERENCE'S OWN filter code on the cases of tests/filterbin_case.py.

* src/toast/ops/filterbin.py is parsed where it lies.  From its syntax tree this script compiles the `SparseTemplates`
  class, the methods `_add_hwp_templates`, `_add_ground_poly_templates`, `_add_poly_templates`, `_get_phase` and
  `_regress_templates` of `FilterBin`, and the detector loop of `FilterBin._exec` (:854-1033, the `for idet, det in
  enumerate(dets)` statement, wrapped into a function that sets the loop's own local variables).  Decorators are dropped;
  nothing is copied into the repository.
* `legendre_templates` / `fourier_templates` are the compiled reference bindings (oracle.load_ref()).
* `build_template_covariance` (src/toast/_libtoast/ops_filterbin.cpp:276-382) is NOT among the compiled bindings of
  oracle/_ref.  The name is bound to this script's own NumPy inner product `template_inner_products`: the sum over the
  overlap of two templates of t_row * t_col * good, and 1 on the diagonal of a template of at most one sample -- what the
  C++ computes (its sparse-index branch is never taken: the index lists are filled into a copy).
* The code runs on stand-in observation objects (`Obs`); `np` inside the compiled code is a proxy that records the calls
  of `np.linalg.inv` / `np.linalg.pinv`, which gives the route the reference took per detector.

The script asserts that every planted edge occurs in the reference's run.  Build container only; the fixture is
committed.

    python tests/golden/make_golden_filterbin.py
"""
import ast
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
REF = "/root/reference/src/toast/ops/filterbin.py"

import filterbin_case as FC  # noqa: E402

ROUTE_INV, ROUTE_PINV, ROUTE_REJECTED, ROUTE_NOFIT = 0, 1, 2, 3
METHODS = ("_add_hwp_templates", "_add_ground_poly_templates", "_add_poly_templates", "_get_phase", "_regress_templates")
EVENTS = []


def template_inner_products(starts, stops, templates, good, invcov):
    EVENTS.append("cov")
    for row in range(len(templates)):
        for col in range(row, len(templates)):
            istart, istop = max(starts[row], starts[col]), min(stops[row], stops[col])
            val = 1.0 if (row == col and istop - istart <= 1) else 0.0
            if istop > istart:
                val += np.sum(templates[row][istart - starts[row]:istop - starts[row]]
                              * templates[col][istart - starts[col]:istop - starts[col]] * good[istart:istop])
            invcov[row, col] = invcov[col, row] = val


class _Linalg:
    def __getattr__(self, name):
        return getattr(np.linalg, name)

    @staticmethod
    def inv(a):
        EVENTS.append("inv")
        return np.linalg.inv(a)

    @staticmethod
    def pinv(a, **kwargs):
        EVENTS.append("pinv")
        return np.linalg.pinv(a, **kwargs)


class _Numpy:
    linalg = _Linalg()

    def __getattr__(self, name):
        return getattr(np, name)


class _Logger:
    @staticmethod
    def get():
        return _Logger()

    def debug(self, *a, **k):
        pass

    warning = info = debug


def load_reference(ref):
    tree = ast.parse(open(REF).read(), REF)
    sparse = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SparseTemplates"]
    fb = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FilterBin"]
    assert len(sparse) == 1 and len(fb) == 1
    methods = [n for n in fb[0].body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(m.name for m in methods) == sorted(METHODS)
    execs = [n for n in fb[0].body if isinstance(n, ast.FunctionDef) and n.name == "_exec"]
    loops = [n for n in ast.walk(execs[0]) if isinstance(n, ast.For) and isinstance(n.target, ast.Tuple)
             and [getattr(e, "id", None) for e in n.target.elts] == ["idet", "det"]]
    assert len(loops) == 1
    wrapper = ast.parse(
        "def _detector_loop(self, data, obs, dets, common_templates, common_flags):\n"
        "    log = Logger.get()\n"
        "    last_good_fit = None\n"
        "    template_amplitudes = {}\n"
        "    n_saved_templates = 0\n"
        "    t1 = time()\n"
        "    pass\n"
        "    return template_amplitudes\n").body[0]
    wrapper.body[5] = loops[0]
    for node in [sparse[0]] + methods:
        for sub in ast.walk(node):
            if isinstance(sub, ast.FunctionDef):
                sub.decorator_list = [d for d in sub.decorator_list if getattr(d, "id", None) == "property"]
    holder = ast.ClassDef(name="RefFilterBin", bases=[], keywords=[], body=methods + [wrapper], decorator_list=[])
    mod = ast.Module(body=[sparse[0], holder], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": _Numpy(), "Logger": _Logger, "time": time.time, "pickle": None, "u": types.SimpleNamespace(radian="rad"),
          "IntervalList": lambda *a, **k: None, "legendre_templates": ref.legendre_templates,
          "fourier_templates": ref.fourier_templates, "build_template_covariance": template_inner_products}
    exec(compile(mod, REF, "exec"), ns)
    return ns["SparseTemplates"], ns["RefFilterBin"]


# ------------------------------------------------------------------ stand-in observation
class Shared:
    def __init__(self, array):
        self.data = array

    def __array__(self, dtype=None, copy=None):
        return self.data

    def set(self, value, offset=(0,), fromrank=0):
        self.data[:] = value


class Angle(float):
    def to_value(self, unit):
        return float(self)


class Intervals(list):
    @property
    def data(self):
        return [(iv.first, iv.last) for iv in self]


class Obs:
    """What the compiled reference code touches of an observation."""

    def __init__(self, case, signal, dflags, shared):
        n = case["cfg"]["n_samp"]
        self.name, self.uid, self.n_local_samples = case["name"], 0, n
        self.dets = [f"D{d}" for d in range(signal.shape[0])]
        self.shared = {"times": Shared(np.arange(n) / 20.0), "azimuth": Shared(case["az"]), "hwp_angle": Shared(case["hwp"]),
                       "flags": Shared(shared)}
        self.detdata = {"signal": {d: signal[i] for i, d in enumerate(self.dets)},
                        "flags": {d: dflags[i] for i, d in enumerate(self.dets)}}
        self.local_detector_flags = {d: 0 for d in self.dets}
        # an interval list of the reference lives inside the local samples (intervals.py: spans beyond the timestamps
        # are cut)
        clip = lambda spans: Intervals(types.SimpleNamespace(first=max(a, 0), last=min(b, n)) for a, b in spans)  # noqa: E731
        self.intervals = {FC.VIEW: clip([(int(a), int(b)) for a, b in case["spans"]]),
                          FC.LEFTRIGHT: clip(FC.direction_spans(case, 1)), FC.RIGHTLEFT: clip(FC.direction_spans(case, 2))}
        self.meta = {"scan_min_az": Angle(FC.AZ_LO), "scan_max_az": Angle(FC.AZ_HI)}

    def __getitem__(self, key):
        return self.meta[key]


def reference_operator(RefFilterBin, cfg):
    op = RefFilterBin()
    t = FC.operator_traits(cfg)
    for key, value in t.items():
        setattr(op, key, value)
    op.times, op.azimuth, op.hwp_angle, op.shared_flags, op.det_data, op.det_flags = (
        "times", "azimuth", "hwp_angle", "flags", "signal", "flags")
    op.ground_template_time_step = None
    op.deproject_map = op.precomputed_templates = op.amplitude_dir = None
    op.write_obs_matrix = False
    op.grank, op.group = 1, 0
    op.binning = types.SimpleNamespace(shared_flag_mask=FC.SHARED_FLAG_MASK, det_flag_mask=FC.DET_FLAG_MASK)
    return op


# ------------------------------------------------------------------ the random part of a case
def draw_case(name, rng):
    cfg = FC.CASES[name]
    n, n_det = cfg["n_samp"], cfg["n_det"]
    k = 0 if cfg["poly"] is None else cfg["poly"] + 1
    # ragged intervals of 60-420 samples with gaps, alternating direction; the last one runs past n_samp
    spans, cursor = [], int(rng.integers(0, 7))
    while True:
        length = int(rng.integers(60, 420))
        if cfg.get("long_interval") and len(spans) == 3:
            length = 1024 + 277                               # longer than one chunk of the accumulate kernel
        if cursor + length + 40 >= n:
            break
        spans.append((cursor, cursor + length))
        cursor += length + int(rng.integers(0, 25))
    spans.append((cursor, n + 13))
    direction = np.array([1 + (i % 2) for i in range(len(spans))], dtype=np.int32)
    shared = np.zeros(n, dtype=np.uint8)
    edges = [0] + [x for s in spans for x in s]
    for a, b in zip(edges[0::2], edges[1::2]):
        shared[a:b] = 2                                        # turnarounds
    shared[rng.random(n) < 0.02] |= 1
    short = None
    if cfg.get("short_interval"):
        short = 5
        a, b = spans[short]
        shared[a + 1:b] |= 1                                   # k - 1 shared-good samples are left
        shared[a] = 0
    dflags = (rng.random((n_det, n)) < 0.10).astype(np.uint8)
    for d in range(n_det):
        for a, b in spans:
            b = min(b, n)
            if rng.random() < 0.5:                             # a flagged block of up to 30 % of the interval
                w = int(rng.integers(1, max(2, int(0.3 * (b - a)))))
                o = int(rng.integers(a, b - w + 1))
                dflags[d, o:o + w] = 1
    dflags *= np.array([1, 2, 1, 2, 1, 2, 1], dtype=np.uint8)[:n_det, None]
    planted = dict(short_interval=-1 if short is None else short, dead_interval=-1, dead_interval_det=-1,
                   dead_direction_det=-1, dead_detector=-1)
    if cfg.get("dead_interval"):
        planted["dead_interval"], planted["dead_interval_det"] = 2, 1
        a, b = spans[2]
        dflags[1, a:b] = 1
    if cfg.get("dead_direction"):
        planted["dead_direction_det"] = 3
        for (a, b), way in zip(spans, direction):
            if way == 2:                                       # ... so the template zeroed in the left-right sweeps is null
                dflags[3, a:min(b, n)] = 2
    if cfg.get("dead_detector"):
        planted["dead_detector"] = 5
        dflags[5] = 1
    return dict(spans=np.array(spans, dtype=np.int64), direction=direction, shared=shared, dflags=dflags,
                **{f"planted_{key}": np.array(v) for key, v in planted.items()}), k


def run_case(SparseTemplates, RefFilterBin, name, rng):
    drawn, k = draw_case(name, rng)
    cfg = FC.CASES[name]
    case = dict(drawn, cfg=cfg, name=name)
    n = cfg["n_samp"]
    case["az"], case["hwp"] = FC.azimuth(n, case["spans"], case["direction"]), FC.hwp_angle(n)
    signal = FC.signals(cfg)
    out, flags, shared = signal.copy(), drawn["dflags"].copy(), drawn["shared"].copy()
    obs = Obs(case, out, flags, shared)
    op = reference_operator(RefFilterBin, cfg)
    # _build_common_templates (:1413-1421) without the binned ground templates
    templates = SparseTemplates(rcond_limit=op.template_rcond_limit)
    op._add_hwp_templates(obs, templates)
    op._add_ground_poly_templates(obs, templates)
    op._add_poly_templates(obs, templates)
    common_flags = obs.shared["flags"].data
    routes = np.full(cfg["n_det"], ROUTE_NOFIT, dtype=np.int32)
    amplitudes = {}
    for i, det in enumerate(obs.dets):
        del EVENTS[:]
        amplitudes.update(op._detector_loop(None, obs, [det], templates, common_flags))
        if "inv" in EVENTS:
            routes[i] = ROUTE_INV
        elif "pinv" in EVENTS:
            routes[i] = ROUTE_PINV
        elif "cov" in EVENTS:
            routes[i] = ROUTE_REJECTED
        assert (amplitudes[det] is not None) == (routes[i] in (ROUTE_INV, ROUTE_PINV))
    names = list(templates.names)
    amps = np.full((cfg["n_det"], len(names)), np.nan)
    for i, det in enumerate(obs.dets):
        if amplitudes[det] is not None:
            for key, value in amplitudes[det].items():
                amps[i, names.index(key)] = value
    detflags = np.array([obs.local_detector_flags[d] for d in obs.dets], dtype=np.int64)
    # ---- the planted edges occurred
    n_dense = len(FC.dense_templates(case))
    assert sum(1 for x in names if not x.startswith("poly-")) == n_dense
    if cfg["hwp"] is not None:
        assert templates.starts[names.index("HWPSS-sin-1")] == 1 and templates.starts[names.index("HWPSS-cos-1")] == 0
    if cfg["limit"] == 0.9:
        assert np.all(routes == ROUTE_PINV)
    elif cfg["limit"] == -0.9:
        assert np.all(routes == ROUTE_REJECTED) and np.all(detflags == FC.FILTER_DETECTOR_MASK)
        assert np.all(flags & FC.FILTER_FLAG_MASK) and np.array_equal(out, signal)
    if cfg.get("short_interval"):
        a, b = case["spans"][int(drawn["planted_short_interval"])]
        assert np.all(shared[a:b] & FC.FILTER_FLAG_MASK) and not np.all(drawn["shared"][a:b] & FC.FILTER_FLAG_MASK)
        assert not any(x.endswith(f"-interval-{int(drawn['planted_short_interval'])}") for x in names)
    if cfg.get("dead_interval"):
        d, v = int(drawn["planted_dead_interval_det"]), int(drawn["planted_dead_interval"])
        assert routes[d] == ROUTE_INV and np.isnan(amps[d, names.index(f"poly-0-interval-{v}")])
        assert not np.isnan(amps[0, names.index(f"poly-0-interval-{v}")])
    if cfg.get("dead_direction"):
        d = int(drawn["planted_dead_direction_det"])
        # the template that is zero inside the left-right sweeps has no good sample: it is dropped and its span -- up to
        # the last right-left sweep -- is flagged; the detector keeps the left-right sweeps that lie outside that span
        gone = [x for x in names if x.endswith(FC.LEFTRIGHT) and np.isnan(amps[d, names.index(x)])]
        assert routes[d] == ROUTE_INV and len(gone) == cfg["ground"] - cfg["poly"] and detflags[d] == 0
        newly = (flags[d] & FC.FILTER_FLAG_MASK != 0) & (drawn["dflags"][d] == 0)
        print(f"        detector {d}: {len(gone)} dense templates dropped, {np.count_nonzero(newly)} samples newly flagged, "
              f"{np.count_nonzero((flags[d] & FC.DET_FLAG_MASK) == 0)} left good")
        assert np.count_nonzero(newly) > 0 and np.count_nonzero((flags[d] & FC.DET_FLAG_MASK) == 0) > 0
    if cfg.get("dead_detector"):
        d = int(drawn["planted_dead_detector"])
        assert routes[d] == ROUTE_NOFIT and detflags[d] == FC.FILTER_FLAG_MASK and np.array_equal(out[d], signal[d])
    if cfg.get("long_interval"):
        assert np.max(case["spans"][:, 1] - case["spans"][:, 0]) > 1024
    if name in ("poly", "ground", "hwp", "all"):
        ordinary = [d for d in range(cfg["n_det"]) if d not in (int(drawn["planted_dead_direction_det"]),
                                                                 int(drawn["planted_dead_detector"]))]
        assert np.all(routes[ordinary] == ROUTE_INV)
        if name != "hwp":                                                      # (no constant among the HWP templates)
            assert np.min(np.max(np.abs(out[ordinary] - signal[ordinary]), axis=1)) > 1.0      # the offsets went
    assert case["spans"][-1, 1] > n
    print(f"{name:7s} templates {len(names):3d} (dense {n_dense:2d})  routes {routes.tolist()}  detector flags "
          f"{detflags.tolist()}")
    result = dict(drawn, out=out, flags_out=flags, shared_out=shared, detflags=detflags, routes=routes, amps=amps,
                  amp_names=np.array(names))
    return {f"{name}_{key}": value for key, value in result.items()}


def main():
    import oracle

    ref = oracle.load_ref()
    assert ref is not None, "build oracle/_ref first"
    SparseTemplates, RefFilterBin = load_reference(ref)
    rng = np.random.default_rng(20261021)
    out = {}
    for name in FC.CASES:
        out.update(run_case(SparseTemplates, RefFilterBin, name, rng))
    path = os.path.join(HERE, "filterbin.npz")
    np.savez_compressed(path, **out)
    z = np.load(path, allow_pickle=False)
    assert set(z.files) == set(out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
