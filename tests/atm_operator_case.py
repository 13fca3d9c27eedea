"""Inputs and host restatements of the ObserveAtmosphere operator kernels (csrc/atm_observe.hip: k_atm_good_ranges,
k_atm_observe_quats, k_atm_flag_failed, k_atm_finish), regenerated from seeds.

Shared by tests/test_atm_operator_case_host.py (no GPU: the conditions on the inputs, and the restatements against
``ObserveAtmosphere._observe_host``) and tests/test_gpu_atm_operator_grid.py (the kernels through the C ABI and the
operator on resident data).  The volumes, ``longdouble_observe``, ``deviation``, ``quat_from_azel`` and ``make_sim`` are
those of tests/atm_observe_case.py.

A launch shape is (n_samp, strided).  Not strided: the rows are as long as the view.  Strided: the view is a window of a
longer observation -- rows of ``n_samp + PAD`` samples, every pointer advanced by ``SHIFT`` samples, everything outside
the window a sentinel.  Buffers have two more rows than a call has entries, and every row table is its own permutation.

The restatements are exact host statements (``good_host``, ``ranges_host``, ``flag_failed_host``), float64 NumPy in
the kernel's order of operations (``finish_host``) and np.longdouble evaluations (``longdouble_azel``,
``finish_longdouble``)."""
import functools

import numpy as np

import atm_observe_case as ac

L = np.longdouble
EPS = ac.EPS
TWOPI = 2 * np.pi
PI_2 = np.pi / 2

#: sample counts: one lane, around a wave (64), around the workgroup (256) and two workgroups plus one sample
N = (1, 63, 64, 65, 255, 256, 257, 513)
N_OBSERVE = (1, 64, 65, 256, 257, 513)
N_FINISH = (1, 65, 256, 257, 513)
PAD, SHIFT = 37, 19
DET_MASK, SHARED_MASK = 3, 5
#: what a float64 sample holds that no kernel may touch, and a byte of the same kind
SENTINEL = -7.25e33
SENTINEL_BYTE = 0xAB
#: roundings of k_atm_finish per sample, in units eps * scale_i (derived in tests/test_gpu_atm_operator_grid.py)
FINISH_ROUNDINGS = 7


def layout(n, strided):
    """(stride, shift) of a launch shape."""
    return (n + PAD, SHIFT) if strided else (n, 0)


def embed(rows, strided, fill, n_rows=None, at=None):
    """``rows`` [r][n] + shape as the windows of a buffer [n_rows][stride] + shape whose other samples hold ``fill``; row
    k of ``rows`` becomes row ``at[k]`` of the buffer."""
    rows = np.asarray(rows)
    r, n = rows.shape[:2]
    stride, shift = layout(n, strided)
    n_rows = r if n_rows is None else n_rows
    at = np.arange(r) if at is None else np.asarray(at)
    buf = np.full((n_rows, stride) + rows.shape[2:], fill, dtype=rows.dtype)
    buf[at, shift:shift + n] = rows
    return buf


def embed1(row, strided, fill):
    """A shared row (times, shared flags) [n] in its buffer [stride]."""
    return embed(np.asarray(row)[None], strided, fill)[0]


def row_tables(entries, n_tables, seed):
    """``n_tables`` independent tables of ``entries`` distinct rows out of ``entries + 2``: none the identity, and no
    two alike where there are enough to choose from (a single entry has two tables that are not the identity)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_tables):
        for attempt in range(100):
            t = rng.permutation(entries + 2)[:entries].astype(np.int32)
            fresh = attempt >= 50 or not any(np.array_equal(t, o) for o in out)
            if fresh and not np.array_equal(t, np.arange(entries)):
                break
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------- quaternions
def quat_from_angles(theta, phi):
    """``ac.quat_from_azel`` with the angles themselves (theta = pi / 2 - el, phi = 2 pi - az), for the azimuths that
    ``2 pi - az`` cannot express."""
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    sy, cy = np.sin(theta / 2), np.cos(theta / 2)
    sz, cz = np.sin(phi / 2), np.cos(phi / 2)
    return np.stack([-sz * sy, cz * sy, sz * cy, cz * cy], axis=-1)


#: phi at which qa_to_angles wraps (phi < 0 -> phi + 2 pi) or returns az = 2 pi
WRAP_PHI = (0.0, 1e-16, -1e-16, TWOPI - 1e-15)


def denormalise(q, rng):
    """Quaternions off the unit sphere by 1e-3, as ``ac.operator_inputs`` leaves them: the kernels normalise."""
    return q * (1.0 + 1e-3 * rng.standard_normal(q.shape[:-1] + (1,)))


def longdouble_azel(quats):
    """qa_to_angles (and az = 2 pi - phi, el = pi / 2 - theta) in long double on quaternions [...][4].  The constants are
    the code's doubles: the statement under test is ``2 * M_PI - phi``, not ``2 pi - phi``."""
    q = np.asarray(quats).astype(L)
    for _ in range(2):
        norm = q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]
        q = q / np.sqrt(norm)[..., None]
    x, y, z, w = (q[..., k] for k in range(4))
    d0 = 2 * (y * w + x * z)
    d1 = 2 * (y * z - x * w)
    d2 = 2 * (-(x * x) - y * y) + 1
    theta = L(PI_2) - np.arcsin(d2)
    phi = np.arctan2(d1, d0)
    phi = np.where(phi < 0, phi + L(TWOPI), phi)
    return L(TWOPI) - phi, L(PI_2) - theta


def azel_deviation(az, el, az_ld, el_ld, wrap=None):
    """Worst |value - long double| of az and of el in units eps * max(1, |value|); az modulo 2 pi where ``wrap``."""
    d = np.abs(np.asarray(az).astype(L) - az_ld)
    if wrap is not None:
        d = np.where(wrap, np.minimum(d, np.abs(d - L(TWOPI))), d)
    d_az = d / (EPS * np.maximum(1, np.abs(az_ld)))
    d_el = np.abs(np.asarray(el).astype(L) - el_ld) / (EPS * np.maximum(1, np.abs(el_ld)))
    return float(max(d_az.max(), d_el.max()))


#: the quaternion rows of the good_ranges cases
RANGE_ROWS = ("cone", "cross", "wide", "circle", "cone2")


@functools.lru_cache(maxsize=None)
def range_rows(n):
    """(quats [5][n][4], wrap [5][n]): a sweep inside a cone, one whose az crosses 0 / 2 pi, one that sweeps 3.4 rad, one
    with az over the full circle that begins with the ``WRAP_PHI`` quaternions, and a second cone.  Elevations of the
    last four lie in [0.1, 1.4]."""
    rng = np.random.default_rng(4000 + n)
    u = (np.arange(n) + 0.5) / n
    quats = np.zeros((len(RANGE_ROWS), n, 4))
    wrap = np.zeros((len(RANGE_ROWS), n), dtype=bool)
    az = 0.33 + 0.34 * (0.5 - 0.5 * np.cos(5 * np.pi * u)) + rng.uniform(-0.004, 0.004, n)
    quats[0] = ac.quat_from_azel(az, 0.65 + 0.2 * rng.uniform(0, 1, n))
    az = np.mod(6.2 + 0.2 * u + rng.uniform(-0.01, 0.01, n), TWOPI)
    quats[1] = ac.quat_from_azel(az, rng.uniform(0.1, 1.4, n))
    az = np.mod(0.3 + 3.4 * u + rng.uniform(-0.002, 0.002, n), TWOPI)
    quats[2] = ac.quat_from_azel(az, rng.uniform(0.1, 1.4, n))
    quats[3] = ac.quat_from_azel(rng.uniform(0, TWOPI, n), rng.uniform(0.1, 1.4, n))
    k = min(n, len(WRAP_PHI))
    quats[3, :k] = quat_from_angles(PI_2 - rng.uniform(0.1, 1.4, k), np.array(WRAP_PHI[:k]))
    wrap[3, :k] = True
    az = 0.36 + 0.3 * (0.5 + 0.5 * np.sin(3 * np.pi * u)) + rng.uniform(-0.004, 0.004, n)
    quats[4] = ac.quat_from_azel(az, 0.7 + 0.15 * rng.uniform(0, 1, n))
    return denormalise(quats, rng), wrap


# ------------------------------------------------------------------------------------------------- flags
PATTERNS = ("random", "first", "last", "s256", "from256", "none", "outside", "no_det", "no_shared", "neither")


def flag_pattern(name, n, entries, seed):
    """(det flags [entries][n] or None, shared flags [n] or None) of a pattern, or None where ``n`` has no such
    pattern.  Every array carries bits outside both masks.  The named pattern is that of the even entries; the odd
    ones are random, so that a row without a good sample stands next to rows with some."""
    if name in ("s256", "from256") and n <= 256:
        return None
    rng = np.random.default_rng(seed)
    i = np.arange(n)

    def noise(shape, mask):
        out = rng.integers(0, 256, shape).astype(np.uint8) & np.uint8(0xFF & ~mask)
        return np.where(rng.uniform(size=shape) < 0.3, out, 0).astype(np.uint8)

    def some(shape, frac, values):
        return np.where(rng.uniform(size=shape) < frac, rng.choice(values, shape), 0).astype(np.uint8)

    det = noise((entries, n), DET_MASK)
    shared = noise(n, SHARED_MASK)
    rand_det = some((entries, n), 0.2, [1, 2, 3])
    if name == "random":
        det |= rand_det
        shared |= some(n, 0.12, [1, 4, 5])
    elif name in ("first", "last", "s256", "from256", "none"):
        bad = {"first": i != 0, "last": i != n - 1, "s256": i != 256, "from256": i < 256, "none": i >= 0}[name]
        if name == "none" and entries == 1:
            shared |= np.uint8(4)                                   # the telescope flags alone can empty a row
        else:
            for e in range(entries):
                det[e] |= np.where(bad, rng.choice([1, 2, 3], n), 0).astype(np.uint8) if e % 2 == 0 else rand_det[e]
    elif name == "no_det":
        det = None
        shared |= some(n, 0.3, [1, 4, 5])
    elif name == "no_shared":
        shared = None
        det |= some((entries, n), 0.3, [1, 2, 3])
    elif name == "neither":
        det = shared = None
    return det, shared


def good_host(det_row, shared, n, det_mask=DET_MASK, shared_mask=SHARED_MASK):
    """sim_tod_atm_observe.py:240-255: the samples a detector observes, as the kernel's bytes."""
    bits = np.zeros(n, dtype=np.uint8)
    if det_row is not None:
        bits |= det_row & np.uint8(det_mask)
    if shared is not None:
        bits |= shared & np.uint8(shared_mask)
    return (bits == 0).astype(np.uint8)


def ranges_host(good, az, el):
    """The eight values k_atm_good_ranges reports of a row, from the az / el the device computes of its samples:
    float64 NumPy min / max with the kernel's wrap statement."""
    idx = np.nonzero(good)[0]
    if idx.size == 0:
        return np.array([-1.0, -1.0, 0, 0, 0, 0, 0, 0])
    d = az[idx] - az[idx[0]]
    d = np.where(d >= np.pi, d - TWOPI, d)
    d = np.where(d < -np.pi, d + TWOPI, d)
    return np.array([idx[0], idx[-1], el[idx].min(), el[idx].max(), az[idx[0]], d.min(), d.max(), 0.0])


#: scratch values of good samples in the flag_failed cases: the threshold is |atm| < 1e-30, NaN compares false
FAILED_VALUES = (0.0, -0.0, 1e-31, -1e-31, 1e-30, 1e-29, np.nan)


def flag_failed_case(n, entries, seed):
    """(good [entries][n], atm [entries][n], flags before [entries][n], enable [entries]): every value of
    ``FAILED_VALUES`` on good samples where n allows, 0.0 on a sample that is not good, earlier bits in the flags."""
    rng = np.random.default_rng(seed)
    good = (rng.uniform(size=(entries, n)) < 0.7).astype(np.uint8)
    atm = rng.standard_normal((entries, n)) * 3.0
    pick = rng.uniform(size=(entries, n)) < 0.4
    atm[pick] = rng.choice(FAILED_VALUES, int(pick.sum()))
    for e in range(entries):
        if n >= 2 * len(FAILED_VALUES):
            at = rng.permutation(n)[:len(FAILED_VALUES) + 1]
            good[e, at[:-1]] = 1
            atm[e, at[:-1]] = FAILED_VALUES
            good[e, at[-1]] = 0
            atm[e, at[-1]] = 0.0
    flags = rng.integers(0, 256, (entries, n)).astype(np.uint8)
    flags[rng.uniform(size=(entries, n)) < 0.5] = 0
    enable = np.array([(1, 0, 1, 1, 0)[e % 5] for e in range(entries)], dtype=np.int32)
    return good, atm, flags, enable


def flag_failed_host(good, atm, flags, enable, mask):
    """sim_tod_atm_observe.py:379-399 with the mask raised: (flags after, n_bad per entry)."""
    out = flags.copy()
    n_bad = np.zeros(len(enable), dtype=np.int64)
    for e in range(len(enable)):
        if enable[e]:
            bad = (good[e] != 0) & (np.abs(atm[e]) < 1e-30)
            out[e, bad] |= np.uint8(mask)
            n_bad[e] = bad.sum()
    return out, n_bad


# ------------------------------------------------------------------------------------------------- finish
def finish_terms(atm, ga, w_i, w_q, pfrac, loading, el, kind):
    """(atm ga) (w_i + w_q pfrac) and loading / sin el in the number type ``kind``."""
    a = atm.astype(kind) * kind(ga)
    a = a * (np.asarray(w_i).astype(kind) + np.asarray(w_q).astype(kind) * kind(pfrac))
    load = np.zeros_like(a) if loading is None else kind(loading) / np.sin(np.asarray(el).astype(kind))
    return a, load


def finish_host(before, atm, ga, w_i, w_q, pfrac, loading, el, scale):
    """k_atm_finish (sim_tod_atm_observe.py:424-483) in float64 NumPy, one rounding per operation, in its order."""
    v = atm * ga
    v = v * (w_i + w_q * pfrac)
    if loading is not None:
        v = v + loading / np.sin(el)
    return before + scale * v


def finish_longdouble(before, atm, ga, w_i, w_q, pfrac, loading, el, scale):
    """(out, scale_i): before + scale ((atm ga)(w_i + w_q pfrac) + loading / sin el) in long double, and
    |scale| (|atm ga w| + |loading / sin el|) + |before|."""
    a, load = finish_terms(atm, ga, w_i, w_q, pfrac, loading, el, L)
    out = before.astype(L) + L(scale) * (a + load)
    return out, (abs(scale) * (np.abs(a) + np.abs(load)) + np.abs(before)).astype(np.float64)


WEIGHT_MODES = {None: (0, 0, -1), "I": (1, 0, -1), "QU": (2, -1, 0), "IQU": (3, 0, 1)}   # nnz, comp_i, comp_q


def weight_components(weights, mode, n):
    """(w_i, w_q) [n] of a row of weights [n][nnz], as the kernel reads them."""
    if mode is None:
        return np.ones(n), np.zeros(n)
    _, ci, cq = WEIGHT_MODES[mode]
    return (weights[:, ci] if ci >= 0 else np.zeros(n)), (weights[:, cq] if cq >= 0 else np.zeros(n))


def make_weights(shape, nnz, rng):
    """Stokes weights [...][nnz] of the modes above: I = 1, |Q|, |U| <= 0.8."""
    cols = {1: ["i"], 2: ["q", "u"], 3: ["i", "q", "u"]}[nnz]
    psi = rng.uniform(0, TWOPI, shape)
    col = {"i": np.ones(shape), "q": 0.8 * np.cos(psi), "u": 0.8 * np.sin(psi)}
    return np.stack([col[c] for c in cols], axis=-1)


# ------------------------------------------------------------------------------------------------- pointing in the cone
def cone_rows(n, entries, seed, phase0=0.0):
    """(times [n], quats [entries][n][4]): sweeps through the cone of the volumes as ``ac.operator_inputs`` draws them,
    every az / el more than 1e-6 rad inside the cone, every time inside tmin .. tmax; the sweep of row d is ahead
    by ``phase0 + 0.4 d``."""
    rng = np.random.default_rng(seed)
    g = ac.BASE
    u = (np.arange(n) + 0.5) / n
    times = g["tmin"] + 0.5 + 10.0 * u
    quats = np.zeros((entries, n, 4))
    for d in range(entries):
        sweep = 0.5 - 0.5 * np.cos(6 * np.pi * u + phase0 + 0.4 * d)
        az = g["azmin"] + 0.03 + 0.32 * sweep + rng.uniform(-0.004, 0.004, n)
        # the band of elevations in which the volumes with holes take some, and at most a quarter, of a row's samples
        el = g["elmin"] + 0.165 + 0.004 * d + 0.05 * np.sin(4 * np.pi * u) + rng.uniform(-0.004, 0.004, n)
        quats[d] = ac.quat_from_azel(az, el)
    return times, denormalise(quats, rng)


OBSERVE_VOLUMES = (("holes",), ("full",), ("near", "far"))
OBSERVE_ENTRIES = (1, 4)


@functools.lru_cache(maxsize=None)
def observe_case(n, entries):
    """(times, quats [entries][n][4], det flags [entries][n]) of an observe_quats shape; a fifth of the samples is
    flagged."""
    times, quats = cone_rows(n, entries, 5000 + 10 * n + entries)
    rng = np.random.default_rng(6000 + 10 * n + entries)
    flags = np.where(rng.uniform(size=(entries, n)) < 0.2, rng.choice([1, 2, 3], (entries, n)), 0).astype(np.uint8)
    if n == 1:
        flags[:] = 0
    return times, quats, flags


def cone_margin(vol_geom, az, el):
    """Smallest distance [rad] of the (long double) az / el from the edges of the cone, az taken modulo 2 pi; negative
    outside."""
    g = vol_geom
    az = np.where(az > g["azmax"] + 1.0, az - L(TWOPI), az)
    return float(min(np.min(az - g["azmin"]), np.min(g["azmax"] - az), np.min(el - g["elmin"]), np.min(g["elmax"] - el)))


def observe_conditions(kinds, times, quats_row, good):
    """What keeps a comparison of two evaluations honest, for the good samples of one row through the slabs ``kinds``:
    (face, cell0, failed [n_good], margin)."""
    use = np.asarray(good) != 0
    az, el = longdouble_azel(quats_row[use])
    face, cell0, failed = np.inf, False, np.zeros(int(use.sum()), dtype=bool)
    margin = np.inf
    for kind in kinds:
        vol = ac.volume(kind)
        ld = ac.longdouble_observe(vol, times[use], az, el)
        assert not np.any(ld["skip"])
        face, cell0 = min(face, ld["face"]), cell0 or ld["cell0"]
        failed |= ld["failed"]
        margin = min(margin, cone_margin(vol[0], az, el))
    return face, cell0, failed, margin


@functools.lru_cache(maxsize=None)
def two_pointings():
    """(time, quats [2][1][4]) for the launches of 65 537 rows of one sample: at one time, a line of sight that fails in
    the ``holes`` volume and one that does not, taken from a grid over the cone."""
    rng = np.random.default_rng(31)
    az, el = (x.reshape(-1) for x in np.meshgrid(np.linspace(0.33, 0.67, 12), np.linspace(0.63, 0.87, 9)))
    quats = denormalise(ac.quat_from_azel(az, el), rng)
    times = np.full(az.size, 105.25)
    _, _, failed, _ = observe_conditions(("holes",), times, quats, np.ones(az.size))
    k_fail, k_ok = int(np.nonzero(failed)[0][0]), int(np.nonzero(~failed)[0][0])
    return 105.25, quats[[k_fail, k_ok]].reshape(2, 1, 4)


# ------------------------------------------------------------------------------------------------- the operator case
OP_DETS = ["D0", "D1", "D2", "D3"]
OP_N = 600
OP_VIEWS = [(0, 257), (257, 600)]
OP_PHASE = 0.4                     # with it every detector loses samples to the holes in both views
OP_WHOLLY_FLAGGED = 2              # this detector is flagged throughout the first view
OP = dict(ac.OP, absorption={"D0": 0.11, "D1": 0.12, "D2": 0.13, "D3": 0.14},
          loading={"D0": 2.5, "D1": 2.75, "D2": 3.0, "D3": 3.25})
#: the traits that differ from ``ac.operator()`` and what the observation holds for them
VARIANTS = {
    "defaults": dict(),
    "no_weights": dict(traits=dict(weights=None)),
    "weights_I": dict(traits=dict(weights_mode="I"), nnz=1),
    "weights_QU": dict(traits=dict(weights_mode="QU"), nnz=2),
    "no_loading": dict(traits=dict(loading=None)),
    "no_det_flags": dict(traits=dict(det_flags=None), det_flags=False),
    "no_shared_flags": dict(traits=dict(shared_flags=None)),
    "subset": dict(detectors=["D3", "D1"]),
    "kelvin": dict(units="K"),
}
VIEW_FORMS = ("wind", None)


@functools.lru_cache(maxsize=None)
def operator_inputs(nnz=3):
    """times, quats [det][samp][4], weights [det][samp][nnz], shared flags, detector flags, signal before."""
    n, nd = OP_N, len(OP_DETS)
    times, quats = cone_rows(n, nd, 78, OP_PHASE)
    rng = np.random.default_rng(79)
    shared = np.where(rng.uniform(size=n) < 0.05, rng.choice([1, 4, 5], n), 0).astype(np.uint8)
    shared[[10, 100, 300]] = 2            # not in the mask
    shared[[256, 257]] = 4
    det_flags = np.where(rng.uniform(size=(nd, n)) < 0.08, rng.choice([1, 2, 3], (nd, n)), 0).astype(np.uint8)
    det_flags[3, [5, 270]] = 4            # not in the mask
    det_flags[OP_WHOLLY_FLAGGED, :OP_VIEWS[0][1]] |= 1
    signal = rng.standard_normal((nd, n)) * 10.0
    weights = make_weights((nd, n), nnz, np.random.default_rng(80))
    return dict(times=times, quats=quats, weights=weights, shared_flags=shared, det_flags=det_flags, signal=signal)


#: the slabs of each wind interval; one view over the whole observation stays in the first (``_wind_index``)
OP_SLABS = [["holes"], ["near", "far"]]


def operator_data(variant):
    """(data, observation, operator, detectors) of a variant: four detectors, 600 samples, wind intervals
    ``OP_VIEWS``."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults

    spec = VARIANTS[variant]
    inp = operator_inputs(spec.get("nnz", 3))
    fp = Focalplane(OP_DETS, np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (len(OP_DETS), 1)), sample_rate=60.0)
    ob = Observation(None, Telescope("atm_tele", fp), OP_N, name="obs_atm_grid")
    ob.set_times(inp["times"].copy())
    ob.shared.create(defaults.shared_flags, inp["shared_flags"].copy())
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=spec.get("units", "mK"))
    ob.detdata.create(defaults.quats_azel, sample_shape=(4,), dtype=np.float64)
    ob.detdata.create(defaults.weights, sample_shape=(inp["weights"].shape[-1],), dtype=np.float64)
    if spec.get("det_flags", True):
        ob.detdata.create(defaults.det_flags, dtype=np.uint8)
    for i, d in enumerate(OP_DETS):
        ob.detdata[defaults.det_data][d] = inp["signal"][i]
        ob.detdata[defaults.quats_azel][d] = inp["quats"][i]
        ob.detdata[defaults.weights][d] = inp["weights"][i]
        if spec.get("det_flags", True):
            ob.detdata[defaults.det_flags][d] = inp["det_flags"][i]
    ob.intervals.create("wind", list(OP_VIEWS))
    ob["absorption"] = dict(OP["absorption"])
    ob["loading"] = dict(OP["loading"])
    data = Data()
    data.obs.append(ob)
    data["atm_sim"] = {ob.session.name: [[ac.make_sim(ac.volume(kind)) for kind in kinds]
                                         for kinds in OP_SLABS]}
    return data, ob, spec.get("detectors")


def operator_of(variant, view):
    return ac.operator(view=view, **VARIANTS[variant].get("traits", {}))


def close_sims(data, ob):
    for slabs in data["atm_sim"][ob.session.name]:
        for sim in slabs:
            sim.close()


def operator_views(view):
    """[(first, last, slab kinds)] of a view form."""
    if view is None:
        return [(0, OP_N, OP_SLABS[0])]
    return [(a, b, OP_SLABS[k]) for k, (a, b) in enumerate(OP_VIEWS)]


def operator_good(variant, d, first, last):
    """The good samples of detector ``d`` in a view, by ``good_host``."""
    spec = VARIANTS[variant]
    traits = spec.get("traits", {})
    inp = operator_inputs(spec.get("nnz", 3))
    det = inp["det_flags"][d, first:last] if spec.get("det_flags", True) and "det_flags" not in traits else None
    sh = None if "shared_flags" in traits else inp["shared_flags"][first:last]
    return good_host(det, sh, last - first, OP["det_flag_mask"], OP["shared_flag_mask"])


def restated_operator(variant, view):
    """(signal, flags or None) of a variant from the restatements: ``good_host``, ``quats_to_azel`` and
    ``AtmSim.observe`` on the host for the scratch rows, ``flag_failed_host`` after a slab that reported a failure,
    ``finish_host``.  Also returns the long-double finish of the same scratch rows and its scale, for the bound."""
    from toast_amd.ops.sim_tod_atm_observe import quats_to_azel
    from toast_amd.data import KELVIN_TO

    spec = VARIANTS[variant]
    traits = spec.get("traits", {})
    inp = operator_inputs(spec.get("nnz", 3))
    dets = [OP_DETS.index(d) for d in (spec.get("detectors") or OP_DETS)]
    mode = None if "weights" in traits else traits.get("weights_mode", "IQU")
    with_flags = spec.get("det_flags", True)
    scale = KELVIN_TO[spec.get("units", "mK")]
    signal, ld_signal = inp["signal"].copy(), inp["signal"].astype(L)
    scale_i = np.zeros(signal.shape)
    flags = inp["det_flags"].copy() if with_flags else None
    for first, last, kinds in operator_views(view):
        n = last - first
        times = inp["times"][first:last]
        good = np.stack([operator_good(variant, d, first, last) for d in dets])
        atm = np.zeros((len(dets), n))
        az, el = np.zeros((len(dets), n)), np.zeros((len(dets), n))
        for k, d in enumerate(dets):
            az[k], el[k] = quats_to_azel(inp["quats"][d, first:last])
        for kind in kinds:
            sim = ac.make_sim(ac.volume(kind))
            status = np.zeros(len(dets), dtype=np.int32)
            for k in range(len(dets)):
                use = good[k] != 0
                if not use.any():
                    continue
                row = np.ascontiguousarray(atm[k, use])
                status[k] = sim.observe(np.ascontiguousarray(times[use]), np.ascontiguousarray(az[k, use]),
                                        np.ascontiguousarray(el[k, use]), row, -1.0, use_accel=False)
                atm[k, use] = row
            sim.close()
            if np.any(status != 0) and with_flags:
                after, _ = flag_failed_host(good, atm, flags[dets, first:last], status, OP["det_flag_mask"])
                flags[dets, first:last] = after
        for k, d in enumerate(dets):
            use = good[k] != 0
            w_i, w_q = weight_components(inp["weights"][d, first:last], mode, n)
            args = (atm[k], OP["gain"] * OP["absorption"][OP_DETS[d]], w_i, w_q, OP["polarization_fraction"],
                    None if "loading" in traits else OP["loading"][OP_DETS[d]], el[k], scale)
            out = finish_host(inp["signal"][d, first:last], *args)
            out_ld, sc = finish_longdouble(inp["signal"][d, first:last], *args)
            signal[d, first:last][use] = out[use]
            ld_signal[d, first:last][use] = out_ld[use]
            scale_i[d, first:last][use] = sc[use]
    return signal, flags, ld_signal, scale_i
