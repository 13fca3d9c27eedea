"""Seeded inputs of the Fourier2D template fixture (tests/golden/fourier2d.npz): the SAME observations are built by
tests/golden/make_golden_fourier2d.py -- which drives the reference's own template methods -- and by the host and GPU
tests, which hand them to ``toast_amd.templates.Fourier2D``.  NumPy + the host-side data model only (no device, no oracle).

Layouts (ragged views with gaps; in the two-observation layouts detector ``d1`` is missing from the second observation,
whose second view has an odd number of samples, so that its filter has one tap less than the view has samples):
  short   d0..d4; views of 50, 2 and 1400 samples / 500 and 601.  One sample is flagged in every detector: its norm is 0
  long    d0..d4; views of 64, 4100 (17 sample tiles) and 181 samples / 500 and 601
  wide    70 detectors x 700 samples in one observation: more detectors than a wave has lanes and three sample tiles, so
          the rule splits the detectors over the grid

The focal plane is spread (a spiral out to 0.9 degrees from the boresight): the modes differ from detector to detector,
and ``check_rank`` asserts that the basis has full rank.  Every detector carries ~30 % random solver flags in bit 1 and
unrelated bits in 4 that the mask must ignore.

The fixture holds the results on a subset of the samples (``sample_subset``): the first and last three samples of every
view and those next to a multiple of 64 (the edges of the kernels' tiles of 64 and 256 samples), plus the sample that is
flagged everywhere; whole vectors would not fit a committed file.
"""
import numpy as np

DET_FLAG_MASK = 1
DET_DATA = "signal"
DET_FLAGS = "flags"
NOISE = "noise_model"
VIEW = "scan"
RATE = 10.0
ALL_FLAGGED = ("short", 0, 777)      # layout, observation, sample: flagged in every detector

_TWO = [dict(n_samp=1201, views=[(0, 500), (560, 1161)], dets=("d0", "d2", "d3", "d4"))]
LAYOUTS = {
    "short": dict(seed=8101, dets=5, obs=[dict(n_samp=1500, views=[(10, 60), (80, 82), (100, 1500)],
                                               dets=("d0", "d1", "d2", "d3", "d4"))] + _TWO),
    "long": dict(seed=8102, dets=5, obs=[dict(n_samp=4401, views=[(3, 67), (71, 4171), (4200, 4381)],
                                              dets=("d0", "d1", "d2", "d3", "d4"))] + _TWO),
    "wide": dict(seed=8103, dets=70, obs=[dict(n_samp=700, views=[(0, 300), (320, 700)],
                                               dets=tuple(f"d{k}" for k in range(70)))]),
}

# fixture cases: name -> (layout, traits).  nmode 5, 7, 17, 19, 37, 39; "floor": a correlation length at which the
# floor of the filter replaces hundreds of frequencies; "above": one order above what the device kernels take
CASES = {
    "m5": ("short", dict(order=1, fit_subharmonics=False, noise_model=None)),
    "m7": ("short", dict(order=1, fit_subharmonics=True, noise_model=NOISE)),
    "m17": ("long", dict(order=2, fit_subharmonics=False, noise_model=NOISE)),
    "m19": ("long", dict(order=2, fit_subharmonics=True, noise_model=None)),
    "m37": ("wide", dict(order=3, fit_subharmonics=False, noise_model=None)),
    "m39": ("wide", dict(order=3, fit_subharmonics=True, noise_model=NOISE)),
    "floor": ("short", dict(order=1, fit_subharmonics=True, noise_model=None, correlation_length=1.0e5)),
    "above": ("wide", dict(order=4, fit_subharmonics=False, noise_model=NOISE)),
}
DEVICE_CASES = tuple(c for c in CASES if c != "above")


class DetectorWeights:
    """The part of a noise model the templates read: ``detector_weight(det)`` in 1 / signal units^2."""

    def __init__(self, weights):
        self._w = dict(weights)

    def detector_weight(self, det):
        return self._w[det]


def focalplane_quats(n_det):
    """Detector k looks ``0.9 deg * sqrt((k + 1) / n_det)`` away from the boresight, at the golden angle times k."""
    k = np.arange(n_det)
    ang = np.radians(0.9) * np.sqrt((k + 1.0) / n_det)
    azim = k * np.pi * (3.0 - np.sqrt(5.0))
    # rotation by `ang` about the axis (cos azim, sin azim, 0)
    return np.stack([np.sin(ang / 2) * np.cos(azim), np.sin(ang / 2) * np.sin(azim), np.zeros(n_det), np.cos(ang / 2)], axis=1)


def build(layout):
    """-> toast_amd.data.Data with the observations of ``layout``: signal, solver flags, time stamps, the view ``VIEW``
    and detector weights."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope

    cfg = LAYOUTS[layout]
    all_dets = tuple(f"d{k}" for k in range(cfg["dets"]))
    quats = focalplane_quats(len(all_dets))
    data = Data()
    for iob, ocfg in enumerate(cfg["obs"]):
        rng = np.random.default_rng(cfg["seed"] * 10 + iob)
        n_samp, dets = ocfg["n_samp"], list(ocfg["dets"])
        fp = Focalplane(all_dets, quats, sample_rate=RATE)
        ob = Observation(data.comm, Telescope("tele", fp), n_samp, name=f"obs{iob}", detectors=dets)
        ob.set_times(np.arange(n_samp) / RATE + 1000.0 * iob)
        ob.intervals.create(VIEW, ocfg["views"])
        ob.detdata.create(DET_DATA, dtype=np.float64)
        ob.detdata.create(DET_FLAGS, dtype=np.uint8)
        sig = ob.detdata[DET_DATA].data
        flg = ob.detdata[DET_FLAGS].data
        sig[:] = rng.standard_normal(sig.shape) + 0.25 * np.arange(len(dets))[:, None]
        flg[:] = (rng.random(sig.shape) < 0.3).astype(np.uint8) * DET_FLAG_MASK
        flg[:] |= (rng.random(sig.shape) < 0.2).astype(np.uint8) * 4
        if (layout, iob) == ALL_FLAGGED[:2]:
            flg[:, ALL_FLAGGED[2]] |= DET_FLAG_MASK
        ob[NOISE] = DetectorWeights({d: 0.5 + 0.75 * (k % 7) for k, d in enumerate(all_dets)})
        data.obs.append(ob)
    return data


def amplitudes(n_local, seed):
    """Input amplitudes: seed 1 add_to_signal / apply_precond / add_prior, seed 2 what project_signal adds on top of."""
    return np.random.default_rng(seed).standard_normal(n_local)


def configure(tmpl, view=VIEW, det_flags=DET_FLAGS):
    """The traits TemplateMatrix would set."""
    tmpl.view = view
    tmpl.det_data = DET_DATA
    tmpl.det_flags = det_flags
    tmpl.det_flag_mask = DET_FLAG_MASK
    tmpl.det_mask = 1
    return tmpl


def view_samples(layout):
    """-> per observation the list of (first, last) of its views, in amplitude order."""
    return [list(o["views"]) for o in LAYOUTS[layout]["obs"]]


def sample_subset(layout):
    """-> (rows, cols): ``rows`` index the samples counted through all views of all observations (the amplitude rows),
    ``cols[iob]`` the same samples as indices into the observation."""
    rows, cols, cum = [], [], 0
    for iob, views in enumerate(view_samples(layout)):
        c = []
        for first, last in views:
            n = last - first
            i = np.arange(n)
            keep = (i < 3) | (i >= n - 3) | (i % 64 == 0) | (i % 64 == 63)
            if (layout, iob) == ALL_FLAGGED[:2] and first <= ALL_FLAGGED[2] < last:
                keep[ALL_FLAGGED[2] - first] = True
            rows.append(cum + i[keep])
            c.append(first + i[keep])
            cum += n
        cols.append(np.concatenate(c))
    return np.concatenate(rows), cols


def all_flagged_row(layout):
    """Index of the all-flagged sample among the amplitude rows, or None."""
    if layout != ALL_FLAGGED[0]:
        return None
    cum = 0
    for iob, views in enumerate(view_samples(layout)):
        for first, last in views:
            if iob == ALL_FLAGGED[1] and first <= ALL_FLAGGED[2] < last:
                return cum + ALL_FLAGGED[2] - first
            cum += last - first
    return None


def check_rank(templates):
    """``templates``: [n_det][nmode] of one observation.  Full rank; full COLUMN rank where there are detectors enough."""
    t = np.asarray(templates)
    rank = np.linalg.matrix_rank(t)
    assert rank == min(t.shape), (rank, t.shape)
    return rank


# ------------------------------------------------------------------ end-to-end case: MapMaker over [Offset, Fourier2D]
E2E = dict(n_det=8, n_samp=3000, rate=50.0, nside=16, step_time=2.0, iters=8, seed=8201, order=1, fit_subharmonics=True,
           correlation_length=5.0, correlation_amplitude=10.0)
E2E_NAMES = ("baselines", "fourier2d")


def term_scales(name, templates):
    """sum|terms| of every output the fixture holds, for bounds in units of eps * sum|terms|.  ``templates[iob]``:
    [n_det][nmode] in the observation's detector order.  -> (add[iob] as [n_det][cols], project as [rows][nmode])"""
    layout, _ = CASES[name]
    data = build(layout)
    rows, cols = sample_subset(layout)
    nmode = np.asarray(templates[0]).shape[1]
    n_total = sum(last - first for views in view_samples(layout) for first, last in views)
    a_add = np.abs(amplitudes(n_total * nmode, 1).reshape(-1, nmode))
    a_proj = np.abs(amplitudes(n_total * nmode, 2).reshape(-1, nmode))
    add, project, at = [], [], 0
    for iob, ob in enumerate(data.obs):
        t = np.abs(np.asarray(templates[iob]))
        sig = np.abs(ob.detdata[DET_DATA].data[:, cols[iob]])
        r = rows[at:at + cols[iob].size]
        at += cols[iob].size
        add.append(sig + t @ a_add[r].T)
        project.append(a_proj[r] + sig.T @ t)
    return add, np.concatenate(project)


def build_e2e():
    """-> (data, cfg): one satellite observation (toast_amd.sim.create_satellite_data, a hex focal plane of 10 degrees)
    with a smooth sky, white noise, baseline drifts per detector and a slow common mode with a gradient across the
    focal plane -- what the Fourier2D amplitudes are there to take up."""
    from toast_amd.data import defaults, detector_direction
    from toast_amd.sim import create_satellite_data

    cfg = dict(E2E)
    n_det, n_samp, rate = cfg["n_det"], cfg["n_samp"], cfg["rate"]
    data = create_satellite_data(comm=None, n_det=n_det, total_det=n_det, first_det=0, n_samp=n_samp, rate=rate,
                                 spin_period_s=20.0, spin_angle_deg=30.0, prec_period_s=60.0, prec_angle_deg=65.0,
                                 net=1.0, fknee=0.05, seed=cfg["seed"])
    ob = data.obs[0]
    sig = ob.detdata[defaults.det_data].data
    bore = ob.shared[defaults.boresight_radec].data
    z = 1.0 - 2.0 * (bore[:, 0] ** 2 + bore[:, 1] ** 2)
    x = 2.0 * (bore[:, 0] * bore[:, 2] + bore[:, 1] * bore[:, 3])
    sky = 3.0 * z + 2.0 * x * z
    step = int(np.rint(cfg["step_time"] * rate))
    t = np.arange(n_samp) / rate
    common = 4.0 * np.sin(2.0 * np.pi * t / 23.0) + 0.05 * t
    fp = ob.telescope.focalplane
    for d, det in enumerate(ob.local_detectors):
        rng = np.random.default_rng(cfg["seed"] * 1000 + d)
        dx, dy, _ = detector_direction(fp[det]["quat"])
        sig[d] = sky * (1.0 + 0.01 * d) + rng.standard_normal(n_samp)
        walk = np.cumsum(rng.standard_normal((n_samp + 2 * step - 1) // (2 * step))) * 0.5
        sig[d] += np.repeat(walk, 2 * step)[:n_samp]
        sig[d] += common * (1.0 + 6.0 * dx - 4.0 * dy)
    return data, cfg
