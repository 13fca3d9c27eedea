"""Seeded inputs of the SubHarmonic / Periodic template fixture (tests/golden/templates_basis.npz): the SAME observations
are built by tests/golden/make_golden_templates.py -- which drives the reference's own template methods -- and by the host
and GPU tests, which hand them to ``toast_amd.templates``.  NumPy + the host-side data model only (no device, no oracle).

Layouts (two observations each; detector ``d1`` is missing from the second one; ragged views with gaps):
  tiny    views of 50, 1, 2 and 1400 samples / 500 and 600: SubHarmonic order 0 and the Periodic cases
  short   as ``tiny`` without the view of one sample (its Gram matrix is singular from order 1 on): order 1
  long    views of 64, 4100 (two reduction chunks) and 180 samples / 500 and 600, odd row length: orders 3 and 8

Every detector carries ~30 % random solver flags in bit 1 (views shorter than 8 samples stay unflagged, so that their
preconditioner exists) and unrelated bits in 2 and 4 that the masks must ignore.  The Periodic key is a slow sweep plus
noise; the first view covers only part of its range, so that several bins reach ``minimum_bin_hits`` only in a later view
(the reference flags them for good), and the key's largest value lies exactly on the top edge of the last bin.
"""
import numpy as np

DET_FLAG_MASK = 1
KEY_FLAG_MASK = 2
DET_DATA = "signal"
DET_FLAGS = "flags"
KEY = "azimuth"
KEY_FLAGS = "az_flags"
NOISE = "noise_model"
VIEW = "scan"

LAYOUTS = {
    "tiny": dict(seed=7101, obs=[dict(n_samp=1500, views=[(10, 60), (70, 71), (80, 82), (100, 1500)], dets=("d0", "d1", "d2")),
                                 dict(n_samp=1201, views=[(0, 500), (560, 1160)], dets=("d0", "d2"))]),
    "short": dict(seed=7102, obs=[dict(n_samp=1500, views=[(10, 60), (80, 82), (100, 1500)], dets=("d0", "d1", "d2")),
                                  dict(n_samp=1201, views=[(0, 500), (560, 1160)], dets=("d0", "d2"))]),
    "long": dict(seed=7103, obs=[dict(n_samp=4401, views=[(3, 67), (71, 4171), (4200, 4380)], dets=("d0", "d1", "d2")),
                                 dict(n_samp=1201, views=[(0, 500), (560, 1160)], dets=("d0", "d2"))]),
}

# fixture cases: name -> (layout, template class, traits)
SUBHARMONIC_CASES = {
    "sub0": ("tiny", dict(order=0, noise_model=None)),
    "sub1": ("short", dict(order=1, noise_model=None)),
    "sub3": ("long", dict(order=3, noise_model=NOISE)),
    "sub8": ("long", dict(order=8, noise_model=NOISE)),
}
PERIODIC_CASES = {
    "per_bins": ("tiny", dict(key=KEY, flags=KEY_FLAGS, flag_mask=KEY_FLAG_MASK, bins=7, increment=None, minimum_bin_hits=3)),
    "per_incr": ("tiny", dict(key=KEY, flags=KEY_FLAGS, flag_mask=KEY_FLAG_MASK, bins=None, increment=7.5,
                              minimum_bin_hits=5)),
    "per_noflags": ("tiny", dict(key=KEY, flags=None, flag_mask=0, bins=12, increment=None, minimum_bin_hits=3)),
}


class DetectorWeights:
    """The part of a noise model the templates read: ``detector_weight(det)`` in 1 / signal units^2."""

    def __init__(self, weights):
        self._w = dict(weights)

    def detector_weight(self, det):
        return self._w[det]


def build(layout):
    """-> toast_amd.data.Data with the observations of ``layout``: signal, solver flags, the key with its own flags, the
    view ``VIEW`` and detector weights."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope

    cfg = LAYOUTS[layout]
    all_dets = ("d0", "d1", "d2")
    quats = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (len(all_dets), 1))
    data = Data()
    for iob, ocfg in enumerate(cfg["obs"]):
        rng = np.random.default_rng(cfg["seed"] * 10 + iob)
        n_samp, dets = ocfg["n_samp"], list(ocfg["dets"])
        fp = Focalplane(all_dets, quats, sample_rate=10.0)
        ob = Observation(data.comm, Telescope("tele", fp), n_samp, name=f"obs{iob}", detectors=dets)
        ob.set_times(np.arange(n_samp) / 10.0 + 1000.0 * iob)
        ob.intervals.create(VIEW, ocfg["views"])
        ob.detdata.create(DET_DATA, dtype=np.float64)
        ob.detdata.create(DET_FLAGS, dtype=np.uint8)
        sig = ob.detdata[DET_DATA].data
        flg = ob.detdata[DET_FLAGS].data
        sig[:] = rng.standard_normal(sig.shape) + 0.25 * np.arange(len(dets))[:, None]
        flg[:] = (rng.random(sig.shape) < 0.3).astype(np.uint8) * DET_FLAG_MASK
        flg[:] |= (rng.random(sig.shape) < 0.2).astype(np.uint8) * 4
        for first, last in ocfg["views"]:
            if last - first < 8:
                flg[:, first:last] &= ~np.uint8(DET_FLAG_MASK)
        i = np.arange(n_samp)
        az = 50.0 + 40.0 * np.sin(2.0 * np.pi * (i + 30.0) / 900.0) + 0.5 * rng.standard_normal(n_samp)
        ob.shared.create(KEY, az)
        kf = (rng.random(n_samp) < 0.1).astype(np.uint8) * KEY_FLAG_MASK
        kf |= (rng.random(n_samp) < 0.2).astype(np.uint8) * 1
        ob.shared.create(KEY_FLAGS, kf)
        ob[NOISE] = DetectorWeights({d: 0.5 + 0.75 * k for k, d in enumerate(all_dets)})
        data.obs.append(ob)
    return data


def amplitudes(n_local, seed):
    """Input amplitudes of the add_to_signal / apply_precond cases."""
    return np.random.default_rng(seed).standard_normal(n_local)


def configure(tmpl, view=VIEW, det_flags=DET_FLAGS):
    """The traits TemplateMatrix would set."""
    tmpl.view = view
    tmpl.det_data = DET_DATA
    tmpl.det_flags = det_flags
    tmpl.det_flag_mask = DET_FLAG_MASK
    tmpl.det_mask = 1
    return tmpl


# ------------------------------------------------------------------ end-to-end case: MapMaker over three templates
E2E = dict(n_det=4, n_samp=6000, rate=100.0, nside=16, step_time=1.0, iters=8, seed=7201, order=3, bins=8,
           minimum_bin_hits=3)
E2E_NAMES = ("baselines", "subharmonic", "ground")


def build_e2e():
    """-> (data, cfg): one satellite observation (toast_amd.sim.create_satellite_data) with a smooth sky, white noise,
    baseline drifts, a cubic trend per detector and a signal that is periodic in a shared ``azimuth`` sweep."""
    from toast_amd.data import defaults
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
    i = np.arange(n_samp)
    az = 50.0 + 40.0 * np.sin(2.0 * np.pi * i / 1700.0) + 0.01 * np.cos(i)
    ob.shared.create(KEY, az)
    step = int(np.rint(cfg["step_time"] * rate))
    r = np.linspace(-1.0, 1.0, n_samp)
    for d in range(n_det):
        rng = np.random.default_rng(cfg["seed"] * 1000 + d)
        sig[d] = sky * (1.0 + 0.01 * d) + rng.standard_normal(n_samp)
        walk = np.cumsum(rng.standard_normal((n_samp + 2 * step - 1) // (2 * step))) * 0.5
        sig[d] += np.repeat(walk, 2 * step)[:n_samp]
        sig[d] += (2.0 + d) * r ** 3 - 1.5 * r + 4.0 * np.sin(az / 9.0 + 0.3 * d)
    return data, cfg
