"""Shared by test_demod_host.py, test_gpu_demod.py and tests/golden/make_golden_demod.py: the shapes and inputs of the
fixture tests/golden/demod.npz, a stand-in Stokes weights operator that hands out the fixture's stored weights (so
that the fixture pins demodulation alone), small observations, and long-double direct evaluations of the filters."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD_PATH = os.path.join(HERE, "golden", "demod.npz")
L = np.longdouble

RATE = 100.0
HWP_HZ = 2.0
N = 5001
NSKIP = 3
DETS = ("D0", "D1", "D2")
ETA = (0.9, 1.0, 0.75)                    # polarization efficiency of the stored weights
SCAN = ((100, 2000), (2500, 4900))        # the intervals "scan"
SAMPLE_SETS = [[1000, 1001], [3000]]
NOISE_INDEX = {"D0": 5, "D1": 6, "D2": 9}
#: operator cases of the fixture: traits and detectors
CASES = {
    "default": dict(dets=DETS, op=dict()),
    "even": dict(dets=DETS[:1], op=dict(wkernel=200)),
    "2f": dict(dets=DETS[:1], op=dict(do_2f=True)),
}
#: constants of the recovery test: signal = I0 + Q0 w_q + U0 w_u with the stored weights (w carries eta)
RECOVERY = (3.0, 0.5, -0.25)


def gold():
    return np.load(GOLD_PATH, allow_pickle=False)


def times():
    return 1000.0 + np.arange(N) / RATE


def hwp_angle():
    return np.mod(2 * np.pi * HWP_HZ * (np.arange(N) / RATE), 2 * np.pi)


def make_inputs():
    """The stored inputs (maker only): weights [det][n][Q, U], signals with a large offset, a random walk and the
    modulated sky, detector and shared flags."""
    rng = np.random.default_rng(20260117)
    t = np.arange(N) / RATE
    weights = np.empty((len(DETS), N, 2))
    signal = np.empty((len(DETS), N))
    for i in range(len(DETS)):
        psi = 0.3 + 0.7 * i + 0.01 * np.sin(2 * np.pi * 0.02 * t)          # detector angle on a slow scan
        ang = 2 * psi + 4 * (2 * np.pi * HWP_HZ * t)
        weights[i, :, 0] = ETA[i] * np.cos(ang)
        weights[i, :, 1] = ETA[i] * np.sin(ang)
        sky_i = 1.0 + 0.3 * np.sin(2 * np.pi * 0.05 * t + i)
        sky_q = 0.2 * np.cos(2 * np.pi * 0.03 * t)
        sky_u = 0.1 * np.sin(2 * np.pi * 0.04 * t + 1.0)
        walk = np.cumsum(rng.standard_normal(N)) * 0.05                      # 1/f^2
        signal[i] = 1.0e4 * (1 + i) + walk + 0.02 * rng.standard_normal(N) + sky_i \
            + sky_q * weights[i, :, 0] + sky_u * weights[i, :, 1]
    det_flags = np.where(rng.random((len(DETS), N)) < 0.05, 1, 0).astype(np.uint8)
    det_flags[:, 7::97] |= 4
    shared_flags = np.zeros(N, dtype=np.uint8)
    shared_flags[2000:2040] = 1
    shared_flags[5::301] |= 8
    return dict(weights_qu=weights, signal=signal, det_flags=det_flags, shared_flags=shared_flags)


def weight_table(G, nnz=3):
    """{det: [n][nnz]} of the stored weights (I = 1)."""
    out = {}
    for i, d in enumerate(DETS):
        w = np.ones((N, 3))
        w[:, 1:] = G["weights_qu"][i]
        out[d] = np.ascontiguousarray(w[:, 3 - nnz:])
    return out


def noise_inputs():
    """(frequencies, {det: psd}) of the input noise model: a 1/f spectrum on a log grid that ends at Nyquist."""
    f = np.concatenate([10.0 ** np.linspace(-4, np.log10(RATE / 2) - 0.01, 60), [RATE / 2]])
    return f, {d: (1.0 + 0.1 * i) * 1.0e-6 * (1 + (0.2 / f) ** 1.5) for i, d in enumerate(DETS)}


def fixed_weights_operator(table, mode="IQU"):
    """An operator with the traits Demodulate asks of ``stokes_weights`` that writes ``table[det]``."""
    from toast_amd.ops import Operator
    from toast_amd.traits import Unicode

    class FixedWeights(Operator):
        weights = Unicode("weights", help="Observation detdata key for output weights")
        view = Unicode(None, allow_none=True, help="unused")
        mode = Unicode("IQU", help="The Stokes weights to generate")
        hwp_angle = Unicode("hwp_angle", allow_none=True, help="Observation shared key for HWP angle")
        calls = 0

        def _exec(self, data, detectors=None, use_accel=None, **kwargs):
            nnz = len(self.mode)
            for ob in data.obs:
                dets = ob.select_local_detectors(detectors)
                ob.detdata.ensure(self.weights, sample_shape=(nnz,), dtype=np.float64, detectors=dets)
                wd = ob.detdata[self.weights]
                for d in dets:
                    wd[d] = table[d][:, 3 - nnz:]
                if use_accel:
                    if not wd.accel_exists():
                        wd.accel_create(self.weights)
                    wd.accel_update_device()
            type(self).calls += 1

        def _finalize(self, data, **kwargs):
            return

        def _requires(self):
            return {}

        def _provides(self):
            return {"detdata": [self.weights]}

    return FixedWeights(mode=mode)


def make_obs(G, dets=DETS, signal=None, name="hwp", noise=True, hwp=True):
    """Data with one observation on the fixture's inputs."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults
    from toast_amd.noise import Noise

    dets = list(dets)
    quats = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (len(dets), 1))
    fp = Focalplane(dets, quats, sample_rate=RATE,
                    columns={"pol_efficiency": [ETA[DETS.index(d)] for d in dets], "wafer": ["w0"] * len(dets)})
    ob = Observation(None, Telescope("demod_tele", fp), N, name="obs_" + name)
    ob.set_times(times())
    if hwp:
        ob.shared.create(defaults.hwp_angle, hwp_angle())
    ob.shared.create(defaults.shared_flags, np.array(G["shared_flags"]))
    ob.shared.create("boresight", np.tile(np.arange(N, dtype=np.float64)[:, None], (1, 4)))
    ob.shared.create("calib", np.arange(7.0))
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=defaults.det_data_units)
    ob.detdata.create(defaults.det_flags, dtype=np.uint8)
    for d in dets:
        i = DETS.index(d)
        ob.detdata[defaults.det_data][d] = G["signal"][i] if signal is None else signal[i]
        ob.detdata[defaults.det_flags][d] = G["det_flags"][i]
    ob.intervals.create("scan", list(SCAN))
    ob["scalar_meta"] = 42
    if noise:
        f, psds = noise_inputs()
        ob[defaults.noise_model] = Noise(detectors=dets, freqs={d: f for d in dets}, psds={d: psds[d] for d in dets},
                                         indices={d: NOISE_INDEX[d] for d in dets})
    data = Data()
    data.obs.append(ob)
    return data


def demodulate(G, case="default", use_accel=None, resident=False, signal=None, **extra):
    """(operator, input data, demodulated data) of a fixture case."""
    from toast_amd import ops
    from toast_amd.data import defaults

    spec = CASES[case]
    data = make_obs(G, dets=spec["dets"], signal=signal, name=case)
    if resident:
        dd = data.obs[0].detdata[defaults.det_data]
        dd.accel_create(defaults.det_data)
        dd.accel_update_device()
    traits = dict(spec["op"])
    traits.update(extra)
    op = ops.Demodulate(stokes_weights=fixed_weights_operator(weight_table(G)), nskip=NSKIP, **traits)
    out = op.apply(data, use_accel=use_accel)
    return op, data, out


def recovery_signal(G):
    """[det][n]: I0 + Q0 w_q + U0 w_u with the stored weights; demodulates to (I0, eta Q0, eta U0)."""
    i0, q0, u0 = RECOVERY
    return i0 + q0 * G["weights_qu"][:, :, 0] + u0 * G["weights_qu"][:, :, 1]


def recovery_leak(dd, flags, dets):
    """Largest |demodulated - constant| over the samples without the demodulation flag."""
    i0, q0, u0 = RECOVERY
    worst = 0.0
    for d in dets:
        eta = ETA[DETS.index(d)]
        for prefix, want in (("demod0", i0), ("demod4r", eta * q0), ("demod4i", eta * u0)):
            good = (flags[f"{prefix}_{d}"] & 1) == 0
            assert np.any(good)
            worst = max(worst, float(np.max(np.abs(dd[f"{prefix}_{d}"][good] - want))))
    return worst


# ---------------------------------------------------------------------------------------------- direct evaluations
def same_longdouble(y, h):
    """fftconvolve(y, h, "same") as a long-double direct sum: out[i] = sum_k h[k] y[i + (W - 1) // 2 - k]."""
    y, h = np.asarray(y, dtype=L), np.asarray(h, dtype=L)
    c = (h.size - 1) // 2
    return np.convolve(y, h, mode="full")[c:c + y.size]


def same_double_direct(y, h):
    """The same in double, one product and one addition per tap, in tap order."""
    y, h = np.asarray(y, dtype=np.float64), np.asarray(h, dtype=np.float64)
    n, w = y.size, h.size
    c = (w - 1) // 2
    pad = np.concatenate([np.zeros(w), y, np.zeros(w)])
    out = np.zeros(n)
    for k in range(w):
        lo = w + c - k
        out += h[k] * pad[lo:lo + n]
    return out


def normalised(w_qu):
    """(q, u) with the polarization efficiency divided out, the reference's statements (demodulation.py:728-730)."""
    q, u = w_qu[:, 0], w_qu[:, 1]
    etainv = 1 / np.sqrt(q**2 + u**2)
    return q * etainv, u * etainv


def chain(x, w_qu, lpf, bpf, off, nskip, same):
    """(demod0, demod4r, demod4i) of one detector with ``same`` as the convolution; the modulation factors are the
    doubles the reference forms."""
    q, u = normalised(w_qu)
    dt = L if same is same_longdouble else np.float64
    band = same(x, bpf)
    return (same(x, lpf)[off % nskip:: nskip], same(band * (2 * q).astype(dt), lpf)[off % nskip:: nskip],
            same(band * (2 * u).astype(dt), lpf)[off % nskip:: nskip])


def chain_scales(x, lpf, bpf):
    """The scale of demod0 and of demod4*: sum |h_lp| max |x| and 2 sum |h_bp| sum |h_lp| max |x|."""
    s0 = float(np.sum(np.abs(lpf)) * np.max(np.abs(x)))
    return s0, 2.0 * float(np.sum(np.abs(bpf))) * s0
