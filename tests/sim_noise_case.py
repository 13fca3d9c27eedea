"""Shared by test_sim_noise_host.py and test_gpu_sim_noise.py: the fixture tests/golden/sim_noise.npz (the reference's
own compiled random streams and PSD interpolation, tests/golden/make_golden_sim_noise.py), small observations with a
noise model, and the periodogram check of a simulated spectrum.

Shared by test_sim_noise_grid_host.py, test_gpu_sim_noise_grid.py and tests/golden/make_golden_sim_noise_grid.py: the
grid of PSD tables, transform lengths and start samples below, the long double restatements of the interpolation and
of a whole timestream, and the per-case bounds from tests/golden/sim_noise_grid.npz."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "sim_noise.npz"), allow_pickle=False)

SAMPLERS = {"gaussian": "normal", "uniform_01": "uniform_01", "uniform_m11": "uniform_11", "uniform_uint64": "uint64"}
TS_CASES = ("a", "b", "c", "d")


def rng_cases():
    """[(key1, key2, counter1, counter2)] as Python ints."""
    return [tuple(int(x) for x in row) for row in GOLD["rng_cases"]]


def ts_case(name):
    """(realization, telescope, component, obsindx, firstsamp, samples, detindices, psds [n][n_binned], expected)"""
    rz, tel, comp, obs, first, samples = (int(x) for x in GOLD[f"ts_{name}_params"])
    det = GOLD[f"ts_{name}_detindx"]
    psds = np.ascontiguousarray(GOLD["psd_psds"][GOLD[f"ts_{name}_psdrow"]])
    want = GOLD[f"ts_{name}_after"] if name == "mix" else GOLD[f"ts_{name}_noise"]
    return rz, tel, comp, obs, first, samples, det, psds, want


def rel_rms(got, want):
    """Largest distance of a stream to the fixture relative to the stream's rms."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    return float(np.max(np.max(np.abs(got - want), axis=1) / np.sqrt(np.mean(want**2, axis=1))))


def make_data(n_det=3, n_samp=3000, rate=37.0, fknee=0.05, alpha=1.0, net=1.0, mixmatrix=None, name="obs_sim"):
    """One observation with timestamps, an empty float64 ``signal`` and an AnalyticNoise model (or, with ``mixmatrix``
    {det: {key: weight}}, a Noise model whose PSDs are those of an AnalyticNoise over the keys)."""
    from toast_amd.data import Data, Focalplane, Observation, Telescope, defaults
    from toast_amd.noise import AnalyticNoise, Noise

    dets = [f"D{i:02d}" for i in range(n_det)]
    quats = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n_det, 1))
    tele = Telescope("sim_tele", Focalplane(dets, quats, sample_rate=rate))
    ob = Observation(None, tele, n_samp, name=name)
    ob.set_times(np.arange(n_samp) / rate)
    keys = dets if mixmatrix is None else sorted({k for row in mixmatrix.values() for k in row})
    an = AnalyticNoise(detectors=keys, rate={k: rate for k in keys}, fmin={k: 1e-5 for k in keys},
                       fknee={k: fknee for k in keys}, alpha={k: alpha for k in keys},
                       NET={k: net * (1.0 + 0.1 * i) for i, k in enumerate(keys)})
    if mixmatrix is None:
        ob[defaults.noise_model] = an
    else:
        ob[defaults.noise_model] = Noise(detectors=dets, freqs={k: an.freq(k) for k in keys},
                                         psds={k: an.psd(k) for k in keys}, mixmatrix=mixmatrix)
    ob.detdata.create(defaults.det_data, dtype=np.float64, units=defaults.det_data_units)
    data = Data()
    data.obs.append(ob)
    return data


# ------------------------------------------------------------------------------------------ statistical check
STAT = dict(n_det=64, samples=1 << 14, rate=100.0, fknee=1.0, alpha=1.0, fmin=1e-5, net=1.0)


def stat_psd():
    from toast_amd.noise import AnalyticNoise

    an = AnalyticNoise(detectors=["d"], rate={"d": STAT["rate"]}, fmin={"d": STAT["fmin"]}, fknee={"d": STAT["fknee"]},
                       alpha={"d": STAT["alpha"]}, NET={"d": STAT["net"]})
    return np.asarray(an.freq("d")), np.asarray(an.psd("d"))


def spectrum_check(ts, interp_scale):
    """Periodogram of the simulated streams ``ts`` [n_det][samples] against the PSD the simulation is asked to realise.

    The target is the input PSD on the simulation's own frequency grid: ``interp_scale`` [fftlen / 2 + 1] is
    sqrt(psd rate fftlen / 2), so psd = scale^2 / (rate fftlen / 2), and bin k of the periodogram (length ``samples``)
    is bin k fftlen / samples of that grid.  With the reference's convention a white PSD P gives the variance P rate,
    so the periodogram is |rfft(x)_k|^2 / (samples rate).  Each mode of each detector is an independent exponential
    variable with unit relative scatter, so the mean over a logarithmic bin of m modes and n_det detectors has
    sigma = 1 / sqrt(m n_det).  Bins are octaves [k0, 2 k0) from the first mode above 2 rate / samples (k = 3) to the
    last complex mode (k = samples / 2 - 1; the Nyquist mode is real and has another distribution); none is left out.
    Returns [(k_first, k_last, ratio, sigma)]."""
    n_det, n = ts.shape
    rate = STAT["rate"]
    fftlen = 2 * (interp_scale.size - 1)
    step = fftlen // n
    target = interp_scale[::step] ** 2 / (rate * (fftlen / 2))
    pgram = np.abs(np.fft.rfft(ts, axis=1)) ** 2 / (n * rate)
    ratio = np.mean(pgram, axis=0)[: n // 2] / target[: n // 2].clip(1e-300)
    out = []
    k0 = 3
    while k0 < n // 2:
        k1 = min(2 * k0, n // 2)
        out.append((k0, k1 - 1, float(np.mean(ratio[k0:k1])), 1.0 / np.sqrt((k1 - k0) * n_det)))
        k0 = k1
    return out


# ------------------------------------------------------------------------------------------ grid and edges
# PSD tables below, at and above the size the kernels keep in LDS (768 points), the two smallest tables, transform
# lengths from 4 to 2^15 (below one block of the spectrum grid, the step from one block to two, three oversampling
# factors, one crop chunk against two) and a start sample whose counter needs 43 bits.
GRID_RATE = 37.0
GRID_NBINNED = (2, 3, 72, 767, 768, 769, 2000)
GRID_LENGTHS = ((1, 2), (2, 2), (3, 2), (511, 2), (512, 2), (1023, 1), (1024, 2), (1025, 3), (4095, 2), (4096, 1),
                (4097, 4))                                   # (samples, oversample)
GRID_FIRST = (0, (1 << 40) + 3)
GRID_IDS = (2, 7, 1, 5)                                      # realization, telescope, component, obsindx
GRID_DET = (3, 4294967295)                                   # stream indices of the two simulated streams
TIE_LENGTH = (3000, 2)
LONG_LENGTH = (1048577 + 4096, 2)                            # 258 crop chunks, fftlen 2^22
LONG_PSD_ROW = 2
LONG_IDS = (1, 3, 0, 8, 17, 5)                               # realization, telescope, component, obsindx, detindx, firstsamp


def fft_length(samples, oversample):
    fftlen = 2
    while fftlen <= oversample * samples:
        fftlen *= 2
    return fftlen


def red_psd(freq, zeros):
    psd = 1e-4 * (1.0 + (0.1 / np.maximum(freq, 1e-6)) ** 1.5)
    for z in zeros:
        if 0 <= z < freq.size:
            psd[z] = 0.0
    return psd


def grid_psds(n_binned):
    """(freq [n_binned], psds [n][n_binned]): the fixture's grid with its four rows at 72 points; otherwise 0 and a
    logarithmic grid up to rate / 2 with a white PSD and a red one with zero bins."""
    if n_binned == 72:
        return GOLD["psd_freq"], GOLD["psd_psds"]
    if n_binned == 2:
        freq = np.array([0.0, GRID_RATE / 2])
    else:
        freq = np.concatenate([[0.0], np.logspace(np.log10(1e-5), np.log10(GRID_RATE / 2), n_binned - 1)])
        freq[-1] = GRID_RATE / 2
    return freq, np.array([np.full(n_binned, 0.3), red_psd(freq, (0, 5, 40, n_binned - 3))])


def tie_grid():
    """(freq, psds, k): PSD frequencies that are transform bins k of the tie length exactly, so that
    log10(freq + inc) on the host is bit for bit the x of bin k."""
    fftlen = fft_length(*TIE_LENGTH)
    inc = GRID_RATE / (fftlen - 1)
    k = np.unique(np.concatenate([[0], np.round(np.logspace(0.0, np.log10(fftlen // 2 - 1), 60))])).astype(np.int64)
    freq = np.concatenate([inc * k.astype(np.float64), [GRID_RATE / 2]])
    return freq, np.array([np.full(freq.size, 0.3), red_psd(freq, (0, 7))]), k


def grid_bins(n_psd):
    """The bins of a case the fixture keeps: the first 64, every 8th and the last."""
    return np.unique(np.concatenate([np.arange(min(64, n_psd)), np.arange(0, n_psd, 8), [n_psd - 1]]))


def grid_cases():
    return [(nb, s, o) for nb in GRID_NBINNED for s, o in GRID_LENGTHS]


def case_key(n_binned, samples, oversample):
    return f"{n_binned}_{samples}_{oversample}"


@functools.lru_cache(maxsize=None)
def grid_gold():
    return np.load(os.path.join(HERE, "golden", "sim_noise_grid.npz"), allow_pickle=False)


def scale_bound(key):
    """4 x the larger of the reference's distance to the long double evaluation on the fixture's grid and on this one."""
    return 4.0 * max(float(GOLD["scale_ref_err"]), float(grid_gold()["scale_err_" + key]))


def ts_bound(key):
    """10 x the larger of the reference's distance to the long double stream on the fixture's cases and on this one."""
    return 10.0 * max(float(GOLD["ts_ref_err"]), float(grid_gold()["ts_err_" + key]))


def noise_keys(realization, telescope, component, obsindx, detindx):
    return realization * 4294967296 + telescope * 65536 + component, obsindx * 4294967296 + detindx


# ---- long double restatements
def interp_longdouble(rate, samples, oversample, freq, psd):
    """Interpolated amplitudes of one PSD, every step after the double inputs in long double (as the function of this
    name in make_golden_sim_noise.py, which writes the fixture this module loads and so cannot import it)."""
    L = np.longdouble
    fftlen = fft_length(samples, oversample)
    psdlen = fftlen // 2 + 1
    norm = L(rate) * L(psdlen - 1)
    inc = L(np.float64(rate) / np.float64(fftlen - 1))
    f, p = np.asarray(freq).astype(L), np.asarray(psd).astype(L)
    logfreq = np.log10(f + inc)
    shift = L(np.float64(0.01) * np.min(psd[psd != 0]))
    logpsd = np.log10(np.sqrt(p * norm) + shift)
    x = np.log10(inc * np.arange(psdlen).astype(L) + inc)
    ibin = np.clip(np.searchsorted(logfreq[1:], x, side="left"), 0, f.size - 2)
    r = (x - logfreq[ibin]) / (logfreq[ibin + 1] - logfreq[ibin])
    out = L(10) ** (logpsd[ibin] + r * (logpsd[ibin + 1] - logpsd[ibin])) - shift
    out[0] = 0
    return out


def scale_distance(got, want):
    """Largest distance of interpolated amplitudes to ``want`` relative to the largest amplitude of ``want``."""
    L = np.longdouble
    return float(np.max(np.abs(np.asarray(got).astype(L) - np.asarray(want).astype(L))) / np.max(want))


def timestream_longdouble(gauss, scale, samples):
    """(stream, rms): the unit Gaussians ``gauss`` [fftlen] times the amplitudes ``scale`` [fftlen / 2 + 1] as a
    half-complex spectrum, its inverse transform, the middle ``samples`` less their mean -- all in long double -- and
    the rms of the full transform, the measure of the stream's distances (the rms of the cropped and de-meaned stream
    is 0 at one sample and arbitrarily small at two or three of a red spectrum)."""
    import scipy.fft

    L = np.longdouble
    n = gauss.size
    half = n // 2
    g, s = gauss.astype(L), np.asarray(scale).astype(L)
    spec = np.zeros(half + 1, dtype=np.clongdouble)
    spec.real[0] = g[0] * s[0]
    spec.real[1:half] = g[1:half] * s[1:half]
    spec.imag[1:half] = g[n - 1:half:-1] * s[1:half]
    spec.real[half] = g[half] * s[half]
    full = scipy.fft.irfft(spec, n)
    assert full.dtype == L
    off = (n - samples) // 2
    x = full[off:off + samples]
    return x - np.sum(x) / L(samples), float(np.sqrt(np.mean(full**2)))


def host_gaussians(key1, key2, counter2, n):
    """The library's host Gaussians: bit for bit the reference's (test_sim_noise_host.py)."""
    from toast_amd import rng

    return rng.random(n, key=(key1, key2), counter=(0, counter2), sampler="gaussian")


@functools.lru_cache(maxsize=None)
def grid_scale_longdouble(n_binned, samples, oversample):
    """Long double amplitudes of every PSD of a grid case [n][n_psd]; computed once per process."""
    freq, psds = grid_psds(n_binned)
    out = np.array([interp_longdouble(GRID_RATE, samples, oversample, freq, p) for p in psds])
    out.setflags(write=False)
    return out


def grid_stream_rows(n_binned):
    """The PSD rows of the two simulated streams of a grid case: the last two."""
    return (2, 3) if n_binned == 72 else (0, 1)


def grid_streams_longdouble(n_binned, samples, oversample, firstsamp, gaussians=host_gaussians):
    """(streams [2][samples] long double, rms [2]) of a grid case from ``gaussians(key1, key2, counter2, n)``."""
    fftlen = fft_length(samples, oversample)
    scale = grid_scale_longdouble(n_binned, samples, oversample)
    out, rms = [], []
    for det, row in zip(GRID_DET, grid_stream_rows(n_binned)):
        key1, key2 = noise_keys(*GRID_IDS, det)
        ts, r = timestream_longdouble(gaussians(key1, key2, firstsamp * oversample, fftlen), scale[row], samples)
        out.append(ts)
        rms.append(r)
    return np.array(out), np.array(rms)


def ts_distance(got, want, rms):
    """Largest distance of streams [n][samples] to the long double ones relative to the full transforms' rms [n]."""
    d = np.max(np.abs(np.atleast_2d(got).astype(np.longdouble) - np.atleast_2d(want)), axis=1)
    return float(np.max(d / np.atleast_1d(rms)))


@functools.lru_cache(maxsize=None)
def long_stream_longdouble():
    """(stream, rms) of the long case from the host Gaussians; computed once per process."""
    samples, oversample = LONG_LENGTH
    rz, tel, comp, obs, det, first = LONG_IDS
    scale = interp_longdouble(GRID_RATE, samples, oversample, GOLD["psd_freq"], GOLD["psd_psds"][LONG_PSD_ROW])
    key1, key2 = noise_keys(rz, tel, comp, obs, det)
    ts, rms = timestream_longdouble(host_gaussians(key1, key2, first * oversample, fft_length(samples, oversample)),
                                    scale, samples)
    ts.setflags(write=False)
    return ts, rms
