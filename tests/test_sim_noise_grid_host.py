"""CPU: the library's host entries of the noise simulation through the grid of tests/sim_noise_case.py -- PSD tables of
2 to 2000 points, transform lengths 4 to 2^15 at three oversampling factors, two start samples, PSD frequencies that
sit on transform bins, and a stream of 258 crop chunks -- against the long double restatements of sim_noise_case.py
and the reference's own amplitudes in tests/golden/sim_noise_grid.npz (tests/golden/make_golden_sim_noise_grid.py).

This is the proof, without a GPU, that the restatements and the bounds test_gpu_sim_noise_grid.py relies on hold:
* amplitudes: <= SCALE_BOUND[case] = 4 x max(scale_ref_err, scale_err[case]) of the largest amplitude, against the
  restatement and against the reference's stored bins;
* timestreams: <= TS_BOUND[case] = 10 x max(ts_ref_err, ts_err[case]) of the rms of the full transform.
scale_err and ts_err are the reference's own distances to the restatement, measured per case when the fixture was
made; on the dense tables they are up to 14 x the 72-point fixture's (narrow intervals amplify the rounding of
(x - logfreq) * stepinv in any double evaluation).  Every figure is printed before it is asserted."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sim_noise_case as sc  # noqa: E402


def check_scale(got, key, scale_ld, worst):
    """Asserts one case of interpolated amplitudes [n][n_psd] (shared with the device test)."""
    gold = sc.grid_gold()
    bound = sc.scale_bound(key)
    bins = sc.grid_bins(got.shape[1])
    d_ld = max(sc.scale_distance(got[b], scale_ld[b]) for b in range(got.shape[0]))
    d_ref = max(sc.scale_distance(got[b, bins], gold["interp_" + key][b]) for b in range(got.shape[0]))
    equal = np.array_equal(got[:, bins], gold["interp_" + key])
    print(f"scale {key:>12s}: {d_ld:.3e} (long double), {d_ref:.3e} (reference bins{', bit-equal' if equal else ''}); "
          f"bound {bound:.3e}")
    assert np.all(got[:, 0] == 0) and np.all(np.isfinite(got)), key
    assert max(d_ld, d_ref) <= bound, key
    if d_ld / bound > worst[0]:
        worst[:] = [d_ld / bound, key]


def test_host_interpolation_grid():
    from toast_amd import capi

    worst = [0.0, None]
    for n_binned, samples, oversample in sc.grid_cases():
        freq, psds = sc.grid_psds(n_binned)
        assert capi.sim_noise_fft_length(samples, oversample) == sc.fft_length(samples, oversample)
        got = capi.tod_sim_noise_psd_interp(sc.GRID_RATE, samples, oversample, freq, psds)
        check_scale(got, sc.case_key(n_binned, samples, oversample),
                    sc.grid_scale_longdouble(n_binned, samples, oversample), worst)
    samples, oversample = sc.TIE_LENGTH
    freq, psds, _ = sc.tie_grid()
    got = capi.tod_sim_noise_psd_interp(sc.GRID_RATE, samples, oversample, freq, psds)
    ld = np.array([sc.interp_longdouble(sc.GRID_RATE, samples, oversample, freq, p) for p in psds])
    check_scale(got, "tie", ld, worst)
    print(f"closest to its bound: case {worst[1]} at {worst[0]:.3f} of it")
    assert sc.fft_length(1, 2) == 4 and max(sc.fft_length(s, o) for s, o in sc.GRID_LENGTHS) == 32768


def test_host_timestream_grid():
    from toast_amd import capi

    worst = [0.0, None]
    rz, tel, comp, obs = sc.GRID_IDS
    det = np.array(sc.GRID_DET, dtype=np.uint64)
    for n_binned, samples, oversample in sc.grid_cases():
        key = sc.case_key(n_binned, samples, oversample)
        freq, psds = sc.grid_psds(n_binned)
        rows = list(sc.grid_stream_rows(n_binned))
        bound = sc.ts_bound(key)
        for first in sc.GRID_FIRST:
            got = np.full((2, samples), np.nan)
            capi.tod_sim_noise_timestream_batch(rz, tel, comp, obs, sc.GRID_RATE, first, oversample, det, freq,
                                                np.ascontiguousarray(psds[rows]), got)
            want, rms = sc.grid_streams_longdouble(n_binned, samples, oversample, first)
            dist = sc.ts_distance(got, want, rms)
            print(f"timestream {key:>12s} firstsamp {first:14d}: {dist:.3e} of the full rms, bound {bound:.3e}")
            assert dist <= bound, (key, first)
            if samples == 1:
                assert np.all(got == 0)
            if dist / bound > worst[0]:
                worst[:] = [dist / bound, key]
    print(f"closest to its bound: case {worst[1]} at {worst[0]:.3f} of it")


def test_host_long_case():
    from toast_amd import capi

    samples, oversample = sc.LONG_LENGTH
    rz, tel, comp, obs, det, first = sc.LONG_IDS
    got = np.full(samples, np.nan)
    capi.tod_sim_noise_timestream(rz, tel, comp, obs, det, sc.GRID_RATE, first, oversample, sc.GOLD["psd_freq"],
                                  np.ascontiguousarray(sc.GOLD["psd_psds"][sc.LONG_PSD_ROW]), got)
    want, rms = sc.long_stream_longdouble()
    dist, bound = sc.ts_distance(got, want, rms), sc.ts_bound("long")
    print(f"long case ({samples} samples, {-(-samples // 4096)} chunks): {dist:.3e} of the full rms, bound {bound:.3e}")
    assert dist <= bound
