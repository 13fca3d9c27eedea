#!/usr/bin/env python3
"""Generate tests/golden/sim_noise_grid.npz from THE REFERENCE'S OWN compiled code.  Build container only.

The reference is compiled where it lies into a temporary directory by make_golden_sim_noise.py's build_reference
(nothing of it is copied into the repository).  The grid of PSD tables, transform lengths and start samples, and the
long double restatements, are those of tests/sim_noise_case.py: the tests measure the library against the same
restatements, and this script measures how far the reference itself is from them.

Per case (n_binned, samples, oversample), key "<n_binned>_<samples>_<oversample>":
  interp_<key>     the reference's interpolated amplitudes of every PSD of the case at sim_noise_case.grid_bins
  scale_err_<key>  max |reference - long double| / max(reference) over all bins and PSDs
  ts_err_<key>     over both start samples and both streams: the distance of the reference's steps (its double
                   amplitudes, its Gaussians, numpy.fft.irfft, the crop and a sequential mean: finish_timestream)
                   to the all-long-double stream (long double amplitudes, scipy.fft.irfft in long double, a long
                   double mean), divided by the rms of the full long double transform
and the same for the tie grid (key "tie": PSD frequencies that are transform bins exactly) and ts_err_long for the
long case (258 crop chunks).

Every scale_err and ts_err must be at most 1e-12.  That is a condition on the inputs, not a tolerance: a case the
reference itself cannot carry to 1e-12 has to be replaced with another grid.

    python tests/golden/make_golden_sim_noise_grid.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sim_noise_case as sc  # noqa: E402
from make_golden_sim_noise import build_reference, finish_timestream, ref_interp, ref_stream  # noqa: E402

CONDITION = 1e-12


def main():
    lib = build_reference(tempfile.mkdtemp(prefix="golden_sim_noise_grid_"))
    out = {}
    rate = sc.GRID_RATE
    worst_scale, worst_ts = (0.0, None), (0.0, None)

    def ref_gaussians(key1, key2, counter2, n):
        return ref_stream(lib, "normal", n, key1, key2, 0, counter2)

    def interp_case(key, samples, oversample, freq, psds):
        nonlocal worst_scale
        ref = ref_interp(lib, rate, samples, oversample, freq, psds)
        err = max(sc.scale_distance(ref[b], sc.interp_longdouble(rate, samples, oversample, freq, psds[b]))
                  for b in range(psds.shape[0]))
        out["interp_" + key] = ref[:, sc.grid_bins(ref.shape[1])]
        out["scale_err_" + key] = np.array(err)
        if err >= worst_scale[0]:
            worst_scale = (err, key)
        return ref

    def ts_error(ref_scale, scale_ld, key1, key2, counter2, samples):
        g = ref_gaussians(key1, key2, counter2, 2 * (ref_scale.size - 1))
        with np.errstate(divide="ignore", invalid="ignore"):     # its own error measure divides by the cropped rms
            ref_ts, _ = finish_timestream(g, ref_scale, samples)
        ld_ts, rms = sc.timestream_longdouble(g, scale_ld, samples)
        return sc.ts_distance(ref_ts, ld_ts, rms)

    for n_binned, samples, oversample in sc.grid_cases():
        key = sc.case_key(n_binned, samples, oversample)
        freq, psds = sc.grid_psds(n_binned)
        ref = interp_case(key, samples, oversample, freq, psds)
        scale_ld = sc.grid_scale_longdouble(n_binned, samples, oversample)
        err = 0.0
        for first in sc.GRID_FIRST:
            for det, row in zip(sc.GRID_DET, sc.grid_stream_rows(n_binned)):
                key1, key2 = sc.noise_keys(*sc.GRID_IDS, det)
                err = max(err, ts_error(ref[row], scale_ld[row], key1, key2, first * oversample, samples))
        out["ts_err_" + key] = np.array(err)
        if err >= worst_ts[0]:
            worst_ts = (err, key)

    # ---- the tie grid: every PSD frequency is a transform bin, in double, bit for bit
    samples, oversample = sc.TIE_LENGTH
    freq, psds, k = sc.tie_grid()
    fftlen = sc.fft_length(samples, oversample)
    inc = rate / (fftlen - 1)
    ties = int(np.count_nonzero(np.log10(inc * k.astype(np.float64) + inc) == np.log10(freq[:-1] + inc)))
    print(f"tie grid: {ties} of {k.size} PSD frequencies sit on their transform bin bit for bit")
    assert ties == k.size and np.all(np.diff(freq) > 0) and k[-1] == fftlen // 2 - 1
    interp_case("tie", samples, oversample, freq, psds)

    # ---- the long case: only its error measure
    samples, oversample = sc.LONG_LENGTH
    rz, tel, comp, obs, det, first = sc.LONG_IDS
    freq, psd = sc.GOLD["psd_freq"], sc.GOLD["psd_psds"][sc.LONG_PSD_ROW]
    assert sc.fft_length(samples, oversample) == 1 << 22 and -(-samples // 4096) == 258
    ref = ref_interp(lib, rate, samples, oversample, freq, psd)[0]
    key1, key2 = sc.noise_keys(rz, tel, comp, obs, det)
    err = ts_error(ref, sc.interp_longdouble(rate, samples, oversample, freq, psd), key1, key2, first * oversample, samples)
    out["ts_err_long"] = np.array(err)
    if err >= worst_ts[0]:
        worst_ts = (err, "long")

    print(f"worst scale_err {worst_scale[0]:.3e} (case {worst_scale[1]}), worst ts_err {worst_ts[0]:.3e} "
          f"(case {worst_ts[1]}); condition {CONDITION:.0e}")
    for name, value in out.items():
        if name.startswith(("scale_err_", "ts_err_")):
            assert np.isfinite(value) and value <= CONDITION, (name, float(value))
    path = os.path.join(HERE, "sim_noise_grid.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "sim_noise.npz"))
    print("wrote", path, size, "bytes; sim_noise.npz has", limit)
    assert size <= limit


if __name__ == "__main__":
    main()
