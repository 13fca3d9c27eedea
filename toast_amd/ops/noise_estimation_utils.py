"""Sample (cross) covariance and its PSD (reference: src/toast/ops/noise_estimation_utils.py:13-494).

``flagged_running_average``, ``highpass_flagged_signal``, ``autocov_psd``, ``crosscov_psd`` and ``smooth_with_hits``
have the reference's signatures.  This data model has one process per sample range, so ``comm`` must be ``None``.

The work is split the way ``ops.NoiseEstim`` needs it:

* ``segment_table``    realization and interval bookkeeping on the host (noise_estimation_utils.py:313-355): which
                       samples [first, last) are summed with which ``all_sums`` into which realization;
* ``lagged_sums_host`` the sums of one pair over that table with the library's host entries (``capi.fod_autosums`` /
                       ``capi.fod_crosssums``); the device path fills the same arrays with ``capi.dev.fod_sums``;
* ``psds_from_sums``   everything after the sums (noise_estimation_utils.py:411-464) with the reference's NumPy calls,
                       batched over pairs and realizations: division by hits, interpolation of empty lags,
                       symmetrisation, ``rfft`` of the 2 lagmax - 1 series, deconvolution of the high-pass, the
                       [0.25, 0.5, 0.25] smoothing, ``irfft``, ``/ fsample``;
* ``log_bin`` / ``bin_psds``   the logarithmic binning of noise_estimation.py:555-617 with ``np.bincount`` (which
                       accumulates in sample order like the reference's loops).
"""

import numpy as np

from .. import capi


def _no_comm(comm):
    if comm is not None:
        raise NotImplementedError("noise estimation: one process per sample range, comm must be None")


def flagged_running_average(signal, flag, wkernel, return_flags=False, downsample=False):
    """Running average over ``wkernel`` samples considering only the unflagged ones (noise_estimation_utils.py:13-66).
    The window of sample i is [i - wkernel // 2, i + (wkernel - 1) // 2], what ``fftconvolve(..., mode="same")``
    computes; ``downsample`` has no effect on the result, as in the reference."""
    if len(signal) != len(flag):
        raise Exception("Signal and flag lengths do not match.")
    bad = np.asarray(flag) != 0
    filtered_signal, hits = capi.flagged_running_average(signal, bad, int(wkernel))
    if return_flags:
        filtered_flags = np.zeros_like(flag)
        filtered_flags[hits == 0] = True
        return filtered_signal, filtered_flags
    return filtered_signal


def highpass_flagged_signal(sig, good, naverage):
    """``sig`` minus its flagged running average, for all samples; zeros when no sample is good
    (noise_estimation_utils.py:69-101)."""
    good = np.asarray(good)
    if np.sum(good) == 0:
        return np.zeros_like(sig)
    trend = flagged_running_average(sig, good == 0, naverage)
    return sig - trend


def segment_table(times, extended_times, global_intervals, stationary_period):
    """(time_start, time_stop, nreal, n_real_local, segments): ``segments`` is a list of (first, last, all_sums,
    realization) in samples of the extended arrays, in the reference's order of evaluation
    (noise_estimation_utils.py:302-355 for one process).  ``n_real_local`` >= nreal counts the realization a last
    sample exactly at a period's end opens; the reference sums it and then drops it."""
    time_start, time_stop = extended_times[0], extended_times[-1]
    nreal = int(np.ceil((time_stop - time_start) / stationary_period))
    realization = ((extended_times - time_start) / stationary_period).astype(np.int64)
    segments = []
    for ireal in range(realization[0], realization[-1] + 1):
        first, last = np.searchsorted(realization, [ireal, ireal + 1])
        if last == first:
            continue
        realtimes = extended_times[first:last]
        for start_time, stop_time in global_intervals:
            if start_time is not None and (start_time > times[-1] or start_time > realtimes[-1]):
                continue
            if stop_time is not None and stop_time < realtimes[0]:
                continue
            # avoid double-counting sample pairs
            all_sums = True if stop_time is None else bool(stop_time < realtimes[-1])
            if start_time is None or stop_time is None:
                istart, istop = 0, realtimes.size
            else:
                istart, istop = np.searchsorted(realtimes, [start_time, stop_time])
            if istop > istart:
                segments.append((int(first + istart), int(first + istop), all_sums, int(ireal)))
    return time_start, time_stop, nreal, int(realization[-1]) + 1, segments


def lagged_sums_host(signal1, signal2, flags, segments, n_real, lagmax, symmetric=False):
    """(hits [n_real][lagmax] int64, sums float64) of one pair over a segment table, by the host entries.  Flagged
    samples count as zero (the entries mask them)."""
    hits = np.zeros((n_real, lagmax), dtype=np.int64)
    sums = np.zeros((n_real, lagmax), dtype=np.float64)
    good_all = (np.asarray(flags) == 0).astype(np.uint8)
    for first, last, all_sums, ireal in segments:
        good = np.ascontiguousarray(good_all[first:last])
        if np.sum(good) == 0:
            continue
        x = np.ascontiguousarray(signal1[first:last], dtype=np.float64)
        if signal2 is None:
            capi.fod_autosums(x, good, lagmax, sums[ireal], hits[ireal], all_sums)
        else:
            y = np.ascontiguousarray(signal2[first:last], dtype=np.float64)
            capi.fod_crosssums(x, y, good, lagmax, sums[ireal], hits[ireal], all_sums, symmetric)
    return hits, sums


def psds_from_sums(hits, sums, lagmax, naverage, fsample, return_cov=False):
    """Rows of lagged sums -> (psdfreq [lagmax], psds [rows][lagmax], smooth covariances or None): the steps of
    noise_estimation_utils.py:411-459 on every row of ``hits`` / ``sums`` [rows][lagmax] (``sums`` is overwritten)."""
    hits = np.atleast_2d(hits)
    cov = np.atleast_2d(sums)
    good = hits != 0
    cov[good] /= hits[good]
    for row in np.flatnonzero(~np.all(good, axis=1) & np.any(good, axis=1)):
        # interpolate any empty bins; the last bins are left empty
        c, h = cov[row], hits[row]
        bad = h == 0
        i = c.size - 1
        while h[i] == 0:
            c[i] = 0
            bad[i] = False
            i -= 1
        if np.sum(bad) > 0:
            ok = np.logical_not(bad)
            lag = np.arange(lagmax)
            c[bad] = np.interp(lag[bad], lag[ok], c[ok])
    # symmetrize the sample autocovariance so that the transform is real-valued
    full = np.hstack([cov, cov[:, :0:-1]])
    psd = np.fft.rfft(full, axis=1).real
    psdfreq = np.fft.rfftfreq(full.shape[1], d=1 / fsample)
    # deconvolve the prewhitening (high-pass) filter
    arg = 2 * np.pi * np.abs(psdfreq) * naverage / fsample
    tf = np.ones(lagmax)
    ind = arg != 0
    tf[ind] -= np.sin(arg[ind]) / arg[ind]
    psd[:, ind] /= tf[ind] ** 2
    # the Hann window
    for row in range(psd.shape[0]):
        psd[row] = np.convolve(psd[row], [0.25, 0.5, 0.25], mode="same")
    smooth = np.fft.irfft(psd, axis=1)[:, :lagmax] if return_cov else None
    # white noise PSD normalization sigma**2 / fsample
    psd /= fsample
    return psdfreq, psd, smooth


def crosscov_psd(times, extended_times, global_intervals, extended_signal1, extended_signal2, extended_flags, lagmax,
                 naverage, stationary_period, fsample, comm=None, return_cov=False, symmetric=False):
    """Sample (cross) covariance and its PSD: a list of (start_time, stop_time, bin_frequency, bin_value) per
    stationary period (noise_estimation_utils.py:258-469).  Like the reference it sets the flagged samples of the
    signals to zero in place."""
    _no_comm(comm)
    extended_signal1[extended_flags != 0] = 0
    if extended_signal2 is not None:
        extended_signal2[extended_flags != 0] = 0
    time_start, time_stop, nreal, n_local, segments = segment_table(times, extended_times, global_intervals,
                                                                    stationary_period)
    hits, sums = lagged_sums_host(extended_signal1, extended_signal2, extended_flags, segments, max(nreal, n_local),
                                  lagmax, symmetric)
    return assemble_psds(hits[:nreal], sums[:nreal], time_start, time_stop, lagmax, naverage, stationary_period, fsample,
                         return_cov)


def assemble_psds(hits, sums, time_start, time_stop, lagmax, naverage, stationary_period, fsample, return_cov=False):
    """The reference's return value from the sums of the realizations [nreal][lagmax]."""
    nreal = hits.shape[0]
    if nreal == 0:
        return ([], []) if return_cov else []
    hits = hits.copy()
    psdfreq, psd, smooth = psds_from_sums(hits, sums, lagmax, naverage, fsample, return_cov)
    my_psds, my_cov = [], []
    for ireal in range(nreal):
        tstart = time_start + ireal * stationary_period
        tstop = min(tstart + stationary_period, time_stop)
        my_psds.append((tstart, tstop, psdfreq, psd[ireal]))
        if return_cov:
            my_cov.append((hits[ireal], smooth[ireal]))
    return (my_psds, my_cov) if return_cov else my_psds


def autocov_psd(times, extended_times, global_intervals, extended_signal, extended_flags, lagmax, naverage,
                stationary_period, fsample, comm=None, return_cov=False):
    """Sample autocovariance and its PSD (noise_estimation_utils.py:202-255)."""
    return crosscov_psd(times, extended_times, global_intervals, extended_signal, None, extended_flags, lagmax, naverage,
                        stationary_period, fsample, comm, return_cov)


def _window_sum(x, width):
    """Sums over the window of ``fftconvolve(x, ones(width), mode="same")``, in extended precision."""
    n = x.size
    c = np.concatenate([[0], np.cumsum(np.asarray(x, dtype=np.longdouble))])
    i = np.arange(n)
    lo = np.clip(i - width // 2, 0, n)
    hi = np.clip(i + (width - 1) // 2 + 1, 0, n)
    return (c[hi] - c[lo]).astype(np.float64)


def smooth_with_hits(hits, cov, wbin):
    """Smooth the covariance function taking the hits of every lag into account (noise_estimation_utils.py:472-494)."""
    hits, cov = np.asarray(hits), np.asarray(cov)
    smooth_hits = _window_sum(hits, int(wbin))
    smooth_cov = _window_sum(cov * hits, int(wbin))
    good = smooth_hits > 0
    smooth_cov[good] /= smooth_hits[good]
    return smooth_hits, smooth_cov


def log_bin(freq, nbin=100, fmin=None, fmax=None):
    """(bin of every frequency, entries per bin) on a logarithmic grid (noise_estimation.py:555-575)."""
    if np.any(freq == 0):
        raise Exception("Logarithmic binning should not include zero frequency")
    if fmin is None:
        fmin = np.amin(freq)
    if fmax is None:
        fmax = np.amax(freq)
    bins = np.logspace(np.log(fmin), np.log(fmax), num=nbin + 1, endpoint=True, base=np.e)
    bins[-1] *= 1.01  # widen the last bin not to have a bin with one entry
    locs = np.digitize(freq, bins).astype(np.int32)
    hits = np.bincount(locs, minlength=nbin + 2).astype(np.int32)
    return locs, hits


def bin_psds(my_psds, nbin_psd, fmin=None, fmax=None):
    """(binned PSDs, start times, bin frequencies) (noise_estimation.py:577-617)."""
    my_binned_psds, my_times = [], []
    binfreq0 = None
    locs = hits = None
    for t0, _, freq, psd in my_psds:
        good = freq != 0
        if nbin_psd is not None:
            if locs is None:
                locs, hits = log_bin(freq[good], nbin=nbin_psd, fmin=fmin, fmax=fmax)
                full = hits != 0
            binfreq = np.bincount(locs, weights=freq[good], minlength=hits.size)[full] / hits[full]
        else:
            binfreq = freq
        if binfreq0 is None:
            binfreq0 = binfreq
        elif np.any(binfreq != binfreq0):
            raise RuntimeError("Binned PSD frequencies change")
        if nbin_psd is not None:
            binpsd = np.bincount(locs, weights=psd[good], minlength=hits.size)[full] / hits[full]
        else:
            binpsd = psd
        my_times.append(t0)
        my_binned_psds.append(binpsd)
    return my_binned_psds, my_times, binfreq0
