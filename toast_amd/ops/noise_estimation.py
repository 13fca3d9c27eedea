"""NoiseEstim: noise PSDs measured from the timestreams (reference: src/toast/ops/noise_estimation.py:34-1261).

For every detector pair the signal is prewhitened with a flagged running average, the lagged (cross) covariance sums
are accumulated per stationary period, and the sample covariance is Fourier transformed into a PSD, deconvolved,
smoothed and binned (``noise_estimation_utils``).  With ``nsum > 1`` a second estimate from the decimated signal
replaces the bins below ``fsample / 2 / naverage / 100``.

Two paths, chosen by where ``det_data`` lives:

* resident on the device (or ``use_accel=True``): the good masks, the high-pass, the decimation and the lagged sums run
  on the device (csrc/noise_estim.hip) in batches of pairs whose scratch is bounded (``max_batch`` attribute, 0 =
  automatic); only sums and hits come back.  ``det_data`` and the flags are not modified;
* on the host: the library's host entries (``capi.flagged_running_average``, ``capi.fod_autosums`` / ``fod_crosssums``).

Everything after the sums is the reference's NumPy on the host, batched over pairs.  Not reproduced: map and mask
scanning (``mapfile`` / ``maskfile`` raise), FITS output (``save_cov`` is accepted, nothing is written), observations
split in the sample direction.
"""

import numpy as np

from .. import capi
from ..accel import Resident, accel_device_ptr, accel_enabled, make_resident
from ..data import defaults
from ..noise import Noise, name_UID
from ..traits import Bool, Float, Instance, Int, List, TraitError, Unicode
from .arithmetic import Combine
from .mapmaker_ops import Copy, Delete
from .noise_estimation_utils import bin_psds, highpass_flagged_signal, lagged_sums_host, psds_from_sums, segment_table
from .operator import Operator
from .poly_filter import CommonModeFilter


def _medfilt(values, width):
    """Median filter with zero padding (what ``scipy.signal.medfilt`` computes)."""
    half = width // 2
    padded = np.concatenate([np.zeros(half), values, np.zeros(half)])
    return np.median(np.lib.stride_tricks.sliding_window_view(padded, width), axis=1)


class _Scratch:
    """A block of device memory from the library's allocator."""

    def __init__(self, shape, dtype, zero=False):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = capi.device_malloc(max(nbytes, 8))
        if zero:
            capi.dev.memset(self.ptr, 0, nbytes)

    def free(self):
        capi.device_free(self.ptr)


class NoiseEstim(Operator):
    """Noise estimation operator"""

    API = Int(0, help="Internal interface version for this operator")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    detector_pointing = Instance(klass=Operator, allow_none=True,
                                 help="Operator that translates boresight pointing into detector frame.  "
                                      "Only relevant if `maskfile` and/or `mapfile` are set")
    pixel_dist = Unicode("pixel_dist", help="The Data key where the PixelDistribution object is located.  "
                                            "Only relevant if `maskfile` and/or `mapfile` are set")
    pixel_pointing = Instance(klass=Operator, allow_none=True,
                              help="An instance of a pixel pointing operator.  "
                                   "Only relevant if `maskfile` and/or `mapfile` are set")
    stokes_weights = Instance(klass=Operator, allow_none=True,
                              help="An instance of a Stokes weights operator.  Only relevant if `mapfile` is set")
    det_mask = Int(defaults.det_mask_invalid, help="Bit mask value for per-detector flagging")
    det_data = Unicode(defaults.det_data, help="Observation detdata key apply filtering to")
    det_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for flags to use")
    det_flag_mask = Int(defaults.det_mask_invalid, help="Bit mask value for detector sample flagging")
    mask_flags = Unicode(defaults.det_flags, allow_none=True, help="Observation detdata key for processing mask flags")
    mask_flag_mask = Int(defaults.det_mask_processing, help="Bit mask for raising processing mask flags")
    shared_flags = Unicode(defaults.shared_flags, allow_none=True, help="Observation shared key for telescope flags to use")
    shared_flag_mask = Int(defaults.shared_mask_nonscience, help="Bit mask value for optional shared flagging")
    out_model = Unicode(None, allow_none=True, help="Create a new noise model with this name")
    maskfile = Unicode(None, allow_none=True, help="Optional HEALPix processing mask")
    mapfile = Unicode(None, allow_none=True, help="Optional HEALPix map to sample and subtract from the signal")
    pol = Bool(True, help="Sample also the polarized part of the map")
    save_cov = Bool(False, help="Save also the sample covariance")
    symmetric = Bool(False, help="If True, treat positive and negative lags as equivalent in the cross correlator")
    nbin_psd = Int(1000, allow_none=True, help="Bin the resulting PSD")
    lagmax = Int(10000, help="Maximum lag to consider for the covariance function. "
                             "Will be truncated the length of the longest view.")
    stationary_period = Float(86400, help="Break the observation into several estimation periods of this length [s]")
    nosingle = Bool(False, help="Do not evaluate individual PSDs.  Overridden by `pairs`")
    nocross = Bool(True, help="Do not evaluate cross-PSDs.  Overridden by `pairs`")
    nsum = Int(1, help="Downsampling factor for decimated data")
    naverage = Int(100, help="Smoothing kernel width for downsampled data")
    view = Unicode(None, allow_none=True, help="Only measure the covariance within each view")
    pairs = List([], help="Detector pairs to estimate noise for.  Overrides `nosingle` and `nocross`")
    focalplane_key = Unicode(None, allow_none=True, help="When set, PSDs are measured over averaged TODs")
    remove_common_mode = Bool(False, help="Remove common mode signal before estimation")

    def _validate_det_mask(self, value):
        if value < 0:
            raise TraitError("Det mask should be a positive integer")
        return value

    def _validate_det_flag_mask(self, value):
        if value < 0:
            raise TraitError("Det flag mask should be a positive integer")
        return value

    def _validate_shared_flag_mask(self, value):
        if value < 0:
            raise TraitError("Shared flag mask should be a positive integer")
        return value

    def _validate_nbin_psd(self, value):
        if value is not None and value <= 1:
            raise TraitError("Number of PSD bins should be greater than one")
        return value

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.max_batch = 0

    # ------------------------------------------------------------------------------------------------ pairs
    def _pairs(self, obs, local_dets):
        """(det_names, pairs, det2key) of noise_estimation.py:394-438."""
        det2key = None
        if self.focalplane_key is not None:
            # one detector represents each key value
            fp = obs.telescope.focalplane
            det_names, key2det, det2key = [], {}, {}
            for det in local_dets:
                key = fp[det][self.focalplane_key]
                if key not in key2det:
                    det_names.append(det)
                    key2det[key] = det
                    det2key[det] = key
            reps = list(key2det.values())
            pairs = [[d1, d2] for d1 in reps for d2 in reps
                     if not (d1 == d2 and self.nosingle) and not (d1 != d2 and self.nocross)]
        else:
            det_names = list(obs.local_detectors)
            if len(self.pairs) > 0:
                pairs = [list(p) for p in self.pairs]
            else:
                pairs = []
                for i1, d1 in enumerate(det_names):
                    for d2 in det_names[i1:]:
                        if (d1 == d2 and self.nosingle) or (d1 != d2 and self.nocross):
                            continue
                        pairs.append([d1, d2])
        if self.symmetric:
            # remove duplicate entries (first occurrence kept: a set's order would change from run to run)
            pairs = [list(p) for p in dict.fromkeys(tuple(sorted(p)) for p in pairs)]
        return det_names, pairs, det2key

    # ------------------------------------------------------------------------------------------------ exec
    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        if detectors is not None:
            raise RuntimeError("NoiseEstim cannot be run with subsets of detectors")
        if self.mapfile is not None or self.maskfile is not None:
            raise NotImplementedError("NoiseEstim: map and mask scanning (mapfile / maskfile) are not reproduced")
        # the path follows the data as it arrives: removing the common mode below may leave det_data on the host
        was_resident = [self.det_data in obs.detdata and obs.detdata[self.det_data].accel_in_use() for obs in data.obs]
        if self.focalplane_key is not None:
            if len(self.pairs) > 0:
                raise RuntimeError("focalplane_key is not compatible with pairs")
            if self.remove_common_mode:
                # measure and subtract the common mode signal across the focalplane
                Copy(detdata=[(self.det_data, "temp_signal")]).apply(data)
                for obs in data.obs:
                    obs.detdata["temp_signal"].update_units(obs.detdata[self.det_data].units)
                CommonModeFilter(det_data="temp_signal", det_mask=self.det_mask, det_flags=self.det_flags,
                                 det_flag_mask=self.det_flag_mask, focalplane_key=self.focalplane_key).apply(data)
                Combine(op="subtract", first=self.det_data, second="temp_signal", result=self.det_data).apply(data)
                Delete(detdata=["temp_signal"]).apply(data)

        for iobs, obs in enumerate(data.obs):
            if not obs.is_distributed_by_detector:
                raise NotImplementedError("NoiseEstim: observations split in the sample direction are not supported")
            if self.view is None:
                global_intervals = [(None, None)]
            else:
                global_intervals = [(ival.start, ival.stop) for ival in obs.intervals[self.view]]
            local_dets = obs.select_local_detectors(None, flagmask=self.det_mask)
            good_dets = set(local_dets)
            det_names, pairs, det2key = self._pairs(obs, local_dets)
            times = np.array(obs.shared[self.times].data, dtype=np.float64)
            fsample = float(obs.telescope.focalplane.sample_rate)
            dd = obs.detdata[self.det_data]
            if dd.dtype != np.dtype(np.float64):
                raise RuntimeError(f"detdata '{self.det_data}' is {dd.dtype}: NoiseEstim reads float64")

            todo, cut = [], []
            for det1, det2 in pairs:
                if det1 not in det_names or det2 not in det_names:
                    continue        # a user-specified pair is invalid
                (todo if det1 in good_dets and det2 in good_dets else cut).append((det1, det2))

            on_device = (was_resident[iobs] or dd.accel_in_use()) if use_accel is None else bool(use_accel)
            if on_device and not accel_enabled():
                raise RuntimeError("NoiseEstim: use_accel=True needs the HIP library and an assigned device")
            plan = self._plan(times, global_intervals)
            results = {}
            if todo:
                estimate = self._estimate_device if on_device else self._estimate_host
                results = self._finish(list(estimate(obs, dd, todo, times, plan)), plan, fsample)

            noise_dets, noise_freqs, noise_psds, noise_indices = [], {}, {}, {}
            fp = obs.telescope.focalplane
            for det1, det2 in pairs:
                if (det1, det2) in results:
                    nse_freqs, nse_psd = results[(det1, det2)]
                elif (det1, det2) in cut:
                    # one of the detectors is cut: a zero PSD
                    nse_freqs = np.array([0.0, 1.0e-5, fsample / 4, fsample / 2], dtype=np.float64)
                    nse_psd = np.zeros_like(nse_freqs)
                else:
                    continue
                key = f"{det1} x {det2}" if det1 != det2 else det1
                if key in noise_freqs:
                    continue
                noise_dets.append(key)
                noise_freqs[key] = nse_freqs[1:]
                noise_psds[key] = nse_psd[1:]
                noise_indices[key] = fp[det1].get("uid", name_UID(det1))
            if self.out_model is not None:
                obs[self.out_model] = Noise(detectors=noise_dets, freqs=noise_freqs, psds=noise_psds,
                                            indices=noise_indices)

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def _plan(self, times, global_intervals):
        """Segment tables of the full-rate and of the decimated estimate."""
        period = float(self.stationary_period)
        lagmax = int(self.lagmax)
        if lagmax < 1:
            raise RuntimeError("NoiseEstim: lagmax must be at least one")
        plan = dict(period=period, lagmax=lagmax, full=segment_table(times, times, global_intervals, period))
        if self.nsum > 1:
            times2 = times[:: self.nsum]
            plan["times2"] = times2
            plan["lagmax2"] = min(lagmax, times2.size)
            plan["decim"] = segment_table(times2, times2, global_intervals, period)
        return plan

    def _pair_flags(self, obs, det1, det2):
        flags = np.zeros(obs.n_local_samples, dtype=bool)
        if self.shared_flags is not None:
            flags |= (obs.shared[self.shared_flags].data & self.shared_flag_mask) != 0
        if self.det_flags is not None:
            flags |= (obs.detdata[self.det_flags][det1] & self.det_flag_mask) != 0
            if det1 != det2:
                flags |= (obs.detdata[self.det_flags][det2] & self.det_flag_mask) != 0
        return flags

    # ------------------------------------------------------------------------------------------------ host path
    def _estimate_host(self, obs, dd, todo, times, plan):
        lagmax = plan["lagmax"]
        for det1, det2 in todo:
            flags = self._pair_flags(obs, det1, det2)
            good = flags == 0
            sig1 = highpass_flagged_signal(np.array(dd[det1]), good, lagmax)
            sig2 = None if det1 == det2 else highpass_flagged_signal(np.array(dd[det2]), good, lagmax)
            sig1[flags] = 0
            if sig2 is not None:
                sig2[flags] = 0
            _, _, nreal, n_local, segments = plan["full"]
            out = [lagged_sums_host(sig1, sig2, flags, segments, max(nreal, n_local), lagmax, self.symmetric)]
            if self.nsum > 1:
                lagmax2 = plan["lagmax2"]
                flags2 = flags[:: self.nsum].copy()
                dec1 = highpass_flagged_signal(sig1[:: self.nsum].copy(), flags2 == 0, lagmax2)
                dec2 = None if sig2 is None else highpass_flagged_signal(sig2[:: self.nsum].copy(), flags2 == 0, lagmax2)
                dec1[flags2] = 0
                if dec2 is not None:
                    dec2[flags2] = 0
                _, _, nreal, n_local, segments = plan["decim"]
                out.append(lagged_sums_host(dec1, dec2, flags2, segments, max(nreal, n_local), lagmax2, self.symmetric))
            yield (det1, det2), out

    # ------------------------------------------------------------------------------------------------ device path
    def _estimate_device(self, obs, dd, todo, times, plan):
        make_resident(dd, self.det_data)
        n_rows, n = dd.buffer.shape
        held = []
        try:
            d_shared = d_flags = 0
            n_flag_rows = 0
            if self.shared_flags is not None:
                sh = obs.shared[self.shared_flags]
                if sh.data.dtype != np.uint8:
                    raise RuntimeError("NoiseEstim: shared flags must be uint8 on the device path")
                held.append(Resident(sh, self.shared_flags))
                d_shared = held[-1].ptr
            if self.det_flags is not None:
                fl = obs.detdata[self.det_flags]
                if fl.dtype != np.dtype(np.uint8) or fl.buffer.shape[1] != n:
                    raise RuntimeError("NoiseEstim: detector flags must be uint8 on the device path")
                held.append(Resident(fl, self.det_flags))
                d_flags, n_flag_rows = held[-1].ptr, fl.buffer.shape[0]
            lagmax = plan["lagmax"]
            _, _, nreal1, nloc1, seg1 = plan["full"]
            nra1 = max(nreal1, nloc1)
            per_pair = n * 17 + nra1 * lagmax * 16
            if self.nsum > 1:
                n2, lagmax2 = plan["times2"].size, plan["lagmax2"]
                _, _, nreal2, nloc2, seg2 = plan["decim"]
                nra2 = max(nreal2, nloc2)
                per_pair += n2 * 34 + nra2 * lagmax2 * 16
            batch = int(self.max_batch) if self.max_batch > 0 else max(1, (2 << 30) // per_pair)
            batch = max(1, min(batch, len(todo), 32767))
            for b0 in range(0, len(todo), batch):
                part = todo[b0:b0 + batch]
                yield from self._device_batch(obs, dd, part, n_rows, n, d_shared, d_flags, n_flag_rows, plan)
        finally:
            for h in held:      # the flags were only read: the resident copy stays, a temporary upload goes
                h.host_stays_current()
                h.drop_if_created()

    def _device_batch(self, obs, dd, part, n_rows, n, d_shared, d_flags, n_flag_rows, plan):
        dev = capi.dev
        nb = len(part)
        rows1 = [int(dd.indices([d1])[0]) for d1, _ in part]
        rows2 = [int(dd.indices([d2])[0]) for _, d2 in part]
        if d_flags:
            fl = obs.detdata[self.det_flags]
            frow1 = [int(fl.indices([d1])[0]) for d1, _ in part]
            frow2 = [int(fl.indices([d2])[0]) for _, d2 in part]
        else:
            frow1 = frow2 = [0] * nb
        # one high-passed row per (signal, pair): entry e of the scratch; an auto pair has one
        in_row, entry_good, xrow, yrow = [], [], [], []
        for b in range(nb):
            xrow.append(len(in_row))
            in_row.append(rows1[b])
            entry_good.append(b)
            if rows2[b] != rows1[b]:
                yrow.append(len(in_row))
                in_row.append(rows2[b])
                entry_good.append(b)
            else:
                yrow.append(xrow[-1])
        ne = len(in_row)
        lagmax = plan["lagmax"]
        scratch = []

        def new(shape, dtype, zero=False):
            scratch.append(_Scratch(shape, dtype, zero))
            return scratch[-1]

        def sums_of(table, lag, d_hp, stride, d_good):
            _, _, nreal, n_local, segments = table
            nra = max(nreal, n_local)
            d_sums, d_hits = new((nb, nra, lag), np.float64, True), new((nb, nra, lag), np.int64, True)
            if segments:
                first, last, all_sums, real = (list(x) for x in zip(*segments))
                dev.fod_sums(xrow, yrow, list(range(nb)), d_hp, ne, stride, d_good, nb, stride, first, last,
                             [1 if a else 0 for a in all_sums], real, nra, lag, self.symmetric, d_sums.ptr, d_hits.ptr)
            sums, hits = np.empty((nb, nra, lag)), np.empty((nb, nra, lag), dtype=np.int64)
            dev.noise_estim_fetch(d_sums.ptr, sums, d_hits.ptr, hits)
            return hits, sums

        try:
            good = new((nb, n), np.uint8)
            hp = new((ne, n), np.float64)
            dev.noise_estim_pair_good(n, d_shared, self.shared_flag_mask, d_flags, n_flag_rows, n, self.det_flag_mask,
                                      frow1, frow2, good.ptr, n)
            dev.noise_estim_highpass(n, lagmax, accel_device_ptr(dd.buffer), n_rows, n, in_row, good.ptr, nb, n,
                                     entry_good, hp.ptr, n)
            out = [sums_of(plan["full"], lagmax, hp.ptr, n, good.ptr)]
            if self.nsum > 1:
                n2, lagmax2 = plan["times2"].size, plan["lagmax2"]
                dec, good2, hp2 = new((ne, n2), np.float64), new((nb, n2), np.uint8), new((ne, n2), np.float64)
                dev.noise_estim_decimate(n, self.nsum, hp.ptr, n, entry_good, good.ptr, nb, n, dec.ptr, n2, good2.ptr, n2)
                dev.noise_estim_highpass(n2, lagmax2, dec.ptr, ne, n2, list(range(ne)), good2.ptr, nb, n2, entry_good,
                                         hp2.ptr, n2)
                out.append(sums_of(plan["decim"], lagmax2, hp2.ptr, n2, good2.ptr))
        finally:
            capi.synchronize()
            for s in scratch:
                s.free()
        for b, pair in enumerate(part):
            yield pair, [(h[b], s[b]) for h, s in out]

    # ------------------------------------------------------------------------------------------------ after the sums
    def discard_outliers(self, binfreq, all_psds, all_times):
        """noise_estimation.py:619-693: empty and NaN PSDs go, and with ten or more periods the 5 sigma outliers."""
        all_psds, all_times = [np.array(p) for p in all_psds], list(all_times)
        nrow = len(all_psds)
        ncol = len(all_psds[0])
        i, nempty = 1, 0
        while i < nrow:
            p = all_psds[i]
            if np.all(p == 0) or np.any(np.isnan(p)):
                del all_psds[i]
                del all_times[i]
                nrow -= 1
                nempty += 1
            else:
                i += 1
        nbad = 0
        if nrow >= 10:
            all_good = np.isfinite(np.sum(all_psds, 1))
            for col in range(ncol - 1):
                if binfreq[col] < 0.001:
                    continue
                psdvalues = np.array([x[col] for x in all_psds])
                smooth_values = _medfilt(psdvalues, 11)
                good = np.ones(psdvalues.size, dtype=bool)
                good[psdvalues == 0] = False
                for _ in range(10):
                    # local test
                    diff = np.zeros(psdvalues.size)
                    diff[good] = np.log(psdvalues[good]) - np.log(smooth_values[good])
                    sdev = np.std(diff[good])
                    good[np.abs(diff) > 5 * sdev] = False
                    # global test
                    diff = np.zeros(psdvalues.size)
                    diff[good] = np.log(psdvalues[good]) - np.mean(np.log(psdvalues[good]))
                    sdev = np.std(diff[good])
                    good[np.abs(diff) > 5 * sdev] = False
                all_good[np.logical_not(good)] = False
            bad = np.logical_not(all_good)
            nbad = int(np.sum(bad))
            for ii in np.argwhere(bad).ravel()[::-1]:
                del all_psds[ii]
                del all_times[ii]
        return all_psds, all_times, nempty + nbad

    def _finish(self, collected, plan, fsample):
        """{pair: (frequencies, PSD)} from the sums of all pairs: the transforms of every pair and period in one batch."""
        period = plan["period"]

        def spectra(which, table, lag, rate):
            time_start, time_stop, nreal, _, _ = table
            if nreal == 0:
                return [[] for _ in collected]
            hits = np.concatenate([sums[which][0][:nreal] for _, sums in collected])
            cov = np.concatenate([sums[which][1][:nreal] for _, sums in collected])
            psdfreq, psd, _ = psds_from_sums(hits, cov, lag, lag, rate)
            out = []
            for k in range(len(collected)):
                out.append([(time_start + r * period, min(time_start + r * period + period, time_stop), psdfreq,
                             psd[k * nreal + r]) for r in range(nreal)])
            return out

        first = spectra(0, plan["full"], plan["lagmax"], fsample)
        second = spectra(1, plan["decim"], plan["lagmax2"], fsample / self.nsum) if self.nsum > 1 else [None] * len(first)
        return {pair: self._finish_pair(p1, p2, plan, fsample) for (pair, _), p1, p2 in zip(collected, first, second)}

    def _finish_pair(self, my_psds1, my_psds2, plan, fsample):
        """(frequencies, PSD) of one pair from its PSDs per period (noise_estimation.py:1071-1231 for one process)."""
        period = plan["period"]
        if self.nsum > 1:
            # both sets start at the same time and advance by the same period: equal length
            keep = min(len(my_psds1), len(my_psds2))
            my_psds1, my_psds2 = my_psds1[:keep], my_psds2[:keep]
        fmin, fmax = 1 / period, fsample / 2
        binned1, my_times, binfreq1 = bin_psds(my_psds1, self.nbin_psd, fmin, fmax)
        if binfreq1 is None:
            raise RuntimeError("None of the processes have valid PSDs")
        if self.nsum > 1:
            binned2, _, binfreq2 = bin_psds(my_psds2, self.nbin_psd, fmin, fmax)
            # frequencies that are usable in the down-sampled PSD
            fcut = fsample / 2 / self.naverage / 100
            ind1 = binfreq1 > fcut
            ind2 = binfreq2 <= fcut
            binfreq = np.hstack([binfreq2[ind2], binfreq1[ind1]])
            binned = [np.hstack([p2[ind2], p1[ind1]]) for p1, p2 in zip(binned1, binned2)]
        else:
            binfreq, binned = binfreq1, binned1
        good_psds, _, _ = self.discard_outliers(binfreq, binned, my_times)
        return binfreq, np.mean(np.array(good_psds), axis=0)

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        req = {"meta": [], "shared": [self.times], "detdata": [self.det_data], "intervals": []}
        if self.shared_flags is not None:
            req["shared"].append(self.shared_flags)
        if self.det_flags is not None:
            req["detdata"].append(self.det_flags)
        if self.view is not None:
            req["intervals"].append(self.view)
        return req

    def _provides(self):
        return {"meta": [] if self.out_model is None else [self.out_model], "shared": [], "detdata": []}
