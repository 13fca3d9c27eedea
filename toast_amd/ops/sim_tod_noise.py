"""SimNoise: noise timestreams drawn from the PSDs of a noise model (reference: src/toast/ops/sim_tod_noise.py:20-432).

Every noise stream is the inverse real transform of unit Gaussians from the counter-based generator
(``toast_amd.rng``; key1 = realization * 2^32 + telescope * 2^16 + component, key2 = session * 2^32 + stream index,
counter2 = sample) scaled by the interpolated PSD, cropped to the observation and mixed into the detectors with the
noise model's mixing matrix.  The compiled path of the reference (``py=False``) is the one reproduced, quirks included
(DESIGN.md).

Two paths, chosen by where ``det_data`` lives:

* resident on the device (or ``use_accel=True``): toast_hip_sim_noise_dev writes straight into the device buffer --
  spectrum kernel, batched rocFFT, crop and mix (csrc/sim_noise.hip);
* on the host: the library's host entries with the same arithmetic (``capi.tod_sim_noise_timestream*``).
"""

import numpy as np

from .. import capi
from ..accel import accel_device_ptr, accel_enabled, make_resident
from ..data import defaults
from ..traits import Bool, Int, TraitError, Unicode
from .operator import Operator


def rate_from_times(timestamps):
    """Sample rate from the median time step (reference src/toast/utils.py:655-685)."""
    return 1.0 / np.median(np.diff(np.asarray(timestamps, dtype=np.float64)))


def sim_noise_timestream(realization=0, telescope=0, component=0, sindx=0, detindx=0, rate=1.0, firstsamp=0, samples=0,
                         oversample=2, freq=None, psd=None, py=False):
    """One noise timestream from a starting RNG state (sim_tod_noise.py:20-188), on the host.  ``py=True`` -- the
    reference's pure-Python variant with its different frequency grid -- is not reproduced."""
    if py:
        raise NotImplementedError("sim_noise_timestream: only the compiled path (py=False) is reproduced")
    tdata = np.zeros(int(samples), dtype=np.float64)
    capi.tod_sim_noise_timestream(realization, telescope, component, sindx, detindx, rate, firstsamp, oversample,
                                  np.ascontiguousarray(freq, dtype=np.float64),
                                  np.ascontiguousarray(psd, dtype=np.float64), tdata)
    return tdata


class SimNoise(Operator):
    """Operator which generates noise timestreams and accumulates them into ``det_data``.

    The observation's session uid enters the random number generation.  There is intentionally no ``view`` trait:
    to avoid discontinuities the whole observation is simulated whatever views later analysis uses.
    ``serial`` is accepted for compatibility; both values give the same numbers.  ``max_batch`` (attribute, 0 =
    automatic) bounds the noise streams per device batch; the result does not depend on it."""

    API = Int(0, help="Internal interface version for this operator")
    noise_model = Unicode("noise_model", help="Observation key containing the noise model")
    realization = Int(0, help="The noise realization index")
    component = Int(0, help="The noise component index")
    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    det_data = Unicode(defaults.det_data, help="Observation detdata key for accumulating noise timestreams")
    det_data_units = Unicode(defaults.det_data_units, help="Output units if creating detector data")
    serial = Bool(True, help="Use legacy serial implementation instead of batched")

    def _validate_realization(self, value):
        if value < 0:
            raise TraitError("realization index must be positive")
        return value

    def _validate_component(self, value):
        if value < 0:
            raise TraitError("component index must be positive")
        return value

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self._oversample = 2
        self.max_batch = 0

    def _exec(self, data, detectors=None, use_accel=None, **kwargs):
        for ob in data.obs:
            dets = ob.select_local_detectors(detectors)
            sindx = int(ob.session.uid)
            telescope = int(ob.telescope.uid)
            if self.noise_model not in ob:
                raise KeyError(f"Observation does not contain noise model key '{self.noise_model}'")
            nse = ob[self.noise_model]
            if not ob.is_distributed_by_detector:
                raise NotImplementedError(
                    "Noise simulation for process grids with multiple ranks in the sample direction not implemented")
            ob.detdata.ensure(self.det_data, detectors=dets, create_units=self.det_data_units)
            if len(dets) == 0:
                continue
            rate = rate_from_times(ob.shared[self.times].data)
            # the streams with weight in any selected detector, in key order (sim_tod_noise.py:304, :337-354)
            keys = nse.all_keys_for_dets(dets)
            if len(keys) == 0:
                continue
            freq = np.ascontiguousarray(nse.freq(keys[0]), dtype=np.float64)
            for key in keys[1:]:
                test = nse.freq(key)
                if len(test) != len(freq) or test[0] != freq[0] or test[-1] != freq[-1]:
                    raise RuntimeError("All psds must have the same frequency values")
            psds = np.ascontiguousarray([nse.psd(key) for key in keys], dtype=np.float64)
            indices = np.array([int(nse.index(key)) for key in keys], dtype=np.uint64)
            dd = ob.detdata[self.det_data]
            if dd.dtype != np.dtype(np.float64):
                raise RuntimeError(f"detdata '{self.det_data}' is {dd.dtype}: SimNoise accumulates into float64")
            on_device = dd.accel_in_use() if use_accel is None else bool(use_accel)
            if on_device:
                if not accel_enabled():
                    raise RuntimeError("SimNoise: use_accel=True needs the HIP library and an assigned device")
                make_resident(dd, self.det_data)
                ptr, rows, weights = [0], [], []
                for key in keys:
                    for det in dets:
                        weight = nse.weight(det, key)
                        if weight == 0:
                            continue
                        rows.append(int(dd.indices([det])[0]))
                        weights.append(float(weight))
                    ptr.append(len(rows))
                n_rows, n_samp = dd.buffer.shape[0], dd.buffer.shape[1]
                capi.dev.sim_noise(self.realization, telescope, self.component, sindx, rate, ob.local_index_offset,
                                   ob.n_local_samples, self._oversample, indices, freq, psds,
                                   accel_device_ptr(dd.buffer), n_rows, row_stride=n_samp, mix_ptr=ptr, mix_row=rows,
                                   mix_weight=weights, max_batch=self.max_batch)
            else:
                noise = np.zeros((len(keys), ob.n_local_samples))
                capi.tod_sim_noise_timestream_batch(self.realization, telescope, self.component, sindx, rate,
                                                    ob.local_index_offset, self._oversample, indices, freq, psds, noise)
                for ikey, key in enumerate(keys):
                    for det in dets:
                        weight = nse.weight(det, key)
                        if weight == 0:
                            continue
                        dd[det] += weight * noise[ikey]

    def _finalize(self, data, **kwargs):
        return

    def _requires(self):
        return {"meta": [self.noise_model], "shared": [self.times], "detdata": [self.det_data]}

    def _provides(self):
        return {"detdata": [self.det_data]}
