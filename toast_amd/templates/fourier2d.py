"""Fourier2D template: smooth 2-D Fourier modes across the focal plane, ``nmode`` amplitudes per SAMPLE shared by all
detectors, with a time-domain correlation prior.  The reference's model for correlated atmosphere and common-mode drifts.

Reference: src/toast/templates/fourier2d.py (NumPy and SciPy, one detector at a time).  The amplitude layout is the
reference's: ``[sample of the view][mode]``, view after view, observation after observation; no amplitude flags.

Two paths.  The host path (``use_accel`` false) is NumPy and SciPy with the reference's own expressions.  The device path
(``add_to_signal_multi`` / ``project_signal_multi``, what ``TemplateMatrix`` looks for, ``_add_prior`` and
``_apply_precond`` on resident vectors, and the norms at set-up when the accelerator is on) runs the kernels of
csrc/fourier2d.hip.  The tables that are small or built once stay host NumPy on both paths: the ``[n_det][nmode]`` basis
(fourier2d.py:213-231) and the filter of every view (``rfft``, floor, ``irfft``: fourier2d.py:266-282).

Properties of the reference that are reproduced on both paths and matter to callers:

* ``project_signal`` applies NO flags and ACCUMULATES (fourier2d.py:416-435);
* ``norms = 1 / sum_d good T^2 w`` with the detector flags applied, 0 where no detector has a good sample (:342-365);
* the filter has ``L`` taps for a view of an even number ``L`` of samples and ``L - 1`` for an odd one, and its floor
  ``fcorr < 1e-6 amp`` compares complex numbers the way NumPy orders them: by the real part, then by the imaginary one.

A view of one sample makes the reference fail inside ``irfft``; here ``_initialize`` raises ``ValueError`` with the
observation and the view.  Amplitudes shared between the processes of a detector-sharded run are not built:
``_initialize`` raises ``NotImplementedError`` when the data communicator has more than one process.
"""

import numpy as np
import scipy.signal

from ..accel import accel_device_ptr, device_scratch
from ..data import defaults, detector_direction
from ..traits import Bool, Float, Int, Unicode
from . import Amplitudes, DeviceMirror, Template, release_borrowed


def evaluate_template(theta, phi, radius, order, fit_subharmonics):
    """The mode values at one detector: fourier2d.py:213-231, the same array expressions."""
    nmode = (2 * order) ** 2 + 1 + (2 if fit_subharmonics else 0)
    values = np.zeros(nmode)
    values[0] = 1
    offset = 1
    if fit_subharmonics:
        values[1:3] = theta / radius, phi / radius
        offset += 2
    if order > 0:
        rinv = np.pi / radius
        orders = np.arange(order) + 1
        thetavec = np.zeros(order * 2)
        phivec = np.zeros(order * 2)
        thetavec[::2] = np.cos(orders * theta * rinv)
        thetavec[1::2] = np.sin(orders * theta * rinv)
        phivec[::2] = np.cos(orders * phi * rinv)
        phivec[1::2] = np.sin(orders * phi * rinv)
        values[offset:] = np.outer(thetavec, phivec).ravel()
    return values


def inverse_correlation(times, corr_len, amplitude):
    """-> (invcorr, number of floored frequencies): the filter of one view, fourier2d.py:266-282.  ``L`` taps for an even
    number of samples, ``L - 1`` for an odd one."""
    corr = np.exp((times[0] - times) / corr_len) * amplitude
    ihalf = times.size // 2
    if times.size % 2 == 0:
        corr[ihalf:] = corr[ihalf - 1:: -1]
    else:
        corr[ihalf + 1:] = corr[ihalf - 1:: -1]
    fcorr = np.fft.rfft(corr)
    floor = 1.0e-6 * amplitude
    # `fcorr < floor` on complex numbers: NumPy's lexicographic order, written out
    too_small = (fcorr.real < floor) | ((fcorr.real == floor) & (fcorr.imag < 0.0))
    fcorr[too_small] = floor
    return np.fft.irfft(1 / fcorr), int(np.count_nonzero(too_small))


def prior_fft_length(view_len, filter_len):
    """Points of the circular convolution that holds the full linear one: the next power of two."""
    n = 2
    while n < view_len + filter_len - 1:
        n *= 2
    return n


def half_complex(spectrum, n_fft):
    """``np.fft.rfft`` output -> FFTW half-complex layout r_0 .. r_{n/2}, i_{n/2-1} .. i_1."""
    out = np.empty(n_fft, dtype=np.float64)
    out[:n_fft // 2 + 1] = spectrum.real
    out[n_fft // 2 + 1:] = spectrum.imag[1:n_fft // 2][::-1]
    return out


class Fourier2D(Template):
    """2-D Fourier modes across the focal plane: ``(2 order)^2 + 1`` amplitudes per sample (+ 2 with subharmonics)."""

    times = Unicode(defaults.times, help="Observation shared key for timestamps")
    correlation_length = Float(10.0, help="Correlation length in time [s]")
    correlation_amplitude = Float(10.0, help="Scale factor of the filter")
    order = Int(1, help="The filter order")
    fit_subharmonics = Bool(True, help="If True, fit subharmonics")
    noise_model = Unicode(None, allow_none=True, help="Observation key containing the optional noise model")
    debug_plots = Unicode(None, allow_none=True, help="If not None, make debugging plots in this directory")

    def __init__(self, **kwargs):
        self._dev_tables = {}
        self._work = (0, 0)
        self._prior_views = None
        super().__init__(**kwargs)

    # ------------------------------------------------------------------ set-up
    @property
    def nmode(self):
        return (2 * self.order) ** 2 + 1 + (2 if self.fit_subharmonics else 0)

    @staticmethod
    def _max_modes():
        from .. import capi

        return capi.dev.fourier2d_max_modes()

    def _initialize(self, new_data):
        from ..accel import accel_enabled

        self.clear()
        if self.order < 1:
            raise RuntimeError("Fourier2D: filter order should be >= 1")      # fourier2d.py:69-74
        if self.debug_plots is not None:
            raise RuntimeError("Fourier2D: debug_plots must be None, there is no plotting here")
        comm = new_data.comm
        if comm is not None and comm.comm_world is not None and comm.world_size > 1:
            raise NotImplementedError("Fourier2D: the amplitudes would be shared between the processes that hold the "
                                      "detectors of an observation; that reduction is not built: run on one process")
        nmode = self.nmode
        all_dets = {}
        self._obs_dets = {}
        self._obs_view_offset = {}      # first local amplitude of every view
        self._local_ranges = []
        offset = 0
        for iob, ob in enumerate(new_data.obs):
            dets = self._obs_detectors(ob)
            self._obs_dets[iob] = set(dets)
            all_dets.update(dict.fromkeys(dets))
            offs = []
            obs_first = offset      # the observation's amplitudes start here in the global vector too
            for ivw, vw in enumerate(ob.intervals[self.view]):
                view_len = int(vw.last - vw.first)
                if view_len == 1:
                    raise ValueError(f"Fourier2D template {self.name}: view {ivw} of observation {ob.name} has one sample: "
                                     "its correlation filter does not exist")
                offs.append(offset)
                # fourier2d.py:169-178: the global index counts from the view's first sample in the observation
                self._local_ranges.append((obs_first + int(vw.first) * nmode, view_len * nmode))
                offset += view_len * nmode
            self._obs_view_offset[iob] = np.array(offs, dtype=np.int64)
        self._all_dets = list(all_dets.keys())
        self._n_local = offset
        self._n_global = offset
        self._mirrors["norms"] = DeviceMirror(np.zeros(self._n_local, dtype=np.float64), f"{self.name}_norms")
        # basis and filters: host NumPy on both paths
        self._templates, self._filters, self._filter_floored = {}, {}, {}
        corr_len, amp = float(self.correlation_length), float(self.correlation_amplitude)
        for iob, ob in enumerate(new_data.obs):
            fp = ob.telescope.focalplane
            radius = 0.5 * fp.field_of_view
            self._templates[iob] = {}
            for det in ob.local_detectors:
                if det not in self._obs_dets[iob]:
                    continue
                x, y, z = detector_direction(fp[det]["quat"])
                theta, phi = np.arcsin([x, y])
                self._templates[iob][det] = evaluate_template(theta, phi, radius, self.order, self.fit_subharmonics)
            self._filters[iob], self._filter_floored[iob] = [], []
            t = ob.shared[self.times].data
            for vw in ob.intervals[self.view]:
                invcorr, floored = inverse_correlation(np.asarray(t[vw.first:vw.last], dtype=np.float64), corr_len, amp)
                self._filters[iob].append(invcorr)
                self._filter_floored[iob].append(floored)
        # fourier2d.py:367-376
        self._filter_scale = np.zeros(nmode)
        self._filter_scale[0] = 1
        first = 1
        if self.fit_subharmonics:
            self._filter_scale[1:3] = 2
            first += 2
        self._filter_scale[first:] = 4
        self._filter_scale *= amp
        if self._n_local == 0:
            return
        if accel_enabled() and self.supports_accel():
            self._norms_device(new_data)
            self._prior_plan(new_data)      # spectra and work rows now: nothing is allocated inside the PCG loop
        else:
            self._norms_host(new_data)

    def _obs_det_list(self, iob, ob):
        """The detectors of one observation in the order the reference's set-up takes them."""
        return [d for d in ob.local_detectors if d in self._obs_dets[iob]]

    def _norms_host(self, new_data):
        """fourier2d.py:320-365"""
        nmode = self.nmode
        norms = self._norms
        for iob, ob in enumerate(new_data.obs):
            dets = self._obs_det_list(iob, ob)
            weights = self._det_weights(ob, dets)
            for ivw, vw in enumerate(ob.intervals[self.view]):
                view_len = int(vw.last - vw.first)
                first = int(self._obs_view_offset[iob][ivw])
                norms_view = norms[first:first + view_len * nmode].reshape((-1, nmode))
                good = np.empty(view_len, dtype=np.float64)
                for det, detweight in zip(dets, weights):
                    good[:] = 1.0
                    if self.det_flags is not None:
                        flags = ob.detdata[self.det_flags][det, vw.first:vw.last]
                        good[(flags & self.det_flag_mask) != 0] = 0
                    norms_view += np.outer(good, self._templates[iob][det] ** 2 * detweight)
        nonzero = norms != 0
        norms[nonzero] = 1.0 / norms[nonzero]

    def _norms_device(self, new_data):
        """The same sums by toast_hip_fourier2d_norms_dev over the resident flags; the norms stay on the device."""
        from .. import capi

        nmode = self.nmode
        norms = self._mirrors["norms"].create(zero_out=True)
        for iob, ob in enumerate(new_data.obs):
            dets = self._obs_det_list(iob, ob)
            if len(dets) == 0 or len(ob.intervals[self.view]) == 0:
                continue
            weights = self._det_weights(ob, dets)
            w2 = np.ascontiguousarray([self._templates[iob][d] ** 2 * w for d, w in zip(dets, weights)], dtype=np.float64)
            borrowed = []
            try:
                with device_scratch(self.name) as s:
                    s.inp("w2", w2)
                    f_idx, f_ptr = self._det_flag_args(ob, dets, borrowed)
                    capi.dev.fourier2d_norms(nmode, s.ptr("w2"), self._obs_view_offset[iob], f_idx, f_ptr,
                                             self.det_flag_mask, len(dets), ob.n_local_samples,
                                             ob.intervals[self.view].data, norms.ptr)
            finally:
                release_borrowed(borrowed)
        norms.written()

    # The norms are computed on the device when the accelerator is on and read there by the preconditioner: the host
    # copy is fetched when somebody asks for it.
    _norms = property(lambda self: self._mirrors["norms"].host)

    # ------------------------------------------------------------------ Template interface
    def _detectors(self):
        return self._all_dets

    def _zeros(self):
        # no amplitude flags: a sample flagged in every detector just does not contribute (fourier2d.py:381-393)
        return Amplitudes(self.data.comm, self._n_global, self._n_local, local_ranges=self._local_ranges)

    def _supports_accel(self):
        return self.nmode <= self._max_modes()

    def _device_table(self, key, build):
        """A small table registered on the device once per template, released by ``clear()``."""
        if key not in self._dev_tables:
            self._dev_tables[key] = DeviceMirror(np.ascontiguousarray(build(), dtype=np.float64),
                                                 f"{self.name}_table{len(self._dev_tables)}")
        return self._dev_tables[key].upload().ptr

    def _template_table(self, iob, dets):
        return self._device_table(("T", iob, tuple(dets)), lambda: [self._templates[iob][d] for d in dets])

    def add_to_signal_multi(self, detectors, amplitudes, n_group=0, **kwargs):
        """All detectors and all views of an observation in one launch (device-resident buffers only)."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            if len(ob.intervals[self.view]) == 0:
                continue
            capi.dev.fourier2d_add_to_signal(self.nmode, self._template_table(iob, dets), self._obs_view_offset[iob],
                                             accel_device_ptr(amplitudes.buffer), dd.indices(dets),
                                             accel_device_ptr(dd.buffer), ob.n_local_samples, ob.intervals[self.view].data,
                                             n_group=n_group)

    def project_signal_multi(self, detectors, amplitudes, n_group=0, **kwargs):
        """No flags, and the amplitudes are accumulated: see the module docstring."""
        from .. import capi

        for iob, ob, dets, dd in self._device_sweep(detectors, amplitudes):
            if len(ob.intervals[self.view]) == 0:
                continue
            capi.dev.fourier2d_project_signal(self.nmode, self._template_table(iob, dets), self._obs_view_offset[iob],
                                              accel_device_ptr(amplitudes.buffer), dd.indices(dets),
                                              accel_device_ptr(dd.buffer), ob.n_local_samples, ob.intervals[self.view].data,
                                              n_group=n_group)

    def _view_slices(self, iob, ob):
        nmode = self.nmode
        for ivw, vw in enumerate(ob.intervals[self.view]):
            first = int(self._obs_view_offset[iob][ivw])
            yield ivw, vw, slice(first, first + int(vw.last - vw.first) * nmode, 1)

    def _add_to_signal_host(self, detector, amplitudes):
        nmode = self.nmode
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            for ivw, vw, amp_slice in self._view_slices(iob, ob):
                row[vw.first:vw.last] += np.sum(local[amp_slice].reshape((-1, nmode)) * self._templates[iob][detector], 1)

    def _project_signal_host(self, detector, amplitudes):
        nmode = self.nmode
        local = amplitudes.local
        for iob, ob in enumerate(self.data.obs):
            if detector not in self._obs_dets[iob]:
                continue
            row = ob.detdata[self.det_data][detector]
            for ivw, vw, amp_slice in self._view_slices(iob, ob):
                amp_view = local[amp_slice].reshape((-1, nmode))
                amp_view[:] += np.outer(row[vw.first:vw.last], self._templates[iob][detector])

    def _prior_plan(self, data=None):
        """Per view: (first amplitude, samples, taps, transform length, key of its spectrum), and the work buffer.
        Built by ``_initialize`` when the accelerator is on; otherwise when the first resident vector arrives."""
        from .. import capi

        if self._prior_views is None:
            nmode = self.nmode
            views, most = [], 0
            for iob, ob in enumerate((self.data if data is None else data).obs):
                for ivw, vw in enumerate(ob.intervals[self.view]):
                    view_len = int(vw.last - vw.first)
                    if view_len <= 0:
                        continue
                    filt = self._filters[iob][ivw]
                    n_fft = prior_fft_length(view_len, filt.size)
                    key = ("S", iob, ivw)
                    self._device_table(key, lambda f=filt, n=n_fft: half_complex(np.fft.rfft(f, n), n))
                    views.append((int(self._obs_view_offset[iob][ivw]), view_len, int(filt.size), n_fft, key))
                    most = max(most, n_fft)
            self._prior_views = views
            nbytes = 8 * 2 * nmode * most
            if nbytes > 0:
                self._work = (capi.device_malloc(nbytes), nbytes)
        return self._prior_views

    def _prior_device(self, amplitudes_in, amplitudes_out):
        from .. import capi

        nmode = self.nmode
        d_in, d_out = accel_device_ptr(amplitudes_in.buffer), accel_device_ptr(amplitudes_out.buffer)
        for first, view_len, taps, n_fft, key in self._prior_plan():
            capi.dev.fourier2d_add_prior(nmode, view_len, d_in + 8 * first, d_out + 8 * first, taps, n_fft,
                                         self._dev_tables[key].ptr, self._filter_scale, self._work[0])

    def _add_prior(self, amplitudes_in, amplitudes_out, use_accel=None, **kwargs):
        from ..accel import accel_enabled

        if self._n_local == 0:
            return
        nmode = self.nmode
        if self.supports_accel() and (accel_enabled() or amplitudes_in.accel_in_use() or amplitudes_out.accel_in_use()):
            # a convolution over every view and mode: on the device whenever there is one, like the Offset template's
            # noise prior, also for vectors that the caller keeps on the host
            self._on_device(amplitudes_in, amplitudes_out, lambda: self._prior_device(amplitudes_in, amplitudes_out))
            return
        # fourier2d.py:437-455
        a_in, a_out = amplitudes_in.local, amplitudes_out.local
        for iob, ob in enumerate(self.data.obs):
            for ivw, vw, amp_slice in self._view_slices(iob, ob):
                in_view = a_in[amp_slice].reshape((-1, nmode))
                out_view = a_out[amp_slice].reshape((-1, nmode))
                for mode in range(nmode):
                    scale = self._filter_scale[mode]
                    out_view[:, mode] += scipy.signal.convolve(in_view[:, mode], self._filters[iob][ivw] * scale, mode="same")

    def _apply_precond(self, amplitudes_in, amplitudes_out, use_accel=None, **kwargs):
        if self._n_local == 0:
            return
        if self.supports_accel() and (amplitudes_in.accel_in_use() or amplitudes_out.accel_in_use()):
            from .. import capi

            amplitudes_in.accel_resident()
            amplitudes_out.accel_resident()
            capi.dev.fourier2d_apply_precond(self._n_local, self._mirrors["norms"].upload().ptr,
                                             accel_device_ptr(amplitudes_in.buffer), accel_device_ptr(amplitudes_out.buffer))
            return
        # fourier2d.py:457-459
        amplitudes_out.local[:] = amplitudes_in.local
        amplitudes_out.local *= self._norms

    def device_tables(self):
        """The host keys of everything this template has registered on the device (tests / inspection)."""
        keys = [m.buffer for m in self._dev_tables.values()]
        return keys + [m.buffer for m in self._mirrors.values() if m.on_device]

    def clear(self):
        """Release everything this template registered: basis tables, spectra, the norms and the prior's work buffer."""
        from .. import capi

        super().clear()          # (fetches first: somebody may still read the norms on the host)
        for mirror in self._dev_tables.values():
            mirror.drop(fetch=False)
        self._dev_tables = {}
        ptr, nbytes = self._work
        if ptr:
            capi.device_release(ptr, nbytes)
        self._work = (0, 0)
        self._prior_views = None
