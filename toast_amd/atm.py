"""AtmSim: one simulated atmosphere slab and its observation (reference: src/toast/atm.py:40-517).

The reference's ``AtmSim`` draws a wind and a turbulence realization, builds a compressed 3-D volume with CHOLMOD
(``simulate()``) and integrates detector lines of sight through it (``observe()`` -> ``toast::atm_sim_observe``,
src/libtoast/src/toast_atm_observe.cpp:246-488).  This class is the OBSERVING half: it holds what the reference's object
holds after ``simulate()`` -- the ``_name`` attributes of atm.py:137-231 and the volume attributes that ``observe``
passes on (atm.py:464-503) -- and is built from that state, whoever produced it: the reference's generator on a host
that has CHOLMOD, a cache, or a stand-in (``toast_amd.atm.standin_slab``).  ``simulate()`` raises.

``observe`` runs ``toast_hip_atm_observe_dev`` (csrc/atm_observe.hip) when a device is usable, with the volume uploaded
once and resident until ``close()``; otherwise a NumPy path that vectorises over samples and loops over the ray steps.
Angles are radians, lengths metres, times seconds, temperatures kelvin: plain floats."""

import numpy as np

from . import capi
from .accel import DeviceMirror, accel_data_present, accel_device_ptr, accel_enabled, device_scratch

TWOPI = 2 * np.pi

#: the launch options of the observe kernel that measured better on an MI355X: the compressed index
#: as int32 whenever nelem allows it, no one-cell register cache
INDEX32 = True
CELL_CACHE = False


def ray_steps(xstep, rmin, rmax, fixed_r, elmax, zmax):
    """(first radius, number of steps) of every line of sight (toast_atm_observe.cpp:359-375, :477-479): r starts at
    1.5 xstep and is advanced by repeated additions of xstep while r < rmin, or is the single ``fixed_r`` > 0; the walk
    ends at r > rmax or r sin(elmax) >= zmax.  None of it depends on the sample."""
    sin_el_max = np.sin(elmax)
    r = 1.5 * xstep
    while r < rmin:
        r += xstep
    if fixed_r > 0:
        r = fixed_r
    first, n = r, 0
    while True:
        if r > rmax or r * sin_el_max >= zmax:
            break
        n += 1
        r += xstep
        if fixed_r > 0:
            break
    return first, n


class AtmSim:
    """A simulated slab of the atmosphere that moves with a constant wind and can be observed by detectors.

    Args:
        azmin, azmax, elmin, elmax (float):  The cone the volume covers [rad].
        tmin, tmax (float):  The time range.
        T0 (float):  Ground temperature [K].
        zatm (float):  Atmosphere extent for the temperature profile [m].
        zmax (float):  Water vapor extent for the integration [m].
        xstep, ystep, zstep (float):  Size of a volume element [m].
        rmin, rmax (float):  Line-of-sight observing distances [m].
        wx, wy, wz (float):  Wind in the scan frame [m/s].
        xstart, delta_x, ystart, delta_y, zstart, delta_z (float):  The box of the volume [m].
        maxdist (float):  Largest distance of the cone [m] (kept for the reference's signature; not read).
        nx, ny, nz (int):  Elements of the box along each axis.
        xstride, ystride, zstride (int):  Strides of the full index; the reference's (ny nz, nz, 1) when None.
        compressed_index (array, int64, nx ny nz):  Element number of every cell of the box; outside [0, nelem) where
            the cell was not simulated.
        full_index (array, int64, nelem):  Cell of every element.
        realization (array, float64, nelem):  The simulated values.
    """

    def __init__(self, azmin, azmax, elmin, elmax, tmin, tmax, *, T0, zatm, zmax, xstep, ystep, zstep, rmin, rmax,
                 wx, wy, wz, xstart, delta_x, ystart, delta_y, zstart, delta_z, maxdist, nx, ny, nz, compressed_index,
                 full_index, realization, xstride=None, ystride=None, zstride=None):
        self._azmin, self._azmax = float(azmin), float(azmax)
        self._elmin, self._elmax = float(elmin), float(elmax)
        self._tmin, self._tmax = float(tmin), float(tmax)
        self._T0 = float(T0)
        self._zatm, self._zmax = float(zatm), float(zmax)
        self._xstep, self._ystep, self._zstep = float(xstep), float(ystep), float(zstep)
        self._rmin, self._rmax = float(rmin), float(rmax)
        self._wx, self._wy, self._wz = float(wx), float(wy), float(wz)
        self._xstart, self._delta_x = float(xstart), float(delta_x)
        self._ystart, self._delta_y = float(ystart), float(delta_y)
        self._zstart, self._delta_z = float(zstart), float(delta_z)
        self._maxdist = float(maxdist)
        self._nx, self._ny, self._nz = int(nx), int(ny), int(nz)
        self._compressed_index = self._full_index = self._realization = None
        self._dev_index = self._dev_realization = None
        self._cached = False

        # the constructor's range errors (atm.py:190-203)
        if self._azmin >= self._azmax:
            raise RuntimeError("AtmSim: azmin >= azmax")
        if self._elmin < 0:
            raise RuntimeError("AtmSim: elmin < 0")
        if self._elmax > 0.5 * np.pi:
            raise RuntimeError("AtmSim: elmax > pi/2")
        if self._elmin > self._elmax:
            raise RuntimeError("AtmSim: elmin >= elmax")
        if self._tmin >= self._tmax:
            raise RuntimeError("AtmSim: tmin >= tmax")
        if not (self._xstep > 0 and self._ystep > 0 and self._zstep > 0):
            raise RuntimeError("AtmSim: the volume element sizes must be positive")
        if self._zatm == 0:
            raise RuntimeError("AtmSim: zatm must not be zero")

        # one process, nothing drawn: what the reference's object holds of its generator is absent, the rest is here
        self._comm, self._ntask, self._rank = None, 1, 0

        self._delta_az = self._azmax - self._azmin
        self._delta_el = self._elmax - self._elmin
        self._delta_t = self._tmax - self._tmin
        self._az0 = self._azmin + self._delta_az / 2
        self._el0 = self._elmin + self._delta_el / 2
        self._sinel0 = np.sin(self._el0)
        self._cosel0 = np.cos(self._el0)
        self._xxstep = self._xstep * self._cosel0 - self._zstep * self._sinel0
        self._yystep = self._ystep
        self._zzstep = self._xstep * self._sinel0 + self._zstep * self._cosel0

        # the volume (atm.py:464-503 passes these on)
        if self._nx < 2 or self._ny < 2 or self._nz < 2:
            raise RuntimeError("AtmSim: the box needs at least two elements along every axis")
        self._nn = self._nx * self._ny * self._nz
        self._xstride = self._ny * self._nz if xstride is None else int(xstride)
        self._ystride = self._nz if ystride is None else int(ystride)
        self._zstride = 1 if zstride is None else int(zstride)
        if min(self._xstride, self._ystride, self._zstride) < 1:
            raise RuntimeError("AtmSim: the strides must be positive")
        reach = (self._nx - 1) * self._xstride + (self._ny - 1) * self._ystride + (self._nz - 1) * self._zstride
        if reach >= self._nn:
            raise RuntimeError(f"AtmSim: the strides reach element {reach} of a box of nn = nx*ny*nz = {self._nn}")
        ci = np.ascontiguousarray(compressed_index, dtype=np.int64).reshape(-1)
        fi = np.ascontiguousarray(full_index, dtype=np.int64).reshape(-1)
        re = np.ascontiguousarray(realization, dtype=np.float64).reshape(-1)
        if ci.size != self._nn:
            raise RuntimeError(f"AtmSim: compressed_index has {ci.size} entries, the box nn = {self._nn}")
        if re.size < 1 or fi.size != re.size:
            raise RuntimeError("AtmSim: full_index and realization sizes are not consistent")
        self._nelem = int(re.size)
        if fi.min() < 0 or fi.max() >= self._nn:
            raise RuntimeError("AtmSim: full_index names a cell outside the box")
        self._compressed_index, self._full_index, self._realization = ci, fi, re
        self._cached = True

    # ------------------------------------------------------------------ the reference's surface
    def close(self):
        """Explicitly free memory: the device copy of the volume, then the arrays (atm.py:233-246)."""
        for name in ("_dev_index", "_dev_realization"):
            mirror = getattr(self, name, None)
            if mirror is not None:
                mirror.drop(fetch=False)
            setattr(self, name, None)
        self._compressed_index = self._full_index = self._realization = None
        self._cached = False

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    azmin = property(lambda self: self._azmin)
    azmax = property(lambda self: self._azmax)
    elmin = property(lambda self: self._elmin)
    elmax = property(lambda self: self._elmax)
    tmin = property(lambda self: self._tmin)
    tmax = property(lambda self: self._tmax)

    def simulate(self, use_cache=False, smooth=False):
        raise NotImplementedError(
            "AtmSim.simulate: generating the volume (GenerateAtmosphere, CHOLMOD) is not part of toast_amd; build the "
            "AtmSim from a volume produced elsewhere (compressed_index, full_index, realization)")

    def observe(self, times, az, el, tod, fixed_r=-1, use_accel=None):
        """Observe the atmosphere with a detector: ``tod`` += the line-of-sight integral at every (times, az, el)
        sample (atm.py:434-517).  Returns the status (zero == good; 1: samples outside the cone were skipped or rays
        left the simulated volume and contribute 0)."""
        if not self._cached:
            raise RuntimeError("There is no cached observation to observe")
        arrays = []
        for name, a in (("times", times), ("az", az), ("el", el), ("tod", tod)):
            if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.ndim != 1 or not a.flags["C_CONTIGUOUS"]:
                raise RuntimeError(f"AtmSim.observe: {name} must be a contiguous 1-D float64 array")
            arrays.append(a)
        n = times.size
        if az.size != n or el.size != n or tod.size != n:
            raise RuntimeError("time domain buffer sizes are not consistent.")
        if n == 0:
            return 0
        if use_accel is None:
            use_accel = accel_enabled()
        if not use_accel:
            return self._observe_host(times, az, el, tod, fixed_r)
        return self.observe_rows(times, az.reshape(1, n), el.reshape(1, n), tod.reshape(1, n), fixed_r)

    # ------------------------------------------------------------------ device path
    def geometry(self, fixed_r=-1):
        """The parameter block of the kernels (capi.AtmGeometry)."""
        return capi.AtmGeometry(
            self._T0, self._azmin, self._azmax, self._elmin, self._elmax, self._tmin, self._tmax, self._rmin, self._rmax,
            float(fixed_r), self._zatm, self._zmax, self._wx, self._wy, self._wz, self._xstep, self._ystep, self._zstep,
            self._xstart, self._delta_x, self._ystart, self._delta_y, self._zstart, self._delta_z, self._maxdist,
            self._nn, self._nx, self._ny, self._nz, self._xstride, self._ystride, self._zstride, self._nelem)

    def device_volume(self):
        """(index pointer, index is int32, realization pointer): the volume on the device, uploaded at the first
        call and resident until ``close()``."""
        if not self._cached:
            raise RuntimeError("There is no cached observation to observe")
        if self._dev_index is None:
            index32 = INDEX32 and self._nelem < 2**31
            idx = self._compressed_index
            if index32:
                # cells outside [0, nelem) stay outside it: every such entry becomes -1
                idx = np.where((idx >= 0) & (idx < self._nelem), idx, -1).astype(np.int32)
            self._index32 = index32
            self._dev_index = DeviceMirror(idx, "atm_compressed_index").upload()
            self._dev_realization = DeviceMirror(self._realization, "atm_realization").upload()
        return self._dev_index.ptr, self._index32, self._dev_realization.ptr

    def observe_rows(self, times, az, el, tod, fixed_r=-1):
        """``observe`` for ``n_row`` rows of az / el / tod [n_row][n_samp] in ONE launch; ``times`` is one row for all
        or [n_row][n_samp].  Arrays that are registered on the device are used there (a registered ``tod`` is not
        downloaded), the others are mirrored for the call."""
        n_row, n = tod.shape
        if az.shape != tod.shape or el.shape != tod.shape or times.shape not in ((n,), tod.shape):
            raise RuntimeError("time domain buffer sizes are not consistent.")
        d_index, index32, d_real = self.device_volume()
        with device_scratch("atm_observe", owner=self) as s:
            ptr = {}
            for key, arr, role in (("times", times, s.inp), ("az", az, s.inp), ("el", el, s.inp), ("tod", tod, s.inout)):
                if accel_data_present(arr):
                    ptr[key] = accel_device_ptr(arr)
                else:
                    role(key, arr)
                    ptr[key] = s.ptr(key)
            status = capi.dev.atm_observe(self.geometry(fixed_r), d_index, index32, d_real, n_row, n, ptr["times"],
                                          n if times.ndim == 2 else 0, ptr["az"], ptr["el"], n, ptr["tod"], n,
                                          cell_cache=CELL_CACHE)
        return status

    def observe_quats(self, n_samp, stride, d_times, quat_row, d_quats, n_quat_rows, d_good, d_atm):
        """The operator's form: device pointers, az / el from detector quaternions, good samples only, into scratch
        rows (toast_hip_atm_observe_quats_dev).  Returns the status of every row."""
        d_index, index32, d_real = self.device_volume()
        return capi.dev.atm_observe_quats(self.geometry(-1.0), d_index, index32, d_real, n_samp, stride, d_times, quat_row,
                                          d_quats, n_quat_rows, d_good, d_atm, cell_cache=CELL_CACHE)

    # ------------------------------------------------------------------ host path
    def _observe_host(self, times, az, el, tod, fixed_r=-1):
        """toast::atm_sim_observe in NumPy: vectorised over the samples, one pass per ray step.  Operand order and
        association are the reference's; a failed check (any of toast_atm_observe.cpp:397, :78, :98, :127, :165) zeroes
        the sample's sum and ends its ray."""
        azm = az - TWOPI
        skip = (~((self._azmin <= az) & (az <= self._azmax)) & ~((self._azmin <= azm) & (azm <= self._azmax))) | ~(
            (self._elmin <= el) & (el <= self._elmax))
        act = np.nonzero(~skip)[0]
        zatm_inv = 1.0 / self._zatm
        xsi, ysi, zsi = 1.0 / self._xstep, 1.0 / self._ystep, 1.0 / self._zstep
        xend, yend, zend = self._xstart + self._delta_x, self._ystart + self._delta_y, self._zstart + self._delta_z
        t_now = times[act] - self._tmin
        az_now = az[act] - self._az0
        xtel, ytel, ztel = self._wx * t_now, self._wy * t_now, self._wz * t_now
        sin_el, cos_el = np.sin(el[act]), np.cos(el[act])
        sin_az, cos_az = np.sin(az_now), np.cos(az_now)
        r, n_step = ray_steps(self._xstep, self._rmin, self._rmax, fixed_r, self._elmax, self._zmax)
        val = np.zeros(act.size)
        alive = np.ones(act.size, dtype=bool)
        failed = np.zeros(act.size, dtype=bool)
        ci, re = self._compressed_index, self._realization
        xs, ys, zs = self._xstride, self._ystride, self._zstride
        for _ in range(n_step):
            k = np.nonzero(alive)[0]
            if k.size == 0:
                break
            zz = r * sin_el[k]
            rproj = r * cos_el[k]
            xx = rproj * cos_az[k]
            yy = rproj * sin_az[k]
            x = xx * self._cosel0 + zz * self._sinel0
            y = yy
            z = -xx * self._sinel0 + zz * self._cosel0
            x = x + xtel[k]
            y = y + ytel[k]
            z = z + ztel[k]
            bad = (x < self._xstart) | (x > xend) | (y < self._ystart) | (y > yend) | (z < self._zstart) | (z > zend)
            bad |= ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))
            # the cell of a point that failed already is never used: park it in cell 0
            qx = np.where(bad, self._xstart, x)
            qy = np.where(bad, self._ystart, y)
            qz = np.where(bad, self._zstart, z)
            ix = ((qx - self._xstart) * xsi).astype(np.int64)
            iy = ((qy - self._ystart) * ysi).astype(np.int64)
            iz = ((qz - self._zstart) * zsi).astype(np.int64)
            dx = (qx - (self._xstart + ix.astype(np.float64) * self._xstep)) * xsi
            dy = (qy - (self._ystart + iy.astype(np.float64) * self._ystep)) * ysi
            dz = (qz - (self._zstart + iz.astype(np.float64) * self._zstep)) * zsi
            bad |= (dx < 0) | (dx > 1) | (dy < 0) | (dy > 1) | (dz < 0) | (dz > 1)
            bad |= (ix < 0) | (ix > self._nx - 2) | (iy < 0) | (iy > self._ny - 2) | (iz < 0) | (iz > self._nz - 2)
            offset = np.where(bad, 0, ix * xs + iy * ys + iz * zs)
            full = [offset, offset + zs, offset + ys, offset + ys + zs, offset + xs, offset + xs + zs,
                    offset + xs + ys, offset + xs + ys + zs]        # 000 001 010 011 100 101 110 111
            for f in full:
                bad |= (f < 0) | (f > self._nn - 1)
            comp = [ci[np.where(bad, 0, f)] for f in full]
            for c in comp:
                bad |= (c < 0) | (c > self._nelem - 1)
            c000, c001, c010, c011, c100, c101, c110, c111 = (re[np.where(bad, 0, c)] for c in comp)
            c00 = c000 + (c100 - c000) * dx
            c01 = c001 + (c101 - c001) * dx
            c10 = c010 + (c110 - c010) * dx
            c11 = c011 + (c111 - c011) * dx
            c0 = c00 + (c10 - c00) * dy
            c1 = c01 + (c11 - c01) * dy
            c = c0 + (c1 - c0) * dz
            good = ~bad
            val[k[good]] += (c * (1.0 - z * zatm_inv))[good]
            val[k[bad]] = 0.0
            failed[k[bad]] = True
            alive[k[bad]] = False
            r += self._xstep
        tod[act] += val * self._xstep * self._T0
        return 1 if (skip.any() or failed.any()) else 0


def atm_sim_observe(*args):
    """``toast._libtoast.atm_sim_observe`` (src/toast/_libtoast/atm.cpp:208-334), the argument list of atm.py:464-503."""
    from .accel import native

    return native().atm_sim_observe(*args)


def azel_to_quat(az, el):
    """Quaternions (x, y, z, w) whose z axis looks at azimuth ``az`` and elevation ``el``: theta = pi / 2 - el,
    phi = 2 pi - az, as ObserveAtmosphere reads them back."""
    az, el = np.broadcast_arrays(np.asarray(az, dtype=np.float64), np.asarray(el, dtype=np.float64))
    theta, phi = np.pi / 2 - el, TWOPI - az
    sy, cy = np.sin(theta / 2), np.cos(theta / 2)
    sz, cz = np.sin(phi / 2), np.cos(phi / 2)
    return np.stack([-sz * sy, cz * sy, sz * cy, cz * cy], axis=-1)      # qz(phi) * qy(theta)


def standin_slab(azmin, azmax, elmin, elmax, tmin, tmax, rmin=0.0, rmax=2000.0, step=20.0, wind=(0.15, 0.1, 0.0),
                 T0=280.0, zatm=40000.0, zmax=2000.0, rms=1.0e-4, correlation=8.0, seed=0):
    """A STAND-IN for the reference's generator (not GenerateAtmosphere: no Kolmogorov statistics, no CHOLMOD): an
    AtmSim whose box encloses the scan cone [azmin, azmax] x [elmin, elmax] out to ``rmax`` for winds acting over
    [tmin, tmax], whose kept cells are those near the cone, and whose realization is a smooth random field -- white
    noise low-passed in Fourier space to a correlation length of ``correlation`` cells, scaled to ``rms``."""
    az0, el0 = azmin + (azmax - azmin) / 2, elmin + (elmax - elmin) / 2
    sinel0, cosel0 = np.sin(el0), np.cos(el0)
    _, n_step = ray_steps(step, rmin, rmax, -1.0, elmax, zmax)
    reach = max(rmax, 1.5 * step) + step if n_step else 2.5 * step

    def scan_frame(az, el, r):
        zz, rproj = r * np.sin(el), r * np.cos(el)
        xx, yy = rproj * np.cos(az - az0), rproj * np.sin(az - az0)
        return xx * cosel0 + zz * sinel0, yy, -xx * sinel0 + zz * cosel0

    # the box: the cone's surface sampled densely, moved by the wind over the whole time range, plus two cells
    a, e, r = np.meshgrid(np.linspace(azmin, azmax, 65), np.linspace(elmin, elmax, 33), np.linspace(0.0, reach, 33),
                          indexing="ij")
    pts = np.stack(scan_frame(a, e, r), axis=0).reshape(3, -1)
    drift = np.array(wind, dtype=np.float64) * (tmax - tmin)
    lo = np.minimum(pts.min(axis=1), pts.min(axis=1) + drift) - 2 * step
    hi = np.maximum(pts.max(axis=1), pts.max(axis=1) + drift) + 2 * step
    nx, ny, nz = (int(np.ceil((hi[k] - lo[k]) / step)) + 1 for k in range(3))
    # kept cells: within the cone (widened by two cells and by the drift) at some time of the range
    x = lo[0] + np.arange(nx)[:, None, None] * step
    y = lo[1] + np.arange(ny)[None, :, None] * step
    z = lo[2] + np.arange(nz)[None, None, :] * step
    keep = np.zeros((nx, ny, nz), dtype=bool)
    for frac in np.linspace(0.0, 1.0, 5):
        px, py, pz = x - frac * drift[0], y - frac * drift[1], z - frac * drift[2]
        xx, zz = px * cosel0 - pz * sinel0, px * sinel0 + pz * cosel0
        rr = np.sqrt(xx * xx + py * py + zz * zz)
        slack = 3 * step / np.maximum(rr, step)
        daz = np.arctan2(py, xx)
        el = np.arcsin(np.clip(zz / np.maximum(rr, 1e-9), -1, 1))
        keep |= ((rr <= reach + 2 * step) & (np.abs(daz) <= (azmax - azmin) / 2 + slack)
                 & (el >= elmin - slack) & (el <= elmax + slack))
    rng = np.random.default_rng(seed)
    white = rng.standard_normal((nx, ny, nz))
    kx = np.fft.fftfreq(nx)[:, None, None]
    ky = np.fft.fftfreq(ny)[None, :, None]
    kz = np.fft.rfftfreq(nz)[None, None, :]
    sigma = 1.0 / (2 * np.pi * correlation)
    field = np.fft.irfftn(np.fft.rfftn(white) * np.exp(-0.5 * (kx**2 + ky**2 + kz**2) / sigma**2), s=(nx, ny, nz),
                          axes=(0, 1, 2))
    field *= rms / field.std()
    keep = keep.reshape(-1)
    full_index = np.nonzero(keep)[0].astype(np.int64)
    compressed = np.full(nx * ny * nz, -1, dtype=np.int64)
    compressed[full_index] = np.arange(full_index.size)
    return AtmSim(azmin, azmax, elmin, elmax, tmin, tmax, T0=T0, zatm=zatm, zmax=zmax, xstep=step, ystep=step, zstep=step,
                  rmin=rmin, rmax=rmax, wx=wind[0], wy=wind[1], wz=wind[2], xstart=lo[0], delta_x=(nx - 1) * step,
                  ystart=lo[1], delta_y=(ny - 1) * step, zstart=lo[2], delta_z=(nz - 1) * step, maxdist=reach, nx=nx,
                  ny=ny, nz=nz, compressed_index=compressed, full_index=full_index,
                  realization=field.reshape(-1)[full_index].copy())
