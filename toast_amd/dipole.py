"""CMB dipole timestreams (reference: src/toast/dipole.py:15-97; the solar velocity of
src/toast/ops/sim_tod_dipole.py:135-153).

The traits of this package carry no ``Quantity``: every value here is a plain float, temperatures in K, speeds in km/s,
angles in degrees, frequencies in Hz.

``dipole`` is the host path and the statement of what the device kernel (csrc/sim_dipole.hip) computes; ``dipole_map``
is not provided (it needs a pixel -> angle call this library does not have, and the reference's own function fails for
any ``coord`` but "G").

A zero speed -- orbital mode with a zero velocity row -- divides by zero and gives NaN, as in the reference.
"""

import numpy as np

# A&A 643, A42 (2020) Table 11; amplitude 3366.6 uK converted to a speed (dipole.py:15-22)
#: CMB monopole [K]
t_cmb = 2.72548
#: speed of the solar system barycentre with respect to the CMB [km/s]
solar_speed = 370.08
#: galactic latitude of the direction of that motion [degrees]
solar_gal_lat = 48.25
#: galactic longitude of the direction of that motion [degrees]
solar_gal_lon = 263.99

# scipy.constants.speed_of_light, .h, .k: exact in the SI of 2019 (CODATA 2018)
SPEED_OF_LIGHT = 299792458.0
PLANCK_H = 6.62607015e-34
BOLTZMANN_K = 1.380649e-23

# The galactic system at J2000 (IAU 1958, as transformed to J2000 by the Hipparcos catalogue, ESA SP-1200 vol. 1 sect.
# 1.5.3): right ascension and declination of the north galactic pole and the position angle of the galactic centre
# at that pole, degrees; the obliquity of the ecliptic at J2000 (IAU 1976).
GAL_POLE_RA, GAL_POLE_DEC, GAL_CENTRE_PA = 192.85948, 27.12825, 122.93192
OBLIQUITY_J2000 = 23.4392911


def array_dot(u, v):
    """Dot product of each row of two 2D arrays, [n, 1] (src/toast/utils.py:743-745)."""
    return np.sum(u * v, axis=1).reshape((-1, 1))


def rotate_zaxis(quats):
    """qa.rotate(quats, [0, 0, 1]) for an array [n, 4] (src/libtoast/src/toast_math_qarray.cpp:200-256: the norm summed
    component by component, every component divided by it, the products, ``2 * (...) + v``; the terms that multiply the
    zeros of the z axis only contribute signed zeros)."""
    q = np.asarray(quats, dtype=np.float64).reshape((-1, 4))
    norm = 0.0
    for k in range(4):
        norm = norm + q[:, k] * q[:, k]
    u = q / np.sqrt(norm)[:, None]
    xw, yw = u[:, 3] * u[:, 0], u[:, 3] * u[:, 1]
    x2, xz, y2, yz = -u[:, 0] * u[:, 0], u[:, 0] * u[:, 2], -u[:, 1] * u[:, 1], u[:, 1] * u[:, 2]
    return np.stack([2 * (yw + xz) + 0.0, 2 * (yz - xw) + 0.0, 2 * (x2 + y2) + 1.0], axis=1)


def dipole(det_pointing, vel=None, solar=None, cmb=t_cmb, freq=0.0):
    """The dipole timestream [K] of detector pointing ``det_pointing`` [n, 4] (dipole.py:26-97, same operation order).

    ``vel``: telescope velocity relative to the solar system barycentre [n, 3], km/s; ``solar``: velocity of the
    barycentre relative to the CMB rest frame [3], km/s -- in the coordinate system of the pointing.  With both, the
    velocities add relativistically; at least one is required.  ``cmb`` in K; ``freq`` in Hz, non-zero selects the
    quadrupole-corrected form."""
    if vel is None and solar is None:
        raise RuntimeError("dipole: a telescope velocity, a solar velocity or both are required")
    det_pointing = np.asarray(det_pointing, dtype=np.float64).reshape((-1, 4))
    nsamp = det_pointing.shape[0]
    inv_light = 1.0e3 / SPEED_OF_LIGHT
    if vel is not None:
        vel = np.asarray(vel, dtype=np.float64)
    if solar is not None:
        solar = np.asarray(solar, dtype=np.float64)

    if (vel is not None) and (solar is not None):
        # relativistic addition of velocities
        speed_solar = np.sqrt(np.sum(solar * solar, axis=0))
        vpar = (array_dot(vel, solar) / speed_solar**2) * solar
        vperp = vel - vpar
        vdot = 1.0 / (1.0 + array_dot(solar, vel) * inv_light**2)
        invgamma = np.sqrt(1.0 - (speed_solar * inv_light) ** 2)
        vpar += solar
        vperp *= invgamma
        v = vdot * (vpar + vperp)
    elif solar is not None:
        v = np.tile(solar, nsamp).reshape((-1, 3))
    else:
        v = vel.copy()

    speed = np.sqrt(array_dot(v, v))
    v /= speed
    beta = inv_light * speed.flatten()
    direct = rotate_zaxis(det_pointing)

    cmb_kelvin = float(cmb)
    freq_hz = float(freq)
    if freq_hz == 0:
        inv_gamma = np.sqrt(1.0 - beta**2)
        num = 1.0 - beta * np.sum(v * direct, axis=1)
        return cmb_kelvin * (inv_gamma / num - 1.0)
    # the frequency enters through the quadrupole correction
    fcor = quadrupole_correction(cmb_kelvin, freq_hz)
    bt = beta * np.sum(v * direct, axis=1)
    return cmb_kelvin * (bt + fcor * bt**2)


def quadrupole_correction(cmb_kelvin, freq_hz):
    """``fcor`` of dipole.py:92-93."""
    fx = PLANCK_H * freq_hz / (BOLTZMANN_K * cmb_kelvin)
    return (fx / 2) * (np.exp(fx) + 1) / (np.exp(fx) - 1)


def _rot_x(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]])


def _rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def galactic_to_equatorial():
    """The matrix that takes galactic Cartesian components to equatorial (J2000) ones, from the IAU definition of the
    galactic system: C -> G is Rz(90 deg - PA) Rx(90 deg - Dec_pole) Rz(RA_pole + 90 deg) as passive rotations; this is
    its transpose."""
    c2g = (_rot_z(np.radians(90.0 - GAL_CENTRE_PA)) @ _rot_x(np.radians(90.0 - GAL_POLE_DEC))
           @ _rot_z(np.radians(GAL_POLE_RA + 90.0)))
    return c2g.T


def equatorial_to_ecliptic():
    """Equatorial (J2000) to ecliptic components: a rotation about the x axis by the J2000 obliquity."""
    return _rot_x(np.radians(OBLIQUITY_J2000))


def solar_velocity(coord="E", speed=solar_speed, gal_lat=solar_gal_lat, gal_lon=solar_gal_lon):
    """Velocity of the solar system barycentre with respect to the CMB [km/s] in ``coord`` -- "G" galactic, "C"
    equatorial, "E" ecliptic (sim_tod_dipole.py:135-153).

    The reference rotates with the matrices of ``healpy.rotator.Rotator(coord=["G", coord])``, which hold nine-digit
    constants.  healpy is not a dependency of this package: G -> C is built from the IAU definition of the galactic
    system at J2000 (pole RA 192.85948, Dec 27.12825, position angle of the centre 122.93192 degrees), C -> E from the
    J2000 obliquity 23.4392911 degrees.  The agreement with healpy's matrices is NOT measured; the expected difference
    is of order 1e-8 of the speed, below 1e-10 K in the signal."""
    if coord not in ("E", "C", "G"):
        raise RuntimeError("coordinate system must be 'E', 'C', or 'G'")
    theta = np.deg2rad(90.0 - gal_lat)
    phi = np.deg2rad(gal_lon)
    projected = speed * np.sin(theta)
    sol_z = speed * np.cos(theta)
    sol_x = projected * np.cos(phi)
    sol_y = projected * np.sin(phi)
    gal = np.array([sol_x, sol_y, sol_z])
    if coord == "G":
        return gal
    rotmat = galactic_to_equatorial()
    if coord == "E":
        rotmat = equatorial_to_ecliptic() @ rotmat
    return np.ravel(np.dot(rotmat, gal))
