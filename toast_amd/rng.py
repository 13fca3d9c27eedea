"""Counter-based random streams with the surface of ``toast.rng`` (reference: src/toast/rng.py:22-164).

Streams are Threefry2x64-20 keyed by ``key``; element ``i`` is the generator's output at counter
``(counter[0], counter[1] + i)``.  ``random`` / ``random_multi`` return host arrays from the library's host entries
(``capi.rng_dist_*``, bit-identical to the reference); ``random_multi_device`` fills a device buffer with the HIP
kernel (csrc/sim_noise.hip) and is what the noise simulation is built on.
"""

import numpy as np

from . import capi

_SAMPLERS = {
    "gaussian": ("normal", np.float64),
    "uniform_01": ("uniform_01", np.float64),
    "uniform_m11": ("uniform_11", np.float64),
    "uniform_uint64": ("uint64", np.uint64),
}
_UNDEFINED = "Undefined sampler. Choose among: gaussian, uniform_01, uniform_m11, uniform_uint64"


def _sampler(sampler):
    if sampler not in _SAMPLERS:
        raise ValueError(_UNDEFINED)
    return _SAMPLERS[sampler]


def _uniform_split(total, n):
    """``distribute_uniform`` of the reference (src/toast/dist.py): n (offset, count) pairs, the first
    ``total % n`` one longer."""
    base, extra = divmod(int(total), int(n))
    out, off = [], 0
    for i in range(n):
        cnt = base + (1 if i < extra else 0)
        out.append((off, cnt))
        off += cnt
    return out


def random(samples, key=(0, 0), counter=(0, 0), sampler="gaussian", threads=False):
    """``samples`` values of one stream (rng.py:22-110).  ``threads=True`` generates the stream in pieces through the
    multi-stream entry, as the reference does; the values are the same either way."""
    kind, dtype = _sampler(sampler)
    samples = int(samples)
    n_piece = 4
    if (not threads) or samples < n_piece:
        ret = np.empty(samples, dtype=dtype)
        getattr(capi, "rng_dist_" + kind)(key[0], key[1], counter[0], counter[1], ret)
        return ret
    dst = _uniform_split(samples, n_piece)
    chunks = getattr(capi, "rng_multi_dist_" + kind)(
        np.array([key[0]] * n_piece, dtype=np.uint64), np.array([key[1]] * n_piece, dtype=np.uint64),
        np.array([counter[0]] * n_piece, dtype=np.uint64),
        np.array([(int(counter[1]) + x[0]) % (1 << 64) for x in dst], dtype=np.uint64), [x[1] for x in dst])
    return np.concatenate(chunks)


def random_multi(samples, keys, counters, sampler="gaussian"):
    """One array per stream: ``samples[s]`` values of the stream ``keys[s]``, ``counters[s]`` (rng.py:113-164)."""
    kind, _ = _sampler(sampler)
    k1 = np.array([x[0] for x in keys], dtype=np.uint64)
    k2 = np.array([x[1] for x in keys], dtype=np.uint64)
    c1 = np.array([x[0] for x in counters], dtype=np.uint64)
    c2 = np.array([x[1] for x in counters], dtype=np.uint64)
    return getattr(capi, "rng_multi_dist_" + kind)(k1, k2, c1, c2, list(samples))


def random_multi_device(samples, keys, counters, d_out, out_len, sampler="gaussian", offsets=None, stream=0):
    """The same streams written by the HIP kernel into the device buffer ``d_out`` (``out_len`` elements of float64, or
    uint64 for ``uniform_uint64``): stream s starts at element ``offsets[s]`` (None: one after the other)."""
    kind, _ = _sampler(sampler)
    capi.dev.rng_multi(kind, list(samples), [x[0] for x in keys], [x[1] for x in keys], [x[0] for x in counters],
                       [x[1] for x in counters], d_out, out_len, offsets=offsets, stream=stream)
