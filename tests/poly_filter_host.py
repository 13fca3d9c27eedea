"""NumPy restatement of the compiled reference kernel `filter_polynomial`
(src/libtoast/src/toast_tod_filter.cpp:18-158) for ONE signal with its own flag vector: exclusive stop, intervals
clipped to [0, n), nothing done without a good sample, the order lowered to the number of good samples, the fit
subtracted from ALL samples.  The least-squares problem is solved by `numpy.linalg.lstsq` (SVD), like the
reference's DGELSS.  Also the reference's `sum_detectors` / `subtract_mean` (src/toast/_libtoast/tod_filter.cpp:9-97)."""
import numpy as np

FITTED, NO_GOOD, REDUCED, NOT_FINITE = 0, 1, 2, 3     # 3: a good sample is NaN or infinite, interval left untouched


def legendre(scanlen, norder):
    """Templates [norder][scanlen] by the reference's recurrence on x_i = (0.5 dx - 1) + i dx, dx = 2 / scanlen."""
    dx = 2.0 / scanlen
    x = (0.5 * dx - 1) + np.arange(scanlen) * dx
    t = np.empty((norder, scanlen))
    t[0] = 1.0
    if norder > 1:
        t[1] = x
    for k in range(2, norder):
        t[k] = ((2 * k - 1) * x * t[k - 1] - (k - 1) * t[k - 2]) * (1.0 / k)
    return t


def filter_polynomial(order, flags, signal, starts, stops):
    """In place on `signal`; `flags` non-zero = flagged.  Returns (coeff [n_interval][order + 1], status)."""
    n = flags.size
    coeff = np.zeros((len(starts), max(order + 1, 0)))
    status = np.zeros(len(starts), dtype=np.int32)
    if order < 0:
        return coeff, status
    for k, (start, stop) in enumerate(zip(starts, stops)):
        start, stop = max(int(start), 0), min(int(stop), n)
        scanlen = stop - start
        good = flags[start:stop] == 0 if scanlen > 0 else np.zeros(0, dtype=bool)
        ngood = int(np.count_nonzero(good))
        if ngood == 0:
            status[k] = NO_GOOD
            continue
        norder = min(ngood, order + 1)
        t = legendre(scanlen, norder)
        c = np.linalg.lstsq(t[:, good].T, signal[start:stop][good], rcond=None)[0]
        for r in range(norder):
            signal[start:stop] -= c[r] * t[r]
        coeff[k, :norder] = c
        status[k] = REDUCED if norder < order + 1 else FITTED
    return coeff, status


def combined_flags(shared_flags, shared_mask, det_flags, det_mask):
    out = np.zeros(shared_flags.size if shared_flags is not None else det_flags.size, dtype=np.uint8)
    if shared_flags is not None:
        out |= (shared_flags & shared_mask).astype(np.uint8)
    if det_flags is not None:
        out |= (det_flags & det_mask).astype(np.uint8)
    return out


def sum_detectors(det_index, flag_index, shared_flags, shared_mask, det_data, det_flags, det_mask, sum_data, hits):
    for d, f in zip(det_index, flag_index):
        good = ((shared_flags & shared_mask) == 0) & ((det_flags[f] & det_mask) == 0)
        sum_data[good] += det_data[d][good]
        hits[good] += 1


def subtract_mean(det_index, det_data, sum_data, hits):
    nz = hits != 0
    sum_data[nz] /= hits[nz]
    for d in det_index:
        det_data[d] -= sum_data


def hashed_uniform(seed, n):
    """`n` doubles in [0, 1) carrying 53 bits each: splitmix64 of (seed, index) in wrapping uint64 arithmetic, so the
    fixture generator and the tests rebuild bit-identical inputs on any NumPy."""
    x = np.arange(n, dtype=np.uint64) + (np.uint64(seed) << np.uint64(32))
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def poly_case_signals(seed, n_det, n_samp):
    """Offsets of 1e3-4e3 plus noise of unit variance, per detector."""
    u = hashed_uniform(seed, n_det * n_samp).reshape(n_det, n_samp)
    offsets = 1.0e3 + 3.0e3 * hashed_uniform(seed + 1000, n_det)
    return offsets[:, None] + (u - 0.5) * np.sqrt(12.0)


def common_mode_signals(seed, n_rows, n_samp):
    return (hashed_uniform(seed, n_rows * n_samp).reshape(n_rows, n_samp) - 0.5) * 20.0


# The operator-level case of the conditioning tests (tests/test_gpu_poly_filter_edges.py and the fixture generator
# tests/golden/make_golden_poly_filter_edges.py build the same inputs from here).
EDGE_OPERATOR_SIM = dict(n_det=3, n_samp=6000, rate=20.0, n_obs=1, flag_samples=False, seed=0)
EDGE_OPERATOR_ORDER = 5
EDGE_OPERATOR_DET = 1
EDGE_OPERATOR_MASKS = (1, 1)        # shared_flag_mask (the sim's invalid bit), det_flag_mask


def edge_operator_inputs(starts, stops, n_samp):
    """(signal [3][n_samp], detector flags [3][n_samp]): detector EDGE_OPERATOR_DET keeps only the first 10 % of every
    [start, stop) good, the others lose 10 % of their samples at random."""
    signal = poly_case_signals(900, 3, n_samp)
    det_flags = (hashed_uniform(901, 3 * n_samp).reshape(3, n_samp) < 0.1).astype(np.uint8)
    det_flags[EDGE_OPERATOR_DET] = 0
    for a, b in zip(starts, stops):
        det_flags[EDGE_OPERATOR_DET, a + int(0.1 * (b - a)):b] = 1
    return signal, det_flags
