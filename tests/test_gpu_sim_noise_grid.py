"""GPU: the six kernels of csrc/sim_noise.hip at every table path, transform length and mix edge, against the long
double restatements of tests/sim_noise_case.py and the reference's own amplitudes (tests/golden/sim_noise_grid.npz,
tests/golden/make_golden_sim_noise_grid.py).  test_sim_noise_grid_host.py holds the host entries to the same bounds
without a GPU.

* Interpolated amplitudes (k_sim_psd_interp): tables of 2, 3, 72, 767, 768, 769 and 2000 points -- in LDS up to 768,
  in global memory above, where the second stream's tables lie behind the first's -- at transform lengths 4 to 2^15,
  and PSD frequencies that sit on transform bins.  <= SCALE_BOUND[case] = 4 x max(scale_ref_err, scale_err[case]).
* Timestreams (k_sim_spectrum, rocFFT, k_crop_partial, k_crop_dc, k_sim_mix): the same grid at two start samples into
  rows longer than the stream.  <= TS_BOUND[case] = 10 x max(ts_ref_err, ts_err[case]) of the full transform's rms.
  scale_err and ts_err are the reference's own distances to the restatement, stored per case in the fixture.
* 258 crop chunks: the second trip of k_crop_dc's stride loop.
* Mixing: bit for bit the sums in stream order, then entry order, at every batch size.
* Random streams (k_rng_multi): the second trip of its grid-stride loop, a second launch of more than 65535 streams,
  empty streams; exact but for the Gaussians (4 x gauss_ref_err, as test_gpu_sim_noise.py).
* SimNoise on a subset of the detectors of resident data.

Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import sim_noise_case as sc  # noqa: E402
from sim_noise_case import GOLD  # noqa: E402
from test_gpu_sim_noise import Dev  # noqa: E402
from test_sim_noise_grid_host import check_scale  # noqa: E402

pytestmark = pytest.mark.gpu

RATE = sc.GRID_RATE


def device_interp(samples, oversample, freq, psds):
    from toast_amd import capi

    n_psd = sc.fft_length(samples, oversample) // 2 + 1
    buf = Dev(np.full((psds.shape[0], n_psd), np.nan))
    capi.dev.sim_noise_psd_interp(RATE, samples, oversample, freq, psds, buf.ptr)
    capi.synchronize()
    got = buf.get()
    buf.free()
    return got


def device_sim(ids, first, samples, oversample, det, freq, psds, start, **kw):
    """toast_hip_sim_noise_dev into a device copy of ``start`` [n_rows][row_stride]."""
    from toast_amd import capi

    rz, tel, comp, obs = ids
    buf = Dev(start)
    capi.dev.sim_noise(rz, tel, comp, obs, RATE, first, samples, oversample, det, freq, psds, buf.ptr, start.shape[0],
                       row_stride=start.shape[1], **kw)
    capi.synchronize()
    out = buf.get()
    buf.free()
    return out


def test_interpolation_grid():
    worst = [0.0, None]
    for n_binned, samples, oversample in sc.grid_cases():
        freq, psds = sc.grid_psds(n_binned)
        got = device_interp(samples, oversample, freq, psds)            # all PSDs of the case in one call
        check_scale(got, sc.case_key(n_binned, samples, oversample),
                    sc.grid_scale_longdouble(n_binned, samples, oversample), worst)
    samples, oversample = sc.TIE_LENGTH
    freq, psds, _ = sc.tie_grid()
    got = device_interp(samples, oversample, freq, psds)
    ld = np.array([sc.interp_longdouble(RATE, samples, oversample, freq, p) for p in psds])
    check_scale(got, "tie", ld, worst)
    print(f"closest to its bound: case {worst[1]} at {worst[0]:.3f} of it")


def test_timestream_grid():
    worst = [0.0, None]
    det = np.array(sc.GRID_DET, dtype=np.uint64)
    for n_binned, samples, oversample in sc.grid_cases():
        key = sc.case_key(n_binned, samples, oversample)
        freq, psds = sc.grid_psds(n_binned)
        rows = list(sc.grid_stream_rows(n_binned))
        bound = sc.ts_bound(key)
        # below the noise, so that the rounding of the sum stays that of the noise
        pattern = 1e-3 * np.linspace(-1.0, 1.0, 3 * (samples + 5)).reshape(3, samples + 5)
        for first in sc.GRID_FIRST:
            got = device_sim(sc.GRID_IDS, first, samples, oversample, det, freq, np.ascontiguousarray(psds[rows]), pattern)
            want, rms = sc.grid_streams_longdouble(n_binned, samples, oversample, first)
            dist = sc.ts_distance(got[:2, :samples], want + pattern[:2, :samples].astype(np.longdouble), rms)
            print(f"timestream {key:>12s} firstsamp {first:14d}: {dist:.3e} of the full rms, bound {bound:.3e}")
            assert dist <= bound, (key, first)
            if samples == 1:
                assert np.array_equal(got[:2, 0], pattern[:2, 0]), (key, first)
            assert np.array_equal(got[:, samples:], pattern[:, samples:]), (key, first)       # the five tail columns
            assert np.array_equal(got[2], pattern[2]), (key, first)                           # the row of no stream
            if dist / bound > worst[0]:
                worst[:] = [dist / bound, key]
    print(f"closest to its bound: case {worst[1]} at {worst[0]:.3f} of it")


def test_chunk_edges_and_the_long_case():
    """258 chunk sums per stream: k_crop_dc's stride loop of 256 takes its second trip.  Without it the level would
    miss the last 4097 samples, a constant offset of some 1e-5 of the rms."""
    samples, oversample = sc.LONG_LENGTH
    rz, tel, comp, obs, det, first = sc.LONG_IDS
    freq, psd = GOLD["psd_freq"], np.ascontiguousarray(GOLD["psd_psds"][sc.LONG_PSD_ROW:sc.LONG_PSD_ROW + 1])
    assert sc.fft_length(samples, oversample) == 1 << 22 and -(-samples // 4096) == 258
    want, rms = sc.long_stream_longdouble()
    bound = sc.ts_bound("long")
    zeros = np.zeros((1, samples))
    got = device_sim((rz, tel, comp, obs), first, samples, oversample, [det], freq, psd, zeros)
    dist = sc.ts_distance(got, want, rms)
    print(f"long case ({samples} samples, 258 chunks): {dist:.3e} of the full rms, bound {bound:.3e}")
    assert dist <= bound
    one = device_sim((rz, tel, comp, obs), first, samples, oversample, [det], freq, psd, zeros, max_batch=1)
    two = device_sim((rz, tel, comp, obs), first, samples, oversample, [det], freq, psd, zeros, max_batch=1)
    dist = sc.ts_distance(one, want, rms)
    print(f"long case, max_batch 1: {dist:.3e} of the full rms, bound {bound:.3e}")
    assert dist <= bound
    assert np.array_equal(one, two) and np.array_equal(one, got)


def test_mixing_order_bit_for_bit():
    """Five streams into six rows: rows 0 and 1 are shared by streams of different batches (at max_batch 1 and 2) and
    of one batch (at 3, 5 and the default), stream 1 has no entry, stream 2 names row 1 twice, weights 0 and < 0,
    row 5 belongs to nobody.  The sums are defined in stream order, then entry order."""
    samples, n_stream, n_rows = 3000, 5, 6
    ids, first = (1, 2, 3, 4), 250
    freq = GOLD["psd_freq"]
    psds = np.ascontiguousarray(GOLD["psd_psds"][[0, 1, 2, 3, 1]])
    det = np.array([10, 11, 12, 4294967295, 14], dtype=np.uint64)
    alone = [device_sim(ids, first, samples, 2, det[s:s + 1], freq, psds[s:s + 1], np.zeros((1, samples)))[0]
             for s in range(n_stream)]
    assert all(np.std(x) > 0 for x in alone)
    entries = [[(0, 1.0), (1, 0.5)], [], [(1, 0.25), (1, -2.0), (2, 0.0)], [(3, 0.0), (0, 3.0)], [(3, -1.5), (4, 1.25)]]
    ptr, rows, weights = [0], [], []
    for ent in entries:
        rows += [r for r, _ in ent]
        weights += [w for _, w in ent]
        ptr.append(len(rows))
    before = 1e-3 * np.linspace(-1.0, 1.0, n_rows * (samples + 3)).reshape(n_rows, samples + 3)
    want = before.copy()
    for s, ent in enumerate(entries):
        for r, w in ent:
            want[r, :samples] += w * alone[s]
    for max_batch in (0, 1, 2, 3, 5):
        got = device_sim(ids, first, samples, 2, det, freq, psds, before, mix_ptr=ptr, mix_row=rows, mix_weight=weights,
                         max_batch=max_batch)
        differ = int(np.count_nonzero(got != want))
        print(f"mixing, max_batch {max_batch}: {differ} of {got.size} elements differ from the sums in stream order")
        assert np.array_equal(got, want), max_batch
        assert np.array_equal(got[:, samples:], before[:, samples:]) and np.array_equal(got[5], before[5])
    assert not np.array_equal(want[1], before[1]) and np.array_equal(want[2], before[2])     # the zero weight


def test_random_streams_at_the_launch_edges():
    from toast_amd import capi, rng

    # the grid of k_rng_multi is capped at 16384 blocks of 256: the last 300 elements of the long stream are its second trip
    lengths = [0, 1, 255, 256, 257, 0, 4194304 + 300]
    keys = [(11, 12)] * len(lengths)
    counters = [(0, 1000003 * i + 5) for i in range(len(lengths))]
    gap = 3
    offsets, pos = [0] * len(lengths), gap
    for i in reversed(range(len(lengths))):              # the last stream first in the buffer
        offsets[i] = pos
        pos += lengths[i] + gap
    owned = np.zeros(pos, dtype=bool)
    for off, n in zip(offsets, lengths):
        owned[off:off + n] = True
    gbound = 4.0 * float(GOLD["gauss_ref_err"])
    for sampler, kind in sc.SAMPLERS.items():
        sentinel = np.uint64(0x5EA1ED5EA1ED5EA1) if kind == "uint64" else -7.5
        buf = Dev(np.full(pos, sentinel))
        rng.random_multi_device(lengths, keys, counters, buf.ptr, pos, sampler=sampler, offsets=offsets)
        capi.synchronize()
        got = buf.get()
        buf.free()
        host = rng.random_multi(lengths, keys, counters, sampler=sampler)
        assert np.all(got[~owned] == sentinel), sampler
        worst = 0.0
        for i, (off, n) in enumerate(zip(offsets, lengths)):
            g, want = got[off:off + n], host[i]
            if kind != "normal":
                assert g.dtype == want.dtype and np.array_equal(g, want), (sampler, i)
            elif n:
                pick = slice(None) if n <= 1000 else np.unique(np.concatenate([np.arange(0, n, 4099), np.arange(n - 1000, n)]))
                worst = max(worst, float(np.max(np.abs(g[pick] - want[pick]) / np.abs(want[pick]))))
        if kind == "normal":
            print(f"gaussian: max relative distance {worst:.3e}, bound {gbound:.3e}")
            assert worst <= gbound
        else:
            print(f"{sampler}: {sum(lengths)} elements equal the host entries'; {int(np.count_nonzero(~owned))} keep the sentinel")
    # more than 65535 streams: a second launch that starts at stream 65535
    n_stream = 65537
    keys = [(7, 1000 + 3 * s) for s in range(n_stream)]
    counters = [(1, 2 * s) for s in range(n_stream)]
    offsets = [3 * s + 1 for s in range(n_stream)]
    sentinel = np.uint64(0x5EA1ED5EA1ED5EA1)
    buf = Dev(np.full(3 * n_stream + 1, sentinel))
    rng.random_multi_device([2] * n_stream, keys, counters, buf.ptr, buf.a.size, sampler="uniform_uint64", offsets=offsets)
    capi.synchronize()
    got = buf.get()
    buf.free()
    host = np.array(rng.random_multi([2] * n_stream, keys, counters, sampler="uniform_uint64"))
    differ = int(np.count_nonzero(got[1:].reshape(n_stream, 3)[:, :2] != host))
    print(f"{n_stream} streams of 2: {differ} elements differ from the host entries'")
    assert differ == 0
    assert np.all(got[::3] == sentinel)


def test_operator_with_a_detector_subset():
    """The CSR of the device path is built from the selected detectors only: key k2 has weight in D01 alone and must
    not be simulated into anything; D01 and D03 keep their content bit for bit on both paths."""
    from toast_amd import ops
    from toast_amd.data import defaults

    mix = {"D00": {"k0": 1.0, "k1": 0.5}, "D01": {"k2": 2.0}, "D02": {"k0": 0.25, "k1": -1.0}, "D03": {"k0": 1.0}}
    start = 1e-3 * np.linspace(-1.0, 1.0, 4 * 3000).reshape(4, 3000)
    results = {}
    for where in ("host", "device"):
        data = sc.make_data(n_det=4, n_samp=3000, mixmatrix=mix)
        dd = data.obs[0].detdata[defaults.det_data]
        dd.data[:] = start
        if where == "device":
            dd.accel_create(defaults.det_data)
            dd.accel_update_device()
            dd.accel_used(True)
        ops.SimNoise(realization=1, component=2).apply(data, detectors=["D00", "D02"])
        assert dd.accel_in_use() == (where == "device")
        results[where] = dd.data.copy()
    bound = 10.0 * float(GOLD["ts_ref_err"])
    sel, unsel = [0, 2], [1, 3]
    noise = results["host"][sel] - start[sel]
    dist = float(np.max(np.max(np.abs(results["device"][sel] - results["host"][sel]), axis=1)
                        / np.sqrt(np.mean(noise**2, axis=1))))
    print(f"operator, detectors D00 and D02 of four: device against the host path {dist:.3e} of the noise rms, "
          f"bound {bound:.3e}")
    assert dist <= bound and np.std(noise) > 0
    for where in results:
        assert np.array_equal(results[where][unsel], start[unsel]), where
