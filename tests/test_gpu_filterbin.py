"""GPU: the FilterBin kernels (csrc/filterbin.hip) through the C ABI, ops.FilterBin on device-resident data against the
reference's own run (tests/golden/filterbin.npz), and FilterBin + BinMap end to end.

C ABI, against float64 sums formed in extended precision (np.longdouble) on the host.

* Fourier templates: the argument is formed in double as the reference forms it, ``order * angle[i]``; cos / sin of that
  double are taken in extended precision and rounded.  The device's cos / sin are documented to 2 ulp, the rounded
  extended value is within 0.5 ulp of the truth, so the distance is at most 2.5 ulp, one more where the two sides fall
  into different binades: the test asserts <= 3 ulp of the reference value.  Largest distance observed on an MI355X:
  0.74 ulp (FOURIER_ULP_OBSERVED).
* Blocks: the polynomials P_j(x_i) are rebuilt in float64 with the kernel's own recurrence (filterbin_case.legendre_rows;
  a different last bit is covered by 2 units per term), each entry is a sum of products, and the bound follows the
  summation tree of the code, in units of eps * sum |terms|:
    p          a lane adds its <= 4 samples of a chunk (kFbChunk / kFbTile), 6 shuffle steps, then 4 atomics (one per wave)
               per chunk: depth 4 + 6 + 4 n_chunk, + 1 for the product and 2 for P               -> DEPTH_STREAM(n_chunk) + 3
    B, C       common part: the same tree as p; flagged part: one thread walks the queue of a sub-tile (<= 256 entries),
               adds the <= 4 sub-tile sums and issues one atomic per chunk: depth 256 + 4 + n_chunk; the difference
               common - flagged rounds once more relative to the common sum
  i.e. |B - exact| <= eps ((DEPTH_STREAM + 4) sum_common |t| + (DEPTH_QUEUE + 3) sum_flagged |t|), the same for C.
  The shapes straddle the sample tile (256), a full queue (a detector that flags a whole sub-tile), the chunk (1024)
  and the detector tile (8 detectors up to order 3, 4 above).

Operator: final flags (detector samples, shared, detector level) and routes equal the reference's exactly.  The
algorithm distance measured on the CPU (tests/test_filterbin_host.py, largest max |delta filtered| / rms(signal) over the
cases) is E_HOST = 1.2e-14 (case ``pinv``; 3.3e-15 for ``all``); the device result is held to 10 E_HOST -- the project's
order-of-magnitude allowance for another summation tree -- and, independently, to the parity bar of 1e-10.  Amplitudes
are compared where the reference inverted (they are not unique under the pseudo-inverse), to the same bound relative to
the largest amplitude.
"""
import numpy as np
import pytest

import filterbin_case as FC
import golden_util as gu
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.ops import filterbin as FB

pytestmark = pytest.mark.gpu

E_HOST = 1.2e-14
PARITY = 1e-10
FOURIER_ULP_OBSERVED = 0.74        # measured, not asserted: the test prints the figure of its own run
EPS = np.finfo(np.float64).eps
TILE, QUEUE = 256, 256


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture(scope="module")
def fixture():
    return gu.load("filterbin")


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_fourier_templates_ulp_distance():
    import torch

    from toast_amd import capi

    n = 3 * TILE + 17
    rng = np.random.default_rng(1)
    angle = np.concatenate([[0.0, np.pi, 2 * np.pi - 1e-9], rng.uniform(0, 2 * np.pi, n - 3)])
    start, stop = 1, 9
    out = torch.full((2 * (stop - start), n), float("nan"), dtype=torch.float64, device="cuda")
    d_angle = dev(angle)
    capi.dev.fourier_templates(d_angle.data_ptr(), n, start, stop, out.data_ptr())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for order in range(start, stop):
        arg = (np.float64(order) * angle).astype(np.longdouble)        # the double the kernel forms, then extended
        for row, want in ((2 * (order - start), np.cos(arg)), (2 * (order - start) + 1, np.sin(arg))):
            want64 = want.astype(np.float64)
            ulp = np.spacing(np.abs(want64))
            worst = max(worst, float(np.max(np.abs(got[row].astype(np.longdouble) - want) / ulp)))
    print(f"\nfourier templates: largest distance {worst:.2f} ulp")
    assert got[1, 0] == 0.0 and got[0, 0] == 1.0                        # sin(0), cos(0): the sine rows start late
    assert worst <= 3.0


def exact_blocks(dense, signal, good_shared, good_det, starts, stops, k):
    """Extended-precision sums and, per entry, sum |terms| of the common and of the flagged part."""
    ld = np.longdouble
    n_det, nd, n_iv = signal.shape[0], dense.shape[0], len(starts)
    out = dict(p=np.zeros((n_det, n_iv, k), dtype=ld), p_abs=np.zeros((n_det, n_iv, k), dtype=ld),
               B=np.zeros((n_det, n_iv, k, k), dtype=ld), B_abs_c=np.zeros((n_iv, k, k), dtype=ld),
               B_abs_f=np.zeros((n_det, n_iv, k, k), dtype=ld), C=np.zeros((n_det, n_iv, nd, k), dtype=ld),
               C_abs_c=np.zeros((n_iv, nd, k), dtype=ld), C_abs_f=np.zeros((n_det, n_iv, nd, k), dtype=ld),
               nnz=np.zeros((n_det, n_iv, k), dtype=np.int64))
    for v, (a, b) in enumerate(zip(starts, stops)):
        P = FC.interval_polynomials(a, b, k).astype(ld)
        T = dense[:, a:b].astype(ld)
        ws = good_shared[a:b].astype(ld)
        out["B_abs_c"][v] = (np.abs(P) * ws) @ np.abs(P).T
        out["C_abs_c"][v] = (np.abs(T) * ws) @ np.abs(P).T
        for d in range(n_det):
            w = (good_shared[a:b] & good_det[d, a:b]).astype(ld)
            wf = (good_shared[a:b] & ~good_det[d, a:b]).astype(ld)
            s = signal[d, a:b].astype(ld)
            out["p"][d, v] = P @ (w * s)
            out["p_abs"][d, v] = np.abs(P) @ (w * np.abs(s))
            out["nnz"][d, v] = np.count_nonzero((P != 0) & (w != 0)[None, :], axis=1)
            out["B"][d, v] = (P * w) @ P.T
            out["C"][d, v] = (T * w) @ P.T
            out["B_abs_f"][d, v] = (np.abs(P) * wf) @ np.abs(P).T
            out["C_abs_f"][d, v] = (np.abs(T) * wf) @ np.abs(P).T
    return out


@pytest.mark.parametrize("order,n_dense,n_det", [(0, 0, 3), (1, 3, 9), (1, 18, 17), (3, 16, 8), (4, 5, 5), (7, 17, 6)])
def test_interval_blocks_against_extended_precision_sums(order, n_dense, n_det):
    import torch

    from toast_amd import capi

    D = capi.dev
    k, kp = order + 1, (order + 1) * (order + 2) // 2
    chunk = D.filterbin_chunk()
    assert chunk == 4 * TILE and D.filterbin_det_tile(order) == (8 if k <= 4 else 4)
    rng = np.random.default_rng(100 + order)
    # intervals: shorter than a tile, one tile + 1, exactly a chunk, a chunk + 1, 2.5 chunks, a gap between each
    lengths = [max(k, 37), TILE + 1, chunk, chunk + 1, 2 * chunk + TILE // 2 + 3]
    starts, stops, cursor = [], [], 5
    for length in lengths:
        starts.append(cursor)
        stops.append(cursor + length)
        cursor += length + 11
    n = cursor + 29
    n_rows = n_det + 2
    sig_rows = rng.permutation(n_rows)[:n_det].astype(np.int32)
    flag_rows = rng.permutation(n_rows)[:n_det].astype(np.int32)
    signal = np.zeros((n_rows, n))
    signal[sig_rows] = 10.0 + rng.standard_normal((n_det, n))
    shared = (rng.random(n) < 0.05).astype(np.uint8) * 2
    dflags = np.zeros((n_rows, n), dtype=np.uint8)
    dflags[flag_rows] = (rng.random((n_det, n)) < 0.1).astype(np.uint8) * 4 + (rng.random((n_det, n)) < 0.2).astype(np.uint8)
    dflags[flag_rows[0], starts[4] + TILE:starts[4] + 2 * TILE + 9] = 4     # a full queue and the next sub-tile's head
    if n_det > 1:
        dflags[flag_rows[1], starts[1]:stops[1]] = 4                          # an interval without a good sample
    dense = rng.standard_normal((n_dense, n))
    if n_dense > 0:
        dense[0, :starts[3] + 100] = 0.0                                      # a row that is zero in some intervals
    d_dense, d_sig, d_fl, d_sh = dev(dense), dev(signal), dev(dflags), dev(shared)
    z = lambda *shape, dtype=torch.float64: torch.full(shape, -7, dtype=dtype, device="cuda")  # noqa: E731
    n_iv = len(starts)
    p, nnz = z(n_det, n_iv, k), z(n_det, n_iv, k, dtype=torch.int64)
    bc, cc = z(n_iv, kp), z(n_iv, max(n_dense, 1), k)
    bf, cf = z(n_det, n_iv, kp), z(n_det, n_iv, max(n_dense, 1), k)
    D.filterbin_accumulate(order, d_dense.data_ptr() if n_dense else 0, n_dense, n, sig_rows, d_sig.data_ptr(), flag_rows,
                           d_fl.data_ptr(), 4, d_sh.data_ptr(), 2, starts, stops, p.data_ptr(), nnz.data_ptr(),
                           bc.data_ptr(), cc.data_ptr(), bf.data_ptr(), cf.data_ptr())
    torch.cuda.synchronize()
    want = exact_blocks(dense, signal[sig_rows], (shared & 2) == 0, (dflags[flag_rows] & 4) == 0, starts, stops, k)
    assert np.array_equal(nnz.cpu().numpy(), want["nnz"])
    n_chunk = np.array([-(-(b - a) // chunk) for a, b in zip(starts, stops)])
    depth_stream = (chunk // TILE + 6 + 4 * n_chunk).astype(np.longdouble)
    depth_queue = (QUEUE + chunk // TILE + n_chunk).astype(np.longdouble)
    got_p = p.cpu().numpy().astype(np.longdouble)
    err = np.abs(got_p - want["p"])
    bound = EPS * (depth_stream[None, :, None] + 3) * want["p_abs"]
    print(f"\nfilterbin blocks order {order} Nd {n_dense}: p worst error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    got_b = FB.unpack_symmetric((bc[None] - bf).cpu().numpy(), k).astype(np.longdouble)
    err = np.abs(got_b - want["B"])
    bound = EPS * ((depth_stream[None, :, None, None] + 4) * want["B_abs_c"][None]
                   + (depth_queue[None, :, None, None] + 3) * want["B_abs_f"])
    print(f"filterbin blocks order {order} Nd {n_dense}: B worst error / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
    assert np.all(err <= bound)
    if n_dense > 0:
        got_c = (cc[None] - cf).cpu().numpy().astype(np.longdouble)
        err = np.abs(got_c - want["C"])
        bound = EPS * ((depth_stream[None, :, None, None] + 4) * want["C_abs_c"][None]
                       + (depth_queue[None, :, None, None] + 3) * want["C_abs_f"])
        print(f"filterbin blocks order {order} Nd {n_dense}: C worst error / bound "
              f"{float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound)
    # rows that were not named stay untouched, and the good counts / spans of the dense rows are exact
    assert np.array_equal(d_sig.cpu().numpy(), signal) and np.array_equal(d_fl.cpu().numpy(), dflags)
    n_good, nnz_d = z(n_det, dtype=torch.int64), z(n_det, max(n_dense, 1), dtype=torch.int64)
    D.filterbin_good_counts(d_dense.data_ptr() if n_dense else 0, n_dense, n, flag_rows, d_fl.data_ptr(), 4, d_sh.data_ptr(), 2,
                            n_det, n_good.data_ptr(), nnz_d.data_ptr())
    first, last = z(max(n_dense, 1), dtype=torch.int64), z(max(n_dense, 1), dtype=torch.int64)
    D.template_spans(d_dense.data_ptr() if n_dense else 0, n_dense, n, first.data_ptr(), last.data_ptr())
    torch.cuda.synchronize()
    good = ((shared & 2) == 0)[None, :] & ((dflags[flag_rows] & 4) == 0)
    assert np.array_equal(n_good.cpu().numpy(), np.count_nonzero(good, axis=1))
    if n_dense > 0:
        assert np.array_equal(nnz_d.cpu().numpy(), np.count_nonzero((dense != 0)[None] & good[:, None, :], axis=2))
        f_want, l_want = FC.row_spans(dense)
        assert np.array_equal(first.cpu().numpy(), f_want) and np.array_equal(last.cpu().numpy(), l_want)


@pytest.mark.parametrize("order,n_dense,n_det", [(1, 18, 37), (3, 0, 5), (5, 3, 6)])
def test_fused_subtract_and_flag_spans(order, n_dense, n_det):
    import torch

    from toast_amd import capi

    D = capi.dev
    k = order + 1
    rng = np.random.default_rng(7 + order)
    starts, stops = [3, 300, 700, 2100], [290, 641, 2000, 2100 + max(k, 2)]
    n = 2100 + max(k, 2) + 2 * TILE + 5
    n_rows = n_det + 1
    rows = rng.permutation(n_rows)[:n_det].astype(np.int32)
    signal = rng.standard_normal((n_rows, n))
    dense = rng.standard_normal((n_dense, n))
    a, b = rng.standard_normal((n_det, n_dense)), rng.standard_normal((n_det, len(starts), k))
    d_sig, d_dense, d_a, d_b = dev(signal), dev(dense), dev(a), dev(b)
    D.filterbin_subtract(order, d_dense.data_ptr() if n_dense else 0, n_dense, n, rows, d_sig.data_ptr(), d_a.data_ptr(),
                         starts, stops, d_b.data_ptr())
    torch.cuda.synchronize()
    want = signal.astype(np.longdouble)
    scale = np.zeros((n_rows, n), dtype=np.longdouble)
    for i, row in enumerate(rows):
        want[row] -= a[i].astype(np.longdouble) @ dense.astype(np.longdouble)
        scale[row] += np.abs(a[i]) @ np.abs(dense)
        for v, (s0, s1) in enumerate(zip(starts, stops)):
            P = FC.interval_polynomials(s0, s1, k)
            want[row, s0:s1] -= b[i, v].astype(np.longdouble) @ P.astype(np.longdouble)
            scale[row, s0:s1] += np.abs(b[i, v]) @ np.abs(P)
    got = d_sig.cpu().numpy()
    # the fit is a sequential sum of n_dense + k products (+ 2 per term for P), then one subtraction
    bound = EPS * ((n_dense + k + 3) * scale + np.abs(want))
    assert np.all(np.abs(got.astype(np.longdouble) - want) <= bound)
    untouched = [r for r in range(n_rows) if r not in rows]
    assert np.array_equal(got[untouched], signal[untouched])
    # flag spans: overlapping spans of one row, a whole row, an empty span
    flags = (rng.random((n_rows, n)) < 0.3).astype(np.uint8) * 2
    d_fl = dev(flags)
    spans = [(0, 0, n), (1, 5, 700), (1, 600, 901), (n_rows - 1, n - 1, n), (1, 40, 40)]
    D.filterbin_flag_spans([s[0] for s in spans], [s[1] for s in spans], [s[2] for s in spans], n_rows, n, d_fl.data_ptr(), 9)
    torch.cuda.synchronize()
    for row, first, last in spans:
        flags[row, first:last] |= 9
    assert np.array_equal(d_fl.cpu().numpy(), flags)
    with pytest.raises(RuntimeError, match="outside"):
        D.filterbin_flag_spans([n_rows], [0], [4], n_rows, n, d_fl.data_ptr(), 1)
    with pytest.raises(RuntimeError, match="sorted"):
        D.filterbin_subtract(order, 0, 0, n, rows, d_sig.data_ptr(), 0, [10, 5], [20, 9], d_b.data_ptr())


def make_operator(cfg, **kw):
    det_pointing = ops.PointingDetectorSimple()
    pixels = ops.PixelsHealpix(detector_pointing=det_pointing, nside=16, nest=True)
    weights = ops.StokesWeights(detector_pointing=det_pointing, mode="IQU")
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pixels, stokes_weights=weights,
                        det_flag_mask=FC.DET_FLAG_MASK, shared_flag_mask=FC.SHARED_FLAG_MASK)
    return ops.FilterBin(name="fb", binning=binner, **FC.operator_traits(cfg), **kw), binner


@pytest.mark.parametrize("name", list(FC.CASES))
def test_operator_on_resident_data_against_the_reference_run(fixture, name):
    case = FC.load_case(fixture, name)
    cfg = case["cfg"]
    data = FC.build_data(case)
    ob = data.obs[0]
    sig, fl = ob.detdata[defaults.det_data], ob.detdata[defaults.det_flags]
    for obj, key in ((sig, defaults.det_data), (fl, defaults.det_flags)):
        obj.accel_create(key)
        obj.accel_update_device()
    fb, _ = make_operator(cfg)
    fb.apply(data)
    assert sig.accel_in_use()                                   # stays where the caller keeps it
    dets = ob.local_detectors
    assert np.array_equal(ob.shared[defaults.shared_flags].data, case["shared_out"])
    assert np.array_equal(fl.data, case["flags_out"])
    assert [fb.routes[ob.name][d] for d in dets] == case["routes"].tolist()
    assert [ob.local_detector_flags.get(d, 0) for d in dets] == case["detflags"].tolist()
    rms = np.sqrt(np.mean(case["signal"] ** 2))
    dist = np.max(np.abs(sig.data - case["out"])) / rms
    print(f"\nfilterbin device {name}: max |delta filtered| / rms(signal) = {dist:.3e}  (10 E_host = {10 * E_HOST:.1e})")
    worst_amp = 0.0
    for i, det in enumerate(dets):
        want = {x: case["amps"][i, t] for t, x in enumerate(case["amp_names"]) if not np.isnan(case["amps"][i, t])}
        got = fb.amplitudes[ob.name][det]
        if case["routes"][i] not in (FB.ROUTE_INV, FB.ROUTE_PINV):
            assert got is None
            continue
        assert sorted(got) == sorted(want)
        if case["routes"][i] == FB.ROUTE_INV:
            scale = max(abs(v) for v in want.values())
            worst_amp = max(worst_amp, max(abs(got[x] - want[x]) for x in want) / scale)
    print(f"filterbin device {name}: max |delta amplitude| / max |amplitude| = {worst_amp:.3e}")
    assert dist <= PARITY
    assert dist <= 10 * E_HOST
    assert worst_amp <= 10 * E_HOST


def test_filterbin_and_binmap_end_to_end(fixture):
    """The filtered map equals the map that the existing operators bin from the reference's filtered signal and flags;
    the unfiltered products exist under the reference's names."""
    case = FC.load_case(fixture, "all")
    data = FC.build_data(case)
    fb, _ = make_operator(case["cfg"], write_binmap=True, keep_final_products=True)
    fb.apply(data)
    for tag in ("filtered", "unfiltered"):
        for key in (f"fb_{tag}_hits", f"fb_{tag}_invcov", f"fb_{tag}_cov", f"fb_{tag}_rcond", f"fb_{tag}_map",
                    f"fb_noiseweighted_{tag}_map"):
            assert key in data, key
    want_data = FC.build_data(case)
    ob = want_data.obs[0]
    ob.detdata[defaults.det_data].data[:] = case["out"]
    ob.detdata[defaults.det_flags].data[:] = case["flags_out"]
    ob.shared[defaults.shared_flags].data[:] = case["shared_out"]
    ob.update_local_detector_flags({d: int(f) for d, f in zip(ob.local_detectors, case["detflags"])})
    _, binner = make_operator(case["cfg"])
    ops.BuildPixelDistribution(pixel_dist=binner.pixel_dist, pixel_pointing=binner.pixel_pointing).apply(want_data)
    binner.covariance, binner.binned = "cov", "map"
    ops.CovarianceAndHits(pixel_dist=binner.pixel_dist, covariance="cov", hits="hits", rcond="rcond",
                          det_mask=binner.det_mask, det_flags=binner.det_flags, det_flag_mask=binner.det_flag_mask,
                          shared_flags=binner.shared_flags, shared_flag_mask=binner.shared_flag_mask,
                          pixel_pointing=binner.pixel_pointing, stokes_weights=binner.stokes_weights,
                          noise_model=binner.noise_model, rcond_threshold=fb.rcond_threshold).apply(want_data)
    binner.apply(want_data)
    got, want = np.asarray(data["fb_filtered_map"].data), np.asarray(want_data["map"].data)
    assert np.array_equal(np.asarray(data["fb_filtered_hits"].data), np.asarray(want_data["hits"].data))
    assert np.count_nonzero(want) > 0
    dist = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"\nfilterbin end to end: max |delta map| / max |map| = {dist:.3e}")
    assert dist <= PARITY
    unfiltered = np.asarray(data["fb_unfiltered_map"].data)
    assert np.max(np.abs(unfiltered - got)) > 1.0               # the offsets of 5-15 are in one and not in the other
    # without keep_final_products nothing stays
    data2 = FC.build_data(case)
    fb2, _ = make_operator(case["cfg"], write_binmap=True)
    fb2.apply(data2)
    assert not [key for key in data2.keys() if str(key).startswith("fb_")]
