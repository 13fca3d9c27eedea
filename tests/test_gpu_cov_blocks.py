"""GPU: the per-pixel covariance kernels that take over after the scatter, at every nnz and at the rcond threshold,
against the 50-digit truth of tests/golden/cov_blocks.npz and the derived bounds of tests/cov_blocks_case.py and
tests/nnz_reference.py (tests/test_cov_blocks_host.py shows on the CPU that the same checks catch a wrong kernel).
Kernel instantiations and the tests that launch them:

  k_cov_invert<2 | 3 | 4>, invert 1 | 0        test_inversion, test_rcond_only, test_threshold_decisions_and_mask,
                                               test_degenerate_and_sizes, test_stride_loop_past_the_grid_cap (3 | 4)
  k_cov_invert<1>                              test_nnz1
  k_threshold_mask                             test_threshold_decisions_and_mask
  k_cov_mult_diag<1..4>, k_cov_apply_diag<1..4>  test_mult_and_apply
  k_cov_accum<2 | 4, 1 | 2>, k_cov_accum<1, 0>   test_accum_streams
  covariance_invert / covariance_rcond         test_operator_level

Every launch of k_cov_invert here has a guard element after ``data`` and after ``cond`` that must keep its bits.

Measured on an MI355X with the committed fixture (rcond figure / inverse figure in eps, threshold 1e-12, invert; the
restatement's stored figures are 6.382 / 4.517, so the bounds 25.527 / 18.068); the plain-double emulation gives the
same figures to the last digit printed:

  family            nnz 2            nnz 3            nnz 4
  cond_1e+00        1.458 / 1.068    4.066 / 2.944    6.061 / 5.543
  cond_1e-01        0.163 / 0.140    0.586 / 0.282    0.713 / 0.404
  cond_1e-02        0.135 / 0.110    0.442 / 0.241    0.277 / 0.173
  cond_1e-04        0.171 / 0.132    0.279 / 0.165    0.540 / 0.319
  cond_1e-06        0.188 / 0.104    0.358 / 0.197    0.261 / 0.169
  cond_1e-08        0.148 / 0.091    0.254 / 0.127    0.261 / 0.152
  cond_1e-10        0.135 / 0.092    0.454 / 0.285    0.466 / 0.245
  cond_1e-12        0.222 / 0.150    0.155 / 0.114    0.235 / 0.135
  diag_exact        0.000 / 0.037    0.000 / 0.037    0.000 / 0.037
  ladder            0.245 / 0.127    0.456 / 0.247    0.524 / 0.350
  scan_close        0.114 / 0.059    0.144 / 0.084    --
  scan_spread       1.791 / 1.117    1.640 / 0.888    --
  scan_two_angles   0.708 / 0.578    (rank 2)         --
  spacer            0.395 / 0.274    1.058 / 0.712    1.845 / 0.827
  tiny_offdiag      0.000 / 0.125    0.083 / 0.083    0.000 / 0.063

cov_mult_diag / cov_apply_diag reach 0.63 / 0.57 of gamma(nnz + 1) sum |terms|, A A^-1 - 1 at most 0.076 of its bound
(0.5 at nnz 1), the accumulation kernels at most 0.57 of theirs.  No family comes within a factor of two of a bound."""
import numpy as np
import pytest

import cov_blocks_case as C
import nnz_reference as R

pytestmark = pytest.mark.gpu

GUARD = -7.25e300


@pytest.fixture(scope="module")
def hip():
    from toast_amd import capi

    assert capi.accel_enabled(), "no HIP device visible"
    capi.accel_assign_device(1, 0, 1.0, False)
    return capi


class DeviceRun:
    """run(packed, threshold, invert) -> (data, cond) of k_cov_invert<nnz> on device buffers with one guard element each;
    ``d_cond`` keeps the condition numbers of the last call on the device."""

    def __init__(self, hip, nnz):
        self.hip, self.nnz, self.d_cond = hip, nnz, None

    def __call__(self, packed, threshold, invert):
        import torch

        packed = np.ascontiguousarray(packed, dtype=np.float64).reshape(-1, C.blk(self.nnz))
        n = packed.shape[0]
        d = torch.full((packed.size + 1,), GUARD, dtype=torch.float64, device="cuda")
        d[:-1] = torch.tensor(packed.reshape(-1))
        c = torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda")
        self.hip.dev.cov_eigendecompose_diag(1, n, self.nnz, d.data_ptr(), c.data_ptr(), threshold, invert)
        torch.cuda.synchronize()
        dh, ch = d.cpu().numpy(), c.cpu().numpy()
        assert dh[-1] == GUARD and ch[-1] == GUARD, "the element after the buffer was written"
        self.d_cond = c
        return dh[:-1].reshape(packed.shape).copy(), ch[:-1].copy()


def run_of(hip):
    return lambda nnz: DeviceRun(hip, nnz)


# ------------------------------------------------------------------------------------------ inversion
@pytest.mark.parametrize("nnz", C.NNZ)
def test_inversion(hip, nnz):
    """All families in one buffer, threshold 1e-12: rcond and inverse figures within 4 x the restatement's."""
    C.check_inversion(DeviceRun(hip, nnz), C.load(nnz), label="device ")


@pytest.mark.parametrize("nnz", C.NNZ)
def test_rcond_only(hip, nnz):
    C.check_rcond_only(DeviceRun(hip, nnz), C.load(nnz), label="device ")


@pytest.mark.parametrize("nnz", C.NNZ)
def test_threshold_decisions_and_mask(hip, nnz):
    """Per tau the decisions of cov_blocks_case.check_threshold, then threshold_mask on the cond just produced and on the
    plain rcond (threshold 0): the bit exactly where cond < tau -- the diagonal blocks at exactly tau stay clear, those at
    nextafter(tau, 0) get it --, the other bits of a pre-filled mask kept, n of 1, 255, 256, 257 and all."""
    import torch

    T, run = C.load(nnz), DeviceRun(hip, nnz)
    pre = np.random.default_rng(7).integers(0, 256, T.n + 1).astype(np.uint8)
    for tau in C.TAUS:
        for thr in (tau, 0.0):
            if thr == tau:
                _, cond = C.check_threshold(run, T, tau, label="device ")
            else:
                _, cond = run(T.packed, 0.0, False)
                exact = T.is_in("diag_exact") & (T.tau == tau)
                assert (cond[exact & (T.side == 1)] == tau).all() and (cond[exact & (T.side == -1)] < tau).all()
            for n, bit in ((1, 1), (255, 16), (256, 1), (257, 128), (T.n, 1)):
                mask = torch.tensor(pre)
                mask = mask.cuda()
                hip.dev.threshold_mask(n, run.d_cond.data_ptr(), tau, bit, mask.data_ptr())
                torch.cuda.synchronize()
                want = pre.copy()
                want[:n][cond[:n] < tau] |= bit
                assert np.array_equal(mask.cpu().numpy(), want), (tau, thr, n)
                assert (cond[:n] < tau).any() or n == 1


@pytest.mark.parametrize("nnz", C.NNZ)
def test_degenerate_and_sizes(hip, nnz):
    T, run = C.load(nnz), DeviceRun(hip, nnz)
    full = run(T.packed, C.MAIN_THRESHOLD, True)
    C.check_degenerate(run, T, full)
    C.check_sizes(run, T, full)
    # a zero block and cond == 0 at every threshold in use, not only at 1e-12
    for tau in C.TAUS:
        data, cond = run(T.packed, tau, True)
        dead = T.is_in(*C.DEAD)
        assert (C.bits(cond[dead]) == 0).all() and (C.bits(data[dead]) == 0).all()


def test_nnz1(hip):
    C.check_nnz1(DeviceRun(hip, 1))


@pytest.mark.parametrize("nnz", (3, 4))
def test_stride_loop_past_the_grid_cap(hip, nnz):
    """4096 x 256 + 257 pixels, the fixture's blocks tiled: past the grid cap of flat_grid every thread takes a second
    pixel.  Every tile has the bits of the first, the first those of the blocks run on their own."""
    import torch

    T = C.load(nnz)
    alone_d, alone_c = DeviceRun(hip, nnz)(T.packed, C.MAIN_THRESHOLD, True)
    b, m = C.blk(nnz), T.n
    n = 4096 * 256 + 257
    reps, rem = divmod(n, m)
    base = torch.tensor(T.packed).cuda()
    d = torch.full((n * b + 1,), GUARD, dtype=torch.float64, device="cuda")
    d[:reps * m * b] = base.reshape(-1).repeat(reps)
    d[reps * m * b:n * b] = base[:rem].reshape(-1)
    c = torch.full((n + 1,), GUARD, dtype=torch.float64, device="cuda")
    hip.dev.cov_eigendecompose_diag(1, n, nnz, d.data_ptr(), c.data_ptr(), C.MAIN_THRESHOLD, True)
    torch.cuda.synchronize()
    assert d[-1].item() == GUARD and c[-1].item() == GUARD
    for out, width, alone in ((d, m * b, alone_d), (c, m, alone_c)):
        ints = out[:-1].view(torch.int64)
        first = ints[:width]
        assert np.array_equal(first.cpu().numpy(), C.bits(alone).reshape(-1))
        assert torch.equal(ints[:reps * width].view(reps, width), first.expand(reps, width))
        assert torch.equal(ints[reps * width:], first[:ints.numel() - reps * width])


# ------------------------------------------------------------------------------------------ cov_mult_diag, cov_apply_diag
def _mult_reference(a, b, nnz):
    """Packed entry (k, m >= k) <- sum_j S1(m, j) S2(j, k) in long double -> (exact, sum of |terms|)."""
    s1, s2 = C.unpack(a.astype(R.LD), nnz), C.unpack(b.astype(R.LD), nnz)
    iu = np.triu_indices(nnz)
    want = np.einsum("pmj,pjk->pmk", s1, s2)[:, iu[1], iu[0]]
    mag = np.einsum("pmj,pjk->pmk", np.abs(s1), np.abs(s2))[:, iu[1], iu[0]]
    return want, mag


@pytest.mark.parametrize("nnz", (1, 2, 3, 4))
def test_mult_and_apply(hip, nnz):
    """Against long double with gamma(nnz + 1) sum |terms| per output element (nnz products, nnz - 1 additions in the
    kernel's fixed order: gamma(nnz) would do, one spare).  Inputs: random symmetric blocks, and the fixture's blocks down
    to rcond 1e-12 times their own device inverse -- that product (and the inverse applied to the block's first column)
    is also held to the identity within nnz x (inverse bound) x eps x kappa per element."""
    rng = np.random.default_rng(100 + nnz)
    b = C.blk(nnz)
    n_rand = 300
    a1 = rng.standard_normal((n_rand, b)) * 10.0 ** rng.uniform(-3, 3, (n_rand, 1))
    a2 = rng.standard_normal((n_rand, b))
    if nnz > 1:
        T = C.load(nnz)
        inv, cond = DeviceRun(hip, nnz)(T.packed, C.MAIN_THRESHOLD, True)
        sel = T.compared & (cond > 0)
        blocks, inverse = T.packed[sel], inv[sel]
        kappa = np.asarray(1.0 / T.rc[sel], dtype=np.float64)
        tol = nnz * T.inv_bound * C.EPS * kappa
    else:
        vals, _ = C.load_nnz1()
        blocks = vals[np.isfinite(vals) & (vals != 0)].reshape(-1, 1)
        inverse, _ = DeviceRun(hip, 1)(blocks, 0.0, True)
        tol = np.full(blocks.shape[0], R.gamma(2))
    a = np.ascontiguousarray(np.concatenate([a1, blocks]))
    bb = np.ascontiguousarray(np.concatenate([a2, inverse]))
    want, mag = _mult_reference(a, bb, nnz)
    got = a.copy()
    hip.cov_mult_diag(1, a.shape[0], nnz, got.reshape(-1), bb.reshape(-1), False)
    worst = R.excess(got, want, R.gamma(nnz + 1) * mag)
    eye = np.eye(nnz)[np.triu_indices(nnz)]
    off_identity = float(np.max(np.abs(got[n_rand:] - eye).max(axis=1) / tol))
    print(f"device cov_mult_diag nnz={nnz}: {worst:.3g} of the bound; A A^-1 - 1: {off_identity:.3g} of its bound")
    assert worst <= 1.0
    assert off_identity <= 1.0
    # cov_apply_diag: random vectors; the inverse applied to the first column of its block
    vec = np.concatenate([rng.standard_normal((n_rand, nnz)), C.unpack(blocks, nnz)[:, :, 0]])
    mat = np.ascontiguousarray(np.concatenate([a1, inverse]))
    full = C.unpack(mat.astype(R.LD), nnz)
    want = np.einsum("pkj,pj->pk", full, vec.astype(R.LD))
    mag = np.einsum("pkj,pj->pk", np.abs(full), np.abs(vec).astype(R.LD))
    got = np.ascontiguousarray(vec.copy())
    hip.cov_apply_diag(1, mat.shape[0], nnz, mat.reshape(-1), got.reshape(-1), False)
    worst = R.excess(got, want, R.gamma(nnz + 1) * mag)
    off_identity = float(np.max(np.abs(got[n_rand:] - np.eye(nnz)[0]).max(axis=1) / tol))
    print(f"device cov_apply_diag nnz={nnz}: {worst:.3g} of the bound; A^-1 a_0 - e_0: {off_identity:.3g} of its bound")
    assert worst <= 1.0
    assert off_identity <= 1.0


# ------------------------------------------------------------------------------------------ cov_accum_*
def _stream(rng, n, nsub, nsubpix):
    """Runs of equal pixels with skipped samples (negative submap or pixel); the first sample is never skipped."""
    runs = rng.integers(1, 13, n)
    pix = np.repeat(rng.integers(0, nsub * nsubpix, n), runs)[:n]
    submap, subpix = (pix // nsubpix).astype(np.int64), (pix % nsubpix).astype(np.int64)
    skip = rng.random(n) < 0.08
    skip[0] = False
    which = rng.random(n) < 0.5
    submap[skip & which] = -1
    subpix[skip & ~which] = -1
    return submap, subpix, ~skip


@pytest.mark.parametrize("n", (1, 255, 257, 5000))
def test_accum_streams(hip, n):
    """cov_accum_diag_invnpp and cov_accum_zmap at nnz 2 and 4, cov_accum_diag_hits: against a long double scatter with
    gamma(terms + 2) S per element (a term is two rounded products, then as many additions as terms, onto what the map
    held), elements that get nothing keep their bits; hits are exact."""
    import toast_amd

    m = toast_amd.load_native()
    rng = np.random.default_rng(n)
    nsub, nsubpix = 3, 40
    submap, subpix, good = _stream(rng, n, nsub, nsubpix)
    key = (submap * nsubpix + subpix)[good]
    hits0 = rng.integers(0, 5, nsub * nsubpix).astype(np.int64)
    hits = hits0.copy()
    m.cov_accum_diag_hits(nsub, nsubpix, 1, submap, subpix, hits, False)
    want = hits0.copy()
    np.add.at(want, key, 1)
    assert np.array_equal(hits, want)
    for nnz in (2, 4):
        w = rng.standard_normal((n, nnz))
        tod = rng.standard_normal(n)
        ju, ku = np.triu_indices(nnz)
        wl = w[good].astype(R.LD)
        inv0 = rng.standard_normal((nsub * nsubpix, ju.size)) * (rng.random((nsub * nsubpix, 1)) < 0.5)
        inv = inv0.copy()
        m.cov_accum_diag_invnpp(nsub, nsubpix, nnz, submap, subpix, np.ascontiguousarray(w.reshape(-1)), 2.5,
                                inv.reshape(-1), False)
        ref = R.Scatter(inv0, [key], [R.LD(2.5) * wl[:, ju] * wl[:, ku]])
        assert np.array_equal(ref.counts(), want - hits0)
        worst_inv = ref.excess(inv)
        z0 = rng.standard_normal((nsub * nsubpix, nnz)) * (rng.random((nsub * nsubpix, 1)) < 0.5)
        z = z0.copy()
        m.cov_accum_zmap(nsub, nsubpix, nnz, submap, subpix, np.ascontiguousarray(w.reshape(-1)), 0.5, tod, z.reshape(-1))
        refz = R.Scatter(z0, [key], [(R.LD(0.5) * tod[good].astype(R.LD))[:, None] * wl])
        worst_z = refz.excess(z)
        print(f"device cov_accum n={n} nnz={nnz}: invnpp {worst_inv:.3g}, zmap {worst_z:.3g} of the bound")
        assert worst_inv <= 1.0 and worst_z <= 1.0


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize("nnz", (3, 4))
def test_operator_level(hip, nnz):
    """pixels.covariance_invert with an rcond map on a device-resident PixelData and on a host one: identical bits in the
    matrix and in rcond, the resident one stays resident; covariance_rcond equals the threshold-0 cond."""
    from toast_amd.pixels import PixelData, PixelDistribution, covariance_invert, covariance_rcond

    T = C.load(nnz)
    nps = 64
    local = [1, 4, 6, 7, 9, 10, 12][:min(7, T.n // nps)]
    n_px = len(local) * nps
    assert T.is_in(*C.DEAD)[:n_px].sum() >= len(C.DEAD)
    dist = PixelDistribution(n_pix=14 * nps, n_submap=14, local_submaps=local)
    tau = 1e-6
    outs = []
    for on_dev in (False, True):
        cov = PixelData(dist, np.float64, n_value=C.blk(nnz))
        cov.data.reshape(-1, C.blk(nnz))[:] = T.packed[:n_px]
        rc = PixelData(dist, np.float64, n_value=1)
        if on_dev:
            cov.accel_create(f"cb_cov{nnz}")
            cov.accel_update_device()
        covariance_invert(cov, tau, rcond=rc)
        if on_dev:
            assert cov.accel_in_use() and rc.accel_in_use(), "a device-resident covariance left the device"
            cov.accel_update_host()
            rc.accel_update_host()
            cov.accel_delete()
            rc.accel_delete()
        outs.append((cov.data.reshape(-1, C.blk(nnz)).copy(), rc.data.reshape(-1).copy()))
    assert C.same_bits(outs[0][0], outs[1][0]) and C.same_bits(outs[0][1], outs[1][1])
    data, cond = DeviceRun(hip, nnz)(T.packed[:n_px], tau, True)
    assert C.same_bits(outs[0][0], data) and C.same_bits(outs[0][1], cond)
    plain = PixelData(dist, np.float64, n_value=C.blk(nnz))
    plain.data.reshape(-1, C.blk(nnz))[:] = T.packed[:n_px]
    _, cond0 = DeviceRun(hip, nnz)(T.packed[:n_px], 0.0, False)
    assert C.same_bits(covariance_rcond(plain).data.reshape(-1), cond0)
    assert C.same_bits(plain.data.reshape(-1, C.blk(nnz)), T.packed[:n_px])
