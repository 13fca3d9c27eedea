"""GPU: the five kernels of csrc/ground_filter.hip at the template counts, lengths, detector counts and flag bytes the
cases of tests/test_gpu_ground_filter.py never take, against the long double truth of tests/ground_filter_case.py (see
its docstring for the cases and the bound; tests/test_ground_filter_host.py ties that yardstick to the reference).

(a) template counts on both sides of every threshold of toast_hip_template_fit_dev: ``k_template_project<8,8>`` (1 .. 8),
    ``<16,4>`` (9, 16), ``<24,3>`` (17 .. 24 in one pass, 33 and 48 in two), ``<32,2>`` (25, 32 in one pass, 49 and 65 in
    two and three); the one-pair path of ``k_template_gram_flagged`` (up to 22 templates = 253 pairs) and its pair loop
    (from 23 = 276 pairs on).  37 detectors: a second block and a clamped duplicate detector in every instantiation.
    9001 samples: three projection slices and nine queue blocks, the last ones ragged.  Indicator / split templates with a
    zero row: ``total != 0.0`` in the Gram kernel, ``v != 0.0`` in the projection and ``acc != 0.0`` / ``slice_acc != 0.0``
    in the flagged Gram kernel see sums that are exactly zero, and the entry must still hold 0.0.
(b) lengths around a wave, a block, a queue block (1024), a projection slice (4096) and the 65536-sample slices of
    ``k_template_gram`` (``blockIdx.y > 0``) and ``k_template_gram_flagged`` (``blockIdx.x > 0``), with the per-slice clamp
    ``i1`` and the cross-slice atomics; 131149 = 2 x 65536 + 77.
(c) flagged samples count as 0 whatever they hold, an unflagged NaN stays in its detector's row.
(d) ``k_template_subtract`` bit for bit: the second register pass (``dpass = 16``: 17 detectors and more), a second block
    in ``y`` (33, 37), a second and third template tile (17, 33, 40 templates), ``first_template`` in the first tile, in a
    later tile (33, 32) and at no tile boundary (19, 3), (40, 7).
(e) ``k_legendre`` (start orders 0 .. 5, up to order 64) and ``k_template_select`` bit for bit, nothing written past the end.
(f) ops.GroundFilter with 27 templates, 35 detectors and 70001 samples against the oracle.

Every output buffer is handed over full of NaN (-1 for n_flagged): the entry promises to overwrite it.  Every figure is
printed before it is asserted.

Observed on an MI355X (worst distance / its bound = 4 x the reference's sequential sums; the case with the largest ratio):
    (a) Legendre    proj 8.2e-17 / 6.9e-16, gram_common 3.9e-17 / 1.6e-16 (1 template), gram_flagged 1.7e-15 / 4.6e-15
    (a) indicator   proj 8.5e-17 / 1.1e-15, gram_common 2.0e-16 / 2.0e-14, gram_flagged 7.5e-15 / 3.0e-14
    (b) 3 templates proj 6.5e-17 / 1.9e-16 (63 samples), gram_common 7.1e-17 / 2.9e-16 (1 sample), gram_flagged 7.7e-16 /
                    1.5e-15 (255 samples); at 131149 samples 3.0e-18 / 5.8e-16, 8.9e-17 / 2.4e-14, 7.7e-15 / 2.4e-14
    (b) 23 templates proj 8.9e-17 / 3.5e-16 and gram_common 9.9e-17 / 4.0e-16 (1 sample: the rounding of the one product),
                    gram_flagged 1.7e-15 / 5.9e-15 (1023 samples)
    (c)             proj 1.1e-17 / 5.9e-16, gram_flagged 8.5e-16 / 3.4e-15; the NaN row is NaN in all its entries
    (d), (e)        0 values differ;  (f) max |device - oracle| 3.3e-13 against 1.1e-08
The sums of the detector that flags every sample are the same sums as the common Gram matrix in the order of the queue:
they are the figures that come close to the reference's own distance (a quarter of the bound).  The first run of
grid (b) found the flagged Gram matrix of 131149 samples and 23 templates unsymmetric in its last bits -- three slices add
into an entry and its mirror in different orders; the Gram kernels now add into the upper triangles and
``k_template_mirror`` copies them.
"""
import numpy as np
import pytest

import ground_filter_case as gc
from test_oracle_ground_filter import LEGENDRE_SPANS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_fit(case, signal_buffer=None):
    """toast_hip_template_fit_dev on a case: (proj, gram_common, gram_flagged, n_flagged), outputs pre-filled with NaN / -1."""
    import torch

    from toast_amd import capi

    nt, n, n_det = case["n_template"], case["n_samp"], case["n_det"]
    d_t = dev(case["templates"])
    d_s = dev(case["signal_buffer"] if signal_buffer is None else signal_buffer)
    d_f = dev(case["flag_buffer"]) if case["with_flags"] else None
    d_sh = dev(case["shared_flags"]) if case["with_flags"] else None
    proj = torch.full((n_det, nt), float("nan"), dtype=torch.float64, device="cuda")
    gram = torch.full((nt, nt), float("nan"), dtype=torch.float64, device="cuda")
    dgram = torch.full((n_det, nt, nt), float("nan"), dtype=torch.float64, device="cuda")
    nflag = torch.full((n_det,), -1, dtype=torch.int64, device="cuda")
    capi.dev.template_fit(d_t.data_ptr(), nt, n, case["signal_index"], d_s.data_ptr(),
                          case["flag_index"] if case["with_flags"] else None, d_f.data_ptr() if case["with_flags"] else 0,
                          case["det_mask"], d_sh.data_ptr() if case["with_flags"] else 0, case["shared_mask"],
                          proj.data_ptr(), gram.data_ptr(), dgram.data_ptr(), nflag.data_ptr())
    torch.cuda.synchronize()
    return proj.cpu().numpy(), gram.cpu().numpy(), dgram.cpu().numpy(), nflag.cpu().numpy()


def check_fit(case, label, got=None, t=None, seq=None, skip_proj_rows=()):
    """Every detector and every entry of the four outputs; returns the figures."""
    if t is None:
        t, seq = gc.cached_truth(case)
    bound = gc.bounds(seq)
    proj, gram, dgram, nflag = run_fit(case) if got is None else got
    rows = np.array([d for d in range(case["n_det"]) if d not in skip_proj_rows])
    figures = dict(proj=gc.distance(proj[rows], t["proj"][rows], t["proj_norm"][rows]),
                   gram_common=gc.distance(gram, t["gram_common"], t["gram_common_norm"]),
                   gram_flagged=gc.distance(dgram, t["gram_flagged"], t["gram_flagged_norm"]))
    compared = {k: int(np.count_nonzero(t[k + "_norm"])) for k in bound}
    exact_zero = {k: int(np.count_nonzero(t[k + "_norm"] == 0)) for k in bound}
    print(f"{label}: " + ", ".join(f"{k} {figures[k]:.3e} / {bound[k]:.3e} ({compared[k]} entries, {exact_zero[k]} exactly 0)"
                                   for k in sorted(bound)) + f"; n_flagged {nflag.min()} .. {nflag.max()}")
    assert np.array_equal(nflag, t["n_flagged"]), label
    # the bound is no formality: far below the weight of one term, and every entry with terms is compared
    n_terms = case["n_samp"]
    for k in bound:
        assert bound[k] < 1e-3 / n_terms, (label, k)
        assert figures[k] <= bound[k], (label, k, figures[k], bound[k])
    assert np.array_equal(bits(gram), bits(gram.T)), label
    assert np.array_equal(bits(dgram), bits(np.swapaxes(dgram, 1, 2))), label
    if not case["with_flags"] or case["det_mask"] == 0:
        assert not np.any(dgram) and not np.any(nflag), label
    return figures


@pytest.mark.parametrize("nt,kind,flag_kind", gc.template_grid())
def test_template_count_grid(nt, kind, flag_kind):
    case = gc.template_grid_case(nt, kind, flag_kind)
    t, _ = gc.cached_truth(case)
    check_fit(case, f"(a) n_template {nt} {kind} {flag_kind}")
    if flag_kind == "random":
        # the detector flagged everywhere has an all-zero projection, the one with one good sample a single term
        d_all, d_one = gc.TEMPLATE_GRID_ALL[0], gc.TEMPLATE_GRID_ONE_GOOD[0]
        assert not np.any(t["proj_norm"][d_all]) and t["n_flagged"][d_all] == t["n_flagged"][d_one] + 1
    if kind == "indicator":
        assert np.count_nonzero(t["gram_common_norm"] == 0) > 0 and np.count_nonzero(t["proj_norm"] == 0) > 0


@pytest.mark.parametrize("n_samp", gc.SAMPLE_LENGTHS)
@pytest.mark.parametrize("nt", gc.LENGTH_GRID_COUNTS)
def test_sample_length_grid(nt, n_samp):
    case = gc.length_grid_case(n_samp, nt)
    t, _ = gc.cached_truth(case)
    check_fit(case, f"(b) n_samp {n_samp} n_template {nt}")
    assert t["n_flagged"][gc.LENGTH_GRID_ALL[0]] == np.count_nonzero(gc.masks_of(case)[0])


@pytest.mark.parametrize("nt", [8, 32])
def test_flagged_nonfinite_samples_count_as_zero(nt):
    """A NaN under a detector flag and an Inf under a shared flag reach no projection: the kernel zeroes the signal of a
    bad sample where the reference multiplies it by ``good``."""
    case = gc.nonfinite_case(nt)
    common, det_bad = gc.masks_of(case)
    k = 3
    i_det = int(np.flatnonzero(common & det_bad[k])[0])
    i_shared = int(np.flatnonzero(~common & ~det_bad[k])[0])
    buf = case["signal_buffer"].copy()
    buf[case["signal_index"][k], i_det] = np.nan
    buf[case["signal_index"][k], i_shared] = np.inf
    signal = buf[case["signal_index"]]
    t = gc.truth(case, signal)                        # replaces the signal of bad samples by 0
    seq = gc.sequential_distance(case, t, np.where(common[None, :] & ~det_bad, signal, 0.0))
    clean_t, _ = gc.cached_truth(case)
    assert np.array_equal(t["proj"], clean_t["proj"])
    got = run_fit(case, buf)
    assert np.all(np.isfinite(got[0]))
    check_fit(case, f"(c) n_template {nt}: NaN at {i_det} (detector flag), Inf at {i_shared} (shared flag) of detector {k}",
              got=got, t=t, seq=seq)


@pytest.mark.parametrize("k", [3, 10])
@pytest.mark.parametrize("nt", [8, 32])
def test_unflagged_nan_stays_in_its_row(nt, k):
    """Detector 3 shares its wave with seven others at 8 templates and with detector 2 at 32; detector 10 is the last one,
    which the clamped lanes of the last wave load again."""
    case = gc.nonfinite_case(nt)
    common, det_bad = gc.masks_of(case)
    i = int(np.flatnonzero(common & ~det_bad[k])[5])
    buf = case["signal_buffer"].copy()
    buf[case["signal_index"][k], i] = np.nan
    got = run_fit(case, buf)
    print(f"(c) n_template {nt}: NaN in good sample {i} of detector {k}: row {k} {got[0][k][:3]} ..")
    assert np.all(np.isnan(got[0][k]))
    check_fit(case, f"(c) n_template {nt}: the other rows", got=got, skip_proj_rows=(k,))


# ------------------------------------------------------------------------------------------------ (d) subtraction
SUBTRACT_DETS = (1, 16, 17, 32, 33, 37)
SUBTRACT_TEMPLATES = ((1, 0), (16, 0), (17, 0), (19, 3), (33, 0), (40, 7), (33, 32))


def check_subtract(n_det, nt, first, n_samp):
    import torch

    from toast_amd import capi

    rng = np.random.default_rng([77, n_det, nt, first, n_samp])
    templates = rng.standard_normal((nt, n_samp))
    coeff = rng.standard_normal((n_det, nt))          # different for every detector and template
    rows = rng.permutation(n_det + 3)[:n_det].astype(np.int32)
    buf = rng.standard_normal((n_det + 3, n_samp))
    d_t, d_c, d_s = dev(templates), dev(coeff), dev(buf)
    capi.dev.template_subtract(d_t.data_ptr(), nt, first, n_samp, rows, d_s.data_ptr(), d_c.data_ptr())
    torch.cuda.synchronize()
    got = d_s.cpu().numpy()
    wrong = [d for d in range(n_det)
             if not np.array_equal(bits(got[rows[d]]), bits(gc.subtract_expected(buf[rows[d]], templates, coeff[d], first)))]
    others = np.setdiff1d(np.arange(n_det + 3), rows)
    print(f"(d) n_det {n_det} n_template {nt} first {first} n_samp {n_samp}: {len(wrong)} rows differ {wrong[:8]}")
    assert not wrong
    assert others.size == 3 and np.array_equal(bits(got[others]), bits(buf[others]))
    assert np.any(got[rows] != buf[rows])
    # first_template >= n_template changes nothing
    for beyond in (nt, nt + 5):
        capi.dev.template_subtract(d_t.data_ptr(), nt, beyond, n_samp, rows, d_s.data_ptr(), d_c.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_s.cpu().numpy()), bits(got))


@pytest.mark.parametrize("nt,first", SUBTRACT_TEMPLATES)
@pytest.mark.parametrize("n_det", SUBTRACT_DETS)
def test_subtract_bit_for_bit(n_det, nt, first):
    check_subtract(n_det, nt, first, 1000)


@pytest.mark.parametrize("n_samp", [1, 255, 256, 257])
def test_subtract_bit_for_bit_tile_edges(n_samp):
    check_subtract(33, 19, 3, n_samp)


# ------------------------------------------------------------------------------------------------ (e) builders
BUILDER_LENGTHS = (1, 255, 256, 257, 1000)


def abscissas(n):
    """Sorted in [-1, 1] with exactly -1, 0 and 1 among them (one each where a single sample is all there is)."""
    if n == 1:
        return [np.array([v]) for v in (-1.0, 0.0, 1.0)]
    x = np.sort(np.random.default_rng(n).uniform(-1, 1, n))
    x[0], x[n // 2], x[-1] = -1.0, 0.0, 1.0
    return [x]


@pytest.mark.parametrize("n_samp", BUILDER_LENGTHS)
def test_legendre_bit_for_bit(n_samp):
    import torch

    from oracle import ground_filter as GF
    from toast_amd import capi

    for x in abscissas(n_samp):
        assert x.size == n_samp and (n_samp == 1 or {-1.0, 0.0, 1.0} <= set(x))
        d_x = dev(x)
        for start, stop in LEGENDRE_SPANS + ((2, 3), (5, 6), (0, 65)):
            out = torch.full((stop - start + 1, n_samp), float("nan"), dtype=torch.float64, device="cuda")
            capi.dev.legendre_templates(d_x.data_ptr(), n_samp, start, stop, out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = GF.legendre_templates(x, start, stop)
            differ = np.count_nonzero(bits(got[:-1]) != bits(want))
            print(f"(e) legendre n_samp {n_samp} x[0] {x[0]} orders [{start}, {stop}): {differ} of {want.size} values differ")
            assert differ == 0 and np.all(np.isnan(got[-1]))
        # stop_order <= start_order writes nothing
        out = torch.full((2, n_samp), float("nan"), dtype=torch.float64, device="cuda")
        for start, stop in ((3, 3), (4, 2), (0, 0)):
            capi.dev.legendre_templates(d_x.data_ptr(), n_samp, start, stop, out.data_ptr())
        torch.cuda.synchronize()
        assert np.all(np.isnan(out.cpu().numpy()))


@pytest.mark.parametrize("n_samp", BUILDER_LENGTHS)
def test_template_select_bit_for_bit(n_samp):
    import torch

    from toast_amd import capi

    rng = np.random.default_rng(500 + n_samp)
    value = -2
    key = rng.integers(-3, 3, n_samp).astype(np.int32)
    key[0] = value
    if n_samp > 1:
        key[-1] = -2147483648
    src = rng.standard_normal(n_samp)
    src[n_samp // 2] = -0.0
    d_key, d_src = dev(key), dev(src)
    for with_src in (False, True):
        for keep_equal in (False, True):
            for v in (value, 0, 7):                        # 7: a value no key has
                out = torch.full((n_samp + 64,), float("nan"), dtype=torch.float64, device="cuda")
                capi.dev.template_select(d_src.data_ptr() if with_src else 0, d_key.data_ptr(), v, keep_equal, n_samp,
                                         out.data_ptr())
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                keep = (key == v) if keep_equal else (key != v)
                want = np.where(keep, src if with_src else 1.0, 0.0)
                assert np.array_equal(bits(got[:n_samp]), bits(want)), (n_samp, with_src, keep_equal, v)
                assert np.all(np.isnan(got[n_samp:]))
    print(f"(e) select n_samp {n_samp}: keys {key.min()} .. {key.max()}, {np.count_nonzero(key == value)} equal to {value}")


# ------------------------------------------------------------------------------------------------ (f) operator
def test_operator_beyond_the_first_block(oracle):
    """27 templates (5 trend + 2 x 11 split): ``k_template_project<32,2>``, the pair loop of the flagged Gram kernel, two
    subtract tiles with ``first_template = 5``; 35 detectors: a second subtract block and register pass; 70001 samples: a
    second slice of both Gram kernels."""
    from oracle import ground_filter as GF
    from test_gpu_ground_filter import inject_ground
    from toast_amd import ops
    from toast_amd.data import defaults
    from toast_amd.sim import create_ground_data

    rng = np.random.default_rng(32)
    data = create_ground_data(n_det=35, n_samp=70001, rate=20.0)
    inject_ground(data, rng)
    for ob in data.obs:
        fl = ob.detdata[defaults.det_flags].data
        fl |= (rng.random(fl.shape) < 0.01).astype(np.uint8)
    before = {ob.name: ob.detdata[defaults.det_data].data.copy() for ob in data.obs}
    gf = ops.GroundFilter(trend_order=5, filter_order=10, split_template=True, detrend=False, name="gf")
    gf.apply(data)
    print(f"(f) ngood {gf.ngood} nsingular {gf.nsingular}")
    assert gf.ngood == 35 and gf.nsingular == 0
    for ob in data.obs:
        n = ob.n_local_samples
        lr = np.zeros(n, dtype=bool)
        rl = np.zeros(n, dtype=bool)
        for iv in ob.intervals[defaults.throw_leftright_interval]:
            lr[iv.first:iv.last] = True
        for iv in ob.intervals[defaults.throw_rightleft_interval]:
            rl[iv.first:iv.last] = True
        templates = GF.build_templates(n, ob.shared[defaults.azimuth].data, 5, 10, bin_width=None, split=True, lr_mask=lr,
                                       rl_mask=rl)
        assert templates.shape == (27, 70001)
        want = before[ob.name].copy()
        failed = GF.apply(want, ob.detdata[defaults.det_flags].data, 1, ob.shared[defaults.shared_flags].data, 1, templates,
                          5, False)
        assert failed == []
        got = ob.detdata[defaults.det_data].data
        worst, scale = np.max(np.abs(got - want)), np.max(np.abs(before[ob.name]))
        print(f"(f) {ob.name}: max |device - oracle| {worst:.3e}, bound {1e-9 * scale:.3e}")
        assert worst < 1e-9 * scale
        good = (ob.shared[defaults.shared_flags].data & 1) == 0
        for i, det in enumerate(ob.local_detectors):
            g = good & ((ob.detdata[defaults.det_flags][det] & 1) == 0)
            old_rms, new_rms = np.std(before[ob.name][i][g]), np.std(got[i][g])
            assert new_rms < 0.4 * old_rms and new_rms < 1.1
