"""The extended-precision references of tests/nnz_reference.py and their derived rounding bounds against the CPU oracle,
on every case the GPU tests of tests/test_gpu_nnz.py run: the oracle's plain fp64 loops must stay inside the bounds
without exception, for every nnz, map type and mode.  A failure here means a bound or a reference is wrong -- before a
GPU sees either."""
import numpy as np
import pytest

import nnz_reference as R


@pytest.mark.parametrize("nnz", R.NNZ)
@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_build_noise_weighted_is_inside_the_bound(oracle, name, nnz):
    c, pt = R.pointing(oracle, name)
    w = R.weights_nnz(pt["weights"], nnz)
    zmap0 = R.seeded_map((pt["n_local"], c["n_pix_submap"], nnz), np.float64, seed=5)
    ref = R.build_noise_weighted(c, pt, w, nnz, zmap0)
    assert ref.n.sum() > 0
    z = zmap0.copy()
    oracle.build_noise_weighted(pt["g2l"], z, c["pixel_index"], pt["pixels"], c["weight_index"],
                                w.reshape(w.shape[0], w.shape[1], nnz), c["data_index"], c["tod"], c["flag_index"],
                                c["det_flags"], c["det_scale"], 1, c["intervals"], c["shared_flags"], 1)
    assert ref.excess(z) <= 1.0
    # the bound is not vacuous: one dropped sample (of average size) of the faintest hit pixel is outside it
    faint = int(np.argmin(ref.mag.max(axis=1)))
    k = int(np.argmax(ref.mag[faint]))
    dropped = z.reshape(ref.initial.shape).copy()
    dropped[ref.idx[faint], k] -= float((ref.mag[faint, k] - abs(ref.initial[ref.idx[faint], k])) / ref.n[faint])
    assert ref.excess(dropped) > 1.0


@pytest.mark.parametrize("dtype", list(R.MAP_DTYPES))
@pytest.mark.parametrize("nnz", R.NNZ)
@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_scan_map_is_inside_the_bound(oracle, name, nnz, dtype):
    c, pt = R.pointing(oracle, name)
    w = R.weights_nnz(pt["weights"], nnz)
    m = R.seeded_map((pt["n_local"], c["n_pix_submap"], nnz), R.MAP_DTYPES[dtype])
    for mode, (zero, sub, mult) in R.SCAN_MODES.items():
        ref = R.scan_map(c, pt, w, nnz, m, c["tod"], 0.37, zero, sub, mult)
        t = c["tod"].copy()
        oracle.scan_map(pt["g2l"], c["n_pix_submap"], m, t, c["data_index"], pt["pixels"], c["pixel_index"],
                        w.reshape(w.shape[0], w.shape[1], nnz), c["weight_index"], c["intervals"], 0.37, zero, sub, mult)
        assert R.scan_excess(t, ref, nnz) <= 1.0, mode
        assert np.any(ref[1] > 0)
        if dtype != "f64":
            continue
        # a wrong sign of the map term is far outside the bound
        wrong = R.scan_map(c, pt, w, nnz, m, c["tod"], -0.37, zero, sub, mult)
        assert R.scan_excess(t, wrong, nnz) > 1.0, mode


@pytest.mark.parametrize("nnz", (1, 2, 3))
@pytest.mark.parametrize("name", list(R.CASES))
def test_numpy_inverse_covariance_is_inside_the_bound(oracle, name, nnz):
    """The oracle has no inverse-covariance kernel: the fp64 NumPy scatter of (w_j det_scale) w_k, the operation order of
    the reference's cov_accum_diag_invnpp, stands in for it."""
    c, pt = R.pointing(oracle, name)
    w = R.weights_nnz(pt["weights"], nnz)
    blk = nnz * (nnz + 1) // 2
    cov0 = R.seeded_map((pt["n_local"], c["n_pix_submap"], blk), np.float64, seed=6)
    ref = R.inverse_covariance(c, pt, w, nnz, cov0)
    got = cov0.copy().reshape(-1, blk)
    hits = np.zeros(got.shape[0], dtype=np.int64)
    nps = c["n_pix_submap"]
    s = R.view_samples(c)
    for d in range(c["n_det"]):
        p = pt["pixels"][c["pixel_index"][d]][s]
        good = p >= 0
        if c["det_flags"].shape[1] == c["n_samp"]:
            good &= (c["det_flags"][c["flag_index"][d], s] & 1) == 0
        if c["shared_flags"].size == c["n_samp"]:
            good &= (c["shared_flags"][s] & 1) == 0
        pg = p[good]
        loc = pt["g2l"][pg // nps] * nps + pg % nps
        wg = w[c["weight_index"][d]][s][good].reshape(pg.size, nnz)
        np.add.at(hits, loc, 1)
        off = 0
        for j in range(nnz):
            for k in range(j, nnz):
                np.add.at(got[:, off], loc, (wg[:, j] * c["det_scale"][d]) * wg[:, k])
                off += 1
    assert np.array_equal(hits, ref.counts())
    assert ref.excess(got) <= 1.0


@pytest.mark.parametrize("nnz", (1, 3))
@pytest.mark.parametrize("name", ["odd_dets_odd_starts", "single_det", "odd_n_samp"])
def test_oracle_operator_sequence_is_inside_the_fused_bounds(oracle, name, nnz):
    """offset_accumulate == add_to_signal + build_noise_weighted and offset_scan_project == add_to_signal +
    scan_map(subtract) + noise_weight + project_signal, run through the oracle's operators."""
    c, pt = R.pointing(oracle, name)
    w = R.weights_nnz(pt["weights"], nnz)
    w3 = w.reshape(w.shape[0], w.shape[1], nnz)
    step = 37
    n_amp_views, amp_offsets, n_amp = R.offset_layout(c, step)
    rng = np.random.default_rng(8)
    amps = rng.standard_normal(n_amp)
    aflags = (rng.random(n_amp) < 0.05).astype(np.uint8)
    zmap0 = R.seeded_map((pt["n_local"], c["n_pix_submap"], nnz), np.float64, seed=5)
    ref = R.offset_accumulate(c, pt, w, nnz, zmap0, step, n_amp_views, amp_offsets, amps, aflags)
    tod = np.zeros_like(c["tod"])
    for d in range(c["n_det"]):
        oracle.template_offset_add_to_signal(step, int(amp_offsets[d]), n_amp_views, amps, aflags, int(c["data_index"][d]),
                                             tod, c["intervals"])
    z = zmap0.copy()
    oracle.build_noise_weighted(pt["g2l"], z, c["pixel_index"], pt["pixels"], c["weight_index"], w3, c["data_index"], tod,
                                c["flag_index"], c["det_flags"], c["det_scale"], 1, c["intervals"], c["shared_flags"], 1)
    assert ref.n.sum() > 0
    assert ref.excess(z) <= 1.0
    # projection half, with a map that is not the accumulated one and amplitudes that hold something already
    m = R.seeded_map(zmap0.shape, np.float64, seed=9)
    out0 = rng.standard_normal(n_amp)
    ref = R.offset_scan_project(c, pt, w, nnz, m, step, n_amp_views, amp_offsets, amps, aflags, out0, c["det_scale"], 4)
    oracle.scan_map(pt["g2l"], c["n_pix_submap"], m, tod, c["data_index"], pt["pixels"], c["pixel_index"], w3,
                    c["weight_index"], c["intervals"], 1.0, False, True, False)
    oracle.noise_weight(tod, c["data_index"], c["intervals"], c["det_scale"])
    out = out0.copy()
    for d in range(c["n_det"]):
        oracle.template_offset_project_signal(int(c["data_index"][d]), tod, int(c["flag_index"][d]), c["det_flags"], 4, step,
                                              int(amp_offsets[d]), n_amp_views, out, aflags, c["intervals"])
    assert ref.excess(out, extra=nnz + 2) <= 1.0
    assert np.array_equal(out[:5], out0[:5]) and np.array_equal(out[-3:], out0[-3:])
    # the right-hand-side form: the same projection of a timestream, M^T N^-1 (d - A z)
    ref = R.offset_scan_project(c, pt, w, nnz, m, step, n_amp_views, amp_offsets, amps, aflags, out0, c["det_scale"], 4,
                                signal=c["tod"])
    tod = c["tod"].copy()
    oracle.scan_map(pt["g2l"], c["n_pix_submap"], m, tod, c["data_index"], pt["pixels"], c["pixel_index"], w3,
                    c["weight_index"], c["intervals"], 1.0, False, True, False)
    oracle.noise_weight(tod, c["data_index"], c["intervals"], c["det_scale"])
    out = out0.copy()
    for d in range(c["n_det"]):
        oracle.template_offset_project_signal(int(c["data_index"][d]), tod, int(c["flag_index"][d]), c["det_flags"], 4, step,
                                              int(amp_offsets[d]), n_amp_views, out, aflags, c["intervals"])
    assert ref.excess(out, extra=nnz + 2) <= 1.0


# ------------------------------------------------------------------------------------------ offset template, every step
def _offset_inputs(c, step, seed=8):
    n_amp_views, amp_offsets, n_amp = R.offset_layout(c, step)
    rng = np.random.default_rng(seed)
    amps = rng.standard_normal(n_amp)
    aflags = (rng.random(n_amp) < 0.05).astype(np.uint8)
    return n_amp_views, amp_offsets, n_amp, amps, aflags


def _longest_view(c):
    return max(int(v["last"]) - int(v["first"]) for v in c["intervals"])


@pytest.mark.parametrize("name", ["long_odd_view", "short_intervals"])
def test_oracle_offset_add_to_signal_equals_the_reference_at_every_step(oracle, name):
    """Bit equality at every baseline length, and the statement with every baseline boundary moved by one sample differs
    from the oracle wherever a view holds a boundary at all (step shorter than the view): the comparison can fail."""
    c, _ = R.pointing(oracle, name)
    for step in R.STEPS:
        n_amp_views, amp_offsets, n_amp, amps, aflags = _offset_inputs(c, step)
        tod = c["tod"].copy()
        for d in range(c["n_det"]):
            oracle.template_offset_add_to_signal(step, int(amp_offsets[d]), n_amp_views, amps, aflags,
                                                 int(c["data_index"][d]), tod, c["intervals"])
        want = R.offset_add_to_signal(c, step, n_amp_views, amp_offsets, amps, aflags, c["tod"])
        assert np.array_equal(tod, want), step
        assert not np.array_equal(tod, c["tod"]), step
        if step < _longest_view(c):
            wrong = R.offset_add_to_signal(c, step, n_amp_views, amp_offsets, amps, aflags, c["tod"], shift=1)
            assert not np.array_equal(tod, wrong), step


@pytest.mark.parametrize("fidx", ["no_flags", "flags"])
@pytest.mark.parametrize("name", ["long_odd_view", "short_intervals"])
def test_oracle_offset_project_signal_is_inside_the_bound_at_every_step(oracle, name, fidx):
    """gamma(n) S per amplitude at every baseline length, amplitudes that receive nothing keep their bits, and the
    statement with the boundaries moved by one sample is outside the bound for every step shorter than the view."""
    c, _ = R.pointing(oracle, name)
    use_flags = fidx == "flags"
    for step in R.STEPS:
        n_amp_views, amp_offsets, n_amp, amps0, aflags = _offset_inputs(c, step)
        out = amps0.copy()
        for d in range(c["n_det"]):
            oracle.template_offset_project_signal(int(c["data_index"][d]), c["tod"], int(c["flag_index"][d]) if use_flags else -1,
                                                  c["det_flags"], 4, step, int(amp_offsets[d]), n_amp_views, out, aflags,
                                                  c["intervals"])
        ref = R.offset_project_signal(c, step, n_amp_views, amp_offsets, amps0, aflags, 4, use_flags)
        assert ref.n.sum() > 0
        worst = ref.excess(out, extra=0)
        assert worst <= 1.0, (step, worst)
        if step < _longest_view(c):
            wrong = R.offset_project_signal(c, step, n_amp_views, amp_offsets, amps0, aflags, 4, use_flags, shift=1)
            assert wrong.excess(out, extra=0) > 1.0, step


def test_offset_count_and_variance_references_on_a_worked_example():
    """The two exact statements by hand: 7 samples in baselines of 3 (lengths 3, 3, 1), flags with the mask bit mixed with
    others; and the cut at exactly good_fraction."""
    c = dict(n_samp=9, n_det=1, intervals=R.intervals(((1, 8),)), flag_index=np.array([0], dtype=np.int32),
             det_flags=np.array([[1, 1, 0, 2, 3, 1, 0, 1, 1]], dtype=np.uint8))
    n_amp_views, amp_offsets, n_amp = R.offset_layout(c, 3, amp_offset=2, spare=1)
    assert list(n_amp_views) == [3] and n_amp == 6
    counts = R.offset_count_flagged(c, 3, n_amp_views, amp_offsets, 1, n_amp)
    assert list(counts) == [0, 0, 1, 2, 1, 0]
    flags, var = R.offset_variance(np.array([[1.0, 2.0000000000000004, 0.0, 0.0]]), [4, 4, 0, 1], [0.5], 0.5)
    assert flags.tolist() == [[0, 1, 1, 0]]
    assert var.tolist() == [[1.0 / (0.5 * 3.0), 0.0, 0.0, 2.0]]
    assert R.offset_variance(np.zeros((1, 1)), [5], [-1.0], 0.0)[0].tolist() == [[1]]
