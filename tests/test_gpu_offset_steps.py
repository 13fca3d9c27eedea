"""GPU: the offset (baseline) template kernels at every baseline length of R.STEPS and every view shape of R.VIEW_CASES,
against the extended-precision statements and derived bounds of tests/nnz_reference.py (its docstring has the
derivations; tests/test_nnz_reference_host.py holds the CPU oracle to them and shows, with the baseline boundaries moved
by one sample, that they can fail).  The baseline length sets the run length of the segmented wave reduction (which DPP
steps run), where lanes of the two-samples-per-lane kernels hand a sample to their neighbour, how many workgroups add
into one amplitude, and which kernel is chosen at all:

  entry                                  instantiation                                   reached by
  offset_accumulate (cached, nnz 3)      k_offset_accumulate_v2<2 | 1, false>            even n_samp, vec2 = 1, pair = 1 | 0
                                         k_offset_accumulate<3, 2 | 1>                   odd_n_samp, or vec2 = 0
  offset_accumulate (cached, nnz 1)      k_offset_accumulate<1, 2 | 1>                   pair = 1 | 0
  offset_clean_accumulate (cached)       k_offset_accumulate_v2<2 | 1, true>             nnz 3 and even n_samp only: elsewhere the
                                                                                         call raises, which is asserted
  offset_scan_project(_signal) (cached)  k_offset_scan_project_v2<false | true>          nnz 3, even n_samp, vec2 = 1
                                         k_offset_scan_project<3 | 1, false | true>      odd_n_samp, vec2 = 0, nnz 1
  otf_offset_* (I, IQU, compact IQU)     k_otf_accumulate / k_otf_scan<.., SIG 1 | 2,    pair = 1 | 0 (E = 2 | 1; the compact scan is
                                         PIX 0 | 1, E>                                   always E = 1); no two-sample form exists
  offset_add_to_signal_multi             k_offset_add_to_signal
  template_offset_project_signal         k_offset_project_signal | _det                  default | deterministic mode
  offset_count_flagged                   k_offset_count_flagged | 16                     step < 16 | step >= 16
  offset_accumulate_packed               k_offset_accumulate_pk<2 | 1>                   pair words off, pair = 1 | 0
                                         k_offset_accumulate_pr<false, false | true>     pair words on, step < 128 | >= 128
  offset_scan_project_packed             k_offset_scan_project_pk                        pair words off
                                         k_offset_scan_project_pr<false, false | true>   pair words on, step < 128 | >= 128

fastdiv sees d = 1, powers of two and other divisors through the grid.  Not reachable in one process: the one-byte flag
count at step >= 16 (TOAST_HIP_COUNT_FLAGGED16=0) and the per-lane amplitude look-up at step >= 128
(TOAST_HIP_PACKED_UNIFORM_AMPS=0 -- tests/test_gpu_packed.py compares the two forms in a child process): both switches
are read from the environment.  The float32 pair-sum forms (k_*_pr<true, .>) stay with tests/test_gpu_packed.py."""
import numpy as np
import pytest

import nnz_reference as R
from test_gpu_nnz import dev, fused_accumulate, fused_scan_project, fused_scan_project_signal, fused_setup, tune

pytestmark = pytest.mark.gpu

VIEWS = list(R.VIEW_CASES)
#: (pointing on the fly, nnz, from the compact pixel cache)
POINTINGS = {"cached_I": (False, 1, False), "cached_IQU": (False, 3, False), "otf_I": (True, 1, False),
             "otf_IQU": (True, 3, False), "otf_IQU_compact": (True, 3, True)}


@pytest.fixture(scope="module")
def hip():
    from toast_amd import capi

    assert capi.accel_enabled(), "no HIP device visible"
    capi.accel_assign_device(1, 0, 1.0, False)
    yield capi
    capi.set_tuning("pair", 1)
    capi.set_tuning("vec2", 1)
    capi.set_tuning("det_major", 0)


def offset_inputs(c, step, seed=8):
    """(layout, amplitudes, amplitude flags, what the output amplitudes hold) of one step: the first amplitude at
    offset 5, three spare ones at the end, about 5 % flagged."""
    lay = R.offset_layout(c, step)
    rng = np.random.default_rng(seed)
    amps = rng.standard_normal(lay[2])
    aflags = (rng.random(lay[2]) < 0.05).astype(np.uint8)
    return lay, amps, aflags, rng.standard_normal(lay[2])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


# ------------------------------------------------------------------------------------------ fused halves
def compact_descriptor(torch, hip, s, c, pt, nnz):
    """The on-the-fly descriptor of ``s`` with the int32 local-pixel cache (as tests/test_gpu_otf.py builds it)."""
    n_samp = c["n_samp"]
    pix = dev(torch, pt["pixels"])
    cp = torch.full((c["rows"], n_samp), -9, dtype=torch.int32, device="cuda")
    hip.dev.compact_pixels(s["g2l"].data_ptr(), c["n_pix_submap"], pt["n_local"], c["pixel_index"], pix.data_ptr(),
                           c["pixel_index"], cp.data_ptr(), n_samp, c["intervals"])
    torch.cuda.synchronize()
    s["compact"] = cp
    s["pt"] = hip.otf_pointing(s["bore"].data_ptr(), c["focalplane"], c["nside"], True, nnz,
                               d_shared_flags=s["sfl"].data_ptr(), n_shared_flags=c["shared_flags"].size, shared_flag_mask=1,
                               d_hwp=s["hwp"].data_ptr(), n_hwp=c["hwp"].size, epsilon=c["epsilon"], gamma=c["gamma"],
                               cal=c["cal"], IAU=False, d_compact_pixels=cp.data_ptr(), compact_index=c["pixel_index"])


def fused_clean_accumulate(hip, s, c, nnz, otf, lay, d_amps, d_afl, d_z, d_sig, step):
    n_amp_views, amp_offsets, _ = lay
    n_samp = c["n_samp"]
    if otf:
        hip.dev.otf_offset_clean_accumulate(s["pt"], step, amp_offsets, n_amp_views, d_amps.data_ptr(), d_afl.data_ptr(),
                                            s["g2l"].data_ptr(), d_z.data_ptr(), c["n_pix_submap"], c["data_index"],
                                            d_sig.data_ptr(), c["flag_index"], s["dfl"].data_ptr(), s["n_flag"],
                                            c["det_scale"], 1, n_samp, c["intervals"], s["sfl"].data_ptr(),
                                            c["shared_flags"].size, 1)
    else:
        hip.dev.offset_clean_accumulate(step, amp_offsets, n_amp_views, d_amps.data_ptr(), d_afl.data_ptr(),
                                        s["g2l"].data_ptr(), d_z.data_ptr(), c["n_pix_submap"], nnz, c["pixel_index"],
                                        s["pix"].data_ptr(), c["weight_index"], s["wts"].data_ptr(), c["data_index"],
                                        d_sig.data_ptr(), c["flag_index"], s["dfl"].data_ptr(), s["n_flag"], c["det_scale"], 1,
                                        n_samp, c["intervals"], s["sfl"].data_ptr(), c["shared_flags"].size, 1)


@pytest.mark.parametrize("pointing", list(POINTINGS))
@pytest.mark.parametrize("name", VIEWS)
def test_fused_halves_at_every_step(hip, oracle, name, pointing):
    """offset_accumulate (gamma(n + 2) S), offset_scan_project and offset_scan_project_signal (gamma(n + nnz + 2) S),
    offset_clean_accumulate (gamma(n + 3) S) and their on-the-fly forms, per map element / amplitude, in every tuning;
    what receives nothing keeps its bits and the inputs are only read."""
    import torch

    otf, nnz, compact = POINTINGS[pointing]
    c, pt = R.pointing(oracle, name)
    tune(hip)
    s, pt, w = fused_setup(torch, hip, c, pt, nnz, otf)
    if compact:
        compact_descriptor(torch, hip, s, c, pt, nnz)
    zmap0 = R.seeded_map((pt["n_local"], c["n_pix_submap"], nnz), np.float64, seed=5)
    m = R.seeded_map(zmap0.shape, np.float64, seed=9)
    d_map, d_sig = dev(torch, m), dev(torch, c["tod"])
    can_clean = otf or (nnz == 3 and c["n_samp"] % 2 == 0)
    if not can_clean:
        lay, amps, aflags, _ = offset_inputs(c, 37)
        d_z = dev(torch, zmap0)
        with pytest.raises(RuntimeError, match="offset_clean_accumulate"):
            fused_clean_accumulate(hip, s, c, nnz, otf, lay, dev(torch, amps), dev(torch, aflags), d_z, d_sig, 37)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_z.cpu().numpy()), bits(zmap0))
    for step in R.STEPS:
        lay, amps, aflags, out0 = offset_inputs(c, step)
        n_amp_views, amp_offsets, n_amp = lay
        ref_z = R.offset_accumulate(c, pt, w, nnz, zmap0, step, n_amp_views, amp_offsets, amps, aflags)
        ref_a = R.offset_scan_project(c, pt, w, nnz, m, step, n_amp_views, amp_offsets, amps, aflags, out0, c["det_scale"], 4)
        ref_s = R.offset_scan_project(c, pt, w, nnz, m, step, n_amp_views, amp_offsets, amps, aflags, out0, c["det_scale"], 4,
                                      signal=c["tod"])
        ref_c = R.offset_clean_accumulate(c, pt, w, nnz, zmap0, step, n_amp_views, amp_offsets, amps, aflags, c["tod"])
        assert ref_z.n.sum() > 0 and ref_a.n.sum() > 0 and ref_s.n.sum() > 0 and ref_c.n.sum() > 0
        d_amps, d_afl = dev(torch, amps), dev(torch, aflags)
        for pair in (1, 0):
            for vec2 in (1, 0):
                tune(hip, pair=pair, vec2=vec2)
                d_z, d_out, d_rhs, d_cz = dev(torch, zmap0), dev(torch, out0), dev(torch, out0), dev(torch, zmap0)
                fused_accumulate(hip, s, c, nnz, otf, lay, d_amps, d_afl, d_z, step)
                fused_scan_project(hip, s, c, nnz, otf, lay, d_amps, d_afl, d_out, d_map, step)
                fused_scan_project_signal(hip, s, c, nnz, otf, lay, d_sig, d_afl, d_rhs, d_map, step)
                if can_clean:
                    fused_clean_accumulate(hip, s, c, nnz, otf, lay, d_amps, d_afl, d_cz, d_sig, step)
                torch.cuda.synchronize()
                wz = ref_z.excess(d_z.cpu().numpy())
                wa = ref_a.excess(d_out.cpu().numpy(), extra=nnz + 2)
                ws = ref_s.excess(d_rhs.cpu().numpy(), extra=nnz + 2)
                wc = ref_c.excess(d_cz.cpu().numpy(), extra=3) if can_clean else 0.0
                print(f"fused {name} {pointing} step={step} pair={pair} vec2={vec2}: accumulate {wz:.3g}, scan_project "
                      f"{wa:.3g}, scan_project_signal {ws:.3g}, clean_accumulate {wc:.3g} of the bound")
                assert wz <= 1.0 and wa <= 1.0 and ws <= 1.0 and wc <= 1.0, (step, pair, vec2)
        # read-only inputs
        assert np.array_equal(bits(d_amps.cpu().numpy()), bits(amps)) and np.array_equal(d_afl.cpu().numpy(), aflags)
    assert np.array_equal(bits(d_sig.cpu().numpy()), bits(c["tod"]))
    assert np.array_equal(bits(d_map.cpu().numpy()), bits(m))


# ------------------------------------------------------------------------------------------ plain kernels
@pytest.mark.parametrize("name", VIEWS)
def test_add_to_signal_at_every_step(hip, oracle, name):
    """offset_add_to_signal_multi through a permuted data_index into a buffer with one more row than detectors: every bit
    of the result is the reference's -- the unused row and the samples outside the views hold what they held."""
    import torch

    c, _ = R.pointing(oracle, name)
    n_samp, n_det = c["n_samp"], c["n_det"]
    rng = np.random.default_rng(21)
    tod = rng.standard_normal((n_det + 1, n_samp))
    c2 = dict(c, data_index=rng.permutation(n_det + 1)[:n_det].astype(np.int32), tod=tod)
    for step in R.STEPS:
        (n_amp_views, amp_offsets, n_amp), amps, aflags, _ = offset_inputs(c, step)
        want = R.offset_add_to_signal(c2, step, n_amp_views, amp_offsets, amps, aflags, tod)
        d_tod, d_amps, d_afl = dev(torch, tod), dev(torch, amps), dev(torch, aflags)
        hip.dev.offset_add_to_signal_multi(step, amp_offsets, n_amp_views, d_amps.data_ptr(), d_afl.data_ptr(),
                                           c2["data_index"], d_tod.data_ptr(), n_samp, c["intervals"])
        torch.cuda.synchronize()
        got = d_tod.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), step
        assert not np.array_equal(got, tod), step


def project_all(impl, c, step, lay, amps0, aflags, use_flags, tail=()):
    n_amp_views, amp_offsets, _ = lay
    out = amps0.copy()
    for d in range(c["n_det"]):
        impl.template_offset_project_signal(int(c["data_index"][d]), c["tod"], int(c["flag_index"][d]) if use_flags else -1,
                                            c["det_flags"], 4, step, int(amp_offsets[d]), n_amp_views, out, aflags,
                                            c["intervals"], *tail)
    return out


@pytest.mark.parametrize("name", VIEWS)
def test_project_signal_at_every_step(hip, oracle, name):
    """template_offset_project_signal without (flag_index -1) and with detector flags: gamma(n) S per amplitude against the
    sum of the raw samples; amplitudes that receive nothing -- flagged, before the first, the spare ones -- keep their bits."""
    c, _ = R.pointing(oracle, name)
    for step in R.STEPS:
        lay, _, aflags, amps0 = offset_inputs(c, step)
        for use_flags in (False, True):
            ref = R.offset_project_signal(c, step, lay[0], lay[1], amps0, aflags, 4, use_flags)
            assert ref.n.sum() > 0
            worst = ref.excess(project_all(hip, c, step, lay, amps0, aflags, use_flags, tail=(False,)), extra=0)
            print(f"project_signal {name} step={step} flags={use_flags}: {worst:.3g} of the bound")
            assert worst <= 1.0, (step, use_flags)


@pytest.mark.parametrize("name", VIEWS)
def test_deterministic_project_signal_at_every_step(hip, oracle, name):
    """Deterministic mode (k_offset_project_signal_det: one thread per amplitude, samples in increasing order): the bits of
    the oracle's host loop at the whole grid."""
    c, _ = R.pointing(oracle, name)
    hip.set_deterministic(True)
    try:
        for step in R.STEPS:
            lay, _, aflags, amps0 = offset_inputs(c, step)
            for use_flags in (False, True):
                got = project_all(hip, c, step, lay, amps0, aflags, use_flags, tail=(False,))
                want = project_all(oracle, c, step, lay, amps0, aflags, use_flags)
                assert np.array_equal(bits(got), bits(want)), (step, use_flags)
                assert not np.array_equal(got, amps0)
    finally:
        hip.set_deterministic(False)


def test_project_signal_refuses_mixed_flag_indices(hip, oracle):
    """flag_index with negative and non-negative rows: whether flags are used is decided once per call, so a negative row
    among valid ones would be read before the flag buffer.  The call raises before any launch; nothing is written."""
    import torch

    c, _ = R.pointing(oracle, "odd_dets_odd_starts")
    (n_amp_views, amp_offsets, n_amp), _, aflags, amps0 = offset_inputs(c, 37)
    d_out, d_tod, d_fl, d_afl = dev(torch, amps0), dev(torch, c["tod"]), dev(torch, c["det_flags"]), dev(torch, aflags)
    for fidx in ([0, -1, 2, 3, 4], [-1, 1, 2, 3, 4]):
        with pytest.raises(RuntimeError, match="flag_index mixes"):
            hip.dev.offset_project_signal_multi(c["data_index"], d_tod.data_ptr(), np.array(fidx, dtype=np.int32),
                                                d_fl.data_ptr(), 4, 37, amp_offsets, n_amp_views, d_out.data_ptr(),
                                                d_afl.data_ptr(), c["n_samp"], c["intervals"])
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(amps0))
    # all rows negative: no flags, as before
    ref = R.offset_project_signal(c, 37, n_amp_views, amp_offsets, amps0, aflags, 4, False)
    hip.dev.offset_project_signal_multi(c["data_index"], d_tod.data_ptr(), np.full(c["n_det"], -1, dtype=np.int32),
                                        d_fl.data_ptr(), 4, 37, amp_offsets, n_amp_views, d_out.data_ptr(), d_afl.data_ptr(),
                                        c["n_samp"], c["intervals"])
    torch.cuda.synchronize()
    assert ref.excess(d_out.cpu().numpy(), extra=0) <= 1.0


# ------------------------------------------------------------------------------------------ set-up kernels
@pytest.mark.parametrize("name", VIEWS)
def test_count_flagged_at_every_step(hip, oracle, name):
    """offset_count_flagged with no, 30 % and all samples flagged, the mask bit (4) mixed with other bits, flag rows through
    a permuted flag_index: exactly the reference's integers.  Steps below 16 run k_offset_count_flagged (one byte per
    lane), steps from 16 up k_offset_count_flagged16 (sixteen bytes per lane, split between two baselines); the switch
    that keeps the one-byte form at every step is read from the environment once per process and is not exercised."""
    import torch

    c, _ = R.pointing(oracle, name)
    n_samp, n_det = c["n_samp"], c["n_det"]
    rng = np.random.default_rng(22)
    c2 = dict(c, flag_index=rng.permutation(n_det + 1)[:n_det].astype(np.int32))
    for density in (0.0, 0.3, 1.0):
        on = rng.random((n_det + 1, n_samp)) < density
        flags = np.where(on, rng.choice([4, 5, 6, 7, 12, 255], on.shape), rng.choice([0, 1, 2, 3, 8, 251], on.shape))
        flags = np.ascontiguousarray(flags.astype(np.uint8))
        d_flags = dev(torch, flags)
        for step in R.STEPS:
            n_amp_views, amp_offsets, n_amp = R.offset_layout(c, step)
            want = R.offset_count_flagged(c2, step, n_amp_views, amp_offsets, 4, n_amp, det_flags=flags)
            d_counts = torch.zeros(n_amp, dtype=torch.float64, device="cuda")
            hip.dev.offset_count_flagged(step, amp_offsets, n_amp_views, d_counts.data_ptr(), c2["flag_index"],
                                         d_flags.data_ptr(), 4, n_samp, c["intervals"])
            torch.cuda.synchronize()
            got = d_counts.cpu().numpy()
            assert np.array_equal(got, want.astype(np.float64)), (density, step)
            assert (want.sum() > 0) == (density > 0)


@pytest.mark.parametrize("n_len", (1, 255, 256, 257, 1024 * 256 + 5))
def test_variance_on_crafted_counts(hip, n_len):
    """offset_variance: baselines of 0, 1 and 8 samples, counts that are integers and counts a few ulp off them (the kernel
    rounds them), a good fraction that n_good / len hits exactly (cut), misses by one ulp from above (kept) and from below
    (cut), detector weights 0, negative and positive, and more baselines than the grid's 1024 x 256 threads.  Flags and
    variances are the reference's, bit for bit; amplitudes of no detector are not written."""
    import torch

    step = 8
    rng = np.random.default_rng(23)
    det_weight = np.array([0.0, -1.5, 0.7, 2.25])
    n_det = det_weight.size
    amp_len = rng.choice([0, 1, step], n_len).astype(np.int64)
    amp_len[0] = step
    n_bad = np.floor(rng.random((n_det, n_len)) * (amp_len[None, :] + 1))
    n_bad[:, 0] = 6.0                                            # n_good / len = 2 / 8
    off = rng.integers(-3, 4, n_bad.shape)
    n_bad = np.where(n_bad > 0, n_bad * (1.0 + off * np.finfo(np.float64).eps), np.where(off > 0, 1e-300, 0.0))
    assert np.any(n_bad != np.rint(n_bad)) and np.all(np.abs(n_bad - np.rint(n_bad)) < 1e-12)
    amp_offsets = 2 + np.arange(n_det, dtype=np.int64) * n_len
    total = 2 + n_det * n_len + 3
    own = np.zeros(total, dtype=bool)
    own[2:2 + n_det * n_len] = True
    d_bad = torch.zeros(total, dtype=torch.float64, device="cuda")
    d_bad[2:2 + n_det * n_len] = dev(torch, n_bad.reshape(-1))
    seen = []
    for good_fraction in (0.25, np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0), 0.0, 1.0):
        want_flags, want_var = R.offset_variance(n_bad, amp_len, det_weight, good_fraction)
        seen.append(int(want_flags[2, 0]))
        d_flags = torch.full((total,), 7, dtype=torch.uint8, device="cuda")
        d_var = torch.full((total,), -3.0, dtype=torch.float64, device="cuda")
        hip.dev.offset_variance(amp_offsets, det_weight, amp_len, d_bad.data_ptr(), good_fraction, d_flags.data_ptr(),
                                d_var.data_ptr())
        torch.cuda.synchronize()
        flags, var = d_flags.cpu().numpy(), d_var.cpu().numpy()
        assert np.array_equal(flags[own], want_flags.reshape(-1)), good_fraction
        assert np.array_equal(bits(var[own]), bits(want_var.reshape(-1))), good_fraction
        assert np.all(flags[~own] == 7) and np.all(var[~own] == -3.0)
        assert np.all(want_flags[:2] == 1) and np.all(want_flags[:, amp_len == 0] == 1)
    assert seen == [1, 0, 1, 0, 1]       # 2 / 8 against 0.25, one ulp less, one ulp more, 0 and 1


@pytest.mark.parametrize("n_amp", (1, 255, 256, 257, 256 * 4096 + 3))
def test_apply_diag_precond(hip, n_amp):
    """template_offset_apply_diag_precond below, at and above a workgroup and above the 256 x 4096 threads of the grid:
    the bits of where(flags == 0, in * var, 0)."""
    rng = np.random.default_rng(24)
    var, amps_in = rng.random(n_amp) + 0.1, rng.standard_normal(n_amp)
    flags = (rng.random(n_amp) < 0.2).astype(np.uint8) * rng.integers(1, 256, n_amp).astype(np.uint8)
    out = np.full(n_amp, -7.0)
    hip.template_offset_apply_diag_precond(var, amps_in, flags, out, False)
    assert np.array_equal(bits(out), bits(np.where(flags == 0, amps_in * var, 0.0)))


# ------------------------------------------------------------------------------------------ packed sweeps
def packed_case(hip, oracle, view):
    """(set-up in the form of tests/test_gpu_packed.py, case and pointing in the form of nnz_reference) of the long odd
    view on the oracle's pointing, or of the packed tests' own three odd views (pointing expanded on the device, one
    hit submap left out of the local map)."""
    import torch

    from test_gpu_packed import _setup

    if view == "packed_odd_views":
        s = _setup(n_det=5)
        host = lambda k: s[k].cpu().numpy()      # noqa: E731
        c = dict(n_det=s["n_det"], n_samp=s["n_samp"], intervals=s["ivl"], n_pix_submap=s["nps"], pixel_index=s["idx"],
                 weight_index=s["idx"], flag_index=s["idx"], data_index=s["idx"], det_flags=host("d_dflags"),
                 shared_flags=host("d_sflags"), det_scale=s["detw"])
        pt = dict(pixels=host("d_pix"), weights=host("d_w"), g2l=host("d_g2l"), n_local=s["n_local"])
        return s, c, pt, host("d_pflags")
    c, pt = R.pointing(oracle, view)
    t = lambda a: dev(torch, a)      # noqa: E731
    pflags = (np.random.default_rng(25).random((c["rows"], c["n_samp"])) < 0.05).astype(np.uint8)
    idx = np.arange(c["n_det"], dtype=np.int32)
    s = dict(D=hip.dev, torch=torch, dev=torch.device("cuda", 0), n_det=c["n_det"], n_samp=c["n_samp"], nps=c["n_pix_submap"],
             n_local=pt["n_local"], idx=idx, ivl=c["intervals"], d_pix=t(pt["pixels"]), d_w=t(pt["weights"]),
             d_g2l=t(pt["g2l"]), d_dflags=t(c["det_flags"]), d_pflags=t(pflags), d_sflags=t(c["shared_flags"]),
             detw=c["det_scale"])
    return s, c, pt, pflags


@pytest.mark.parametrize("view", ["long_odd_view", "packed_odd_views"])
def test_packed_sweeps_at_every_step(hip, oracle, view):
    """offset_accumulate_packed and offset_scan_project_packed from per-detector words (both pair tunings) and from pair
    words, at every step of the grid from 15 up -- 127, 128 and 129 lie on both sides of the wave-uniform amplitude
    look-up -- against the statements of the sweeps over the original arrays: the packed kernels form the same products in
    the same order, with the I weight from ``cal`` (equal to weights[..., 0] in every sample, or the pack refuses) and
    Q / U from ``qu`` (copies), so gamma(n + 2) S per map element and gamma(n + 3 + 2) S per amplitude hold unchanged; the
    pair forms add the two detectors' terms of a sample first, one of the n additions."""
    import torch

    from test_gpu_packed import _pack

    tune(hip)
    s, c, pt, pflags = packed_case(hip, oracle, view)
    c_proj = dict(c, det_flags=pflags)
    w = np.ascontiguousarray(pt["weights"])
    ok, key, qu, cal = _pack(s)
    (ok_p, pair), key_p, qu_p, cal_p = _pack(s, pair_words=True)
    assert ok and ok_p and pair
    zmap0 = R.seeded_map((pt["n_local"], c["n_pix_submap"], 3), np.float64, seed=5)
    m = R.seeded_map(zmap0.shape, np.float64, seed=9)
    d_map = dev(torch, m)
    forms = (("words pair=1", 1, False, key, qu, cal), ("words pair=0", 0, False, key, qu, cal),
             ("pair words", 1, True, key_p, qu_p, cal_p))
    for step in (st for st in R.STEPS if st >= 15):
        lay, amps, aflags, out0 = offset_inputs(c, step)
        n_amp_views, amp_offsets, n_amp = lay
        ref_z = R.offset_accumulate(c, pt, w, 3, zmap0, step, n_amp_views, amp_offsets, amps, aflags, skip_non_local=True)
        ref_a = R.offset_scan_project(c_proj, pt, w, 3, m, step, n_amp_views, amp_offsets, amps, aflags, out0, s["detw"], 1)
        assert ref_z.n.sum() > 0 and ref_a.n.sum() > 0
        d_amps, d_afl = dev(torch, amps), dev(torch, aflags)
        for label, pair_tuning, pair_words, k, q, cl in forms:
            tune(hip, pair=pair_tuning)
            d_z, d_out = dev(torch, zmap0), dev(torch, out0)
            hip.dev.offset_accumulate_packed(step, amp_offsets, n_amp_views, d_amps.data_ptr(), d_afl.data_ptr(),
                                             d_z.data_ptr(), k.data_ptr(), q.data_ptr(), cl.data_ptr(), s["detw"], c["n_samp"],
                                             c["intervals"], pair_words=pair_words)
            hip.dev.offset_scan_project_packed(step, amp_offsets, n_amp_views, d_amps.data_ptr(), d_out.data_ptr(),
                                               d_afl.data_ptr(), d_map.data_ptr(), k.data_ptr(), q.data_ptr(), cl.data_ptr(),
                                               s["detw"], c["n_samp"], c["intervals"], pair_words=pair_words)
            torch.cuda.synchronize()
            wz, wa = ref_z.excess(d_z.cpu().numpy()), ref_a.excess(d_out.cpu().numpy(), extra=3 + 2)
            print(f"packed {view} step={step} {label}: accumulate {wz:.3g}, scan_project {wa:.3g} of the bound")
            assert wz <= 1.0 and wa <= 1.0, (step, label)
        assert np.array_equal(bits(d_amps.cpu().numpy()), bits(amps)) and np.array_equal(d_afl.cpu().numpy(), aflags)
    assert np.array_equal(bits(d_map.cpu().numpy()), bits(m))
