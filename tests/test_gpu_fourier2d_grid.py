"""GPU: the Fourier2D kernels (csrc/fourier2d.hip) through the C ABI at every compiled width x every launch shape, against
the plain references of tests/focalplane_grid.py (see its docstring for the layout, the references and the derived
bound).  tests/test_gpu_fourier2d.py holds the same kernels to the fixture of the reference implementation, every width on
one layout and on a subset of the samples; tests/test_focalplane_grid_host.py holds the plain references to that fixture.
This file reaches what the fixture's layouts never take:

* nmode 5, 7, 17, 19, 37, 39, each with 1, 2, 5, 9 and 70 detectors (and once with a random table holding exact zeros) on
  one observation of 2401 samples whose views have 0, 1, 2, 3, 255, 256, 257, 511, 512 and 513 samples after clipping:
  14 sample tiles, two pairs of adjacent views, an empty view between two others, a view clipped at either end, amplitude
  blocks in another order than the views with sentinel slots between them;
* ``n_group`` 1, 2, 0 (the rule), n_det and n_det + 3: the split projection (``k_f2d_project<N, true>`` and
  ``k_f2d_combine``) at every width with groups of one detector up to 70 groups, judged on EVERY amplitude;
* the norms with flags and with a null flag pointer;
* the prior's three kernels on synthetic views: transforms of 2 to 1024 points (``n_fft < 64``: the early exit of
  ``k_f2d_gather``), odd and even tap counts, more taps than samples, 1, 5, 8, 39 and 40 modes (40: the LDS tile is full).

Bit equality (asserted as such): add_to_signal for every ``n_group``, project_signal whenever the launch has one group, the
norms, apply_precond; everything outside the views -- the sentinel row, the sentinel slots, the amplitudes of the samples
cut off a clipped view -- keeps its bits.

Worst observed figures on an MI355X (every test prints its own before it asserts):
    split project_signal       0.75 of gamma(n_det + 1) (|a0| + sum|s T|) + n_det 2^-63 sum|...|   (2 detectors in 2 groups,
                               37 modes; at most 0.52 with 5, 0.31 with 9 and 0.087 with 70 detectors).  With one detector
                               per group the split sum has the bits of the sequential one.
    groups by the rule         on the 14 tiles: 1 detector -> 1 group, 2 -> 1, 5 -> 2, 9 -> 3, 70 -> 18; n_det + 3 gives n_det
    add_prior                  d_ref (the reference's own call against the longdouble window) 1.4e-17 to 5.6e-16 max|out|
                               over the cases, so the bound 8 x max(d_ref, 2.85e-16) is 2.28e-15 to 4.44e-15 max|out|;
                               the device is at most 5.4e-16 max|out| away (L 65, F 128, 8 modes; d_ref 4.9e-16 there)
                               and reaches at most 0.23 of its bound (L 63, F 62, 8 modes: 5.25e-16, d_ref 1.5e-16).
                               The printed lines hold d_ref, the device's distance and the bound of all 60 cases.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import focalplane_grid as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "fourier2d.npz"), allow_pickle=False)
YARD = float(GOLD["yard_prior_max"])
N_TILE = G.f2d_tiles()


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)     # (its own host key)
        accel_data_create(self.a, "test_fourier2d_grid")
        accel_data_update_device(self.a, "test_fourier2d_grid")
        self.ptr = accel_device_ptr(self.a)

    def put(self, value):
        from toast_amd.accel import accel_data_update_device

        self.a[...] = value
        accel_data_update_device(self.a, "test_fourier2d_grid")

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_fourier2d_grid")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_fourier2d_grid")


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


@pytest.fixture
def dev():
    """Dev(array) whose device copies are released when the test ends, also when it fails."""
    made = []

    def make(arr):
        made.append(Dev(arr))
        return made[-1]

    yield make
    for d in made:
        d.free()


def _intervals(views):
    from toast_amd.capi import interval_dtype

    ivl = np.zeros(len(views), dtype=interval_dtype)
    ivl["first"], ivl["last"] = [v[0] for v in views], [v[1] for v in views]
    return ivl


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _cases(nmode):
    for n_det in G.F2D_NDETS:
        yield G.f2d_case(nmode, n_det)
    yield G.f2d_case(nmode, 5, "random")


def _layout(case):
    return case["nmode"], case["views"], case["n_samp"], case["offsets"]


def _group_counts(n_det):
    return (1, 2, 0, n_det, n_det + 3)


def test_the_rule_and_the_clipping_of_the_group_count():
    from toast_amd import capi

    groups = capi.dev.fourier2d_groups
    rule = {n_det: groups(n_det, N_TILE, 0) for n_det in G.F2D_NDETS}
    print(f"fourier2d groups by the rule on {N_TILE} tiles: {rule}")
    assert rule[1] == 1 and rule[2] == 1 and rule[5] == 2 and rule[9] == 3 and rule[70] > 1
    for n_det in G.F2D_NDETS:
        assert groups(n_det, N_TILE, 1) == 1
        assert groups(n_det, N_TILE, n_det) == n_det and groups(n_det, N_TILE, n_det + 3) == n_det
    assert groups(5, N_TILE, 2) == 2 and groups(9, N_TILE, 2) == 2 and groups(70, N_TILE, 2) == 2
    # enough sample tiles: the detectors stay in one group
    assert groups(70, 1024, 0) == 1 and groups(70, 1023, 0) == 2
    assert groups(0, N_TILE, 0) == 0 and groups(5, 0, 0) == 0


@pytest.mark.parametrize("nmode", G.F2D_NMODES)
def test_add_to_signal(nmode, dev):
    from toast_amd import capi

    for case in _cases(nmode):
        n_det = case["n_det"]
        want = G.f2d_add(case["signal"], case["rows"], case["T"], case["amps"], *_layout(case))
        unlisted = (set(range(n_det + 1)) - set(case["rows"])).pop()
        assert np.all(want[unlisted] == G.SENTINEL) and np.any(want[case["rows"][0]] != case["signal"][case["rows"][0]])
        d_sig, d_t, d_amps = dev(case["signal"]), dev(case["T"]), dev(case["amps"])
        ivl = _intervals(case["views"])
        for n_group in _group_counts(n_det):
            d_sig.put(case["signal"])
            capi.dev.fourier2d_add_to_signal(nmode, d_t.ptr, case["offsets"], d_amps.ptr, case["rows"], d_sig.ptr,
                                             case["n_samp"], ivl, n_group=n_group)
            got = d_sig.get()
            wrong = np.count_nonzero(_bits(got) != _bits(want))
            print(f"add_to_signal nmode {nmode} n_det {n_det} n_group {n_group}: {wrong} of {got.size} samples differ")
            assert wrong == 0
        assert np.array_equal(_bits(d_amps.get()), _bits(case["amps"]))


@pytest.mark.parametrize("nmode", G.F2D_NMODES)
def test_project_signal(nmode, dev):
    from toast_amd import capi

    worst = {}
    for case in _cases(nmode):
        n_det, used, start = case["n_det"], case["used"], case["start"]
        args = (case["signal"], case["rows"], case["T"], start) + _layout(case)
        seq = G.f2d_project(*args)
        truth, bound = G.f2d_project_truth(*args)
        assert np.array_equal(_bits(seq[~used]), _bits(start[~used])) and np.any(seq[used] != start[used])
        cut = G.f2d_blocks(nmode) & ~used
        assert np.count_nonzero(cut) == (5 + 6) * nmode          # the samples cut off the two clipped views
        d_sig, d_t, d_out = dev(case["signal"]), dev(case["T"]), dev(start)
        ivl = _intervals(case["views"])
        split = 0
        for n_group in _group_counts(n_det):
            groups = capi.dev.fourier2d_groups(n_det, N_TILE, n_group)
            runs = []
            for _ in range(2):
                d_out.put(start)
                capi.dev.fourier2d_project_signal(nmode, d_t.ptr, case["offsets"], d_out.ptr, case["rows"], d_sig.ptr,
                                                  case["n_samp"], ivl, n_group=n_group)
                runs.append(d_out.get())
            got = runs[0]
            assert np.array_equal(_bits(got), _bits(runs[1])), "two runs differ"
            # sentinel slots, and the amplitudes of the samples cut off a clipped view
            assert np.array_equal(_bits(got[~used]), _bits(start[~used]))
            if groups == 1:
                wrong = np.count_nonzero(_bits(got) != _bits(seq))
                print(f"project_signal nmode {nmode} n_det {n_det} n_group {n_group}: one group, {wrong} amplitudes differ "
                      "from the sequential sum")
                assert wrong == 0
            else:
                split += 1
                err = np.abs(got.astype(G.LD) - truth).astype(np.float64)
                frac = float(np.max(err[used] / bound[used]))
                worst[n_det] = max(worst.get(n_det, 0.0), frac)
                print(f"project_signal nmode {nmode} n_det {n_det} n_group {n_group}: {groups} groups, worst fraction of the "
                      f"derived bound {frac:.4f}; {np.count_nonzero(got != seq)} amplitudes differ from the sequential sum")
                assert np.all(err[used] <= bound[used])
        assert split == (0 if n_det == 1 else (3 if n_det == 2 else 4)), (n_det, split)
        assert np.array_equal(_bits(d_sig.get()), _bits(case["signal"]))
    print(f"project_signal nmode {nmode}: worst fraction of the bound by detector count {worst}")


@pytest.mark.parametrize("nmode", G.F2D_NMODES)
def test_norms_and_apply_precond(nmode, dev):
    from toast_amd import capi

    for case in _cases(nmode):
        n_det, used, size = case["n_det"], case["used"], case["size"]
        fill = np.full(size, -1.0)
        layout = _layout(case)
        want = {True: G.f2d_norms(case["flags"], case["flag_rows"], G.DET_FLAG_MASK, case["w2"], fill, *layout),
                False: G.f2d_norms(None, None, 0, case["w2"], fill, *layout)}
        view = 3                                              # the view that holds the sample flagged everywhere
        first = case["views"][view][0]
        assert first <= G.F2D_ALL_FLAGGED < case["views"][view][1]
        at = int(case["offsets"][view]) + (G.F2D_ALL_FLAGGED - first) * nmode
        d_flags, d_w2, d_norms = dev(case["flags"]), dev(case["w2"]), dev(fill)
        d_amps, d_out = dev(case["amps"]), dev(np.full(size, -3.0))
        ivl = _intervals(case["views"])
        for with_flags in (True, False):
            d_norms.put(fill)
            capi.dev.fourier2d_norms(nmode, d_w2.ptr, case["offsets"], case["flag_rows"] if with_flags else None,
                                     d_flags.ptr if with_flags else 0, G.DET_FLAG_MASK, n_det, case["n_samp"], ivl, d_norms.ptr)
            got = d_norms.get()
            wrong = np.count_nonzero(_bits(got) != _bits(want[with_flags]))
            print(f"norms nmode {nmode} n_det {n_det} flags {with_flags}: {wrong} of {got.size} norms differ")
            assert wrong == 0
            assert np.all(got[~used] == -1.0) and not np.any(got[used] == -1.0)
            assert np.all(got[at:at + nmode] == 0.0) == with_flags
            d_out.put(-3.0)
            capi.dev.fourier2d_apply_precond(size, d_norms.ptr, d_amps.ptr, d_out.ptr)
            out = d_out.get()
            assert np.array_equal(_bits(out), _bits(case["amps"] * got))
            assert np.all(out[at:at + nmode] == 0.0) == with_flags
        assert np.any(want[True] != want[False])
        assert np.array_equal(d_flags.get(), case["flags"])


def _prior_runs():
    from toast_amd.templates.fourier2d import prior_fft_length

    for view_len, filter_len in G.PRIOR_SHAPES:
        n_fft = prior_fft_length(view_len, filter_len)
        yield view_len, filter_len, n_fft
        if (view_len, filter_len) in G.PRIOR_DOUBLED:
            yield view_len, filter_len, 2 * n_fft


def test_add_prior_at_every_transform_length_and_mode_count(dev):
    from toast_amd import capi
    from toast_amd.accel import native
    from toast_amd.templates.fourier2d import half_complex

    assert capi.dev.fourier2d_max_modes() == max(G.PRIOR_NMODES) == G.PRIOR_MAX_MODES
    tail = 7
    runs = list(_prior_runs())
    assert sum(n_fft < 64 for _, _, n_fft in runs) >= 3 and [r[2] for r in runs[:4]] == [2, 2, 4, 16]
    failed = []
    for view_len, filter_len, n_fft in runs:
        a, filt, scale = G.prior_inputs(view_len, filter_len)
        d_spec = dev(half_complex(np.fft.rfft(filt, n_fft), n_fft))
        for nmode in G.PRIOR_NMODES:
            d_ref, peak = G.prior_distance(G.prior_scipy(view_len, filter_len, nmode), view_len, filter_len, nmode)
            d_ref /= peak
            start = np.full(view_len * nmode + tail, G.PRIOR_FILL)
            start[view_len * nmode:] = G.SENTINEL
            made = [Dev(a[:, :nmode]), Dev(start), Dev(np.zeros(2 * nmode * n_fft))]
            try:
                d_in, d_out, d_work = made
                capi.dev.fourier2d_add_prior(nmode, view_len, d_in.ptr, d_out.ptr, filter_len, n_fft, d_spec.ptr,
                                             scale[:nmode], d_work.ptr)
                native().accel_synchronize()
                got, kept = d_out.get(), d_in.get()
            finally:
                for d in made:
                    d.free()
            d_dev, _ = G.prior_distance(got[:view_len * nmode].reshape(view_len, nmode), view_len, filter_len, nmode)
            bound = 8.0 * max(d_ref, YARD) * peak
            print(f"add_prior L {view_len} F {filter_len} n_fft {n_fft} nmode {nmode}: d_ref {d_ref:.3e}, device {d_dev / peak:.3e}, "
                  f"bound {bound / peak:.3e} (max|out| {peak:.3e})")
            assert np.all(got[view_len * nmode:] == G.SENTINEL)
            assert np.array_equal(kept, a[:, :nmode])
            if not d_dev <= bound:
                failed.append((view_len, filter_len, n_fft, nmode, d_dev, bound))
    assert not failed, failed


def test_add_prior_refuses_what_it_cannot_take(dev):
    from toast_amd import capi

    d_in, d_out, d_spec, d_work = dev(np.zeros(8 * 41)), dev(np.zeros(8 * 41)), dev(np.zeros(16)), dev(np.zeros(2 * 41 * 16))
    with pytest.raises(Exception, match="1 to 40 modes"):
        capi.dev.fourier2d_add_prior(41, 8, d_in.ptr, d_out.ptr, 8, 16, d_spec.ptr, np.ones(41), d_work.ptr)
    with pytest.raises(Exception, match="n_fft must be even"):
        capi.dev.fourier2d_add_prior(5, 8, d_in.ptr, d_out.ptr, 8, 15, d_spec.ptr, np.ones(5), d_work.ptr)
    with pytest.raises(Exception, match="n_fft must be even"):
        capi.dev.fourier2d_add_prior(5, 8, d_in.ptr, d_out.ptr, 8, 14, d_spec.ptr, np.ones(5), d_work.ptr)      # too short
    assert not np.any(d_out.get())
