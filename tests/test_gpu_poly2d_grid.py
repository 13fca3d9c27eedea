"""GPU: the PolyFilter2D kernels (csrc/poly2d_filter.hip) at the view, group and batch shapes the fixture cases of
tests/test_gpu_poly2d.py never take, on the cases of tests/focalplane_grid.py (see its docstring).

* ``edges_o0`` .. ``edges_o3`` against the coefficients of the reference's own kernel (tests/golden/poly2d_grid.npz,
  poly2d_grid_o3.npz; bounds stored per case: 4 x max |reference - host emulation|): five interleaved groups of 30, 1, 3,
  12 and 7 detectors (``blockIdx.y`` up to 4, a group of one detector, groups with fewer detectors than modes); views of
  0, 1, 2, 255, 256, 257 and 513 samples, adjacent, clipped, on the last sample; a solved, a no-good, a truncated and a
  not-finite system inside one wave of ``k_p2d_solve``.
* ``empty_group_o1``: a group index that no detector carries gets zero coefficients and status no-good at every view
  sample and changes nothing else -- the other groups are bit-equal to a run with the indices compacted.
* ``batches_o3``: 64 groups at order 3 make the launcher cut the 20 sample tiles of the call into batches
  (``filter_poly2d_batch_tiles``): ``tile_begin > 0``, a last batch shorter than the slab was sized for, a view across a
  batch boundary.  The call is BITWISE equal to the same buffers processed one piece of a view per call: a system's
  result does not depend on which systems share its wave or its batch.

Observed on an MI355X (every test prints its own figures before it asserts):
    edges_o0 .. edges_o3    filtered signal, fit and coefficients each at 0.25 of the stored bound on both paths (the
                            distance of the host emulation to the reference, which the device reproduces); no status differs
                            from the emulation; edges_o2 without flags: 0 from the emulation in signal and coefficients
    batches_o3              9 sample tiles per batch of the 20: batches of 9, 9 and 2 tiles; 307200 systems (2115 solved,
                            46493 no good, 258592 truncated); one call and 25 calls differ in 0 values
"""
import numpy as np
import pytest

import focalplane_grid as G
import poly2d_host as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import accel

    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


def paths():
    from toast_amd import capi

    return capi.dev.POLY2D_PATHS


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Buffers:
    """The device copies of a case's buffers and of the optional outputs: several calls may work on them."""

    def __init__(self, case):
        import torch

        self.case = case
        n = case["n_samp"]
        self.signal, self.flags, self.shared = dev(case["signal"]), dev(case["det_flags"]), dev(case["shared"])
        self.coeff = torch.zeros((n, case["n_group"], case["n_mode"]), dtype=torch.float64, device="cuda")
        self.status = torch.full((n, case["n_group"]), -1, dtype=torch.int32, device="cuda")

    def run(self, starts=None, stops=None, path=0, with_flags=True, with_outputs=True):
        from toast_amd import capi

        case = self.case
        capi.dev.filter_poly2d(case["order"], case["n_samp"], case["sig_rows"], self.signal.data_ptr(),
                               case["flag_rows"] if with_flags else None, self.flags.data_ptr() if with_flags else 0,
                               P.DET_MASK, self.shared.data_ptr(), P.SHARED_MASK, P.POLY_MASK, case["det_group"],
                               case["n_group"], case["templates"], case["starts"] if starts is None else starts,
                               case["stops"] if stops is None else stops,
                               d_coeff=self.coeff.data_ptr() if with_outputs else 0,
                               d_status=self.status.data_ptr() if with_outputs else 0, path=path)

    def get(self):
        import torch

        torch.cuda.synchronize()
        return self.signal.cpu().numpy(), self.flags.cpu().numpy(), self.coeff.cpu().numpy(), self.status.cpu().numpy()


def run_device(case, **kwargs):
    b = Buffers(case)
    b.run(**kwargs)
    return b.get()


def same_bits(got, want):
    return (np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(got[3], want[3]))


_fixtures, _runs, _emulations = {}, {}, {}


def cached_run(name, path):
    """One device run per (case, path), shared by the tests below and never modified."""
    if (name, path) not in _runs:
        _runs[(name, path)] = run_device(G.edge_fixture_case(name, _fixtures)[0], path=path)
    return _runs[(name, path)]


def cached_emulation(name):
    if name not in _emulations:
        _emulations[name] = P.emulate(G.edge_fixture_case(name, _fixtures)[0])
    return _emulations[name]


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", list(G.EDGE_CASES))
def test_edges_against_reference_fixture(name, path):
    assert path in paths()
    case, ref_coeff, excluded, bounds = G.edge_fixture_case(name, _fixtures)
    sig, flags, coeff, status = cached_run(name, path)
    # values, flags, and bit-for-bit: the unlisted sentinel rows, the flagged samples, everything outside the views
    P.check_result(case, ref_coeff, excluded, bounds, sig, flags, coeff, label=f"device {name} path {path}")
    unlisted = np.setdiff1d(np.arange(sig.shape[0]), case["sig_rows"])
    assert unlisted.size == 4 and np.all(sig[unlisted] == G.SENTINEL)
    samples = P.view_samples(case)
    outside = np.ones(case["n_samp"], dtype=bool)
    outside[samples] = False
    assert np.count_nonzero(outside) == case["n_samp"] - 1284
    assert np.array_equal(_bits(sig[:, outside]), _bits(case["signal"][:, outside]))
    assert np.array_equal(flags[:, outside], case["det_flags"][:, outside])
    assert np.all(status[outside] == -1) and np.all(coeff[outside] == 0)
    emu_status = cached_emulation(name)[3]
    differ = np.count_nonzero(status[samples][~excluded] != emu_status[samples][~excluded])
    counts = np.bincount(status[samples].ravel(), minlength=4)
    print(f"device {name} path {path}: statuses solved / no good / truncated / not finite {counts.tolist()}, "
          f"{differ} differ from the emulation outside the border band")
    assert differ == 0
    # every status inside one wave of the solve: 64, 16, 4 and 4 systems at order 0 .. 3
    span = np.arange(G.EDGE_FIRST, G.EDGE_FIRST + 8)
    assert list(status[span, 0]) == G.edge_statuses(case["order"])
    wave = {0: 64, 1: 16, 2: 4, 3: 4}[case["order"]]
    assert set(status[G.EDGE_FIRST:G.EDGE_FIRST + min(wave, 8), 0]) == ({0, 1, 3} if case["order"] == 0 else {0, 1, 2, 3})
    # the view of one sample on the observation's last sample, and the views of 1 and 2 samples, were solved
    assert np.all(status[-1] >= 0) and np.all(status[776:778] >= 0) and np.any(coeff[-1] != 0)


@pytest.mark.parametrize("name", list(G.EDGE_CASES))
def test_edges_runs_and_variants_are_bitwise_equal(name):
    case = G.edge_fixture_case(name, _fixtures)[0]
    first = cached_run(name, 0)
    assert same_bits(run_device(case, path=0), first), "two runs differ"
    assert same_bits(cached_run(name, 1), first), "the paths differ"
    # the optional outputs change nothing
    bare = run_device(case, path=0, with_outputs=False)
    assert np.array_equal(_bits(bare[0]), _bits(first[0])) and np.array_equal(bare[1], first[1])
    assert np.all(bare[2] == 0) and np.all(bare[3] == -1)


def test_edges_null_flag_pointer():
    """No detector flags: every detector is good where the shared flag is clear, and no flag is written."""
    name = "edges_o2"
    case, _, _, bounds = G.edge_fixture_case(name, _fixtures)
    clean = dict(case)
    clean["signal"] = np.nan_to_num(case["signal"], nan=1.25)       # the NaNs sit in samples that are all good now
    sig, flags, coeff, status = run_device(clean, with_flags=False)
    assert np.array_equal(flags, case["det_flags"])
    emu_sig, _, emu_coeff, emu_status, _ = P.emulate(clean, with_flags=False)
    # the same algorithm in the same order: a quarter of the stored bound is the distance reference <-> emulation
    d_sig, d_coeff = np.max(np.abs(sig - emu_sig)), np.max(np.abs(coeff - emu_coeff))
    print(f"device {name} without flags: filtered {d_sig:.3e} / {bounds['filtered']:.3e}, coeff {d_coeff:.3e} / {bounds['coeff']:.3e}")
    assert d_sig <= bounds["filtered"] and d_coeff <= bounds["coeff"]
    samples = P.view_samples(case)
    assert np.array_equal(status[samples], emu_status[samples])
    good = ((case["shared"] & P.SHARED_MASK) == 0)
    good[np.setdiff1d(np.arange(case["n_samp"]), samples)] = False
    assert np.array_equal(_bits(sig[:, ~good]), _bits(clean["signal"][:, ~good]))


def test_empty_group():
    from toast_amd import capi

    case, compact = G.build_empty_group_case(), G.build_empty_group_case(compact=True)
    samples = P.view_samples(case)
    assert samples.size == case["n_samp"]                      # one view, clipped at both ends
    for path in paths():
        sig, flags, coeff, status = run_device(case, path=path)
        csig, cflags, ccoeff, cstatus = run_device(compact, path=path)
        assert np.all(coeff[:, 1] == 0) and np.all(status[:, 1] == capi.dev.POLY2D_NO_GOOD)
        # no signal and no flag is touched because of it: the same bits as without that group
        assert np.array_equal(_bits(sig), _bits(csig)) and np.array_equal(flags, cflags)
        assert np.array_equal(_bits(coeff[:, [0, 2]]), _bits(ccoeff)) and np.array_equal(status[:, [0, 2]], cstatus)
        # ... and those are what the emulation of the compacted case gives
        emu_sig, emu_flags, emu_coeff, emu_status, _ = P.emulate(compact)
        assert np.array_equal(cflags, emu_flags) and np.array_equal(cstatus, emu_status)
        d = np.max(np.abs(csig - emu_sig))
        print(f"empty group path {path}: statuses {np.bincount(status.ravel(), minlength=4).tolist()}, compacted run against the "
              f"emulation {d:.3e}")
        assert d <= 1e-10 * np.max(np.abs(case["signal"])) and np.any(csig != case["signal"])


def test_batches_are_bitwise_equal_to_one_call_per_piece():
    from toast_amd import capi

    per_batch = capi.dev.filter_poly2d_batch_tiles(3, 64)
    tile0, n_tile = G.batch_tiles()
    n_tiles = (G.BATCH_STOPS - G.BATCH_STARTS + G.TILE - 1) // G.TILE
    print(f"batches_o3: {per_batch} sample tiles per batch of {n_tile}: batches of "
          f"{[min(per_batch, n_tile - t) for t in range(0, n_tile, per_batch)]} tiles")
    assert 1 <= per_batch < n_tile / 2                                         # at least three batches
    assert n_tile % per_batch != 0                                             # the last one shorter
    assert any(t0 < per_batch < t0 + k for t0, k in zip(tile0, n_tiles))       # a view across the first boundary
    assert 2 * per_batch in tile0                                              # a view starting on the second
    pieces = G.batch_pieces()
    assert all((b - a + G.TILE - 1) // G.TILE <= per_batch for a, b in pieces)
    assert capi.dev.filter_poly2d_batch_tiles(3, 1) > 64 * per_batch - 64 and capi.dev.filter_poly2d_batch_tiles(0, 64) > per_batch
    assert capi.dev.filter_poly2d_batch_tiles(4, 64) == 0 and capi.dev.filter_poly2d_batch_tiles(3, 0) == 0
    case = G.build_batches_case()
    whole = Buffers(case)
    whole.run()
    whole = whole.get()
    again = run_device(case)
    assert same_bits(again, whole), "two runs differ"
    apart = Buffers(case)
    for a, b in pieces:
        apart.run(starts=np.array([a], dtype=np.int64), stops=np.array([b], dtype=np.int64))
    apart = apart.get()
    samples = P.view_samples(case)
    for label, w, p in zip(("signal", "flags", "coefficients", "status"), whole, apart):
        differ = np.count_nonzero(_bits(w) != _bits(p)) if w.dtype == np.float64 else np.count_nonzero(w != p)
        print(f"batches_o3: {label}: {differ} of {w.size} values differ between one call and {len(pieces)} calls")
    assert same_bits(whole, apart)
    sig, flags, coeff, status = whole
    counts = np.bincount(status[samples].ravel(), minlength=4)
    print(f"batches_o3: {samples.size * 64} systems, statuses {counts.tolist()}")
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and np.all(status[samples] >= 0)
    outside = np.ones(case["n_samp"], dtype=bool)
    outside[samples] = False
    assert np.all(status[outside] == -1) and np.all(coeff[outside] == 0)
    assert np.array_equal(_bits(sig[:, outside]), _bits(case["signal"][:, outside]))
    unlisted = np.setdiff1d(np.arange(sig.shape[0]), case["sig_rows"])
    assert np.all(sig[unlisted] == G.SENTINEL)
    # every batch did its work: a solved system of a full group leaves its good detectors free of the fitted modes.
    # The views 0, 2 and 3 lie in the first, second and third batch.
    t = case["templates"]
    for view in (0, 2, 3):
        span = np.arange(G.BATCH_STARTS[view], G.BATCH_STOPS[view])
        at, g = np.argwhere(status[span, :4] == 0)[0]
        s = int(span[at])
        members = np.flatnonzero(case["det_group"] == g)
        good = (case["det_flags"][case["flag_rows"][members], s] & P.DET_MASK) == 0
        rows = case["sig_rows"][members[good]]
        left = np.max(np.abs(t[members[good]].T @ sig[rows, s]))
        # T^T (s - T c) = b - A c: a solved system has an eigenvalue ratio below 1 / rcond = 1e6, so the roundings of c leave
        # at most about u * 1e6 * sum|T s|
        bound = 2.0 ** -53 * 1.0e6 * np.max(np.abs(t[members[good]]).T @ np.abs(case["signal"][rows, s]))
        print(f"batches_o3: view {view}, sample {s}, group {g}: {np.count_nonzero(good)} good detectors, max |T^T residual| "
              f"{left:.2e} (bound {bound:.2e})")
        assert left <= bound and np.any(coeff[s, g] != 0)
