"""GPU: the SubHarmonic and Periodic kernels (csrc/template_basis.hip) through the C ABI at every term count and on every
bin path, against the plain reference of tests/templates_reference.py (``math.fsum`` sums, derived bounds: see its
docstring).  tests/test_gpu_templates.py holds the same kernels to the fixture of the reference implementation on one
small case; this file reaches the branches that case never takes.

SubHarmonic, 1..9 terms on one layout (three detectors in a buffer of four odd rows; views of 1, 2, 3, 63, 64, 65, 4095,
4096, 4097 and 8193 samples, one empty, one ending on the row's last sample, odd and even starts; ~30 % flags, one
(detector, view) fully flagged): the compiled widths N = 2, 4, 9 run with n = N and with every n < N, so the ``k < n`` and
``c < n`` guards, the ``view * n`` and ``blk * n * n`` strides and the packed-triangle decode are all taken with n != N.

Periodic, 1 to 5000 bins x {sweep, random, single} index rows x {shared, per-detector} on three chunks of 16384 samples
(the last partial): every kernel runs with ``blockIdx.x > 0``; the LDS kernels loop ``b += kThreads``; 1024 and 1025 bins
sit on the LDS limit; ``periodic_hits`` takes its LDS and its global-atomic branch, from sample ranges that start off a
chunk boundary; the projection runs by the rule, on the LDS path and on the atomic path; the index rows hold values that
are no bins of the call (nbins, nbins + 5, 2^31 - 1) next to -1.

Every case keeps an unused signal row and unused amplitude slots between the detectors' blocks filled with a sentinel:
they come back untouched.  Detector rows, flag rows, index rows and amplitude blocks are permuted differently.

Worst observed fractions of the derived bounds on an MI355X (every test prints its own before it asserts):
    SubHarmonic project_signal   0.72   of gamma(m - 1) S        (a view of 3 samples: two additions against gamma(2);
                                                                  0.10 at 11 samples, 0.0075 from 63 samples on, 1e-4 from 4095)
    SubHarmonic Gram matrix      0.22   of gamma(m) S w          (7 good samples; 0.042 from 40 good samples on, 7e-4 from 2848)
    SubHarmonic apply_precond    0.975  of gamma(n) sum|P x|     (1 term: one rounded product against u |P x|)
    Periodic project_signal      0.16   of gamma(m) (|a0| + S)   on the LDS path (and by the rule up to 1024 bins),
                                 0.9964 on the atomic path       (5000 bins, a bin of one term: one rounded addition
                                                                  against u (|a0| + |s|))
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import templates_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
NORDERS = list(range(1, tr.SUBH_MAX_TERMS + 1))
SWEEPS = [(nbins, pattern, mode) for nbins in tr.SWEEP_NBINS for pattern in tr.SWEEP_PATTERNS for mode in tr.SWEEP_MODES]
SWEEP_IDS = [f"{nbins}-{pattern}-{mode}" for nbins, pattern, mode in SWEEPS]


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)     # (its own host key)
        accel_data_create(self.a, "test_templates_grid")
        accel_data_update_device(self.a, "test_templates_grid")
        self.ptr = accel_device_ptr(self.a)

    def put(self, value):
        from toast_amd.accel import accel_data_update_device

        self.a[...] = value
        accel_data_update_device(self.a, "test_templates_grid")

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_templates_grid")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_templates_grid")


@pytest.fixture
def dev():
    """Dev(array) whose device copies are released when the test ends, also when it fails: a buffer left behind would
    make later tests fail on a reused host address."""
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


def _i32(a):
    return np.asarray(a, dtype=np.int32)


# ------------------------------------------------------------------------------------ SubHarmonic
def _subh(norder):
    g = tr.subharmonic_grid()
    offs, size = tr.subharmonic_offsets(norder)
    used = tr.used_slots(offs, len(g["views"]) * norder, size)
    lengths = [max(0, min(l, g["n_samp"]) - max(f, 0)) for f, l in g["views"]]
    assert sorted(set(lengths)) == [0, 1, 2, 3, 11, 63, 64, 65, 4095, 4096, 4097, 8193]
    assert {f % 2 for f, _ in g["views"]} == {0, 1} and g["n_samp"] % 2 == 1
    return g, offs, size, used


@pytest.mark.parametrize("norder", NORDERS)
def test_subharmonic_add_to_signal(norder, dev):
    from toast_amd import capi

    g, offs, size, used = _subh(norder)
    amps = np.random.default_rng(100 + norder).standard_normal(size)
    amps[~used] = tr.SENTINEL
    d_sig, d_amps = dev(g["signal"]), dev(amps)
    capi.dev.subharmonic_add_to_signal(norder, offs, d_amps.ptr, _i32(g["rows"]), d_sig.ptr, g["n_samp"], _intervals(g["views"]))
    got = d_sig.get()
    want = tr.subharmonic_add(g["signal"], g["rows"], offs, amps, g["views"], norder)
    assert np.all(got[1] == tr.SENTINEL) and np.any(want[0] != g["signal"][0])
    assert np.array_equal(got, want)
    assert np.array_equal(d_amps.get(), amps)


@pytest.mark.parametrize("norder", NORDERS)
def test_subharmonic_project_signal(norder, dev):
    from toast_amd import capi

    g, offs, size, used = _subh(norder)
    n_view = len(g["views"])
    d_sig, d_out = dev(g["signal"]), dev(np.full(size, tr.SENTINEL))
    args = (norder, offs, d_out.ptr, _i32(g["rows"]), d_sig.ptr, g["n_samp"], _intervals(g["views"]))
    capi.dev.subharmonic_project_signal(*args)
    got = d_out.get()
    assert np.all(got[~used] == tr.SENTINEL), "slots between the detectors' blocks were written"
    assert not np.any(got[used] == tr.SENTINEL), "an amplitude was not assigned"
    blocks = np.stack([got[o:o + n_view * norder].reshape(n_view, norder) for o in offs])
    assert np.all(blocks[:, g["empty_view"]] == 0.0)
    sums = tr.Sums(*(a[:, :, :norder] for a in g["project"]))
    frac = tr.fraction_of(tr.deviation(blocks, sums), tr.gamma(np.maximum(sums.m - 1, 0)) * sums.S)
    by_len = {int(m): float(frac[sums.m == m].max()) for m in np.unique(sums.m)}
    print(f"subharmonic project_signal, {norder} terms: worst fraction of gamma(m-1) S {float(frac.max()):.4f}; by view length {by_len}")
    assert np.all(frac <= 1)
    d_out.put(-3.0)
    capi.dev.subharmonic_project_signal(*args)
    again = d_out.get()
    assert np.array_equal(again[used], got[used]) and np.all(again[~used] == -3.0)
    assert np.array_equal(d_sig.get(), g["signal"])


@pytest.mark.parametrize("norder", NORDERS)
def test_subharmonic_precond_build(norder, dev):
    from toast_amd import capi

    g, _, _, _ = _subh(norder)
    n_view = len(g["views"])
    d_flags = dev(g["flags"])
    d_gram = dev(np.full((3, n_view, norder, norder), tr.SENTINEL))
    d_ngood = dev(np.full((3, n_view), -5, dtype=np.int64))
    args = (norder, _i32(g["flag_rows"]), d_flags.ptr, tr.DET_MASK, np.array(g["weights"]), g["n_samp"], _intervals(g["views"]),
            d_gram.ptr, d_ngood.ptr)
    capi.dev.subharmonic_precond_build(*args)
    gram, ngood = d_gram.get(), d_ngood.get()
    assert np.array_equal(ngood, g["ngood"])
    fd, fv = g["flagged"]
    assert ngood[fd, fv] == 0 and np.all(ngood[:, g["empty_view"]] == 0)
    assert np.all(gram[fd, fv] == 0.0) and np.all(gram[:, g["empty_view"]] == 0.0)
    sums = tr.Sums(*(a[:, :, :norder, :norder] for a in g["gram"]))
    err, bound = tr.gram_check(gram, sums, g["weights"])
    frac = tr.fraction_of(err, bound)
    by_len = {int(m): float(frac[sums.m == m].max()) for m in np.unique(sums.m)}
    print(f"subharmonic Gram, {norder} terms: worst fraction of gamma(m) S w {float(frac.max()):.4f}; by good samples {by_len}")
    assert np.all(frac <= 1)
    assert np.array_equal(gram, gram.transpose(0, 1, 3, 2))
    d_gram.put(1.0)
    d_ngood.put(9)
    capi.dev.subharmonic_precond_build(*args)
    assert np.array_equal(d_gram.get(), gram) and np.array_equal(d_ngood.get(), ngood)


@pytest.mark.parametrize("norder", NORDERS)
def test_subharmonic_apply_precond(norder, dev):
    from toast_amd import capi

    rng = np.random.default_rng(300 + norder)
    n_block, tail = 300, 4
    precond = rng.standard_normal((n_block, norder, norder))
    x = rng.standard_normal(n_block * norder)
    d_p, d_x, d_out = dev(precond), dev(x), dev(np.full(n_block * norder + tail, tr.SENTINEL))
    capi.dev.subharmonic_apply_precond(norder, n_block, d_p.ptr, d_x.ptr, d_out.ptr)
    got = d_out.get()
    want, bound = tr.subharmonic_precond(precond, x)
    frac = tr.fraction_of(np.abs(got[:-tail].astype(LD) - want), bound)
    print(f"subharmonic apply_precond, {norder} terms: worst fraction of gamma(n) sum|P x| {float(frac.max()):.4f}")
    assert np.all(got[-tail:] == tr.SENTINEL) and np.all(frac <= 1)


@pytest.mark.parametrize("norder", [0, tr.SUBH_MAX_TERMS + 1])
def test_subharmonic_term_count_is_refused(norder, dev):
    """Host-side argument checks: they return before any launch."""
    from toast_amd import capi

    assert capi.dev.subharmonic_max_terms() == tr.SUBH_MAX_TERMS
    ivl = _intervals([(0, 8)])
    d_sig, d_amps, d_flags = dev(np.zeros((1, 8))), dev(np.zeros(16)), dev(np.zeros((1, 8), dtype=np.uint8))
    d_gram, d_ngood = dev(np.zeros(128)), dev(np.zeros(1, dtype=np.int64))
    offs, rows = np.zeros(1, dtype=np.int64), _i32([0])
    with pytest.raises(RuntimeError, match="terms"):
        capi.dev.subharmonic_add_to_signal(norder, offs, d_amps.ptr, rows, d_sig.ptr, 8, ivl)
    with pytest.raises(RuntimeError, match="terms"):
        capi.dev.subharmonic_project_signal(norder, offs, d_amps.ptr, rows, d_sig.ptr, 8, ivl)
    with pytest.raises(RuntimeError, match="terms"):
        capi.dev.subharmonic_precond_build(norder, rows, d_flags.ptr, 1, np.ones(1), 8, ivl, d_gram.ptr, d_ngood.ptr)
    with pytest.raises(RuntimeError, match="terms"):
        capi.dev.subharmonic_apply_precond(norder, 1, d_gram.ptr, d_amps.ptr, d_sig.ptr)
    assert not np.any(d_sig.get()) and not np.any(d_amps.get()) and not np.any(d_gram.get())


# ------------------------------------------------------------------------------------ Periodic: the bin index
INDEX_VIEWS = [(0, 1), (5, 4101), (4102, 8300), (8990, 9001)]
INDEX_SPAN, INDEX_MIN, INDEX_SAMP = 57400.0, -3.0, 9001          # the span is a multiple of 7 and of 1025
INDEX_CASES = [(n_row, with_flags, nbins, None) for n_row in (1, 3) for with_flags in (False, True) for nbins in (1, 7, 1025)]
INDEX_CASES.append((3, True, None, 7.5))


@pytest.mark.parametrize("n_row,with_flags,nbins,increment", INDEX_CASES)
def test_periodic_index(n_row, with_flags, nbins, increment, dev):
    from toast_amd import capi

    rng = np.random.default_rng(700 + 10 * n_row + (nbins or 0))
    if increment is None:
        incr = INDEX_SPAN / nbins          # (max - min) / nbins: the largest value lands on the top edge
    else:
        incr, nbins = increment, int(INDEX_SPAN / increment)
    key = INDEX_MIN + rng.uniform(0.0, INDEX_SPAN, (n_row, INDEX_SAMP))
    edges = rng.integers(0, INDEX_SAMP, 400)
    key[:, edges] = INDEX_MIN + rng.integers(0, nbins + 1, (n_row, 400)) * incr      # values on the edges of bins
    key[:, 6], key[:, 7] = INDEX_MIN + INDEX_SPAN, INDEX_MIN
    flags = None
    if with_flags:
        flags = ((rng.random(key.shape) < 0.1).astype(np.uint8) * 2) | ((rng.random(key.shape) < 0.3).astype(np.uint8) * 1) | 4
        flags[:, 6] &= ~np.uint8(2)
    want, clamped = tr.periodic_index(key, flags, 2, INDEX_VIEWS, INDEX_MIN, incr, nbins)
    assert clamped >= n_row and want.max() == nbins - 1 and (want[:, 1:5] == -1).all() and (want[:, 8300:8990] == -1).all()
    assert not with_flags or np.count_nonzero(want[:, 5:4101] == -1) > 100
    d_key, d_index = dev(key), dev(np.full(key.shape, 12345, dtype=np.int32))
    d_flags = dev(flags) if with_flags else None
    capi.dev.periodic_index(d_key.ptr, d_flags.ptr if with_flags else 0, 2, n_row, INDEX_SAMP, INDEX_MIN, incr, nbins,
                            _intervals(INDEX_VIEWS), d_index.ptr)
    assert np.array_equal(d_index.get(), want)


def test_periodic_index_refuses_zero_increment_and_zero_bins(dev):
    from toast_amd import capi

    d_key, d_index = dev(np.zeros((1, 16))), dev(np.full((1, 16), 5, dtype=np.int32))
    with pytest.raises(RuntimeError, match="increment is zero"):
        capi.dev.periodic_index(d_key.ptr, 0, 0, 1, 16, 0.0, 0.0, 4, _intervals([(0, 16)]), d_index.ptr)
    with pytest.raises(RuntimeError, match="number of bins"):
        capi.dev.periodic_index(d_key.ptr, 0, 0, 1, 16, 0.0, 1.0, 0, _intervals([(0, 16)]), d_index.ptr)
    assert np.all(d_index.get() == 5)


# ------------------------------------------------------------------------------------ Periodic: the three sweeps
_CONDITIONS = {}


def _sweep(nbins, pattern, mode):
    """The case, with what it is for asserted from the reference alone before any kernel runs."""
    case = tr.periodic_sweep(nbins, pattern, mode)
    key = (nbins, pattern, mode)
    if key not in _CONDITIONS:
        _CONDITIONS[key] = tr.sweep_conditions(case)
    c = _CONDITIONS[key]
    assert case["n_samp"] == 2 * tr.PERIODIC_CHUNK + 7233 and case["n_samp"] % 2 == 1
    assert c["take_part"] >= 0.60, c
    if pattern != "single":          # (``single`` puts every sample into one bin: that is what it is for)
        assert c["bins_hit"] >= 0.5, c
    assert c["bins_in_all_chunks"] >= 1, c
    if pattern == "random" and nbins >= 7:
        assert c["widest_step"] >= 7, c
    if pattern == "single" or (pattern == "sweep" and nbins <= 7):
        assert c["widest_step"] <= 2, c
    index = case["index"]
    assert np.count_nonzero(index == -1) > 0.08 * index.size
    for junk in (nbins, nbins + 5, 2 ** 31 - 1):
        assert np.count_nonzero(index == junk) > 0.004 * index.size
    if mode == "per_detector":
        assert index.shape[0] == 3 and not np.array_equal(index[0], index[1]) and not np.array_equal(index[1], index[2])
    return case


def _blocks(buf, case):
    return np.stack([buf[o:o + case["nbins"]] for o in case["offs"]])


@pytest.mark.parametrize("nbins,pattern,mode", SWEEPS, ids=SWEEP_IDS)
def test_periodic_hits_and_apply_precond(nbins, pattern, mode, dev):
    from toast_amd import capi

    case = _sweep(nbins, pattern, mode)
    n_samp, offs, size = case["n_samp"], case["offs"], case["size"]
    used = tr.used_slots(offs, nbins, size)
    start = np.where(used, 3 + np.arange(size) % 5, -99).astype(np.int32)
    d_index, d_flags = dev(case["index"]), dev(case["flags"])
    ref = (case["index"], case["index_rows"], case["flags"], case["flag_rows"], tr.DET_MASK, nbins, 3)
    irows = None if case["index_rows"] is None else _i32(case["index_rows"])
    args = (d_index.ptr, irows, _i32(case["flag_rows"]), d_flags.ptr, tr.DET_MASK, offs, n_samp, nbins)
    hits = None
    for split in (5, tr.PERIODIC_CHUNK + 1, 2 * tr.PERIODIC_CHUNK):
        head, rest = tr.periodic_hits(*ref, 0, split), tr.periodic_hits(*ref, split, n_samp)
        assert np.array_equal(head + rest, case["project"].m)
        d_hits = dev(start)
        capi.dev.periodic_hits(*args, 0, split, d_hits.ptr)
        got = d_hits.get()
        assert np.array_equal(got[~used], start[~used]), (split, "slots between the detectors' blocks were written")
        assert np.array_equal(_blocks(got, case), _blocks(start, case) + head), (split, "first range")
        capi.dev.periodic_hits(*args, split, n_samp, d_hits.ptr)
        hits = d_hits.get()
        assert np.array_equal(hits[~used], start[~used]), (split, "slots between the detectors' blocks were written")
        assert np.array_equal(_blocks(hits, case), _blocks(start, case) + head + rest), (split, "second range")
    # out = in * hits on the unflagged amplitudes, on the counts that are on the device
    rng = np.random.default_rng(900 + nbins)
    amp_flags = (rng.random(size) < 0.3).astype(np.uint8)
    x, out0 = rng.standard_normal(size), rng.standard_normal(size)
    d_af, d_x, d_out = dev(amp_flags), dev(x), dev(out0)
    capi.dev.periodic_apply_precond(size, d_hits.ptr, d_af.ptr, d_x.ptr, d_out.ptr)
    assert np.array_equal(d_out.get(), np.where(amp_flags == 0, x * hits.astype(np.float64), out0))


@pytest.mark.parametrize("nbins,pattern,mode", SWEEPS, ids=SWEEP_IDS)
def test_periodic_add_to_signal(nbins, pattern, mode, dev):
    from toast_amd import capi

    case = _sweep(nbins, pattern, mode)
    offs, size = case["offs"], case["size"]
    used = tr.used_slots(offs, nbins, size)
    amps = np.where(used, np.random.default_rng(1100 + nbins).standard_normal(size), tr.SENTINEL)
    d_index, d_sig, d_amps = dev(case["index"]), dev(case["signal"]), dev(amps)
    irows = None if case["index_rows"] is None else _i32(case["index_rows"])
    capi.dev.periodic_add_to_signal(d_index.ptr, irows, offs, d_amps.ptr, _i32(case["rows"]), d_sig.ptr, case["n_samp"], nbins)
    got = d_sig.get()
    want = tr.periodic_add(case["signal"], case["rows"], case["index"], case["index_rows"], _blocks(amps, case), nbins)
    assert np.all(got[1] == tr.SENTINEL) and np.count_nonzero(want != case["signal"]) > 0.8 * 3 * case["n_samp"]
    assert np.array_equal(got, want)
    assert np.array_equal(d_amps.get(), amps) and np.array_equal(d_index.get(), case["index"])


@pytest.mark.parametrize("nbins,pattern,mode", SWEEPS, ids=SWEEP_IDS)
def test_periodic_project_signal(nbins, pattern, mode, dev):
    from toast_amd import capi

    D = capi.dev
    assert D.periodic_lds_bins() == tr.PERIODIC_LDS_BINS
    case = _sweep(nbins, pattern, mode)
    offs, size, sums, a0 = case["offs"], case["size"], case["project"], case["a0"]
    used = tr.used_slots(offs, nbins, size)
    amps0 = np.full(size, tr.SENTINEL)
    for k, o in enumerate(offs):
        amps0[o:o + nbins] = a0[k]
    assert np.all(a0 != 0)
    d_index, d_sig, d_flags, d_amps = dev(case["index"]), dev(case["signal"]), dev(case["flags"]), dev(amps0)
    irows = None if case["index_rows"] is None else _i32(case["index_rows"])
    bound = tr.periodic_bound(sums, a0)
    lds_ok = nbins <= tr.PERIODIC_LDS_BINS
    paths = [("rule", D.PERIODIC_PATH_RULE)] + ([("lds", D.PERIODIC_PATH_LDS)] * 2 if lds_ok else []) + [("atomic", D.PERIODIC_PATH_ATOMIC)]
    results = []
    for label, path in paths:
        d_amps.put(amps0)
        D.periodic_project_signal(d_index.ptr, irows, _i32(case["rows"]), d_sig.ptr, _i32(case["flag_rows"]), d_flags.ptr,
                                  tr.DET_MASK, offs, d_amps.ptr, case["n_samp"], nbins, path=path)
        got = d_amps.get()
        assert np.all(got[~used] == tr.SENTINEL), (label, "slots between the detectors' blocks were written")
        frac = tr.fraction_of(tr.deviation(_blocks(got, case), sums), bound)
        print(f"periodic project_signal {nbins}-{pattern}-{mode} ({label}): worst fraction of gamma(m) (|a0| + S) "
              f"{float(frac.max()):.4f} (at m = {int(sums.m.reshape(-1)[int(np.argmax(frac))])})")
        assert np.all(frac <= 1), label
        results.append((label, got))
    if lds_ok:          # the rule picks the LDS path: order-deterministic, identical bits in every run
        for label, got in results[1:3]:
            assert np.array_equal(got, results[0][1]), label
    assert np.array_equal(d_sig.get(), case["signal"])


def test_periodic_project_path_is_checked(dev):
    """Host-side argument checks: they return before any launch."""
    from toast_amd import capi

    nbins = tr.PERIODIC_LDS_BINS + 1
    d_index, d_sig = dev(np.zeros((1, 64), dtype=np.int32)), dev(np.ones((1, 64)))
    d_amps = dev(np.zeros(nbins))
    args = (d_index.ptr, None, _i32([0]), d_sig.ptr, None, 0, 0, np.zeros(1, dtype=np.int64), d_amps.ptr, 64, nbins)
    with pytest.raises(RuntimeError, match="LDS path holds at most"):
        capi.dev.periodic_project_signal(*args, path=capi.dev.PERIODIC_PATH_LDS)
    with pytest.raises(RuntimeError, match="path must be"):
        capi.dev.periodic_project_signal(*args, path=3)
    assert not np.any(d_amps.get())
