"""GPU: the four kernels ``ops.ObserveAtmosphere`` runs on (csrc/atm_observe.hip: k_atm_good_ranges, k_atm_observe_quats,
k_atm_flag_failed, k_atm_finish) through the C ABI at every launch shape, and the operator's device path against its
host path in every configuration that changes a kernel argument.  Inputs and host restatements:
tests/atm_operator_case.py; their conditions: tests/test_atm_operator_case_host.py.

Shapes: n_samp in (1, 63, 64, 65, 255, 256, 257, 513) -- one lane, around a wave, around the workgroup of 256 that the
sample-parallel kernels tile with and k_atm_good_ranges strides by, and a third workgroup of one sample -- each once with
rows as long as the view and once as a window of a longer observation (stride n + 37, pointers advanced by 19 samples,
sentinels around the window).  Buffers have two more rows than entries; quat_row, flag_row, weight_row and data_row are
independent permutations.  The scratch arrays (good, atm) are dense [entry][n_samp] by the C ABI; their two extra rows
are the guard.

1. k_atm_good_ranges.  The device's own az / el of a sample is read out with one entry per sample whose flag row leaves
   only that sample good.  The readout is held to 4 x the worst deviation of ``quats_to_azel`` (float64 NumPy) from
   qa_to_angles in long double on the same quaternions, in units eps * max(1, |value|) -- 4 being the project's factor
   for another libm.  Everything else is exact: the good bytes, first / last, and el min / max, az_first and the extent
   of the wrapped offsets as float64 NumPy min / max over the readout values.
2. k_atm_observe_quats.  Bit for bit what ``atm_observe`` (tests/test_gpu_atm_observe.py) adds to a zero row from the
   readout az / el: the kernels share atm_quat_azel and atm_ray and contraction is off.  Status per row = status of
   ``atm_observe`` on the row's good samples alone.  65 537 entries of one sample reach the second launch of the row
   loop of both entries.  Values of one case against the long-double chain, by the rule of ``ac.check_operator``.
3. k_atm_flag_failed.  Exact.
4. k_atm_finish: out = before + scale ((atm ga) (w_i + w_q pfrac) + loading / sin el) against long double with el from
   the readout.  Roundings, each at most eps relative to its result: atm ga (1), w_q pfrac (1), w_i + . (1), the
   product (1) -- 4 on |atm ga w|; the device's sin (documented: 2 ulp) and the division (1) -- 3 on |loading / sin el|;
   the sum of the two, the product with scale and the sum with before -- 1 each on everything they cover.  So
   |out - exact| <= 7 eps scale_i with scale_i = |scale| (|atm ga w| + |loading / sin el|) + |before|.  (In the
   weights of the cases |w_q pfrac| <= 0.08 |w_i| wherever both are read, so its rounding is covered by one unit of
   |w|.)  Without weights and loading the result equals float64 NumPy bit for bit.
5. Operator: device path on resident data against ``use_accel=False`` -- flags and the set of changed samples exactly,
   values within 1e-11 of the largest (the bar of test_wide_scan_takes_the_host_range_and_matches_the_host_path).

Every figure is printed before it is asserted.  Measured on an MI355X: readout deviation of the device 1.217 (n = 1)
.. 2.834 (n = 513), of the host statement 2.834 eps * max(1, |value|), the same for both stride forms; observe_quats
(513 samples, strided, ``holes``) 19.144 eps * scale_i, the host path's 19.144, the fixture's floor 9.960; finish: worst
error / bound 0.245 (n = 257); operator: device against host path at most 7.3e-15 of the largest value.  All exact
comparisons held: no kernel had to change."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import atm_observe_case as ac  # noqa: E402
import atm_operator_case as oc  # noqa: E402
from test_gpu_atm_observe import Dev  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(n, s) for n in oc.N for s in (False, True)]
NAN = np.nan


def shape_id(shape):
    return f"{shape[0]}{'-strided' if shape[1] else ''}"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Buf(Dev):
    """``Dev`` whose host side can be rewritten, with the pointer to a sample of its first row."""

    def put(self, arr=None):
        from toast_amd.accel import accel_data_update_device

        if arr is not None:
            self.a[...] = arr
        accel_data_update_device(self.a, "test_atm")
        return self

    def at(self, sample):
        return self.ptr + int(sample) * int(np.prod(self.a.shape[2:], dtype=np.int64)) * self.a.itemsize


class Pool:
    """The device buffers of a test; all go at its end."""

    def __init__(self):
        self.bufs = []

    def __enter__(self):
        return self

    def dev(self, arr):
        self.bufs.append(Buf(arr))
        return self.bufs[-1]

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()
        return False


_SIMS = {}


def sim_of(kind):
    if kind not in _SIMS:
        _SIMS[kind] = ac.make_sim(ac.volume(kind))
    return _SIMS[kind]


@pytest.fixture(scope="module", autouse=True)
def close_sims():
    yield
    for sim in _SIMS.values():
        sim.close()
    _SIMS.clear()


def readout(pool, n, strided, q, n_quat_rows, rows):
    """The device's az / el [len(rows)][n] of rows of the quaternion buffer ``q``: entry (r, i) names row r and a flag row
    in which only sample i is good; ranges[., 4] is az of that sample, ranges[., 2] == ranges[., 3] its el."""
    from toast_amd import capi

    stride, shift = oc.layout(n, strided)
    ident = np.full((n, n), 2, dtype=np.uint8)
    ident[np.arange(n), np.arange(n)] = 4                            # a bit outside the mask: good
    f = pool.dev(oc.embed(ident, strided, 0))
    good = pool.dev(np.zeros((len(rows) * n, n), dtype=np.uint8))
    r = capi.dev.atm_good_ranges(n, stride, np.repeat(rows, n), q.at(shift), n_quat_rows, np.tile(np.arange(n), len(rows)),
                                 f.at(shift), n, oc.DET_MASK, 0, 0, good.ptr)
    i = np.tile(np.arange(n), len(rows)).astype(np.float64)
    assert np.array_equal(r[:, 0], i) and np.array_equal(r[:, 1], i)
    assert np.array_equal(bits(r[:, 2]), bits(r[:, 3])) and np.all(r[:, 5:] == 0)
    assert np.array_equal(good.get(), np.tile(np.eye(n, dtype=np.uint8), (len(rows), 1)))
    return r[:, 4].reshape(len(rows), n).copy(), r[:, 2].reshape(len(rows), n).copy()


# ================================================================================================ 1. k_atm_good_ranges
_HOST_READOUT = []


def host_readout_deviation():
    """Worst deviation of ``quats_to_azel`` from the long-double evaluation over the quaternions of all shapes."""
    from toast_amd.ops.sim_tod_atm_observe import quats_to_azel

    if not _HOST_READOUT:
        worst = 0.0
        for n in oc.N:
            quats, wrap = oc.range_rows(n)
            az, el = quats_to_azel(quats.reshape(-1, 4))
            worst = max(worst, oc.azel_deviation(az.reshape(wrap.shape), el.reshape(wrap.shape), *oc.longdouble_azel(quats),
                                                 wrap))
        _HOST_READOUT.append(worst)
    return _HOST_READOUT[0]


def range_buffers(pool, n, strided):
    """(quaternion buffer of 7 rows, the row of each of the five ``oc.RANGE_ROWS``, device az, el [5][n])."""
    quats, _ = oc.range_rows(n)
    q_at = oc.row_tables(5, 1, 100 + n)[0]
    q = pool.dev(oc.embed(quats, strided, NAN, n_rows=7, at=q_at))
    az, el = readout(pool, n, strided, q, 7, q_at)
    return q, q_at, az, el


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_readout_accuracy(shape):
    n, strided = shape
    quats, wrap = oc.range_rows(n)
    with Pool() as pool:
        _, _, az, el = range_buffers(pool, n, strided)
    dev = oc.azel_deviation(az, el, *oc.longdouble_azel(quats), wrap)
    host = host_readout_deviation()
    print(f"readout n={n} strided={strided}: device {dev:.3f}, host statement {host:.3f} eps * max(1, |value|)")
    assert np.all((az >= 0) & (az <= oc.TWOPI))
    assert dev <= 4.0 * host


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_good_ranges_reduction_is_exact(shape):
    from toast_amd import capi

    n, strided = shape
    stride, shift = oc.layout(n, strided)
    seen = set()
    with Pool() as pool:
        q, q_at, az, el = range_buffers(pool, n, strided)
        for entries in (1, 3, 5):
            kinds = {1: [0], 3: [1, 2, 3], 5: [4, 2, 0, 1, 3]}[entries]
            flag_row = oc.row_tables(entries, 1, 200 + entries)[0]
            f = pool.dev(np.zeros((entries + 2, stride), dtype=np.uint8))
            s = pool.dev(np.zeros(stride, dtype=np.uint8))
            g = pool.dev(np.full((entries + 2, n), oc.SENTINEL_BYTE, dtype=np.uint8))
            for p, name in enumerate(oc.PATTERNS):
                pat = oc.flag_pattern(name, n, entries, 1000 * n + 10 * entries + p)
                if pat is None:
                    continue
                det, shared = pat
                if det is not None:
                    f.put(oc.embed(det, strided, oc.SENTINEL_BYTE, n_rows=entries + 2, at=flag_row))
                if shared is not None:
                    s.put(oc.embed1(shared, strided, oc.SENTINEL_BYTE))
                r = capi.dev.atm_good_ranges(n, stride, q_at[kinds], q.at(shift), 7, None if det is None else flag_row,
                                             0 if det is None else f.at(shift), entries + 2, oc.DET_MASK,
                                             0 if shared is None else s.at(shift), oc.SHARED_MASK, g.ptr)
                good = g.get()
                want_good = np.stack([oc.good_host(None if det is None else det[e], shared, n) for e in range(entries)])
                assert np.array_equal(good[:entries], want_good), (name, entries)
                assert np.all(good[entries:] == oc.SENTINEL_BYTE), (name, entries)
                want = np.stack([oc.ranges_host(want_good[e], az[kinds[e]], el[kinds[e]]) for e in range(entries)])
                assert np.array_equal(r[:, :2], want[:, :2]), (name, entries, r[:, :2], want[:, :2])
                assert np.array_equal(bits(r), bits(want)), (name, entries)
                for e in range(entries):
                    if not want_good[e].any():
                        assert r[e].tolist() == [-1.0, -1.0, 0, 0, 0, 0, 0, 0]
                        seen.add("empty")
                    elif want_good[e].all() and n >= 63 and kinds[e] in (1, 2):
                        # the row that crosses 0 / 2 pi is short once unwrapped; the wide one reports its sweep of >= pi
                        assert (r[e, 6] - r[e, 5] < 0.3) if kinds[e] == 1 else (r[e, 6] - r[e, 5] >= np.pi)
                        seen.add(("cross", "wide")[kinds[e] - 1])
    assert "empty" in seen and (n < 63 or {"cross", "wide"} <= seen)


def test_good_ranges_argument_errors():
    from toast_amd import capi

    n = 65
    with Pool() as pool:
        q = pool.dev(np.zeros((3, n, 4)))
        f = pool.dev(np.zeros((3, n), dtype=np.uint8))
        g = pool.dev(np.zeros((3, n), dtype=np.uint8))
        for args, text in (((n, n - 1, [0], q.ptr, 3, [0], f.ptr, 3), "shorter than their samples"),
                           ((n, n, [0, 3], q.ptr, 3, [0, 1], f.ptr, 3), "outside its array"),
                           ((n, n, [0, -1], q.ptr, 3, [0, 1], f.ptr, 3), "outside its array"),
                           ((n, n, [0, 1], q.ptr, 3, [0, 3], f.ptr, 3), "outside its array"),
                           ((n, n, [0, 1], q.ptr, 3, None, f.ptr, 3), "need their rows")):
            with pytest.raises(RuntimeError, match=text):
                capi.dev.atm_good_ranges(*args, oc.DET_MASK, 0, 0, g.ptr)
        assert np.all(g.get() == 0)


# ================================================================================================ 2. k_atm_observe_quats
class ObserveShape:
    """The buffers of one observe_quats shape: quaternions and good bytes of ``entries`` rows, times, the scratch rows,
    and the device's az / el of every row."""

    def __init__(self, pool, n, strided, entries, good=None, quats=None):
        self.pool, self.n, self.strided, self.entries = pool, n, strided, entries
        self.stride, self.shift = oc.layout(n, strided)
        times, case_quats, flags = oc.observe_case(n, entries)
        self.times = times.copy()
        self.quats = case_quats if quats is None else quats
        self.good = np.stack([oc.good_host(flags[e], None, n) for e in range(entries)]) if good is None else good
        self.quat_row = oc.row_tables(entries, 1, 300 + n + entries)[0]
        self.q = pool.dev(oc.embed(self.quats, strided, NAN, n_rows=entries + 2, at=self.quat_row))
        self.t = pool.dev(oc.embed1(self.times, strided, NAN))
        self.g = pool.dev(np.concatenate([self.good, np.full((2, n), oc.SENTINEL_BYTE, dtype=np.uint8)]))
        self.scratch0 = np.full((entries + 2, n), oc.SENTINEL)
        self.scratch0[:entries][self.good != 0] = 0.0
        self.atm = pool.dev(self.scratch0)
        self.az, self.el = readout(pool, n, strided, self.q, entries + 2, self.quat_row)
        # what atm_observe reads: contiguous times, az, el and a zero tod, whole rows and the good samples of one row
        self.d_times = pool.dev(self.times)
        self.d_az, self.d_el = pool.dev(self.az), pool.dev(self.el)
        self.d_tod = pool.dev(np.zeros((entries, n)))
        self.c = [pool.dev(np.zeros(n)) for _ in range(4)]

    def volume(self, kind, index32=True):
        sim = sim_of(kind)
        d_index, is32, d_real = sim.device_volume()
        assert is32
        if not index32:
            d_index = self.pool.dev(sim._compressed_index).ptr
        return sim.geometry(-1.0), d_index, index32, d_real

    def observe_quats(self, kinds, index32=True, cell_cache=False):
        """(scratch after [entries + 2][n], status [len(kinds)][entries])."""
        from toast_amd import capi

        self.atm.put(self.scratch0)
        status = [capi.dev.atm_observe_quats(*self.volume(kind, index32), self.n, self.stride, self.t.at(self.shift),
                                             self.quat_row, self.q.at(self.shift), self.entries + 2, self.g.ptr, self.atm.ptr,
                                             cell_cache=cell_cache) for kind in kinds]
        return self.atm.get(), np.array(status)

    def observe_rows(self, kinds):
        """What ``atm_observe`` adds to zero rows from the readout az / el: tod [entries][n]."""
        from toast_amd import capi

        n = self.n
        self.d_tod.put(0.0)
        for kind in kinds:
            capi.dev.atm_observe(*self.volume(kind), self.entries, n, self.d_times.ptr, 0, self.d_az.ptr, self.d_el.ptr, n,
                                 self.d_tod.ptr, n)
        return self.d_tod.get()

    def observe_good_alone(self, kinds):
        """Status [len(kinds)][entries] of ``atm_observe`` on the good samples of each row alone."""
        from toast_amd import capi

        out = np.zeros((len(kinds), self.entries), dtype=np.int32)
        for e in range(self.entries):
            use = self.good[e] != 0
            m = int(use.sum())
            if m == 0:
                continue
            for buf, src in zip(self.c, (self.times, self.az[e], self.el[e], np.zeros(self.n))):
                buf.a[:m] = src[use]
                buf.put()
            for k, kind in enumerate(kinds):
                out[k, e] = capi.dev.atm_observe(*self.volume(kind), 1, m, self.c[0].ptr, 0, self.c[1].ptr, self.c[2].ptr, m,
                                                 self.c[3].ptr, m)
        return out

    def check(self, got, tod, what):
        use = np.concatenate([self.good != 0, np.zeros((2, self.n), dtype=bool)])
        assert np.array_equal(bits(got[use]), bits(tod[self.good != 0])), what
        # samples that are not good and the guard rows keep the sentinel
        assert np.array_equal(bits(got[~use]), bits(self.scratch0[~use])), what


@pytest.mark.parametrize("entries", oc.OBSERVE_ENTRIES)
@pytest.mark.parametrize("shape", [(n, s) for n in oc.N_OBSERVE for s in (False, True)], ids=shape_id)
def test_observe_quats_gives_the_bits_of_observe(shape, entries):
    n, strided = shape
    with Pool() as pool:
        sh = ObserveShape(pool, n, strided, entries)
        for kinds in oc.OBSERVE_VOLUMES:
            got, status = sh.observe_quats(kinds)
            sh.check(got, sh.observe_rows(kinds), (kinds, shape, entries))
            assert np.array_equal(status, sh.observe_good_alone(kinds)), (kinds, status)
            if kinds == ("full",):
                assert not status.any() and np.all(got[:entries][sh.good != 0] != 0)
            elif n >= 64:
                assert np.all(status.max(axis=0) == 1)          # every row loses a good sample to the holes


def test_observe_quats_status_per_row():
    """One launch with a row that fails, the same row without its failing samples, and a wholly flagged row."""
    n, entries = 257, 4
    times, quats, flags = oc.observe_case(n, entries)
    quats = quats[[0, 0, 1, 2]]
    good = np.stack([oc.good_host(flags[e], None, n) for e in range(entries)])
    _, _, failed, _ = oc.observe_conditions(("holes",), times, quats[0], good[0])
    good[1] = good[0]
    good[1, np.nonzero(good[0])[0][failed]] = 0
    good[2] = 0
    with Pool() as pool:
        sh = ObserveShape(pool, n, True, entries, good=good, quats=quats)
        got, status = sh.observe_quats(("holes",))
        want = sh.observe_good_alone(("holes",))
        print(f"status per row {status[0].tolist()}, of atm_observe on the good samples alone {want[0].tolist()}")
        assert status[0].tolist() == want[0].tolist() and status[0, :3].tolist() == [1, 0, 0]
        sh.check(got, sh.observe_rows(("holes",)), "status")
        live = got[1][good[1] != 0]
        assert np.all(np.abs(live) >= 1e-30) and np.any(got[0][good[0] != 0] == 0)


def test_observe_quats_kernel_options_give_the_same_bits():
    with Pool() as pool:
        sh = ObserveShape(pool, 257, True, 4)
        for kinds in (("holes",), ("near", "far")):
            base, st = sh.observe_quats(kinds)
            for index32, cache in ((False, False), (True, True), (False, True)):
                got, st2 = sh.observe_quats(kinds, index32=index32, cell_cache=cache)
                assert np.array_equal(st2, st) and np.array_equal(bits(got), bits(base)), (kinds, index32, cache)


def test_second_launch_of_the_row_loops():
    """65 537 entries of one sample: the row loops of observe_quats and observe launch a second time (row0 = 65535)."""
    from toast_amd import capi

    n_rows = 65537
    t, quats = oc.two_pointings()
    which = np.random.default_rng(8).integers(0, 2, n_rows)
    which[[0, 1, 65534, 65535, 65536]] = [0, 1, 1, 0, 1]
    with Pool() as pool:
        sh = ObserveShape(pool, 1, False, 2, good=np.ones((2, 1), dtype=np.uint8), quats=quats)
        sh.times[:] = t
        sh.t.put(sh.times)
        sh.d_times.put(sh.times)
        two, st_two = sh.observe_quats(("holes",))
        assert st_two[0].tolist() == [1, 0] and two[0, 0] == 0 and abs(two[1, 0]) > 1e-3
        sh.check(two, sh.observe_rows(("holes",)), "two entries")
        g = pool.dev(np.ones((n_rows + 2, 1), dtype=np.uint8))
        atm0 = np.zeros((n_rows + 2, 1))
        atm0[n_rows:] = oc.SENTINEL
        atm = pool.dev(atm0)
        st = capi.dev.atm_observe_quats(*sh.volume("holes"), 1, 1, sh.t.ptr, sh.quat_row[which], sh.q.ptr, 4, g.ptr, atm.ptr)
        got = atm.get()
        assert np.array_equal(st, st_two[0][which])
        assert np.array_equal(bits(got[:n_rows, 0]), bits(two[which, 0]))
        assert np.array_equal(bits(got[n_rows:]), bits(atm0[n_rows:]))
        # the row form: az / el [65537][1]
        az, el = pool.dev(sh.az[which]), pool.dev(sh.el[which])
        tod = pool.dev(np.zeros((n_rows, 1)))
        status = capi.dev.atm_observe(*sh.volume("holes"), n_rows, 1, sh.d_times.ptr, 0, az.ptr, el.ptr, 1, tod.ptr, 1)
        assert status == 1
        assert np.array_equal(bits(tod.get()[:, 0]), bits(two[which, 0]))


def test_observe_quats_values():
    """The strided 513-sample ``holes`` case against the long-double chain on the long-double az / el, held to ten
    times the deviation of the host path (``AtmSim.observe`` on ``quats_to_azel``), floored at the fixture's
    ``op_ref_dev``: the rule of ``ac.check_operator``."""
    from toast_amd.ops.sim_tod_atm_observe import quats_to_azel

    n, entries = 513, 4
    vol = ac.volume("holes")
    with Pool() as pool:
        sh = ObserveShape(pool, n, True, entries)
        got, _ = sh.observe_quats(("holes",))
    dev = host_dev = 0.0
    sim = ac.make_sim(vol)
    for e in range(entries):
        use = sh.good[e] != 0
        ld = ac.longdouble_observe(vol, sh.times[use], *oc.longdouble_azel(sh.quats[e][use]))
        az, el = quats_to_azel(sh.quats[e][use])
        host = np.zeros(int(use.sum()))
        sim.observe(np.ascontiguousarray(sh.times[use]), az, el, host, -1.0, use_accel=False)
        dev = max(dev, ac.deviation(got[e][use], ld["val"], ld["scale"]))
        host_dev = max(host_dev, ac.deviation(host, ld["val"], ld["scale"]))
    sim.close()
    floor = float(ac.gold()["op_ref_dev"])
    print(f"observe_quats: deviation {dev:.3f} eps * scale_i, the host path's {host_dev:.3f}, the reference's own {floor:.3f}")
    assert dev <= 10.0 * max(host_dev, floor)


# ================================================================================================ 3. k_atm_flag_failed
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_flag_failed_is_exact(shape):
    from toast_amd import capi

    n, strided = shape
    stride, shift = oc.layout(n, strided)
    mask = 2
    with Pool() as pool:
        for entries in (1, 4):
            good, atm, flags, enable = oc.flag_failed_case(n, entries, 7000 + 10 * n + entries)
            flag_row = oc.row_tables(entries, 1, 400 + n + entries)[0]
            before = oc.embed(flags, strided, oc.SENTINEL_BYTE, n_rows=entries + 2, at=flag_row)
            f = pool.dev(before)
            g = pool.dev(np.concatenate([good, np.ones((2, n), dtype=np.uint8)]))
            a = pool.dev(np.concatenate([atm, np.zeros((2, n))]))
            n_bad = capi.dev.atm_flag_failed(n, stride, g.ptr, a.ptr, flag_row, enable, f.at(shift), entries + 2, mask)
            after, want_bad = oc.flag_failed_host(good, atm, flags, enable, mask)
            want = oc.embed(after, strided, oc.SENTINEL_BYTE, n_rows=entries + 2, at=flag_row)
            got = f.get()
            print(f"flag_failed n={n} strided={strided} entries={entries}: n_bad {n_bad.tolist()}")
            # raised exactly where good & |atm| < 1e-30 on enabled rows; earlier bits, the rows no entry names and the
            # samples around the window as they were
            assert np.array_equal(got, want)
            assert np.array_equal(got & np.uint8(~mask & 255), before & np.uint8(~mask & 255))
            assert np.array_equal(n_bad, want_bad) and np.all(n_bad[enable == 0] == 0)
            if n >= 63:
                assert np.all(n_bad[enable != 0] > 0) and np.any(got != before)


def test_flag_failed_argument_errors():
    from toast_amd import capi

    n = 65
    with Pool() as pool:
        f = pool.dev(np.zeros((3, n), dtype=np.uint8))
        g = pool.dev(np.ones((3, n), dtype=np.uint8))
        a = pool.dev(np.zeros((3, n)))
        many = np.arange(65536)
        for rows, limit, text in (([1, 1], 3, "two entries name one row"), (many, 65536, "too many rows"),
                                  ([0, 3], 3, "outside its array"), ([-1, 0], 3, "outside its array")):
            with pytest.raises(RuntimeError, match=text):
                capi.dev.atm_flag_failed(n, n, g.ptr, a.ptr, rows, np.ones(len(rows)), f.ptr, limit, 1)
        with pytest.raises(RuntimeError, match="shorter than their samples"):
            capi.dev.atm_flag_failed(n, n - 1, g.ptr, a.ptr, [0], [1], f.ptr, 3, 1)
        assert np.all(f.get() == 0)


# ================================================================================================ 4. k_atm_finish
@pytest.mark.parametrize("shape", [(n, s) for n in oc.N_FINISH for s in (False, True)], ids=shape_id)
def test_finish_grid(shape):
    from toast_amd import capi

    n, strided = shape
    stride, shift = oc.layout(n, strided)
    entries = 4
    rng = np.random.default_rng(8000 + n)
    times, quats = oc.cone_rows(n, entries, 8100 + n)
    quat_row, weight_row, data_row = oc.row_tables(entries, 3, 500 + n)
    good = (rng.uniform(size=(entries, n)) < 0.7).astype(np.uint8)
    good[1] = 1
    if n > 1:
        good[2, 1:] = 0
    atm = rng.standard_normal((entries, n)) * 5.0
    before = rng.standard_normal((entries, n)) * 10.0
    ga = np.array([0.143, 0.156, 0.169, 0.182])
    load = np.array([2.5, 2.75, 3.0, 3.25])
    before_buf = oc.embed(before, strided, oc.SENTINEL, n_rows=entries + 2, at=data_row)
    touched = oc.embed(good != 0, strided, False, n_rows=entries + 2, at=data_row)
    worst = 0.0
    with Pool() as pool:
        q = pool.dev(oc.embed(quats, strided, NAN, n_rows=entries + 2, at=quat_row))
        _, el = readout(pool, n, strided, q, entries + 2, quat_row)
        g = pool.dev(np.concatenate([good, np.ones((2, n), dtype=np.uint8)]))
        a = pool.dev(np.concatenate([atm, np.full((2, n), oc.SENTINEL)]))
        d = pool.dev(before_buf)
        for mode, (nnz, comp_i, comp_q) in oc.WEIGHT_MODES.items():
            weights = None if mode is None else oc.make_weights((entries, n), nnz, np.random.default_rng(8200 + n + nnz))
            w = None if mode is None else pool.dev(oc.embed(weights, strided, NAN, n_rows=entries + 2, at=weight_row))
            for loading in (None, load):
                for pfrac in (0.0, 0.1):
                    for scale in (1.0, 1000.0):
                        d.put(before_buf)
                        capi.dev.atm_finish(n, stride, g.ptr, a.ptr, ga, loading, quat_row, q.at(shift), entries + 2,
                                            None if mode is None else weight_row, 0 if mode is None else w.at(shift),
                                            entries + 2, nnz, comp_i, comp_q, pfrac, scale, data_row, d.at(shift),
                                            entries + 2)
                        got = d.get()
                        what = (mode, loading is not None, pfrac, scale)
                        # samples that are not good, rows no entry names and the samples around the window keep their bits
                        assert np.array_equal(bits(got[~touched]), bits(before_buf[~touched])), what
                        out = got[data_row, shift:shift + n]
                        for e in range(entries):
                            use = good[e] != 0
                            if not use.any():
                                continue
                            w_i, w_q = oc.weight_components(None if mode is None else weights[e], mode, n)
                            args = (before[e], atm[e], ga[e], w_i, w_q, pfrac, None if loading is None else loading[e],
                                    el[e], scale)
                            want, scale_i = oc.finish_longdouble(*args)
                            err = np.abs(out[e].astype(oc.L) - want)[use] / (oc.FINISH_ROUNDINGS * oc.EPS * scale_i[use])
                            worst = max(worst, float(err.max()))
                            if mode != "QU" or pfrac != 0.0 or loading is not None:
                                assert np.all(out[e][use] != before[e][use]), what
                            if mode is None and loading is None:
                                assert np.array_equal(bits(out[e][use]), bits(oc.finish_host(*args)[use])), what
    print(f"finish n={n} strided={strided}: worst error / bound {worst:.3f} (bound: {oc.FINISH_ROUNDINGS} eps scale_i)")
    assert worst <= 1.0


def test_finish_argument_errors():
    from toast_amd import capi

    n = 65
    with Pool() as pool:
        q = pool.dev(np.tile(np.array([0.0, 0.3, 0.0, 0.95]), (3, n, 1)))
        w = pool.dev(np.ones((3, n, 2)))
        g = pool.dev(np.ones((3, n), dtype=np.uint8))
        a = pool.dev(np.ones((3, n)))
        d = pool.dev(np.zeros((3, n)))

        def finish(rows, weight_row, nnz, comp_i, comp_q):
            k = len(rows)
            capi.dev.atm_finish(n, n, g.ptr, a.ptr, np.ones(k), None, rows, q.ptr, 3, weight_row, w.ptr, 3, nnz, comp_i, comp_q,
                                0.1, 1.0, rows, d.ptr, 3)

        for args, text in ((([0, 1], [0, 1], 2, 0, 2), "no such component"), (([0, 1], [0, 1], 2, 2, 0), "no such component"),
                           (([0, 1], None, 2, 0, 1), "need their rows"), (([0, 1], [0, 3], 2, 0, 1), "outside its array"),
                           ((np.zeros(65536, dtype=np.int32), np.zeros(65536, dtype=np.int32), 2, 0, 1), "too many rows")):
            with pytest.raises(RuntimeError, match=text):
                finish(*args)
        assert np.all(d.get() == 0)


# ================================================================================================ 5. the operator
def operator_run(variant, view, use_accel):
    from toast_amd.data import defaults

    data, ob, detectors = oc.operator_data(variant)
    names = [k for k in (defaults.det_data, defaults.det_flags, defaults.quats_azel, defaults.weights) if k in ob.detdata]
    if use_accel:
        for key in names:
            ob.detdata[key].accel_create(key)
            ob.detdata[key].accel_update_device()
    oc.operator_of(variant, view).apply(data, detectors=detectors, use_accel=use_accel)
    if use_accel:
        # resident data stays resident
        assert ob.detdata[defaults.det_data].accel_in_use()
        assert all(ob.detdata[key].accel_exists() for key in names)
    has_flags = defaults.det_flags in ob.detdata
    signal = ob.detdata[defaults.det_data].data.copy()
    flags = ob.detdata[defaults.det_flags].data.copy() if has_flags else None
    for key in names:
        if ob.detdata[key].accel_exists():
            ob.detdata[key].accel_delete()
    oc.close_sims(data, ob)
    return signal, flags


@pytest.mark.parametrize("view", oc.VIEW_FORMS)
@pytest.mark.parametrize("variant", list(oc.VARIANTS))
def test_operator_device_path_matches_its_host_path(variant, view):
    spec = oc.VARIANTS[variant]
    before = oc.operator_inputs(spec.get("nnz", 3))
    s_host, f_host = operator_run(variant, view, False)
    s_dev, f_dev = operator_run(variant, view, True)
    if spec.get("det_flags", True):
        assert np.array_equal(f_dev, f_host)
        if "det_flags" not in spec.get("traits", {}):
            assert np.any(f_host != before["det_flags"])
    else:
        assert f_dev is None and f_host is None                      # no flag array is created
    changed = bits(s_host) != bits(before["signal"])
    assert np.array_equal(bits(s_dev) != bits(before["signal"]), changed)
    named = [oc.OP_DETS.index(d) for d in (spec.get("detectors") or oc.OP_DETS)]
    assert not np.any(np.delete(changed, named, axis=0)) and np.all(changed[named].sum(axis=1) > 200)
    if view == "wind" and spec.get("det_flags", True) and oc.OP_WHOLLY_FLAGGED in named:
        assert not np.any(changed[oc.OP_WHOLLY_FLAGGED, :oc.OP_VIEWS[0][1]])
    err = float(np.max(np.abs(s_dev - s_host)) / np.max(np.abs(s_host)))
    print(f"operator {variant} view={view}: device against host path {err:.3e} of the largest value")
    assert err <= 1e-11
