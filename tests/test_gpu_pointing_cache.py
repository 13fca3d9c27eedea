"""GPU: the packed pointing cache of build_noise_weighted / scan_map (csrc/pointing_cache.hpp).

One small case with every edge of the pair kernels in it: 5 detectors (a lone last one), 1030 samples, Nside 64, three
intervals (one starting on an odd sample, one of odd length, one shorter than a workgroup trip), a shared-flag block
that gives -1 pixels, 0.5 % detector flags, a global2local with a non-local submap; buffers from ``capi.device_malloc``,
pointing from ``pixels_healpix`` + ``stokes_weights_IQU``.

Checked: the third eligible call packs and the later ones hit; every scan_map output equals the cache-disabled run bit for
bit; every map agrees with the oracle and with the cache-disabled run at test_gpu_parity's tolerance (max|dz| / max|z| <
1e-12: fp64 sums in another order); every event that should drop a seal does, is named in the counters, and the next
results are those of an un-cached computation; buffers the library does not own, odd n_samp, nnz 1 and deterministic mode
never hit."""

import numpy as np
import pytest

from toast_amd import capi, synth

pytestmark = pytest.mark.gpu

ZTOL = 1e-12          # tests/test_gpu_parity.py
N_DET, N_SAMP, NSIDE, NPS = 5, 1030, 64, 3072
N_SUBMAP = 12 * NSIDE * NSIDE // NPS
RATE = 10.0
D = capi.dev


def _intervals(n_samp=N_SAMP):
    ivl = np.zeros(3, dtype=synth.interval_dtype)
    for k, (a, b) in enumerate(((1, 301), (400, 707), (900, 950))):    # odd start; odd length; 50 samples
        b = min(b, n_samp)
        ivl[k] = (a / RATE, b / RATE, a, b)
    return ivl


class Arena:
    """Blocks from the library's arena with a torch view each (the library does not see what torch writes)."""

    def __init__(self):
        self.ptrs = []

    def block(self, shape, dtype, init=None):
        import torch

        tdt = {np.int64: torch.int64, np.float64: torch.float64, np.uint8: torch.uint8, np.float32: torch.float32}[dtype]
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = capi.device_malloc(nbytes)
        self.ptrs.append(ptr)

        class _B:
            pass

        b = _B()
        b.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=np.dtype(dtype).str, data=(ptr, False), version=3)
        t = torch.as_tensor(b, device="cuda")
        assert t.dtype == tdt and t.data_ptr() == ptr
        if init is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        else:
            t.zero_()
        torch.cuda.synchronize()
        return t

    def free(self, t):
        import torch

        torch.cuda.synchronize()
        self.ptrs.remove(t.data_ptr())
        capi.device_free(t.data_ptr())

    def close(self):
        import torch

        torch.cuda.synchronize()
        for p in self.ptrs:
            capi.device_free(p)
        self.ptrs = []


def _host_case(hwp, seed=11, prec_angle=7.0):
    rng = np.random.default_rng(seed)
    fp, gamma = synth.hex_focalplane(N_DET, fov_deg=10.0)
    c = dict(
        fp=fp, gamma=np.ascontiguousarray(gamma), eps=np.ascontiguousarray(0.02 * rng.random(N_DET)),
        cal=np.ascontiguousarray(1.0 + 0.1 * rng.random(N_DET)),
        bore=synth.satellite_boresight(N_SAMP, RATE, 30.0, 3.0, 300.0, prec_angle),
        sflags=synth.shared_flags_block(N_SAMP, 0.05, value=1),      # samples 381..431: inside the second interval
        dflags=synth.det_flags_random(N_DET, N_SAMP, 0.005, value=1, seed=seed + 1),
        tod=np.ascontiguousarray(rng.standard_normal((N_DET, N_SAMP))),
        det_scale=np.ascontiguousarray(0.5 + rng.random(N_DET)),
        det_w=np.linspace(0.5, 0.9, N_DET),
        hwp=(np.ascontiguousarray(2 * np.pi * ((np.arange(N_SAMP) * (9.0 / 60.0) / RATE) % 1.0)) if hwp else None),
        idx=np.arange(N_DET, dtype=np.int32), ivl=_intervals(),
    )
    return c


@pytest.fixture(scope="module")
def gpu():
    assert capi.accel_enabled(), "no HIP device visible"
    capi.accel_assign_device(1, 0, 1.0, False)
    yield
    capi.pointing_cache_enable(True)
    capi.set_deterministic(False)


class Setup:
    """Device buffers of one case, with the pointing expanded by the library's own calls."""

    def __init__(self, c, owned=True, n_samp=N_SAMP):
        import torch

        self.c, self.n_samp, self.owned = c, n_samp, owned
        self.A = Arena()
        self.keep = []
        mk = self.A.block if owned else self._torch_block
        self.bore = mk((n_samp, 4), np.float64, c["bore"][:n_samp])
        self.sflags = mk((n_samp,), np.uint8, c["sflags"][:n_samp])
        self.dflags = mk((N_DET, n_samp), np.uint8, c["dflags"][:, :n_samp])
        self.hwp = mk((n_samp,), np.float64, c["hwp"][:n_samp]) if c["hwp"] is not None else None
        self.quats = mk((N_DET, n_samp, 4), np.float64)
        self.pixels = mk((N_DET, n_samp), np.int64)
        self.weights = mk((N_DET, n_samp, 3), np.float64)
        self.tod = mk((N_DET, n_samp), np.float64, c["tod"][:, :n_samp])
        self.tod2 = mk((N_DET, n_samp), np.float64)
        self.hsub = mk((N_SUBMAP,), np.uint8)
        self.ivl = _intervals(n_samp)
        self.make_quats(self.bore, self.quats)
        self.expand_pixels()
        self.expand_weights()
        torch.cuda.synchronize()
        g2l, hit = synth.global_to_local(self.hsub.cpu().numpy())
        assert hit.size >= 2
        self.g2l_full = g2l.copy()
        g2l[hit[-1]] = -1                      # a hit submap that is not local: the last local submap stays empty
        self.g2l_h, self.n_local = g2l, int(hit.size)
        self.g2l = mk((N_SUBMAP,), np.int64, g2l)
        self.zmap = mk((self.n_local, NPS, 3), np.float64)
        # the map scan_map reads: a fixed one (the accumulated map differs from run to run in its last bits -- atomics --
        # and the scanned timestreams are compared bit for bit)
        self.smap = mk((self.n_local, NPS, 3), np.float64,
                       np.random.default_rng(5).standard_normal((self.n_local, NPS, 3)))
        # quaternions of another scan, for a re-expansion of the pixels later (made now: pointing_detector is not one of
        # the calls that leave seals alone)
        self.quats_other = mk((N_DET, n_samp, 4), np.float64)
        other = mk((n_samp, 4), np.float64, synth.satellite_boresight(n_samp, RATE, 30.0, 3.0, 300.0, 7.0, sample_offset=40))
        self.make_quats(other, self.quats_other)
        self.expand_pixels()
        self.expand_weights()

    def _torch_block(self, shape, dtype, init=None):
        import torch

        t = torch.zeros(tuple(shape), dtype={np.int64: torch.int64, np.float64: torch.float64, np.uint8: torch.uint8}[dtype],
                        device="cuda")
        if init is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(init)))
        self.keep.append(t)
        return t

    def make_quats(self, bore, quats):
        c = self.c
        D.pointing_detector(c["fp"], bore.data_ptr(), c["idx"], quats.data_ptr(), self.n_samp, self.ivl,
                            self.sflags.data_ptr(), self.n_samp, 1)

    def expand_pixels(self, quats=None):
        c = self.c
        q = self.quats if quats is None else quats
        D.pixels_healpix(c["idx"], q.data_ptr(), self.sflags.data_ptr(), self.n_samp, 1, c["idx"],
                         self.pixels.data_ptr(), self.n_samp, self.ivl, self.hsub.data_ptr(), N_SUBMAP, NPS, NSIDE, True)

    def expand_weights(self, weights=None):
        c = self.c
        w = self.weights if weights is None else weights
        hp, hn = (self.hwp.data_ptr(), self.n_samp) if self.hwp is not None else (0, 0)
        D.stokes_weights_IQU(c["idx"], self.quats.data_ptr(), c["idx"], w.data_ptr(), self.n_samp, hp, hn, self.ivl,
                             c["eps"], c["gamma"], c["cal"], False)

    def bnw(self):
        c = self.c
        self.zmap.zero_()
        D.build_noise_weighted(self.g2l.data_ptr(), self.zmap.data_ptr(), NPS, 3, c["idx"], self.pixels.data_ptr(), c["idx"],
                               self.weights.data_ptr(), c["idx"], self.tod.data_ptr(), c["idx"], self.dflags.data_ptr(),
                               self.n_samp, c["det_scale"], 1, self.n_samp, self.ivl, self.sflags.data_ptr(), self.n_samp, 1)
        return self.zmap.cpu().numpy()

    def scan(self, variant="subtract", map_dtype=np.float64):
        """tod2 <- tod, then scan_map of the fixed map into it; returns tod2."""
        import torch

        c = self.c
        self.tod2.copy_(self.tod)
        m = self.smap if map_dtype == np.float64 else self.smap.to(torch.float32)
        zero, sub, dw = {"zero": (True, False, None), "subtract": (False, True, None),
                         "fused": (False, True, c["det_w"])}[variant]
        D.scan_map(map_dtype, self.g2l.data_ptr(), NPS, m.data_ptr(), 3, self.tod2.data_ptr(), c["idx"],
                   self.pixels.data_ptr(), c["idx"], self.weights.data_ptr(), c["idx"], self.n_samp, self.ivl, 1.0, zero, sub,
                   False, dw)
        torch.cuda.synchronize()
        return self.tod2.cpu().numpy()

    def rounds(self, n):
        out = []
        for _ in range(n):
            out.append((self.bnw(), self.scan("fused")))
        return out

    def close(self):
        self.A.close()
        self.keep = []


VARIANTS = [(v, dt) for dt in (np.float64, np.float32) for v in ("zero", "subtract", "fused")]


def _sequence(c, enabled):
    """Expansion, four rounds, then every scan_map variant on the last map; also the counters."""
    capi.pointing_cache_enable(enabled)
    s = Setup(c)
    try:
        st0 = capi.pointing_cache_stats()
        r = s.rounds(4)
        st1 = capi.pointing_cache_stats()
        var = {(v, dt.__name__): s.scan(v, dt) for v, dt in VARIANTS}
        st2 = capi.pointing_cache_stats()
        pix, wts = s.pixels.cpu().numpy(), s.weights.cpu().numpy()
        return dict(rounds=r, variants=var, st=(st0, st1, st2), pixels=pix, weights=wts, g2l=s.g2l_full, n_local=s.n_local)
    finally:
        s.close()
        capi.pointing_cache_enable(True)


def _oracle(oracle, c, g2l, n_local):
    n = N_SAMP
    quats = np.zeros((N_DET, n, 4))
    oracle.pointing_detector(c["fp"], c["bore"], c["idx"], quats, c["ivl"], c["sflags"], 1)
    pixels = np.full((N_DET, n), -7, dtype=np.int64)
    hsub = np.zeros(N_SUBMAP, dtype=np.uint8)
    oracle.pixels_healpix(c["idx"], quats, c["sflags"], 1, c["idx"], pixels, c["ivl"], hsub, NPS, NSIDE, True)
    weights = np.zeros((N_DET, n, 3))
    hwp = c["hwp"] if c["hwp"] is not None else np.zeros(1)
    oracle.stokes_weights_IQU(c["idx"], quats, c["idx"], weights, hwp, c["ivl"], c["eps"], c["gamma"], c["cal"], False)
    zmap = np.zeros((n_local, NPS, 3))
    oracle.build_noise_weighted(g2l, zmap, c["idx"], pixels, c["idx"], weights, c["idx"], c["tod"], c["idx"], c["dflags"],
                                c["det_scale"], 1, c["ivl"], c["sflags"], 1)
    return pixels, zmap


def _close(a, b):
    return np.max(np.abs(a - b)) <= ZTOL * max(np.max(np.abs(b)), 1e-300)


@pytest.fixture(scope="module", params=[False, True], ids=["nohwp", "hwp"])
def both(request, gpu):
    c = _host_case(request.param)
    return c, _sequence(c, False), _sequence(c, True)


def test_packs_on_third_call_and_hits(both):
    _, off, on = both
    st0, st1, st2 = on["st"]
    d = {k: st1[k] - st0[k] for k in st1}
    assert d["seals"] == 0 and st0["live_seals"] == 2
    assert d["packs"] == 1
    assert d["hits"] >= 5 and d["hits"] == 6 and d["misses"] == 2       # calls 1, 2 miss; 3 .. 8 hit
    assert st1["packed_bytes"] == N_DET * N_SAMP * 20
    assert st2["hits"] - st1["hits"] == len(VARIANTS)
    o0, o1, o2 = off["st"]
    assert o2["hits"] == o0["hits"] and o2["packs"] == o0["packs"] and o1["live_seals"] == 0


def test_scan_map_bit_identical(both):
    _, off, on = both
    for (_, t_off), (_, t_on) in zip(off["rounds"], on["rounds"]):
        assert np.array_equal(t_off, t_on)
    for k in off["variants"]:
        assert np.array_equal(off["variants"][k], on["variants"][k]), k
    # the shared-flag block really gives samples without a pixel inside an interval
    assert np.any(on["pixels"][:, 400:707] == -1) and np.array_equal(off["pixels"], on["pixels"])


def test_maps_agree_with_oracle_and_uncached(both, oracle):
    c, off, on = both
    # (the oracle has no notion of a submap that is not local: it gets every hit submap, and the last local submap --
    #  the one the device runs leave out -- is compared with zero)
    pixels, zmap = _oracle(oracle, c, on["g2l"], on["n_local"])
    for iv in c["ivl"]:
        assert np.array_equal(pixels[:, iv["first"]:iv["last"]], on["pixels"][:, iv["first"]:iv["last"]])
    assert np.max(np.abs(zmap[:-1])) > 0 and np.max(np.abs(zmap[-1])) > 0
    zmap[-1] = 0.0
    for (z_off, _), (z_on, _) in zip(off["rounds"], on["rounds"]):
        assert not np.any(z_on[-1]) and not np.any(z_off[-1])
        assert _close(z_on, zmap) and _close(z_off, zmap) and _close(z_on, z_off)


def _fresh(s):
    """What the buffers hold now, computed without the cache."""
    capi.pointing_cache_enable(False)
    try:
        return s.bnw(), s.scan("fused")
    finally:
        capi.pointing_cache_enable(True)


def _packed_setup(c):
    s = Setup(c)
    before = s.rounds(2)          # the third call packs
    assert capi.pointing_cache_stats()["live_seals"] == 2
    assert capi.pointing_cache_stats()["packed_bytes"] == N_DET * N_SAMP * 20
    return s, before


def _check_after_drop(s, before, changed=True):
    st = capi.pointing_cache_stats()
    h0 = st["hits"]
    z, t = s.bnw(), s.scan("fused")
    assert capi.pointing_cache_stats()["hits"] == h0
    z_f, t_f = _fresh(s)
    assert np.array_equal(t, t_f) and _close(z, z_f)
    if changed:
        assert not _close(z, before[-1][0])       # ... and the stale copy would have shown
    return st


def test_reseal_from_other_boresight(gpu):
    c = _host_case(False)
    s, before = _packed_setup(c)
    try:
        r0 = capi.pointing_cache_stats()["drops_reseal"]
        s.expand_pixels(s.quats_other)
        st = _check_after_drop(s, before)
        assert st["drops_reseal"] == r0 + 1
    finally:
        s.close()


def test_manager_upload_into_weights(gpu):
    c = _host_case(False)
    host_w = np.zeros((N_DET, N_SAMP, 3))
    capi.accel_create(host_w, "weights")
    s = None
    try:
        import torch

        s = Setup(c)

        class _B:
            pass

        b = _B()
        b.__cuda_array_interface__ = dict(shape=host_w.shape, typestr="<f8", data=(capi.accel_device_ptr(host_w), False), version=3)
        s.weights = torch.as_tensor(b, device="cuda")      # the manager's block from now on
        s.expand_weights()
        before = s.rounds(2)
        assert capi.pointing_cache_stats()["packed_bytes"] == N_DET * N_SAMP * 20
        m0 = capi.pointing_cache_stats()["drops_manager"]
        torch.cuda.synchronize()
        host_w[...] = s.weights.cpu().numpy()
        host_w[:, :, 1:] *= 0.5
        capi.accel_update_device(host_w, "weights")
        st = _check_after_drop(s, before)
        assert st["drops_manager"] == m0 + 1
    finally:
        if s is not None:
            s.close()
        capi.accel_delete(host_w, "weights")


def test_scan_map_into_the_weights_block(gpu):
    c = _host_case(False)
    s, before = _packed_setup(c)
    try:
        o0 = capi.pointing_cache_stats()["drops_overlap_write"]
        # a timestream of two rows that lies inside the weights block
        D.scan_map(np.float64, s.g2l.data_ptr(), NPS, s.smap.data_ptr(), 3, s.weights.data_ptr(), c["idx"][:2],
                   s.pixels.data_ptr(), c["idx"][:2], s.weights.data_ptr(), c["idx"][:2], N_SAMP, s.ivl, 1.0, True, False, False,
                   None)
        st = capi.pointing_cache_stats()
        assert st["drops_overlap_write"] == o0 + 1 and st["live_seals"] == 1      # (the pixels are still sealed)
        _check_after_drop(s, before)
    finally:
        s.close()


def test_non_whitelisted_call(gpu):
    c = _host_case(False)
    s, before = _packed_setup(c)
    try:
        f0 = capi.pointing_cache_stats()["drops_foreign_call"]
        D.memset(s.pixels.data_ptr(), 0, 8 * N_SAMP * 2)      # two rows of pixel 0
        st = _check_after_drop(s, before)
        assert st["drops_foreign_call"] == f0 + 2 and st["live_seals"] == 0
    finally:
        s.close()


def test_free_the_block(gpu):
    c = _host_case(False)
    s, before = _packed_setup(c)
    try:
        import torch

        f0 = capi.pointing_cache_stats()["drops_free"]
        w = s.weights.cpu().numpy()
        s.A.free(s.weights)
        assert capi.pointing_cache_stats()["drops_free"] == f0 + 1
        w[:, :, 1] *= -1.0
        s.weights = s.A.block((N_DET, N_SAMP, 3), np.float64, w)       # most likely the same address
        torch.cuda.synchronize()
        _check_after_drop(s, before)
    finally:
        s.close()


def _never_hits(run):
    st0 = capi.pointing_cache_stats()
    run()
    st1 = capi.pointing_cache_stats()
    assert st1["hits"] == st0["hits"] and st1["packs"] == st0["packs"]


def test_torch_owned_buffers_never_hit(gpu):
    s = Setup(_host_case(False), owned=False)
    try:
        assert capi.pointing_cache_stats()["live_seals"] == 0
        _never_hits(lambda: s.rounds(4))
    finally:
        s.close()


def test_odd_n_samp_never_hits(gpu):
    c = _host_case(False)
    c["ivl"] = _intervals(N_SAMP - 1)
    s = Setup(c, n_samp=N_SAMP - 1)
    try:
        _never_hits(lambda: s.rounds(4))
    finally:
        s.close()


def test_nnz1_never_hits(gpu):
    c = _host_case(False)
    s = Setup(c)
    try:
        w1 = s.A.block((N_DET, N_SAMP), np.float64)
        z1 = s.A.block((s.n_local, NPS, 1), np.float64)
        D.stokes_weights_I(c["idx"], w1.data_ptr(), N_SAMP, s.ivl, c["cal"])

        def run():
            for _ in range(4):
                D.build_noise_weighted(s.g2l.data_ptr(), z1.data_ptr(), NPS, 1, c["idx"], s.pixels.data_ptr(), c["idx"],
                                       w1.data_ptr(), c["idx"], s.tod.data_ptr(), c["idx"], s.dflags.data_ptr(), N_SAMP,
                                       c["det_scale"], 1, N_SAMP, s.ivl, s.sflags.data_ptr(), N_SAMP, 1)
                D.scan_map(np.float64, s.g2l.data_ptr(), NPS, z1.data_ptr(), 1, s.tod2.data_ptr(), c["idx"],
                           s.pixels.data_ptr(), c["idx"], w1.data_ptr(), c["idx"], N_SAMP, s.ivl, 1.0, False, True, False, None)

        _never_hits(run)
    finally:
        s.close()


def test_deterministic_mode_never_hits(gpu):
    capi.set_deterministic(True)
    try:
        s = Setup(_host_case(False))
        try:
            assert capi.pointing_cache_stats()["live_seals"] == 0
            _never_hits(lambda: s.rounds(4))
        finally:
            s.close()
    finally:
        capi.set_deterministic(False)


def test_on_the_fly_expansion_seals_too(gpu):
    """Pixels and weights written by the quaternion-free expansion calls are sealed like the others: the third call
    packs, and what the packed kernels compute is what an un-cached run computes from the same arrays."""
    c = _host_case(False)
    s = Setup(c)
    try:
        pt = capi.otf_pointing(s.bore.data_ptr(), c["fp"], NSIDE, True, 3, d_shared_flags=s.sflags.data_ptr(),
                               n_shared_flags=N_SAMP, shared_flag_mask=1, epsilon=c["eps"], gamma=c["gamma"], cal=c["cal"])
        st0 = capi.pointing_cache_stats()
        D.otf_pixels_healpix(pt, c["idx"], s.pixels.data_ptr(), N_SAMP, s.ivl, s.hsub.data_ptr(), N_SUBMAP, NPS)
        D.otf_stokes_weights(pt, c["idx"], s.weights.data_ptr(), N_SAMP, s.ivl)
        st1 = capi.pointing_cache_stats()
        assert st1["live_seals"] == 2 and st1["drops_reseal"] == st0["drops_reseal"] + 2
        r = s.rounds(3)
        st2 = capi.pointing_cache_stats()
        assert st2["packs"] == st1["packs"] + 1 and st2["hits"] == st1["hits"] + 4
        z_f, t_f = _fresh(s)
        assert np.array_equal(r[-1][1], t_f) and _close(r[-1][0], z_f)
        assert np.max(np.abs(z_f)) > 0
    finally:
        s.close()
