"""GPU: the demodulation kernels (csrc/demod.hip) and the device paths of ops.Demodulate / ops.StokesWeightsDemod.

* FIR kernel grid against a long-double direct sum evaluated here with NumPy: |device - long double| as a fraction of
  sum |h| max |m x| <= 4 x max(fft_ref_err, direct_ref_err) of the fixture.  The kernel differs from the fixture's
  double direct sum only in the order over the taps (by decimation phase) and in FMA contraction, each worth at most a
  factor of about two in the standard summation bound.
* Flags kernel: equal to the host statement for n below, at and above wkernel and every offset.
* Determinism: identical bits across a repeated call, two batch sizes and a permuted row order.
* Operator on resident data against the fixture (same bound) and against its own host path; the outputs stay resident
  and no timestream is downloaded.
* Recovery of constant I0, Q0, U0 within 10 x the leakage of the reference's method on the same input (fixture).

Every figure is printed before it is asserted."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import demod_case as dc  # noqa: E402

pytestmark = pytest.mark.gpu

G = dc.gold()
BOUND = 4.0 * max(float(G["fft_ref_err"]), float(G["direct_ref_err"]))
L = np.longdouble


class Dev:
    """A host array with a device copy."""

    def __init__(self, arr):
        from toast_amd.accel import accel_data_create, accel_data_update_device, accel_device_ptr

        self.a = np.array(arr, order="C", copy=True)
        accel_data_create(self.a, "test_demod")
        accel_data_update_device(self.a, "test_demod")
        self.ptr = accel_device_ptr(self.a)

    def get(self):
        from toast_amd.accel import accel_data_update_host

        accel_data_update_host(self.a, "test_demod")
        return self.a.copy()

    def free(self):
        from toast_amd.accel import accel_data_delete

        accel_data_delete(self.a, "test_demod")


def n_out_of(n, nskip, off):
    return len(range(off % nskip, n, nskip))


def device_fir(d_x, n_rows, n, h, nskip, off, in_row, mode=0, d_mod=None, mod_row=None, mod_comp=None, nnz=3, out_rows=None):
    """toast_hip_demod_fir_dev into a fresh output [len(in_row)][n_out] (returned with a guard column intact)."""
    from toast_amd import capi

    ne = len(in_row)
    n_out = n_out_of(n, nskip, off)
    d_out = Dev(np.full((ne, n_out + 1), -7.0))
    out_row = list(range(ne)) if out_rows is None else out_rows
    try:
        kw = {}
        if mode == capi.DEMOD_MOD_WEIGHTS:
            kw = dict(mod_mode=mode, d_mod=d_mod.ptr, n_mod_rows=d_mod.a.shape[0], mod_stride=n * nnz, mod_row=mod_row,
                      mod_comp=mod_comp, nnz=nnz, comp_q=nnz - 2)
        elif mode == capi.DEMOD_MOD_ARRAY:
            kw = dict(mod_mode=mode, d_mod=d_mod.ptr, n_mod_rows=d_mod.a.shape[0], mod_stride=n, mod_row=mod_row)
        capi.dev.demod_fir(n, h, nskip, off, d_x.ptr, n_rows, n, in_row, d_out.ptr, ne, n_out + 1, out_row, **kw)
        capi.synchronize()
        got = d_out.get()
    finally:
        d_out.free()
    assert np.all(got[:, n_out] == -7.0), "the kernel wrote past the end of a row"
    return got[:, :n_out]


NROW = 5
W_VALUES = (1, 2, 3, 63, 64, 255, 513, 1023, 2047, 7 * 512 + 1)     # 513 / 3585: just past the tap chunk (nskip 1 / 7)
DECIMATIONS = ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (7, 0), (7, 1), (7, 6))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4099])
def test_fir_kernel_grid(n):
    from toast_amd import capi

    assert capi.DEMOD_TAP_CHUNK == 512
    rng = np.random.default_rng(5000 + n)
    x = 50.0 + rng.standard_normal((NROW, n))
    ang = rng.uniform(0, 2 * np.pi, (NROW, n))
    eta = rng.uniform(0.5, 1.0, (NROW, 1))
    w = np.stack([np.ones((NROW, n)), eta * np.cos(ang), eta * np.sin(ang)], axis=2)
    arr = rng.standard_normal((NROW, n))
    # the modulated inputs in double, the reference's statements
    mods = {0: [x], 2: [x * arr]}
    qn, un = zip(*(dc.normalised(w[r][:, 1:]) for r in range(NROW)))
    mods[1] = [x * 2 * np.array(qn), x * 2 * np.array(un)]
    d_x, d_w, d_arr = Dev(x), Dev(w), Dev(arr)
    worst, count = 0.0, 0
    try:
        for iw, W in enumerate(W_VALUES):
            h = rng.standard_normal(W) / np.sqrt(W)
            hsum = float(np.sum(np.abs(h)))
            for mode in (0, 1, 2):
                full = [np.array([dc.same_longdouble(y[r], h) for r in range(NROW)]) for y in mods[mode]]
                scales = [hsum * np.max(np.abs(y), axis=1) for y in mods[mode]]
                for idec, (nskip, off) in enumerate(DECIMATIONS):
                    for rows in (list(range(NROW)), [(iw + idec) % NROW]):
                        if mode == 0:
                            got = [device_fir(d_x, NROW, n, h, nskip, off, rows)]
                        elif mode == 1:
                            both = device_fir(d_x, NROW, n, h, nskip, off, rows + rows, mode=1, d_mod=d_w,
                                              mod_row=rows + rows, mod_comp=[1] * len(rows) + [2] * len(rows))
                            got = [both[:len(rows)], both[len(rows):]]
                        else:
                            got = [device_fir(d_x, NROW, n, h, nskip, off, rows, mode=2, d_mod=d_arr, mod_row=rows)]
                        for g, f, s in zip(got, full, scales):
                            want = f[rows][:, off % nskip:: nskip]
                            assert g.shape == want.shape
                            if want.size == 0:          # the offset lies past the end of the row: no output
                                continue
                            dist = float(np.max(np.abs(g.astype(L) - want) / s[rows][:, None].astype(L)))
                            worst = max(worst, dist)
                            count += 1
    finally:
        for d in (d_x, d_w, d_arr):
            d.free()
    print(f"n {n}: {count} comparisons over W {W_VALUES}, (nskip, offset) {DECIMATIONS}, 1 and {NROW} rows, three "
          f"modulation modes: worst distance {worst:.3e}; bound {BOUND:.3e}")
    assert worst <= BOUND


@pytest.mark.parametrize("n", [700, 1023, 1024, 5001])
def test_flags_kernel(n):
    from toast_amd import capi, ops

    wk = 1023
    flags = np.array(G["det_flags"][:, :n])
    op = ops.Demodulate(demod_flag_mask=3)
    d_in = Dev(flags)
    try:
        for nskip, off in DECIMATIONS:
            op.nskip = nskip
            n_out = n_out_of(n, nskip, off)
            d_out = Dev(np.full((4, n_out + 1), 200, dtype=np.uint8))
            try:
                capi.dev.demod_flags(n, wk, 3, nskip, off, d_in.ptr, 3, n, [2, 0, 1, 0], d_out.ptr, 4, n_out + 1, [0, 1, 3, 2])
                capi.synchronize()
                got = d_out.get()
            finally:
                d_out.free()
            assert np.all(got[:, n_out] == 200)
            for r_in, r_out in zip([2, 0, 1, 0], [0, 1, 3, 2]):
                assert np.array_equal(got[r_out, :n_out], op._demodulate_flag(flags[r_in], wk, off)), (n, nskip, off)
    finally:
        d_in.free()


def test_determinism():
    from toast_amd import capi

    n, W, nskip, off = 4099, 1023, 3, 1
    rng = np.random.default_rng(77)
    x = 10.0 + rng.standard_normal((NROW, n))
    ang = rng.uniform(0, 2 * np.pi, (NROW, n))
    w = np.stack([np.ones((NROW, n)), 0.8 * np.cos(ang), 0.8 * np.sin(ang)], axis=2)
    h = rng.standard_normal(W)
    d_x, d_w = Dev(x), Dev(w)
    try:
        def run(rows):
            return device_fir(d_x, NROW, n, h, nskip, off, rows, mode=capi.DEMOD_MOD_WEIGHTS, d_mod=d_w, mod_row=rows,
                              mod_comp=[1 + (r % 2) for r in rows])

        all_rows = list(range(NROW))
        first = run(all_rows)
        assert np.array_equal(first, run(all_rows)), "a repeated call changed bits"
        singles = np.vstack([run([r]) for r in all_rows])
        assert np.array_equal(first, singles), "the batch size changed bits"
        perm = [3, 0, 4, 2, 1]
        shuffled = run(perm)
        assert np.array_equal(first[perm], shuffled), "the row order changed bits"
    finally:
        d_x.free()
        d_w.free()


def _tod_distance(dd, case):
    worst = 0.0
    keys = [k for k in G.files if k.startswith(f"{case}_tod_")]
    assert sorted(k[len(case) + 5:] for k in keys) == sorted(dd.detectors)
    for k in keys:
        name = k[len(case) + 5:]
        prefix, det = name.split("_", 1)
        x = G["signal"][dc.DETS.index(det)]
        s0 = float(np.sum(np.abs(G[f"{case}_lpf"])) * np.max(np.abs(x)))
        band = G[f"{case}_bpf2"] if prefix.startswith("demod2") else G[f"{case}_bpf4"]
        scale = s0 if prefix == "demod0" else 2.0 * float(np.sum(np.abs(band))) * s0
        worst = max(worst, float(np.max(np.abs(dd[name] - G[k])) / scale))
    return worst


@pytest.mark.parametrize("case", sorted(dc.CASES))
def test_operator_resident(case):
    from toast_amd.data import defaults

    op, data, out = dc.demodulate(G, case, resident=True)
    ob, dob = data.obs[0], out.obs[0]
    dd = dob.detdata[defaults.det_data]
    # everything stayed on the device: the input was not downloaded, the outputs are resident and current there
    assert ob.detdata[defaults.det_data].accel_in_use()
    assert dd.accel_in_use() and dob.detdata[defaults.det_flags].accel_in_use()
    if case == "default":
        assert type(op.stokes_weights).calls == 1, "the weights are computed per batch of detectors"
    dist = _tod_distance(dd, case)            # the first host access copies the outputs back
    print(f"{case}: device path against the fixture {dist:.3e} of the scale; bound {BOUND:.3e}")
    assert dist <= BOUND

    _, _, host = dc.demodulate(G, case)
    hd = host.obs[0].detdata[defaults.det_data]
    worst = 0.0
    for name in hd.detectors:
        prefix, det = name.split("_", 1)
        x = G["signal"][dc.DETS.index(det)]
        s0 = float(np.sum(np.abs(G[f"{case}_lpf"])) * np.max(np.abs(x)))
        band = G[f"{case}_bpf2"] if prefix.startswith("demod2") else G[f"{case}_bpf4"]
        scale = s0 if prefix == "demod0" else 2.0 * float(np.sum(np.abs(band))) * s0
        worst = max(worst, float(np.max(np.abs(dd[name] - hd[name])) / scale))
    print(f"{case}: device path against the host path {worst:.3e} of the scale; bound {BOUND:.3e}")
    assert worst <= BOUND
    assert np.array_equal(dob.detdata[defaults.det_flags].data, host.obs[0].detdata[defaults.det_flags].data)
    assert np.array_equal(dob.shared[defaults.shared_flags].data, host.obs[0].shared[defaults.shared_flags].data)


def test_operator_batches_do_not_change_bits():
    from toast_amd.data import defaults

    _, _, one = dc.demodulate(G, "default", resident=True)
    op, data, out = dc.demodulate(G, "default", use_accel=True)      # uploaded by the operator
    a = one.obs[0].detdata[defaults.det_data].data
    assert np.array_equal(a, out.obs[0].detdata[defaults.det_data].data)
    from toast_amd import ops

    data = dc.make_obs(G)
    op = ops.Demodulate(stokes_weights=dc.fixed_weights_operator(dc.weight_table(G)), nskip=dc.NSKIP)
    op.max_batch = 2
    out2 = op.apply(data, use_accel=True)
    assert np.array_equal(a, out2.obs[0].detdata[defaults.det_data].data)


def test_recovery():
    from toast_amd.data import defaults

    op, data, out = dc.demodulate(G, "default", resident=True, signal=dc.recovery_signal(G))
    dob = out.obs[0]
    assert dob.detdata[defaults.det_data].accel_in_use()
    tod = {d: dob.detdata[defaults.det_data][d] for d in dob.local_detectors}
    # the samples the fixture's leakage was measured on: all but the first and last wkernel
    ends = op._demodulate_flag(np.zeros(dc.N, dtype=np.uint8), int(G["wkernel"]), 0)
    flags = {d: ends for d in dob.local_detectors}
    leak = dc.recovery_leak(tod, flags, dc.DETS)
    bound = 10.0 * float(G["recovery_leak"])
    print(f"recovery: largest deviation from (I0, eta Q0, eta U0) on the interior {leak:.3e}; bound {bound:.3e} "
          f"(10 x the host path's {float(G['recovery_leak']):.3e})")
    assert leak <= bound


@pytest.mark.parametrize("single", [False, True])
def test_stokes_weights_demod_device(single):
    from toast_amd import ops

    op, data, out = dc.demodulate(G, "2f", resident=True)
    ops.StokesWeightsDemod(mode="IQU", single_precision=single).apply(out)
    w = out.obs[0].detdata["weights"]
    assert w.accel_in_use(), "resident timestreams get resident weights"
    dev = {d: np.array(w[d]) for d in w.detectors}
    _, _, host = dc.demodulate(G, "2f")
    ops.StokesWeightsDemod(mode="IQU", single_precision=single).apply(host)
    hw = host.obs[0].detdata["weights"]
    assert not hw.accel_in_use() and hw.dtype == w.dtype
    for d in w.detectors:
        assert np.array_equal(dev[d], hw[d]), d
    assert np.array_equal(dev["demod4i_D0"][17], np.array([0.0, 0.0, dc.ETA[0]], dtype=w.dtype))


# ---------------------------------------------------------------------------------------------- pybind entries
def test_pybind_entries():
    """_libtoast_hip.demod_fir / demod_flags / stokes_weights_demod against the ctypes entries: same bits."""
    from toast_amd import capi
    from toast_amd.accel import native

    nat = native()
    n, nskip, off = 1000, 3, 1
    n_out = n_out_of(n, nskip, off)
    rng = np.random.default_rng(9)
    x = 5.0 + rng.standard_normal((2, n))
    ang = rng.uniform(0, 2 * np.pi, (2, n))
    w = np.stack([np.ones((2, n)), 0.7 * np.cos(ang), 0.7 * np.sin(ang)], axis=2)
    arr = rng.standard_normal((2, n))
    h = rng.standard_normal(65)
    i32 = lambda v: np.array(v, dtype=np.int32)       # noqa: E731
    none = i32([])
    d_x, d_w, d_arr = Dev(x), Dev(w), Dev(arr)
    try:
        for mode, d_mod, stride, rows, comp in ((capi.DEMOD_MOD_NONE, None, 0, none, none),
                                                (capi.DEMOD_MOD_WEIGHTS, d_w, n * 3, i32([1, 0]), i32([2, 1])),
                                                (capi.DEMOD_MOD_ARRAY, d_arr, n, i32([1, 0]), none)):
            d_out = Dev(np.zeros((2, n_out)))
            try:
                nat.demod_fir(n, h, nskip, off, d_x.ptr, 2, n, i32([1, 0]), mode, 0 if d_mod is None else d_mod.ptr, 2, stride,
                              rows, comp, 3, 1, d_out.ptr, 2, n_out, i32([0, 1]))
                capi.synchronize()
                got = d_out.get()
            finally:
                d_out.free()
            want = device_fir(d_x, 2, n, h, nskip, off, [1, 0], mode=mode, d_mod=d_mod,
                              mod_row=None if mode == 0 else [1, 0], mod_comp=[2, 1] if mode == 1 else None)
            assert np.array_equal(got, want), mode
        with pytest.raises(RuntimeError):      # the weights mode needs one component per entry
            nat.demod_fir(n, h, nskip, off, d_x.ptr, 2, n, i32([1, 0]), capi.DEMOD_MOD_WEIGHTS, d_w.ptr, 2, n * 3, i32([1, 0]),
                          none, 3, 1, d_x.ptr, 2, n, i32([0, 1]))
    finally:
        for d in (d_x, d_w, d_arr):
            d.free()

    from toast_amd import ops

    flags = np.array(G["det_flags"][:2, :n])
    d_f, d_o = Dev(flags), Dev(np.zeros((2, n_out), dtype=np.uint8))
    try:
        nat.demod_flags(n, 100, 2, nskip, off, d_f.ptr, 2, n, i32([1, 0]), d_o.ptr, 2, n_out, i32([0, 1]))
        capi.synchronize()
        got = d_o.get()
    finally:
        d_f.free()
        d_o.free()
    op = ops.Demodulate(demod_flag_mask=2, nskip=nskip)
    assert np.array_equal(got[0], op._demodulate_flag(flags[1], 100, off))
    assert np.array_equal(got[1], op._demodulate_flag(flags[0], 100, off))

    for single, dt in ((False, np.float64), (True, np.float32)):
        d_wt = Dev(np.full((3, 50, 3), 9, dtype=dt))
        try:
            nat.stokes_weights_demod(50, np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.75]]), i32([2, 0]), d_wt.ptr, 3, single)
            capi.synchronize()
            got = d_wt.get()
        finally:
            d_wt.free()
        assert np.all(got[2] == np.array([1, 0, 0], dtype=dt)) and np.all(got[0] == np.array([0, 0, 0.75], dtype=dt))
        assert np.all(got[1] == 9)


# ---------------------------------------------------------------------------------------------- end to end
E2E = {}


def _e2e_inputs():
    """A tiny HWP simulation (2 detectors x 6000 samples at 100 Hz, HWP at 2 Hz) and its signal, made once."""
    if not E2E:
        rng = np.random.default_rng(31)
        E2E["signal"] = 10.0 + rng.standard_normal((2, 6000))
    return E2E["signal"]


def _e2e_map(resident, full_pointing):
    """Demodulate -> StokesWeightsDemod -> MapMaker without templates (covariance, hits, BinMap)."""
    from toast_amd import ops
    from toast_amd.data import defaults
    from toast_amd.sim import create_satellite_data

    data = create_satellite_data(n_det=2, n_samp=6000, rate=100.0, spin_period_s=60.0, spin_angle_deg=30.0,
                                 prec_period_s=600.0, prec_angle_deg=65.0, hwp_rpm=120.0)
    dd = data.obs[0].detdata[defaults.det_data]
    dd.data[:] = _e2e_inputs()
    if resident:
        dd.accel_create(defaults.det_data)
        dd.accel_update_device()
    dp = ops.PointingDetectorSimple()
    sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", hwp_angle=defaults.hwp_angle)
    demod = ops.Demodulate(stokes_weights=sw, nskip=3)
    out = demod.apply(data, use_accel=True if resident else False)
    dob = out.obs[0]
    assert dob.detdata[defaults.det_data].accel_in_use() == resident
    tod = None
    if not resident:
        tod = {d: np.array(dob.detdata[defaults.det_data][d]) for d in dob.local_detectors}
    pix = ops.PixelsHealpix(detector_pointing=ops.PointingDetectorSimple(), nside=16, nest=True)
    swd = ops.StokesWeightsDemod(mode="IQU")
    binner = ops.BinMap(pixel_dist="pixel_dist", pixel_pointing=pix, stokes_weights=swd, full_pointing=full_pointing)
    ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=None).apply(out)
    hits = np.array(out["mm_hits"].data).reshape(-1)
    return np.array(out["mm_map"].data).reshape(-1, 3), hits, tod, demod


@pytest.mark.parametrize("full_pointing", [True, False])
def test_end_to_end_binmap(full_pointing):
    """The binned map of the demodulated data is the same on the device and the host path.  With the constant unit
    weights of the pseudo-detectors the covariance is diagonal and every map value is a weighted mean of the
    demodulated samples that hit the pixel: a difference delta between the two paths' timestreams moves it by at most
    delta, i.e. BOUND x the chain's scale, and the two accumulations of at most max(hits) samples, whose order is
    not fixed, differ by at most 2 x max(hits) x 2^-53 x max |sample| (the standard summation bound)."""
    m_dev, h_dev, _, _ = _e2e_map(True, full_pointing)
    m_host, h_host, tod, demod = _e2e_map(False, full_pointing)
    assert np.array_equal(h_dev, h_host) and np.count_nonzero(h_host) > 10
    x = _e2e_inputs()
    fmod = 2.0
    from toast_amd.ops.demodulation import Bandpass, Lowpass

    lpf = Lowpass(0.95 * fmod, 100.0).lpf
    bpf = Bandpass(3.05 * fmod, 4.95 * fmod, 100.0).bpf
    s0, s4 = dc.chain_scales(x, lpf, bpf)
    top = max(float(np.max(np.abs(v))) for v in tod.values())
    sum_term = 2.0 * float(np.max(h_host)) * 2.0 ** -53 * top
    good = h_host > 0
    assert np.all(np.isfinite(m_host[good]))
    worst_i = float(np.max(np.abs(m_dev[good, 0] - m_host[good, 0])))
    worst_p = float(np.max(np.abs(m_dev[good, 1:] - m_host[good, 1:])))
    print(f"full_pointing {full_pointing}: {np.count_nonzero(good)} hit pixels; I map difference {worst_i:.3e} (bound "
          f"{BOUND * s0 + sum_term:.3e}); Q / U {worst_p:.3e} (bound {BOUND * s4 + sum_term:.3e})")
    assert np.any(m_host[good, 0] != 0) and np.any(m_host[good, 1] != 0)
    assert worst_i <= BOUND * s0 + sum_term
    assert worst_p <= BOUND * s4 + sum_term
