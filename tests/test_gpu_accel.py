"""GPU: mirrors of the reference's accelerator tests (src/toast/tests/accelerator.py):
``test_memory`` (:131-184: create / update_device / update_host / delete round trip for every
dtype) and ``test_data_stage`` (:186-351: Data.accel_create / update_device / update_host /
delete by requires()-style dictionaries over detdata, shared and global objects)."""
import os

import numpy as np
import pytest

from toast_amd import accel
from toast_amd.data import SharedData, defaults
from toast_amd.pixels import PixelData, PixelDistribution
from toast_amd.sim import create_satellite_data

pytestmark = pytest.mark.gpu

TYPES = {"f64": np.float64, "f32": np.float32, "i64": np.int64, "i32": np.int32, "i16": np.int16, "i8": np.int8,
         "u64": np.uint64, "u32": np.uint32, "u16": np.uint16, "u8": np.uint8}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert accel.accel_enabled()
    accel.accel_assign_device(1, 0, 1.0, False)


def test_memory():
    data = {k: np.ones(100, dtype=tp) for k, tp in TYPES.items()}
    check = {k: 2 * np.array(v) for k, v in data.items()}
    for buf in data.values():
        assert not accel.accel_data_present(buf)
    for buf in data.values():
        accel.accel_data_create(buf)
        accel.accel_data_update_device(buf)
    for buf in data.values():
        assert accel.accel_data_present(buf)
    with pytest.raises(RuntimeError, match="already present"):
        accel.accel_data_create(data["f64"])
    for buf in data.values():
        buf[:] *= 2
        accel.accel_data_update_device(buf)
        buf[:] = 0
    for k, buf in data.items():
        accel.accel_data_update_host(buf)
        np.testing.assert_array_equal(buf, check[k])
    # reset zeroes the device copy only
    accel.accel_data_reset(data["i32"])
    np.testing.assert_array_equal(data["i32"], check["i32"])
    accel.accel_data_update_host(data["i32"])
    assert not np.any(data["i32"])
    for buf in data.values():
        accel.accel_data_delete(buf)
        assert not accel.accel_data_present(buf)
    with pytest.raises(RuntimeError, match="not present"):
        accel.accel_data_update_host(data["f64"])


def test_data_stage():
    data = create_satellite_data(n_det=4, n_samp=300)
    data.lazy_host = False
    ob = data.obs[0]
    names = {"global": ["test_pix"], "meta": [], "detdata": [], "shared": [], "intervals": []}
    for itp, (tname, tp) in enumerate(TYPES.items()):
        for sname, sshape in (("1", ()), ("2", (2,))):
            name = f"{tname}_{sname}"
            ob.detdata.create(name, sample_shape=sshape, dtype=tp)
            ob.detdata[name].data[:] = itp + 1
            ob.shared[name] = SharedData((itp + 1) * np.ones((ob.n_local_samples,) + sshape, dtype=tp), name)
            names["detdata"].append(name)
            names["shared"].append(name)
    dist = PixelDistribution(n_pix=100, n_submap=10, local_submaps=[0, 2, 4, 6, 8])
    data["test_pix"] = PixelData(dist, np.float64, n_value=3)
    data["test_pix"].data[:] = 7.0
    data.accel_create(names)
    data.accel_update_device(names)
    # clearing the host buffers does not touch the device copies
    for name in names["detdata"]:
        ob.detdata[name].buffer[:] = 0
        ob.shared[name].data[:] = 0
    data["test_pix"].buffer[:] = 0
    for name in names["detdata"]:
        assert ob.detdata[name].accel_in_use() and ob.shared[name].accel_in_use()
    data.accel_update_host(names)
    for itp, (tname, tp) in enumerate(TYPES.items()):
        for sname in ("1", "2"):
            name = f"{tname}_{sname}"
            assert np.all(ob.detdata[name].data == itp + 1), name
            assert np.all(ob.shared[name].data == itp + 1), name
            assert not ob.detdata[name].accel_in_use()
    assert np.all(data["test_pix"].data == 7.0)
    data.accel_delete(names)
    for name in names["detdata"]:
        assert not ob.detdata[name].accel_exists() and not ob.shared[name].accel_exists()
    assert not data["test_pix"].accel_exists()
    assert defaults.det_data in ob.detdata   # untouched objects stay where they were


_EVICT_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.ops.pipeline import Pipeline
from toast_amd.sim import create_satellite_data

data = create_satellite_data(n_det=4, n_samp=100000)
dp = ops.PointingDetectorSimple()
pix = ops.PixelsHealpix(detector_pointing=dp, nside=64, skip_quaternions=False)
sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", skip_quaternions=False)
Pipeline(operators=[dp, pix, sw]).apply(data)          # quats 12.8 MB + pixels 3.2 MB + weights 9.6 MB stay resident
ob = data.obs[0]
resident = [k for k in (defaults.quats, defaults.pixels, defaults.weights) if ob.detdata[k].accel_in_use()]
Pipeline(operators=[ops.Copy(detdata=[(defaults.det_data, "copy")])]).apply(data)   # + 2 x 3.2 MB
after = [k for k in (defaults.quats, defaults.pixels, defaults.weights) if ob.detdata[k].accel_exists()]
chk = [float(np.sum(ob.detdata[k].data.astype(np.float64))) for k in (defaults.quats, defaults.pixels, defaults.weights)]
same = bool(np.array_equal(ob.detdata["copy"].data, ob.detdata[defaults.det_data].data))
print("RESULT", len(resident), len(after), same, *chk)
"""


def test_eviction_under_memory_cap(tmp_path):
    """A failed device allocation evicts lazily retained detector data (written back to the host
    first) and retries: run once unconstrained and once with the manager capped at 28 MB
    (TOAST_HIP_MEM_LIMIT_MB), same results."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "evict.py"
    script.write_text(_EVICT_SCRIPT)
    out = {}
    for limit in (None, "28"):
        env = dict(os.environ)
        env.pop("TOAST_HIP_MEM_LIMIT_MB", None)
        env["TOAST_HIP_LAZY_HOST"] = "1"   # this is a test of the lazily retained buffers
        if limit:
            env["TOAST_HIP_MEM_LIMIT_MB"] = limit
        res = subprocess.run([sys.executable, str(script), root], capture_output=True, text=True, env=env, timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT")][0].split()
        out[limit] = line[1:]
    free, capped = out[None], out["28"]
    assert free[0] == "3" and free[1] == "3" and free[2] == "True"          # nothing evicted without a cap
    assert capped[0] == "3" and int(capped[1]) < 3 and capped[2] == "True"  # something had to go
    assert free[3:] == capped[3:]                                           # and came back intact


def test_transfer_sizes_through_the_bounce_ring():
    """Round trips of pageable buffers at every size class of the transfer paths (runtime.cpp: copy_to_device /
    copy_to_host through the 2 x 4 MiB page-locked ring, page-locked in place from 16 MiB): below, at and just past
    the slot size and its multiples, odd byte counts, and the first registered size."""
    rng = np.random.default_rng(5)
    slot = 4 << 20
    sizes = [1, 7, 4096, slot - 1, slot, slot + 1, 2 * slot, 2 * slot + 3, 3 * slot - 5, 3 * slot + 1, (16 << 20) - 1,
             16 << 20, (16 << 20) + 9]
    for n in sizes:
        want = rng.integers(0, 256, size=n, dtype=np.uint8)
        buf = want.copy()
        accel.accel_data_create(buf, "t")
        accel.accel_data_update_device(buf, "t")
        buf[:] = 0
        accel.accel_data_update_host(buf, "t")
        assert np.array_equal(buf, want), n
        # a second, different upload into the same device buffer (slots are reused in a different phase)
        want2 = (want ^ 0x5A).astype(np.uint8)
        buf[:] = want2
        accel.accel_data_update_device(buf, "t")
        buf[:] = 1
        accel.accel_data_update_host(buf, "t")
        assert np.array_equal(buf, want2), n
        accel.accel_data_delete(buf, "t")


def test_upload_in_parts_page_locks_range_by_range():
    """toast_hip_accel_update_device_parts on a buffer that is not page-locked yet locks it one range per part (each right
    before its part is enqueued, ending on a 4 KB boundary past the part): parts that end anywhere, a buffer that starts
    anywhere in a page, then a blocking upload, a download and the release over the same ranges -- always the same bytes."""
    from toast_amd import capi

    rng = np.random.default_rng(11)
    n = (48 << 20) + 12345
    for shift, ends in ((0, [5000001, 17 << 20, (17 << 20) + 1, 40000003, n]), (777, [n // 3, 2 * (n // 3) + 5, n]),
                        (8, [4096, 8192, n]), (1, [n])):
        raw = np.zeros(n + 4096, dtype=np.uint8)
        buf = raw[shift:shift + n]
        want = rng.integers(0, 256, size=n, dtype=np.uint8)
        buf[:] = want
        accel.accel_data_create(buf, "parts")
        capi.accel_update_device_parts(buf, np.array(ends), "parts")
        for k in range(len(ends)):
            capi.accel_update_device_wait(buf, k)
        capi.accel_update_device_finish(buf)
        buf[:] = 0
        accel.accel_data_update_host(buf, "parts")          # one download across all ranges
        assert np.array_equal(buf, want), (shift, ends)
        want2 = (want ^ 0xA5).astype(np.uint8)
        buf[:] = want2
        accel.accel_data_update_device(buf, "parts")        # one blocking upload across all ranges
        buf[:] = 3
        accel.accel_data_update_host(buf, "parts")
        assert np.array_equal(buf, want2), (shift, ends)
        capi.accel_update_device_parts(buf, np.array(ends), "parts")     # already locked: straight to the copies
        capi.accel_update_device_finish(buf)
        accel.accel_data_delete(buf, "parts")               # unlocks every range
        # the memory can be locked again afterwards (nothing was left registered)
        accel.accel_data_create(buf, "parts")
        accel.accel_data_update_device(buf, "parts")
        accel.accel_data_delete(buf, "parts")


def test_host_staged_call_with_a_large_argument():
    """A host-level entry point whose array argument is past the pinning threshold (page-locked for the call, released
    before it returns): cov_apply_diag on 2^21 pixels x 6 covariance values (100 MB) against NumPy."""
    rng = np.random.default_rng(6)
    n_sub, n_pix = 512, 4096
    cov = rng.standard_normal((n_sub * n_pix, 6))
    m = rng.standard_normal((n_sub * n_pix, 3))
    want = np.empty_like(m)
    tri = [(0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 1, 3), (1, 2, 4), (2, 2, 5)]
    full = np.zeros((n_sub * n_pix, 3, 3))
    for i, j, k in tri:
        full[:, i, j] = cov[:, k]
        full[:, j, i] = cov[:, k]
    want = np.einsum("pij,pj->pi", full, m)
    got = m.copy()
    accel.native().cov_apply_diag(n_sub, n_pix, 3, cov.reshape(-1), got.reshape(-1), False)
    assert np.max(np.abs(got - want)) < 1e-13 * np.max(np.abs(want))
    # the arrays can be released and their addresses reused right away
    del cov, got
    again = np.ones(n_sub * n_pix * 6)
    accel.accel_data_create(again, "again")
    accel.accel_data_update_device(again, "again")
    accel.accel_data_delete(again, "again")


def test_pixel_data_lazy_host_coherence():
    """PixelData copies back on the first host access only: device-side work goes through .buffer / .arg(True), a
    device-current map is duplicated and reset on the device, a map that was never handed out is known to be zero."""
    from toast_amd import capi
    from toast_amd.accel import accel_device_ptr

    dist = PixelDistribution(n_pix=4000, n_submap=10, local_submaps=[1, 3, 4])
    pd = PixelData(dist, np.float64, n_value=3)
    assert pd.host_is_zero()
    pd.accel_create("lazy", zero_out=True)
    pd.accel_used(True)
    n = pd.buffer.size
    ones = np.ones(n)
    accel.accel_data_create(ones, "ones")
    accel.accel_data_update_device(ones, "ones")
    capi.dev.vec_axpby(n, 2.5, accel_device_ptr(ones), 0.0, accel_device_ptr(pd.buffer))   # pd = 2.5 on the device
    assert pd.accel_in_use()
    assert not np.any(pd.buffer)                      # the key view is not synchronised
    assert pd.arg(True).ctypes.data == pd.buffer.ctypes.data
    dup = pd.duplicate()                              # device-to-device
    assert dup.accel_in_use() and pd.accel_in_use() and not np.any(dup.buffer)
    assert np.all(pd.data == 2.5)                     # first host access copies back ...
    assert not pd.accel_in_use() and pd.accel_exists()
    assert np.all(dup.raw == 2.5) and not dup.accel_in_use()
    assert not pd.host_is_zero()
    pd.data[:] = 7.0                                  # ... and the host is the current side again
    pd.accel_update_device()
    pd.reset()                                        # device-current: cleared there, host refreshed on access
    assert pd.accel_in_use() and np.all(pd.buffer == 7.0)
    assert not np.any(pd.data)
    host_dup = pd.duplicate()                         # host-current now: a host copy
    assert not host_dup.accel_exists() and not np.any(host_dup.data)
    accel.accel_data_delete(ones, "ones")
    for obj in (pd, dup):
        obj.accel_delete()



def test_amplitudes_lazy_host_coherence():
    """Amplitudes.local copies back on the first host access only (the solver leaves its vectors device-current under
    Data.lazy_host); device-side code goes through .buffer / .arg(True); duplicates, scalings and dot products of a
    device-current vector stay on the device."""
    from toast_amd import capi
    from toast_amd.accel import accel_device_ptr
    from toast_amd.templates import Amplitudes

    n = 5000
    a = Amplitudes(None, n, n)
    a.local[:] = np.arange(n, dtype=np.float64)
    a.local_flags[7] = 1
    a.accel_resident("lazy_amps")
    assert a.accel_in_use()
    capi.dev.vec_axpby(n, 2.0, accel_device_ptr(a.buffer), 0.0, accel_device_ptr(a.buffer))     # a *= 2 on the device
    assert a.accel_in_use() and a.buffer[3] == 3.0            # the key array is not synchronised
    assert a.arg(True).ctypes.data == a.buffer.ctypes.data
    b = a.duplicate()                                          # device-to-device, flags included
    b *= -1.0
    assert a.accel_in_use() and b.accel_in_use() and b.buffer[3] == 0.0
    want = 2.0 * np.arange(n, dtype=np.float64)
    keep = np.ones(n, dtype=bool)
    keep[7] = False
    assert np.isclose(a.dot(b), -np.sum(want[keep] ** 2), rtol=1e-13)
    assert a.accel_in_use() and b.accel_in_use()
    assert np.array_equal(b.local, -want)                      # first host access copies back ...
    assert not b.accel_in_use() and b.accel_exists()
    assert np.array_equal(a.arg(False), want) and not a.accel_in_use()
    a.local[0] = 5.0                                           # ... and the host is the current side again
    a.accel_resident()
    a.axpby(1.0, b)                                            # either operand device-current: both go there
    assert a.accel_in_use() and b.accel_in_use()
    got = a.local
    assert got[0] == 5.0 and not np.any(got[1:])
    for v in (a, b):
        v.clear()


def test_mapmaker_leaves_solution_and_offset_variances_on_the_device():
    """With lazy host coherence (the default) ops.MapMaker hands its solution back device-current -- ApplyAmplitudes read it
    there -- and the Offset template's variances were never on the host until somebody asked: both equal what the eager
    mode and the host-side initialisation produce."""
    from toast_amd import ops
    from toast_amd.templates import Offset
    from test_gpu_ops import make_solver_setup

    def run(lazy):
        data, pix, sw, truth, sky = make_solver_setup(noise_rms=0.2)
        data.lazy_host = lazy
        binner = ops.BinMap(pixel_dist="dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=True)
        tmpl = Offset(step_time=20.0, noise_model=defaults.noise_model, name="baselines", good_fraction=0.2)
        mapper = ops.MapMaker(name="mm", keep_solver_products=True, det_data=defaults.det_data, binning=binner,
                              template_matrix=ops.TemplateMatrix(templates=[tmpl]), iter_max=30, convergence=1e-20,
                              solve_rcond_threshold=1e-3, map_rcond_threshold=1e-3)
        mapper.apply(data)
        return data, tmpl

    data, tmpl = run(True)
    amps = data["mm_solve_amplitudes"]["baselines"]
    assert amps.accel_in_use()                                 # not copied back by the solver
    assert tmpl._mirrors["offsetvar"].stale                    # computed on the device, host copy pending
    var_dev = np.array(tmpl._offsetvar)                        # fetched now
    assert not tmpl._mirrors["offsetvar"].stale
    # the host-side form of the same initialisation on the same data (keep_solver_products: the solver flags are still there)
    host = Offset(step_time=20.0, noise_model=defaults.noise_model, name="host_side", good_fraction=0.2)
    for trait in ("view", "det_data", "det_flags", "det_flag_mask", "det_mask"):
        setattr(host, trait, getattr(tmpl, trait))
    for ob in data.obs:
        _ = ob.detdata[tmpl.det_flags].data                    # (host-current before the accelerator is "switched off")
    saved = accel.accel_enabled
    try:
        accel.accel_enabled = lambda: False
        host._initialize(data)
    finally:
        accel.accel_enabled = saved
    assert np.array_equal(host._amp_flags, tmpl._amp_flags)
    assert np.allclose(var_dev, host._offsetvar, rtol=1e-14, atol=0.0)
    sol_lazy = np.array(amps.local)
    assert not amps.accel_in_use()
    data_e, _ = run(False)
    sol_eager = np.array(data_e["mm_solve_amplitudes"]["baselines"].local)
    assert np.max(np.abs(sol_lazy - sol_eager)) <= 1e-12 * np.max(np.abs(sol_eager))


_CAP_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from toast_amd import ops
from toast_amd.data import defaults
from toast_amd.sim import create_satellite_data
from toast_amd.templates import Offset

data = create_satellite_data(n_det=4, n_samp=200000, rate=20.0)
rng = np.random.default_rng(1)
ob = data.obs[0]
ob.detdata[defaults.det_data].data[:] = rng.standard_normal((4, 200000))
dp = ops.PointingDetectorSimple()
pix = ops.PixelsHealpix(detector_pointing=dp, nside=256, nest=True)
sw = ops.StokesWeights(detector_pointing=dp, mode="IQU", hwp_angle=defaults.hwp_angle)
binner = ops.BinMap(pixel_dist="dist", pixel_pointing=pix, stokes_weights=sw, full_pointing=sys.argv[2] == "full")
tm = ops.TemplateMatrix(templates=[Offset(step_time=10.0, noise_model=defaults.noise_model, name="baselines")])
mm = ops.MapMaker(name="mm", det_data=defaults.det_data, binning=binner, template_matrix=tm, iter_max=5,
                  convergence=1e-30, keep_solver_products=True)
mm.apply(data)
maps = [float(np.sum(np.abs(data[k].data))) for k in ("mm_hits", "mm_map", "mm_cov", "mm_solve_cov")]
print("RESULT", int(data.accel_evict() >= 0), *maps, float(np.sum(np.abs(data["mm_solve_amplitudes"]["baselines"].local))))
"""


@pytest.mark.parametrize("pointing", ["full", "uncached"])
def test_mapmaker_under_memory_cap(tmp_path, pointing):
    """A complete MapMaker run with the manager capped at 52 MB, below what it keeps resident without a cap (timestreams
    6.4 MB, cached pointing 25.6 MB, a dozen maps; tools: TOAST_HIP_TRACE=1 shows 84 - 90 write-backs / releases instead
    of 78): allocations fail, lazily retained timestreams AND maps are written back and released, the collection of
    device pointers for the fused solver passes is repeated -- same products as without a cap."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "cap.py"
    script.write_text(_CAP_SCRIPT)
    out = {}
    for limit in (None, "52"):
        env = dict(os.environ)
        env.pop("TOAST_HIP_MEM_LIMIT_MB", None)
        env["TOAST_HIP_LAZY_HOST"] = "1"
        env["TOAST_HIP_ALLOC_CACHE_MB"] = "0"
        if limit:
            env["TOAST_HIP_MEM_LIMIT_MB"] = limit
        res = subprocess.run([sys.executable, str(script), root, pointing], capture_output=True, text=True, env=env,
                             timeout=600)
        assert res.returncode == 0, res.stderr[-3000:]
        out[limit] = [float(x) for x in [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT")][0].split()[1:]]
    free, capped = np.array(out[None]), np.array(out["52"])
    assert free[1] > 0 and free[2] > 0
    assert free[1] == capped[1]                                 # hits
    assert np.all(np.abs(free[2:] - capped[2:]) <= 1e-9 * np.abs(free[2:]))


def test_arena_serves_every_block_without_the_driver():
    """The device arena (csrc/arena.cpp; reference: OmpPoolResource, accelerator.cpp:13-230): raw blocks (what bench.py
    and the packed cache allocate) and registered arrays are ranges of slabs; releasing and allocating again does not
    call hipMalloc; contents survive the neighbours; ``release_cached`` gives empty slabs back; ``TOAST_HIP_ALLOC=plain``
    turns it off."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import numpy as np
        from toast_amd import capi
        from toast_amd.accel import accel_assign_device, accel_data_create, accel_data_delete, accel_data_update_device, accel_data_update_host
        accel_assign_device(1, 0, 2.0, False)                  # mem_gb = 2: the reservation
        s0 = capi.alloc_stats()
        small = capi.device_malloc(64 << 20)
        big = [capi.device_malloc(3 << 28) for _ in range(2)]  # 0.75 GB each: inside the 2 GB
        s1 = capi.alloc_stats()
        host = np.arange((1 << 28) // 8, dtype=np.float64)     # 256 MB registered array
        accel_data_create(host, "big")
        accel_data_update_device(host, "big")
        tiny = np.arange(100, dtype=np.int32)                  # below 1 MB: the small arena
        accel_data_create(tiny, "tiny")
        accel_data_update_device(tiny, "tiny")
        for p in big + [small]:
            capi.device_free(p)
        again = [capi.device_malloc(3 << 28) for _ in range(2)]
        s2 = capi.alloc_stats()
        host2 = host.copy(); host[:] = 0
        accel_data_update_host(host, "big")
        assert np.array_equal(host, host2)
        tiny2 = tiny.copy(); tiny[:] = 0
        accel_data_update_host(tiny, "tiny")
        assert np.array_equal(tiny, tiny2)
        accel_data_delete(host, "big")
        accel_data_delete(tiny, "tiny")
        for p in again:
            capi.device_free(p)
        s3 = capi.alloc_stats()
        accel_assign_device(1, 0, 2.0, False)                  # clear(): the slabs stay
        s4 = capi.alloc_stats()
        capi.accel_release_cached()
        s5 = capi.alloc_stats()
        print("STATS", s0["slab_mallocs"], s0["slab_GB"], s1["slab_mallocs"], s2["slab_mallocs"], s3["used_GB"],
              s4["slab_mallocs"], s4["slabs"], s5["slabs"], s2["direct_mallocs"])
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB", "TOAST_HIP_ARENA_SLAB_GB"):
        env.pop(key, None)
    env["TOAST_HIP_ARENA_STREAM_GB"] = "0"        # (the slab counts below are those of the plain arenas)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    f = [ln for ln in out.stdout.splitlines() if ln.startswith("STATS")][0].split()
    m0, gb0, m1, m2, used3, m4, slabs4, slabs5, direct = (int(f[1]), float(f[2]), int(f[3]), int(f[4]), float(f[5]),
                                                          int(f[6]), int(f[7]), int(f[8]), int(f[9]))
    assert m0 == 1 and abs(gb0 - 2.0) < 0.01        # the reservation: one slab of mem_gb
    assert m1 == 1                                  # 64 MB + 2 x 0.75 GB fit into it
    assert m2 == 2                                  # + one 64 MB slab of the small arena for `tiny`; none for the second round
    assert used3 == 0.0 and m4 == 2 and slabs4 == 2 and slabs5 == 0 and direct == 0
    env["TOAST_HIP_ALLOC"] = "plain"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    f = [ln for ln in out.stdout.splitlines() if ln.startswith("STATS")][0].split()
    assert int(f[3]) == 0 and int(f[4]) == 0 and int(f[9]) >= 7


def test_arena_grows_by_slabs():
    """A request that no free range holds takes a new slab (TOAST_HIP_ARENA_SLAB_GB, or the request when that is larger);
    slabs that still hold a block stay when the empty ones are given back."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        from toast_amd import capi
        from toast_amd.accel import accel_assign_device
        accel_assign_device(1, 0, 0.0, False)
        a = capi.device_malloc(1 << 28)                        # 256 MB -> a 1 GB slab (the default size here)
        s1 = capi.alloc_stats()
        b = capi.device_malloc(3 << 30)                        # 3 GB -> a slab of its own size
        s2 = capi.alloc_stats()
        c = capi.device_malloc(1 << 29)                        # 512 MB: fits the first slab
        s3 = capi.alloc_stats()
        capi.device_free(b)
        capi.accel_release_cached()                            # the 3 GB slab is empty, the first one is not
        s4 = capi.alloc_stats()
        capi.device_free(a); capi.device_free(c)
        print("STATS", s1["slabs"], s1["slab_GB"], s2["slabs"], s2["slab_GB"], s3["slabs"], s4["slabs"], s4["slab_frees"])
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB"):
        env.pop(key, None)
    env["TOAST_HIP_ARENA_SLAB_GB"] = "1"
    env["TOAST_HIP_ARENA_STREAM_GB"] = "0"        # (the slab counts below are those of the plain arenas)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    f = [ln for ln in out.stdout.splitlines() if ln.startswith("STATS")][0].split()
    assert int(f[1]) == 1 and abs(float(f[2]) - 1.0) < 1e-6
    assert int(f[3]) == 2 and abs(float(f[4]) - 4.0) < 1e-6 and int(f[5]) == 2
    assert int(f[6]) == 1 and int(f[7]) == 1




def test_second_workflow_run_allocates_nothing_from_the_driver():
    """after set-up no operator calls hipMalloc.  workflows/mapmaker_pcg.py (NoiseFilter +
    MapMaker with offset templates) twice in one process: the second run finds every block in the arena's slabs -- the
    counters of hipMalloc calls and of the time inside them do not move -- and produces the same map."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import importlib.util, os, sys
        import numpy as np
        root = os.getcwd()
        spec = importlib.util.spec_from_file_location("wf", os.path.join(root, "workflows", "mapmaker_pcg.py"))
        wf = importlib.util.module_from_spec(spec); spec.loader.exec_module(wf)
        from toast_amd import capi
        argv = ["--ndet", "32", "--minutes", "10", "--rate", "100", "--nside", "128", "--iter", "5"]
        d1 = wf.main(argv)
        m1 = d1["mapmaker_map"].data.copy()
        s1 = capi.alloc_stats()
        del d1
        d2 = wf.main(argv)
        s2 = capi.alloc_stats()
        m2 = d2["mapmaker_map"].data
        same = bool(np.allclose(m1, m2, rtol=1e-9, atol=1e-12 * np.abs(m1).max()))
        print("STATS", s1["slab_mallocs"], s2["slab_mallocs"], s1["malloc_ms"], s2["malloc_ms"], s1["direct_mallocs"],
              s2["direct_mallocs"], s2["allocs"] - s1["allocs"], same)
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB", "TOAST_HIP_ARENA_SLAB_GB"):
        env.pop(key, None)
    env["TOAST_HIP_ARENA_STREAM_GB"] = "0"        # (the slab counts below are those of the plain arenas)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    f = [ln for ln in out.stdout.splitlines() if ln.startswith("STATS")][0].split()
    assert int(f[1]) >= 1 and int(f[2]) == int(f[1])          # no slab was taken during the second run
    assert float(f[4]) == float(f[3])                         # ... so no time inside hipMalloc either
    assert int(f[5]) == 0 and int(f[6]) == 0                  # and nothing went around the arena
    assert int(f[7]) > 20                                     # (the second run did allocate its blocks -- from the slabs)
    assert f[8] == "True"


def test_reference_call_sequence_gets_the_zone_placement():
    """a caller that only speaks the reference's accel_* API -- accel_assign_device with the
    reference's token mem_gb, accel_create(array, name), kernels -- gets the zone placement: assign_device reserves the
    interleaved slab itself (on a thread of its own; whoever needs it waits), a [detector][sample] float64 array lands in
    it with chunks of both zones under it, and a map created as a scatter target lies inside ONE run of chunks of the
    other zone, also when it is larger than a chunk (the 1.2 GB map of Nside 2048 IQU)."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import ctypes as C, numpy as np
        from toast_amd import _libtoast_hip as m, capi
        m.accel_assign_device(1, 0, 1.0, False)
        tod = np.zeros((200, 1500000), dtype=np.float64)          # 2.4 GB
        small = np.zeros((64, 3000000), dtype=np.float64)          # 1.5 GB: too small to cover both zones wherever it lies
        zmap = np.zeros((16384, 3072, 3), dtype=np.float64)       # 1.2 GB: the Nside 2048 IQU map
        pix = np.zeros((200, 1500000), dtype=np.int64)
        m.accel_create(tod, "signal")
        m.accel_create(small, "signal2")
        m.accel_create(pix, "pixels")
        m.accel_create(zmap, "zmap", 2)
        st = capi.alloc_stats()
        where = {}
        for name, arr in (("tod", tod), ("small", small), ("zmap", zmap), ("pix", pix)):
            p = C.c_void_p(0)
            assert capi.real_lib().toast_hip_accel_device_ptr(C.c_void_p(arr.ctypes.data), C.byref(p)) == 0
            where[name] = capi.arena_block_zone(p.value, arr.nbytes)
        print("ZONES", st["interleaved_slabs"], st["chunks"], st["chunks_other_zone"], where)
        for arr, name in ((tod, "signal"), (small, "signal2"), (pix, "pixels"), (zmap, "zmap")):
            m.accel_delete(arr, name)
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB", "TOAST_HIP_ARENA_STREAM_GB", "TOAST_HIP_ARENA_INTERLEAVE",
                "TOAST_HIP_ARENA_BUILDER"):
        env.pop(key, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("ZONES")][0]
    f = line.split(None, 4)
    assert int(f[1]) >= 1 and int(f[2]) >= 8, line
    where = eval(f[4])
    assert where["tod"][0] and where["tod"][1] >= 1 and where["tod"][2] >= 1, line       # in the slab, rows in both zones
    assert where["small"][0] and where["small"][1] >= 1 and where["small"][2] >= 1, line
    # one run of chunks of ONE class: this slab was built before any read-mostly array existed, so its classes are relative
    # to its own first chunk and the map goes to whichever of the two measured clear of `pix` (asserting
    # "the Q chunks" made the test depend on which zone the driver handed out first)
    own, other = where["zmap"][1], where["zmap"][2]
    assert where["zmap"][0] and (own == 0) != (other == 0) and own + other <= 2, line
    assert not where["pix"][0], line                                                         # read-mostly: a plain slab


def test_zone_search_survives_a_slow_box():
    """the search for chunks of the other HBM zone is budgeted in measuring passes, not in wall
    time, and its passes are timed by the device clock inside the probe kernel.  With every chunk creation and every pass
    slowed down by 20 ms of host time (a driver that is still clearing memory, a profiler: the round-5 search gave up
    after 500 ms with 1 chunk of the other zone) the slab still gets every chunk it wants from the other zone, and the
    status call says so.  A search with a budget of 4 passes reports itself exhausted instead."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        import os, time
        from toast_amd import capi
        capi.accel_assign_device(1, 0, 1.0, False)
        capi.arena_reserve(40 << 30)               # read-mostly slab first: the chunks are measured against both of its ends
        t0 = time.time()
        capi.arena_reserve(12 << 30, streamed=True)
        st = capi.alloc_stats()
        print("SLOW", capi.arena_placement_status(), st["chunks"], st["chunks_other_zone"], st["chunks_other_wanted"],
              st["probes"], st["probes_by_clock"], st["searches_exhausted"], st["searches_capped_ms"],
              round(st["create_ms_per_chunk"], 1), round(time.time() - t0, 2))
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB", "TOAST_HIP_ARENA_INTERLEAVE", "TOAST_HIP_ARENA_BUILDER",
                "TOAST_HIP_ARENA_SEARCH_MS", "TOAST_HIP_ARENA_SEARCH_PROBES", "TOAST_HIP_PROBE_CLOCK"):
        env.pop(key, None)
    env["TOAST_HIP_ARENA_STREAM_GB"] = "0"         # (no default slab: the one slab of this test is the measured one)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, **extra), timeout=900,
                             cwd=root)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("SLOW")][0]
        return line, eval(line[5:].split(")")[0] + ")"), line[5:].split(")")[1].split()

    line, status, f = run({"TOAST_HIP_ARENA_TEST_SLOW_MS": "20"})
    ok, exhausted, other, wanted = status
    # 12 chunks, 6 wanted from the other zone; every probe by the device clock; slow creation was seen and did not matter
    assert int(f[0]) == 12 and wanted == 6, line
    assert other >= wanted // 2 and (ok or exhausted), line          # the verdict's bar: at least half ...
    assert int(f[3]) > 0 and int(f[4]) == int(f[3]), line            # (probes, all by the clock)
    assert float(f[7]) >= 20.0, line                                 # (the hook was active)
    assert int(f[6]) == 0, line                                      # the hard cap in ms was not what ended the search
    # ... and on a box that has three zones to offer within the budget, all of them (an exhausted search says so)
    assert ok or exhausted, line
    line2, status2, f2 = run({"TOAST_HIP_ARENA_SEARCH_PROBES": "4"})
    assert status2[0] or status2[1], line2                           # too small a budget: either lucky or reported
    assert int(f2[3]) <= 4 + 2 * 12 + 4, line2                       # the budget binds once the slab's own chunks exist


def test_written_timestreams_avoid_the_zone_of_the_read_mostly_slab():
    """Round 6 (profiles/r06_e): when both ends of the read-mostly slab lie in ONE HBM zone, the interleaved slab takes BOTH of
    its chunk classes from the two other zones -- a written timestream then shares a zone with none of the streams the sweeps
    read (scan_map 6.13 instead of 6.31 ms in every process).  Checked by measurement from outside the library: one read +
    write pass over 1 GB of either end of a read-mostly block together with a chunk of either class runs at the level of two
    different zones, not at the level a chunk shows with itself.  ``TOAST_HIP_ARENA_THIRD_ZONE=0`` keeps the two-class slab
    of rounds 4-5 (even slots: whatever is not clear of the read-mostly slab)."""
    import subprocess
    import sys
    import textwrap

    code = textwrap.dedent("""
        from toast_amd import capi
        capi.accel_assign_device(1, 0, 1.0, False)
        gb = 1 << 30
        capi.arena_reserve(40 * gb)                 # ONE read-mostly slab (TOAST_HIP_ARENA_RESERVE_GB=0: none at assign_device):
        capi.arena_reserve(8 * gb, streamed=True)   # the chunks are measured against its first and its last GB
        before = capi.alloc_stats()["slab_mallocs"]
        rd = capi.device_malloc(40 * gb, -1)        # ... which are the first and the last GB of this block
        wr = capi.device_malloc(7 * gb, -3)
        assert capi.alloc_stats()["slab_mallocs"] == before     # (both from the slabs that exist)
        cls = {}
        for k in range(6):
            inside, own, other = capi.arena_block_zone(wr + k * gb, 1)
            assert inside
            cls.setdefault("P" if own else "Q", wr + k * gb)
        rate = lambda a, b, n: 4.0 * n / (min(capi.probe_stream_split([a, b], n) for _ in range(3)) * 1e-3) / 1e12
        same = rate(cls["P"], cls["P"] + gb // 4, gb // 4)
        same1 = rate(cls["P"], cls["P"] + gb // 4, gb // 4)
        cross = {"%s-%s" % (rn, cn): rate(rp, cp, gb // 2) for rn, rp in (("start", rd), ("end", rd + 39 * gb + gb // 2)) for cn, cp in cls.items()}
        cross["P-Q"] = rate(cls["P"], cls["Q"], gb // 2)
        st = capi.alloc_stats()
        # (the split is for a read-mostly range that the survey found in ONE zone throughout)
        assert st["read_mostly_zones"] in (0, 1, 2, 3) and (st["slabs_third_zone"] == 0 or st["read_mostly_zones"] == 1), st
        print("THIRD", st["slabs_third_zone"], st["placement_ok"], st["search_exhausted"], round(max(same, same1), 3), cross)
    """)
    env = dict(os.environ)
    for key in ("TOAST_HIP_ALLOC", "TOAST_HIP_ARENA_RESERVE_GB", "TOAST_HIP_ARENA_INTERLEAVE", "TOAST_HIP_ARENA_BUILDER",
                "TOAST_HIP_ARENA_SEARCH_MS", "TOAST_HIP_ARENA_SEARCH_PROBES", "TOAST_HIP_PROBE_CLOCK", "TOAST_HIP_ARENA_THIRD_ZONE"):
        env.pop(key, None)
    env["TOAST_HIP_ARENA_STREAM_GB"] = "0"
    env["TOAST_HIP_ARENA_RESERVE_GB"] = "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(env, **extra), timeout=900,
                             cwd=root)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("THIRD")][0]
        f = line.split(None, 5)
        return line, int(f[1]), f[2] == "True", f[3] == "True", float(f[4]), eval(f[5])

    line, third, ok, exhausted, same, cross = run({})
    print(line)
    assert ok or exhausted, line
    assert third in (0, 1), line
    if third:
        # every pair (end of the read-mostly block, chunk class) and the two classes among themselves: different zones
        for k, v in cross.items():
            assert v > 1.05 * same, (k, line)
    line0, third0, ok0, exhausted0, same0, cross0 = run({"TOAST_HIP_ARENA_THIRD_ZONE": "0"})
    print(line0)
    assert third0 == 0 and (ok0 or exhausted0), line0
    # the chunks of the odd slots are clear of both ends in either form
    if ok0:
        assert cross0["start-Q"] > 1.05 * same0 and cross0["end-Q"] > 1.05 * same0, line0
