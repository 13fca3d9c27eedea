"""GPU: ``device_scratch`` of ``toast_amd.accel`` on arrays of five and of zero doubles -- what comes back on a normal
exit, and that an exception inside the block leaves the host arrays alone and nothing on the device.  The values are
small integers and halves, so ``2 x + 3 y`` is exact however the kernel contracts it."""

import numpy as np
import pytest

from toast_amd.accel import accel_data_present, device_scratch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    from toast_amd import capi

    assert capi.accel_enabled()
    capi.accel_assign_device(1, 0, 1.0, False)


X = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
Y0 = np.array([0.5, -1.0, 2.0, 8.0, -3.0])


def used_bytes():
    from toast_amd import capi

    return capi.alloc_stats()["used_GB"] * 2.0 ** 30      # (exact: the counter divided by a power of two)


def run_block(x, y, z, empty, fail):
    from toast_amd import capi

    with device_scratch("scratch_test") as s:
        s.inp("x", x)
        s.inout("y", y)
        s.out("z", z)
        s.inout("empty", empty)
        assert s.ptr("empty") == 0 and not accel_data_present(empty)
        assert all(accel_data_present(a) for a in (x, y, z))
        capi.dev.vec_axpby(5, 2.0, s.ptr("x"), 3.0, s.ptr("y"))
        capi.dev.copy(s.ptr("z"), s.ptr("y"), 40)
        if fail:
            raise KeyError("raised by ordinary Python inside the block")


def test_roles_round_trip_and_release():
    before = used_bytes()
    x, y, z, empty = X.copy(), Y0.copy(), np.full(5, -7.0), np.zeros(0)
    run_block(x, y, z, empty, fail=False)
    assert np.array_equal(y, 2.0 * X + 3.0 * Y0)
    assert np.array_equal(z, y)
    assert np.array_equal(x, X)
    assert not any(accel_data_present(a) for a in (x, y, z))
    assert used_bytes() == before


def test_exception_leaves_host_untouched_and_device_empty():
    before = used_bytes()
    x, y, z, empty = X.copy(), Y0.copy(), np.full(5, -7.0), np.zeros(0)
    with pytest.raises(KeyError):
        run_block(x, y, z, empty, fail=True)
    assert np.array_equal(x, X) and np.array_equal(y, Y0) and np.array_equal(z, np.full(5, -7.0))
    assert not any(accel_data_present(a) for a in (x, y, z))
    assert used_bytes() == before
    # whatever address the allocator hands out next, a stale entry would be in its way
    del x, y, z
    fresh = [np.zeros(5) for _ in range(8)]
    with device_scratch("scratch_test") as s:
        for i, arr in enumerate(fresh):
            s.inp(f"fresh{i}", arr)
    assert not any(accel_data_present(a) for a in fresh)
    assert used_bytes() == before
