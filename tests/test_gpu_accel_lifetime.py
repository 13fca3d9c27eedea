"""GPU: a device copy made without an owner is bounded by the lifetime of the host array that keys it.

Device copies are keyed by host address.  An array dropped between accel_data_create and accel_data_delete (an exception
on the way) gives its memory back to the allocator; the entry it left behind used to be mistaken for the next array at
that address ("is present, but has N bytes instead of M")."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _present(ptr, nbytes):
    from toast_amd import capi

    out = ctypes.c_int(0)
    rc = capi.real_lib().toast_hip_accel_present(ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), ctypes.byref(out))
    return rc == 0 and bool(out.value)


def test_dropped_array_releases_its_device_copy():
    from toast_amd import accel

    a = np.zeros((2, 3000))
    ptr, nbytes = a.ctypes.data, a.nbytes
    accel.accel_data_create(a, "dropped")
    assert _present(ptr, nbytes)
    del a
    gc.collect()
    assert not _present(ptr, nbytes)
    # the next arrays of other sizes, wherever the allocator puts them, register without complaint
    for n in (1201, 3000, 6000):
        b = np.zeros((2, n))
        assert not accel.accel_data_present(b, "next")
        accel.accel_data_create(b, "next")
        accel.accel_data_delete(b, "next")


def test_views_and_explicit_deletes_are_unchanged():
    from toast_amd import accel

    base = np.arange(4000, dtype=np.float64)
    view = base[:2000]                    # does not own its memory: no lifetime of its own
    accel.accel_data_create(view, "view")
    ptr, nbytes = view.ctypes.data, view.nbytes
    del view
    gc.collect()
    assert _present(ptr, nbytes)
    accel.accel_data_delete(base[:2000], "view")
    assert not _present(ptr, nbytes)
    # an explicit delete detaches the finalizer: a new copy at the same address outlives the old array object
    a = np.zeros(500)
    accel.accel_data_create(a, "first")
    accel.accel_data_delete(a, "first")
    accel.accel_data_create(a, "second")
    assert accel.accel_data_present(a, "second")
    accel.accel_data_delete(a, "second")
