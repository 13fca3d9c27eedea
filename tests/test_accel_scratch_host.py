"""``device_scratch`` in ``toast_amd.accel``: the native calls it issues for every role, on a normal exit and on an
exception, against a fake native module that logs ``(call, registration name)``.  No GPU, no native library.

The expected logs were written down from the sequences the sites spelled out by hand before the helper existed:
``PolyFilter._exec`` (two outputs), ``PolyFilter2D._device`` (one in/out array), ``GroundFilter.build_templates``
(inputs plus a work row) and ``PixelsHealpix._exec_from_boresight`` (one in/out array under a bare name).  One thing is
normalised: the hand-written exits downloaded and deleted array by array, the helper downloads everything in
registration order and then deletes everything; what is called, on which array, on which side of the kernel is the same."""

import numpy as np
import pytest

from toast_amd import accel
from toast_amd.accel import device_scratch


class FakeNative:
    """The memory manager's entry points without a device: a log and the set of registered names."""

    def __init__(self, fail_create_of=None):
        self.log = []
        self.registered = {}      # host address -> registration name
        self.fail_create_of = fail_create_of

    def _note(self, call, name):
        self.log.append((call, name))

    def accel_create(self, arr, name, kind):
        if name == self.fail_create_of:
            raise RuntimeError(f"toast_hip: bad argument ({name})")
        assert arr.ctypes.data not in self.registered
        self._note("create", name)
        self.registered[arr.ctypes.data] = name

    def accel_reset(self, arr, name):
        self._note("reset", name)

    def accel_update_device(self, arr, name):
        assert self.registered[arr.ctypes.data] == name
        self._note("update_device", name)

    def accel_update_host(self, arr, name):
        assert self.registered[arr.ctypes.data] == name
        self._note("update_host", name)

    def accel_delete(self, arr, name):
        assert self.registered.pop(arr.ctypes.data) == name
        self._note("delete", name)

    def accel_present(self, arr, name):
        return arr.ctypes.data in self.registered

    def accel_device_ptr(self, arr):
        assert arr.ctypes.data in self.registered
        return 0x1000 + arr.ctypes.data

    def accel_synchronize(self):
        self._note("synchronize", None)

    def accel_assign_device(self, node_procs, node_rank, mem_gb, disabled):
        self._note("assign_device", None)

    def accel_get_device(self):
        return -1


@pytest.fixture
def fake(monkeypatch):
    nat = FakeNative()
    monkeypatch.setattr(accel, "native", lambda: nat)
    monkeypatch.setattr(accel, "_assigned", True)
    monkeypatch.setattr(accel, "_finalizers", {})
    return nat


class Owner:
    name = "op"


def _clean(fake, *arrays):
    assert fake.registered == {}
    assert not any(a.ctypes.data in accel._finalizers for a in arrays if a.size > 0)


KERNEL = ("kernel", None)


def test_two_outputs_like_polyfilter(fake):
    op = Owner()
    coeff, status = np.zeros((3, 2, 2)), np.zeros((3, 2), dtype=np.int32)
    with device_scratch(op.name, owner=op) as s:
        assert s.out("coeff", coeff) is coeff
        assert s.out("status", status) is status
        assert s.ptr("coeff") == 0x1000 + coeff.ctypes.data and s.ptr("status") == 0x1000 + status.ctypes.data
        assert set(accel._finalizers) == {coeff.ctypes.data, status.ctypes.data}
        fake.log.append(KERNEL)
    assert fake.log == [("create", "op_coeff"), ("create", "op_status"), KERNEL, ("synchronize", None),
                        ("update_host", "op_coeff"), ("update_host", "op_status"),
                        ("delete", "op_coeff"), ("delete", "op_status")]
    _clean(fake, coeff, status)


def test_inout_like_polyfilter2d(fake):
    op = Owner()
    with device_scratch(op.name, owner=op) as s:
        coeff = s.inout("coeff", np.zeros((5, 1, 4)))
        fake.log.append(KERNEL)
    assert fake.log == [("create", "op_coeff"), ("update_device", "op_coeff"), KERNEL, ("synchronize", None),
                        ("update_host", "op_coeff"), ("delete", "op_coeff")]
    _clean(fake, coeff)


def test_inputs_and_work_row_like_ground_templates(fake):
    op = Owner()
    x, phase, direction = np.zeros(7), np.zeros(7), np.zeros(7, dtype=np.int32)
    row, ibin = np.empty(14), np.zeros(7, dtype=np.int32)
    with device_scratch(op.name, owner=op) as s:
        s.inp("x", x)
        s.inp("phase", phase)
        s.inp("direction", direction)
        assert s.work("row", row) is row
        s.inp("ibin", ibin)
        fake.log.append(KERNEL)
    names = ["op_x", "op_phase", "op_direction", "op_row", "op_ibin"]
    setup = []
    for name in names:
        setup.append(("create", name))
        if name != "op_row":
            setup.append(("update_device", name))
    assert fake.log == setup + [KERNEL, ("synchronize", None)] + [("delete", name) for name in names]
    _clean(fake, x, phase, direction, row, ibin)


def test_bare_name_like_pixels_healpix(fake):
    hs = np.zeros(12, dtype=np.uint8)
    with device_scratch() as s:
        s.inout("hit_submaps", hs)
        assert accel._finalizers[hs.ctypes.data].alive      # (no owner given: the array bounds its device copy)
        fake.log.append(KERNEL)
    assert fake.log == [("create", "hit_submaps"), ("update_device", "hit_submaps"), KERNEL, ("synchronize", None),
                        ("update_host", "hit_submaps"), ("delete", "hit_submaps")]
    _clean(fake, hs)


def test_exception_in_block_downloads_nothing_and_releases(fake):
    op, boom = Owner(), KeyError("inside the block")
    a, b, c = np.zeros(3), np.zeros(3), np.zeros(3)
    with pytest.raises(KeyError) as info:
        with device_scratch(op.name, owner=op) as s:
            s.inp("a", a)
            s.inout("b", b)
            s.out("c", c)
            raise boom
    assert info.value is boom
    assert fake.log == [("create", "op_a"), ("update_device", "op_a"), ("create", "op_b"), ("update_device", "op_b"),
                        ("create", "op_c"), ("delete", "op_a"), ("delete", "op_b"), ("delete", "op_c")]
    _clean(fake, a, b, c)


def test_failing_third_registration_releases_the_first_two(fake):
    fake.fail_create_of = "op_c"
    op = Owner()
    a, b, c = np.zeros(3), np.zeros(3), np.zeros(3)
    with pytest.raises(RuntimeError, match="op_c"):
        with device_scratch(op.name, owner=op) as s:
            s.out("a", a)
            s.out("b", b)
            s.out("c", c)
    assert fake.log == [("create", "op_a"), ("create", "op_b"), ("delete", "op_a"), ("delete", "op_b")]
    _clean(fake, a, b, c)


def test_failing_delete_does_not_mask_the_error(fake, monkeypatch):
    boom = KeyError("inside the block")
    a, b = np.zeros(3), np.zeros(3)
    real_delete = fake.accel_delete

    def delete(arr, name):
        real_delete(arr, name)
        if name == "a":
            raise RuntimeError("delete failed")

    monkeypatch.setattr(fake, "accel_delete", delete)
    with pytest.raises(KeyError) as info:
        with device_scratch() as s:
            s.inp("a", a)
            s.inp("b", b)
            raise boom
    assert info.value is boom
    _clean(fake, a, b)
    # without an error on its way out the failed release is reported, after every entry was tried
    with pytest.raises(RuntimeError, match="delete failed"):
        with device_scratch() as s:
            s.inp("a", a)
            s.inp("b", b)
    _clean(fake, a, b)


@pytest.mark.parametrize("role", ["inp", "out", "inout", "work"])
def test_empty_array_costs_no_native_call(fake, role):
    empty = np.zeros(0)
    with device_scratch("op", owner=Owner()) as s:
        assert getattr(s, role)("empty", empty) is empty
        assert s.ptr("empty") == 0
        s.fetch("empty")
    assert fake.log == []
    _clean(fake, empty)


def test_fetch_downloads_one_entry_and_keeps_it(fake):
    hits = np.zeros(4, dtype=np.int64)
    with device_scratch("op", owner=Owner()) as s:
        s.inp("hits", hits)
        fake.log.append(KERNEL)
        del fake.log[:]
        assert s.fetch("hits") is hits
        assert fake.log == [("synchronize", None), ("update_host", "op_hits")]
        assert fake.registered == {hits.ctypes.data: "op_hits"}
    assert fake.log[2:] == [("synchronize", None), ("delete", "op_hits")]      # an input: not downloaded again
    _clean(fake, hits)


def test_device_mirror_is_one_class():
    from toast_amd.accel import DeviceMirror
    from toast_amd.templates import DeviceMirror as from_templates

    assert DeviceMirror is from_templates
