"""Accelerator interface with the names of ``toast.accelerator.accel``
(reference: src/toast/accelerator/accel.py:20-305), routed to the HIP memory manager."""

import os

import numpy as np

from . import load_native

_native = None


def native():
    """The pybind11 module (``toast._libtoast`` counterpart); raises if not built."""
    global _native
    if _native is None:
        _native = load_native()
    return _native


_assigned = False


def accel_enabled():
    """True when a gfx950 device is usable (reference accel.py:69-77)."""
    if os.environ.get("TOAST_GPU_DISABLE", "0") not in ("0", "", "false", "False"):
        return False
    return bool(native().accel_enabled())


def accel_assign_device(node_procs, node_rank, mem_gb, disabled=False):
    """reference accel.py:94-118"""
    global _assigned
    native().accel_assign_device(int(node_procs), int(node_rank), float(mem_gb), bool(disabled))
    _assigned = True
    # one HIP runtime, one current device: torch (device tensors handed to RCCL, the collectives'
    # scratch tensors) must sit on the GPU the memory manager chose for this process
    dev = int(native().accel_get_device())
    if dev >= 0:
        import torch

        if torch.cuda.is_available() and torch.cuda.current_device() != dev:
            torch.cuda.set_device(dev)


def ensure_assigned():
    """Assign a device on first use: one process per GPU, device = LOCAL_RANK."""
    if not _assigned:
        nproc = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
        rank = int(os.environ.get("LOCAL_RANK", "0"))
        # the reference's default pool size and its knob (src/toast/mpi.py:60-63)
        accel_assign_device(max(nproc, 1), rank, float(os.environ.get("TOAST_GPU_MEM_GB", "2.0")), False)


def accel_get_device():
    ensure_assigned()
    return native().accel_get_device()


def _key(data):
    return np.asarray(data)


def accel_data_present(data, name="None"):
    """reference accel.py:121-144"""
    if data is None:
        return False
    ensure_assigned()
    arr = _key(data)
    if arr.size == 0:
        return False   # empty buffers (an observation without valid detectors) are never registered
    return bool(native().accel_present(arr, name))


_finalizers = {}


def _release(ptr, nbytes, name):
    """Finalizer: drop the device copy of a host buffer whose owner was garbage collected.
    Device copies are keyed by host address (like the reference's OmpManager), so a leaked
    entry would be mistaken for the next allocation at that address."""
    import ctypes

    from . import capi

    _finalizers.pop(ptr, None)
    try:
        # the real handle: a garbage collection inside a capi.capture() block must free the device
        # copy now, not record the call into the plan that is replayed every iteration
        lib = capi.real_lib()
        present = ctypes.c_int(0)
        rc = lib.toast_hip_accel_present(ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), ctypes.byref(present))
        if rc == 0 and present.value:
            lib.toast_hip_accel_delete(ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), name.encode())
    except Exception:  # interpreter shutdown
        pass


_eviction_handlers = []


def add_eviction_handler(fn):
    """Register ``fn() -> bytes_freed``; called when a device allocation fails so that lazily
    retained buffers can be written back and released before one retry."""
    _eviction_handlers.append(fn)


#: what an array is to the kernels (toast_hip_accel_create_kind): decides where in HBM the arena puts its device copy
KIND_DEFAULT, KIND_STREAMED, KIND_SCATTER = 0, 1, 2


def accel_data_create(data, name="None", zero_out=False, owner=None, kind=KIND_DEFAULT):
    """reference accel.py:147-176.  ``owner``: object whose lifetime bounds the device copy (None: the array itself
    when it owns its memory).  ``kind``: KIND_STREAMED for
    a timestream that kernels read and write in their sweeps, KIND_SCATTER for the target of a scatter with atomics (a
    map, an amplitude vector); toast_hip_accel_create_kind."""
    import weakref

    ensure_assigned()
    arr = _key(data)
    if arr.size == 0:
        return data
    try:
        native().accel_create(arr, name, int(kind))
    except RuntimeError as err:
        if "allocation failed" not in str(err):
            raise
        freed = 0
        for fn in list(_eviction_handlers):
            freed += int(fn() or 0)
        if freed == 0:
            raise
        native().accel_create(arr, name, int(kind))
    if zero_out:
        native().accel_reset(arr, name)
    if owner is None and arr is data and arr.flags.owndata:
        # an array that owns its memory and has no other owner bounds its device copy itself: when it is dropped
        # without accel_data_delete (an exception between create and delete), its memory goes back to the allocator
        # and the entry would be mistaken for the next array at that address
        owner = arr
    if owner is not None:
        ptr = arr.ctypes.data
        stale = _finalizers.pop(ptr, None)
        if stale is not None:
            stale.detach()
        _finalizers[ptr] = weakref.finalize(owner, _release, ptr, arr.nbytes, name)
    return data


def accel_data_reset(data, name="None"):
    ensure_assigned()
    if _key(data).size > 0:
        native().accel_reset(_key(data), name)
    return data


def accel_data_update_device(data, name="None"):
    ensure_assigned()
    if _key(data).size > 0:
        native().accel_update_device(_key(data), name)
    return data


def accel_data_update_host(data, name="None"):
    ensure_assigned()
    if _key(data).size > 0:
        native().accel_update_host(_key(data), name)
    return data


def accel_data_delete(data, name="None"):
    ensure_assigned()
    arr = _key(data)
    if arr.size == 0:
        return data
    fin = _finalizers.pop(arr.ctypes.data, None)
    if fin is not None:
        fin.detach()
    native().accel_delete(arr, name)
    return data


def accel_device_ptr(data):
    ensure_assigned()
    if _key(data).size == 0:
        return 0
    return int(native().accel_device_ptr(_key(data)))


class DeviceMirror:
    """A host array that a template derives at set-up, its device copy under one registration name, and which side is
    current: host only, both, or device newer (then the first ``host`` access fetches the values, once)."""

    def __init__(self, buffer, name):
        self.buffer = buffer        # the host array WITHOUT synchronisation: the accelerator key
        self.name = name
        self.on_device = False      # registered on the device?
        self.stale = False          # device newer than host?

    def create(self, zero_out=False):
        """Register without an upload, as the side that kernels write; ``written()`` once they were launched."""
        accel_data_create(self.buffer, self.name, zero_out=zero_out, owner=self)
        self.on_device = True
        return self

    def upload(self):
        """Make sure the host values are on the device (copied once; the host array does not change afterwards)."""
        if not self.on_device:
            self.create()
            accel_data_update_device(self.buffer, self.name)
        return self

    @property
    def ptr(self):
        return accel_device_ptr(self.buffer)

    def written(self):
        self.stale = True

    @property
    def host(self):
        """The host array, brought up to date first."""
        if self.stale:
            self.stale = False
            accel_data_update_host(self.buffer, self.name)
        return self.buffer

    def drop(self, fetch=True):
        """Release the device copy; ``fetch``: somebody may still read the values on the host."""
        if self.on_device:
            if fetch:
                _ = self.host
            accel_data_delete(self.buffer, self.name)
        self.on_device = self.stale = False


class device_scratch:
    """``with device_scratch(prefix, owner=op) as s: ...`` -- small host arrays mirrored on the device for the span of a
    few kernel calls, registered as ``f"{prefix}_{key}"`` (the bare key when ``prefix`` is None).  The role says what is
    copied: ``inp`` up at registration, ``out`` down on a normal exit, ``inout`` both, ``work`` neither; each returns its
    host array.  A normal exit synchronizes once, downloads in registration order and releases everything; an exception
    (also one from a later registration) only releases.  Empty arrays are never registered: their pointer is 0."""

    def __init__(self, prefix=None, owner=None, kind=KIND_DEFAULT):
        self._prefix, self._owner, self._kind = prefix, owner, kind
        self._entries = {}      # key -> (host array, registration name, downloaded on a normal exit?)

    def __enter__(self):
        return self

    def _add(self, key, arr, upload, download):
        name = key if self._prefix is None else f"{self._prefix}_{key}"
        accel_data_create(arr, name, owner=self._owner, kind=self._kind)
        self._entries[key] = (arr, name, download)
        if upload:
            accel_data_update_device(arr, name)
        return arr

    def inp(self, key, arr):
        return self._add(key, arr, True, False)

    def out(self, key, arr):
        return self._add(key, arr, False, True)

    def inout(self, key, arr):
        return self._add(key, arr, True, True)

    def work(self, key, arr):
        return self._add(key, arr, False, False)

    def ptr(self, key):
        return accel_device_ptr(self._entries[key][0])

    def fetch(self, key):
        """The host needs one entry inside the block: wait for the kernels and download it."""
        arr, name, _ = self._entries[key]
        if _key(arr).size > 0:
            native().accel_synchronize()
        return accel_data_update_host(arr, name)

    def __exit__(self, exc_type, exc, tb):
        live = [entry for entry in self._entries.values() if _key(entry[0]).size > 0]
        self._entries = {}
        unwinding = exc is not None
        try:
            if not unwinding and live:
                native().accel_synchronize()
                for arr, name, download in live:
                    if download:
                        accel_data_update_host(arr, name)
        except BaseException:
            unwinding = True
            raise
        finally:
            failed = None
            for arr, name, _ in live:
                try:
                    accel_data_delete(arr, name)
                except Exception as err:
                    failed = failed or err
            # (every entry was tried; a release that fails while an error is on its way out does not replace that error)
            if failed is not None and not unwinding:
                raise failed
        return False


class accel_hold:
    """``with accel_hold(a, b): ...`` -- the device copies of ``a`` and ``b`` are not evicted inside the block
    (``Data.accel_evict`` skips held objects).  For code outside a Pipeline that allocates device memory while it
    holds another object's device state: a failed allocation triggers eviction, and writing back / freeing the very
    operand the code is about to read would leave it with a stale device pointer."""

    def __init__(self, *objs):
        self._objs = [o for o in objs if o is not None]

    def __enter__(self):
        for o in self._objs:
            o._accel_hold = getattr(o, "_accel_hold", 0) + 1
        return self

    def __exit__(self, *exc):
        for o in self._objs:
            o._accel_hold -= 1
        return False


def _host_key(obj):
    """The host array whose address keys the device copy of ``obj``, WITHOUT synchronisation."""
    return obj.buffer if hasattr(obj, "buffer") else obj.data


class Resident:
    """``obj`` made current on the device for one operator call, and what that took: ``created`` -- it had to be
    registered, ``uploaded`` -- the host values had to be copied.  An object that is current there already costs no
    native call; one whose buffer is empty (an observation without valid detectors) is left untouched.  The caller ends
    with the release that fits what it did to the device copy; each does nothing for an object it found resident."""

    def __init__(self, obj, name):
        self.obj, self.created, self.uploaded = obj, False, False
        if not obj.accel_in_use() and _host_key(obj).size > 0:
            self.created = not obj.accel_exists()
            if self.created:
                obj.accel_create(name)
            obj.accel_update_device()
            self.uploaded = True

    @property
    def ptr(self):
        return accel_device_ptr(_host_key(self.obj))

    def write_back_unless_lazy(self, data):
        """The kernels wrote it.  Eager coherence (``data.lazy_host`` False): back to the host and freed; lazy: it
        stays resident for the operators that follow."""
        if self.uploaded and not getattr(data, "lazy_host", False):
            self.obj.accel_update_host()
            self.obj.accel_delete()

    def drop_if_created(self):
        """It was only read and nobody else asked for a device copy: freed without a write-back."""
        if self.created:
            self.obj.accel_delete()

    def host_stays_current(self):
        """It was only read: the host copy is still right and becomes the current side again, so a later edit on the
        host is uploaded instead of being shadowed by a stale device copy."""
        if self.uploaded:
            self.obj.accel_used(False)


def make_resident(obj, name, borrowed=None):
    """Make the device copy of ``obj`` current and leave it there.  ``borrowed``: a list that collects the objects this
    call had to upload, for ``release_borrowed``."""
    if Resident(obj, name).uploaded and borrowed is not None:
        borrowed.append(obj)
    return obj


def release_borrowed(borrowed):
    """``Resident.host_stays_current`` for the objects that ``make_resident`` collected."""
    for obj in borrowed:
        obj.accel_used(False)
    del borrowed[:]


def accel_place(obj, name, use_accel, zero_new=False):
    """Make ``obj`` current where the kernel will look for it: on the device with ``use_accel``, else on the host.
    ``zero_new``: an object not yet registered is created zeroed there and marked current without an upload."""
    if not use_accel:
        if obj.accel_in_use():
            obj.accel_update_host()
    elif zero_new and not obj.accel_exists():
        obj.accel_create(name, zero_out=True)
        obj.accel_used(True)
    else:
        make_resident(obj, name)


class AcceleratorObject:
    """Mix-in for objects with a device copy (reference: accel.py:308-520).

    ``accel_exists``: a device buffer is allocated.  ``accel_in_use``: the device copy is the
    current one (the host copy may be stale)."""

    def __init__(self, accel_name="(blank)"):
        self._accel_used = False
        self._accel_name = accel_name

    def _accel_exists(self):
        return False

    def accel_exists(self):
        if not accel_enabled():
            return False
        return self._accel_exists()

    def accel_in_use(self):
        return self._accel_used

    def accel_used(self, state):
        if state and not self.accel_exists():
            raise RuntimeError("Data is not present on device, cannot set as 'used'")
        self._accel_used = bool(state)

    def _accel_create(self, **kwargs):
        pass

    def accel_create(self, name=None, **kwargs):
        if name is not None:
            self._accel_name = name
        if self.accel_exists():
            raise RuntimeError(f"Data already exists on device, cannot create ({self._accel_name})")
        self._accel_create(**kwargs)

    def _accel_update_device(self):
        pass

    def accel_update_device(self):
        if not self.accel_exists():
            raise RuntimeError(f"Data does not exist on device, cannot update ({self._accel_name})")
        if self.accel_in_use():
            raise RuntimeError("Active data is already on device, cannot update")
        self._accel_update_device()
        self.accel_used(True)

    def _accel_update_host(self):
        pass

    def accel_update_host(self):
        if not self.accel_exists():
            raise RuntimeError(f"Data does not exist on device, cannot update host ({self._accel_name})")
        if not self.accel_in_use():
            raise RuntimeError("Active data is already on host, cannot update")
        self._accel_update_host()
        self.accel_used(False)

    def _accel_delete(self):
        pass

    def accel_delete(self):
        if not self.accel_exists():
            raise RuntimeError(f"Data does not exist on device, cannot delete ({self._accel_name})")
        self._accel_delete()
        self._accel_used = False

    def _accel_reset(self):
        pass

    def accel_reset(self):
        if not self.accel_exists():
            raise RuntimeError(f"Data does not exist on device, cannot reset ({self._accel_name})")
        self._accel_reset()
