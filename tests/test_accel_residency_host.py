"""The transition table of the residency helpers in ``toast_amd.accel`` (``Resident``, ``make_resident`` /
``release_borrowed``, ``accel_place``), on a fake AcceleratorObject that logs the calls which would move or free data.
No GPU, no native library.

The expected logs and end states were recorded from the idioms as the operators carried them before the helper
existed (GroundFilter's "write back unless lazy", Demodulate's "drop if created", the templates' "host stays current",
NoiseEstim's private upload plus delete, the map operators' ``_global_to``); the helper has to reproduce every one."""

import numpy as np
import pytest

from toast_amd.accel import AcceleratorObject, Resident, accel_place, make_resident, release_borrowed

STARTS = ("unregistered", "host", "device")


class FakeObject(AcceleratorObject):
    """Registered / current states without a device; ``log`` collects the calls that reach the memory manager."""

    def __init__(self, start, size=4):
        super().__init__("fake")
        self.buffer = np.zeros(size)
        self.present = start != "unregistered"
        self._accel_used = start == "device"
        self.log = []

    def accel_exists(self):
        return self.present

    def _accel_create(self, zero_out=False):
        self.log.append("create_zeroed" if zero_out else "create")
        self.present = True

    def _accel_update_device(self):
        self.log.append("update_device")

    def _accel_update_host(self):
        self.log.append("update_host")

    def _accel_delete(self):
        self.log.append("delete")
        self.present = False

    def state(self):
        return self.accel_exists(), self.accel_in_use()


class FakeData:
    def __init__(self, lazy_host):
        self.lazy_host = lazy_host


def _write_back(handle, data):
    handle.write_back_unless_lazy(data)


def _drop(handle, data):
    handle.drop_if_created()


def _host_current(handle, data):
    handle.host_stays_current()


def _host_current_drop(handle, data):
    handle.host_stays_current()
    handle.drop_if_created()


RELEASES = {"write_back": _write_back, "drop": _drop, "host_current": _host_current,
            "host_current_drop": _host_current_drop}

# (release kind, starting state, data.lazy_host) -> (call log, (accel_exists, accel_in_use) afterwards)
EXPECTED = {
    ("write_back", "unregistered", True): (["create", "update_device"], (True, True)),
    ("write_back", "unregistered", False): (["create", "update_device", "update_host", "delete"], (False, False)),
    ("write_back", "host", True): (["update_device"], (True, True)),
    ("write_back", "host", False): (["update_device", "update_host", "delete"], (False, False)),
    ("write_back", "device", True): ([], (True, True)),
    ("write_back", "device", False): ([], (True, True)),
    ("drop", "unregistered", True): (["create", "update_device", "delete"], (False, False)),
    ("drop", "unregistered", False): (["create", "update_device", "delete"], (False, False)),
    ("drop", "host", True): (["update_device"], (True, True)),
    ("drop", "host", False): (["update_device"], (True, True)),
    ("drop", "device", True): ([], (True, True)),
    ("drop", "device", False): ([], (True, True)),
    ("host_current", "unregistered", True): (["create", "update_device"], (True, False)),
    ("host_current", "unregistered", False): (["create", "update_device"], (True, False)),
    ("host_current", "host", True): (["update_device"], (True, False)),
    ("host_current", "host", False): (["update_device"], (True, False)),
    ("host_current", "device", True): ([], (True, True)),
    ("host_current", "device", False): ([], (True, True)),
    ("host_current_drop", "unregistered", True): (["create", "update_device", "delete"], (False, False)),
    ("host_current_drop", "unregistered", False): (["create", "update_device", "delete"], (False, False)),
    ("host_current_drop", "host", True): (["update_device"], (True, False)),
    ("host_current_drop", "host", False): (["update_device"], (True, False)),
    ("host_current_drop", "device", True): ([], (True, True)),
    ("host_current_drop", "device", False): ([], (True, True)),
}


@pytest.mark.parametrize("lazy_host", [True, False])
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("kind", list(RELEASES))
def test_handle_transition_table(kind, start, lazy_host):
    obj = FakeObject(start)
    handle = Resident(obj, "fake")
    assert obj.state() == (True, True)
    assert handle.created == (start == "unregistered")
    assert handle.uploaded == (start != "device")
    RELEASES[kind](handle, FakeData(lazy_host))
    log, state = EXPECTED[(kind, start, lazy_host)]
    assert obj.log == log
    assert obj.state() == state


@pytest.mark.parametrize("lazy_host", [True, False])
@pytest.mark.parametrize("kind", list(RELEASES))
def test_device_current_object_is_left_alone(kind, lazy_host):
    """Somebody else made it resident: neither the handle nor any release touches it."""
    obj = FakeObject("device")
    handle = Resident(obj, "fake")
    assert (handle.created, handle.uploaded) == (False, False)
    RELEASES[kind](handle, FakeData(lazy_host))
    assert obj.log == [] and obj.state() == (True, True)


@pytest.mark.parametrize("start", STARTS)
def test_make_resident_and_release_borrowed(start):
    obj, borrowed = FakeObject(start), []
    assert make_resident(obj, "fake", borrowed) is obj
    assert obj.state() == (True, True)
    assert borrowed == ([] if start == "device" else [obj])
    release_borrowed(borrowed)
    log, state = EXPECTED[("host_current", start, True)]
    assert borrowed == [] and obj.log == log and obj.state() == state


def test_empty_buffer_is_returned_untouched():
    obj, borrowed = FakeObject("unregistered", size=0), []
    assert make_resident(obj, "fake", borrowed) is obj
    handle = Resident(obj, "fake")
    assert (handle.created, handle.uploaded) == (False, False)
    accel_place(obj, "fake", True)
    assert obj.log == [] and borrowed == [] and obj.state() == (False, False)


# (starting state, use_accel, zero_new) -> (call log, state): recorded from the map operators' ``_global_to``
PLACED = {
    ("unregistered", True, False): (["create", "update_device"], (True, True)),
    ("unregistered", True, True): (["create_zeroed"], (True, True)),
    ("unregistered", False, False): ([], (False, False)),
    ("unregistered", False, True): ([], (False, False)),
    ("host", True, False): (["update_device"], (True, True)),
    ("host", True, True): (["update_device"], (True, True)),
    ("host", False, False): ([], (True, False)),
    ("host", False, True): ([], (True, False)),
    ("device", True, False): ([], (True, True)),
    ("device", True, True): ([], (True, True)),
    ("device", False, False): (["update_host"], (True, False)),
    ("device", False, True): (["update_host"], (True, False)),
}


@pytest.mark.parametrize("start,use_accel,zero_new", list(PLACED))
def test_accel_place(start, use_accel, zero_new):
    obj = FakeObject(start)
    accel_place(obj, "fake", use_accel, zero_new=zero_new)
    log, state = PLACED[(start, use_accel, zero_new)]
    assert obj.log == log
    assert obj.state() == state
