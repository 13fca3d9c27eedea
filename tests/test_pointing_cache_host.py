"""CPU: the sealed-pointing registry of the packed pointing cache (csrc/pointing_cache.cpp) driven on host memory through
toast_hip_pointing_cache_selftest -- no device needed.

Scenario 0 is a seeded random sequence of seal / consume / overlapping write / free / non-whitelisted call / allocation
pressure / explicit drop steps on a small host arena.  The selftest keeps its own model of which arrays still hold what
their expansion wrote and fails when a hit follows an event that should have dropped the seal, when a hit comes before
the third eligible call, when the packed copy or the per-detector cal differs from the arrays, when a packed block leaks,
or when any function of the backend is called with the registry's lock held -- the stand-in backend's pack allocates under
pressure and releases through the harness, as the device one can through the parameter-block cache and the arena, and its
give says "not yet" the first time.  Scenarios 1-7 are the named cases, one by one."""

import pytest

from toast_amd import capi


@pytest.mark.parametrize("seed", [1, 2, 3, 5, 8, 13, 21, 34])
def test_random_sequences(seed):
    capi.pointing_cache_selftest(seed, 6000, 0)


@pytest.mark.parametrize("scenario,what", [
    (1, "the pack happens at the third call"),
    (2, "a different interval list gives a miss"),
    (3, "a reseal discards the copy"),
    (4, "eviction under allocation pressure, after which the allocation succeeds"),
    (5, "a non-whitelisted call drops every seal"),
    (6, "an expansion that does not seal (too many rows, Nside above 8192, a row written twice, caching not allowed) "
        "still drops the seals and copies over the rows it wrote"),
    (7, "the backend's pack comes back into the registry (an allocation that evicts, a release) without finding its lock held"),
])
def test_named_scenario(scenario, what):
    capi.pointing_cache_selftest(0, 0, scenario)


def test_unknown_scenario_is_an_error():
    with pytest.raises(RuntimeError, match="unknown scenario"):
        capi.pointing_cache_selftest(0, 0, 99)


def test_stats_and_switch_without_a_device():
    st = capi.pointing_cache_stats()
    assert st["pack_after_calls"] == 3
    assert st["live_seals"] == 0 and st["packed_bytes"] == 0
    was = bool(st["enabled"])
    try:
        capi.pointing_cache_enable(False)
        assert capi.pointing_cache_stats()["enabled"] == 0
        capi.pointing_cache_enable(True)
        assert capi.pointing_cache_stats()["enabled"] == 1
        capi.pointing_cache_drop()
    finally:
        capi.pointing_cache_enable(was)
