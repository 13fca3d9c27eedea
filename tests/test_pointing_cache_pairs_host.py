"""CPU: the pair form of the packed pointing cache in the sealed-pointing registry (csrc/pointing_cache.cpp), driven on host
memory through toast_hip_pointing_cache_selftest -- no device needed.

The stand-in backend implements the pair pack with the device kernel's arithmetic (common pixel or escape word, (q_a, u_a),
float2 sums or NaN marker) and "reads back" the escape count.  Scenarios 8-10 are the named cases.  Scenario 0's model
knows the pair form's hit rule -- the call's detectors, taken in twos, are pairs of the call that packed, in the same
orientation; a lone last detector is that call's lone -- and checks on every pair hit that what the consumer kernels
would reconstruct from the copy (or read from the arrays where the copy says "escape") is what the arrays hold.  Two
expansions in three write co-pointing pairs, some of them with escapes over the threshold behind the probe's reach; a
sequence of 20000 steps must have taken the pair form, demoted it and taken the plain form at least once each."""

import pytest

from toast_amd import capi


@pytest.mark.parametrize("scenario,what", [
    (8, "co-pointing pairs take the pair form on the third call and hit (28 B per pair-sample, one escape counted); a "
        "reseal of either array gives the copy up; with the pair form switched off the plain form is packed"),
    (9, "escapes over the threshold that the probe cannot see demote to the plain form in the same call, and the pair "
        "block goes back to the arena"),
    (10, "a call that splits a pair, turns one round or brings another lone detector misses; any subset of the pairs in "
         "any order hits"),
])
def test_named_scenario(scenario, what):
    capi.pointing_cache_selftest(0, 0, scenario)


@pytest.mark.parametrize("seed", [1, 4, 9, 16, 25])
def test_random_sequences_with_pairs(seed):
    capi.pointing_cache_selftest(seed, 20000, 0)


def test_pair_counters_are_reported():
    st = capi.pointing_cache_stats()
    for k in ("pair_packs", "pair_demotions", "pair_escapes"):
        assert k in st and st[k] >= 0
    assert list(st)[-3:] == ["pair_packs", "pair_demotions", "pair_escapes"]      # appended: the older fields keep their place
    assert st["pair_escapes"] == 0 or st["packed_bytes"] > 0
