"""CPU tier for the launch forms (csrc/rt_forms.h through the device-free rt_launch_form / rt_any_hit_walk): which instantiation of k_generate_*,
k_shade_s and k_light_s each round of a dense path batch launches and what it is handed, and which any-hit walk a queue takes, held to
tests/forms_ref.py -- the ladders the host code spelt out before the tables -- over the whole space of facts.  A wrong pick here renders the
same bits and only loses speed (a missing table record is never wrong, only slower), so no frame comparison can see it."""
import itertools

import pytest

import forms_ref as ref


def batches():
    """every combination of the raw facts primary_table_for can hand run_rounds_stream: a current bounce table implies a current primary
    table, chain levels above 1 imply a current bounce table; rounds 1 .. 6"""
    for table, bounce, chain, knob, r0, sampler, fisheye, rounds in itertools.product((0, 1), (0, 1), (1, 2, 3, 4), (0, 1), (0, 1, 2), (0, 1), (0, 1), range(1, 7)):
        if (bounce and not table) or (chain > 1 and not bounce):
            continue
        yield (table, bounce, chain, knob, r0, sampler, fisheye, rounds)


def test_every_launch_of_every_batch_is_the_ladders(host_api):
    shade_cases, generates, lights = set(), set(), set()
    n = 0
    for b in batches():
        rounds = b[7]
        got = [host_api.launch_form(b, rnd) for rnd in range(rounds)]
        for rnd, g in enumerate(got):
            branch, bits, fresh, bt, masked, p = ref.shade(b, rnd)
            assert (g["shade"], g["fresh"], g["bt"], g["masked"], g["p"]) == (bits, fresh, bt, masked, p), (b, rnd, branch, g)
            assert g["generate"] == ref.generate(b), (b, g)
            shade_cases.add((branch, rnd == 0) if branch == 8 else branch)
            generates.add(g["generate"])
            n += 1
        for mixed in (False, True):
            for site, rnd, table0 in ref.light_launches(b, mixed):
                assert got[rnd]["light_mixed" if site == "mixed" else "light"] == table0, (b, mixed, site, rnd)
                lights.add((site, table0))
        assert got[0]["light_mixed"] == -1  # no launch over the records of a round before round 0
    # the enumeration is not vacuous: every branch of the shade ladder (its last one at round 0 and at a later round), every generate
    # kernel, both k_light_s at both sites
    assert shade_cases == {1, 2, 3, 4, 5, 6, 7, (8, True), (8, False)}, shade_cases
    assert generates == {ref.GENERATE_C, ref.GENERATE_T, ref.GENERATE_S}
    assert lights == {(s, t) for s in ("mixed", "connect") for t in (0, 1)}, lights
    assert n == sum(b[7] for b in batches()) == 3024


def test_the_three_any_hit_rules(host_api):
    walks = set()
    for counting, wide, wide8 in itertools.product((0, 1, 2), (0, 1), (0, 1)):  # counting: RT_COUNT_*
        # the slot pipeline has no 8-wide walk: it passes wide8 = false whatever the scene has
        assert host_api.any_hit_walk(counting, wide, False) == ref.walk_connect(counting, wide), (counting, wide)
        w = host_api.any_hit_walk(counting, wide, wide8)
        assert w == ref.walk_connect_s(counting, wide, wide8) == ref.walk_occluded_scope(counting, wide, wide8), (counting, wide, wide8)
        walks.add(w)
    assert walks == {ref.WALK_COUNTING, ref.WALK_BINARY, ref.WALK_WIDE4, ref.WALK_WIDE8}


def test_what_the_entry_point_refuses(host_api):
    ok = (1, 1, 4, 1, 0, 0, 0, 5)
    assert host_api.launch_form(ok, 4)["shade"] == 0
    for facts, rnd in ((ok, 5), (ok, -1), (ok[:7] + (0,), 0), (ok[:2] + (0,) + ok[3:], 0), (ok[:2] + (5,) + ok[3:], 0)):
        with pytest.raises(RuntimeError, match="rt_launch_form: -"):
            host_api.launch_form(facts, rnd)
