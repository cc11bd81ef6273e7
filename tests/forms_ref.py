"""The launch ladders of the dense pipeline and the three any-hit rules as the host code spelt them before csrc/rt_forms.h, restated branch
by branch and in the same order, with the lines of commit 846b7ec they stood on (csrc/rt_api_render.inc unless another file is named).
tests/test_forms_cpu.py holds rt_launch_form / rt_any_hit_walk to this file over the whole space of facts.  A new form is a new case here.

A batch is the tuple of raw facts run_rounds_stream learns: (table, bounce_current, chain, bounce_knob, round0_entries, sampler, fisheye, rounds)."""

QL, BOUNCE, TABLE0, CHAIN = 1, 2, 4, 8  # k_shade_s's template parameters as bits
GENERATE_C, GENERATE_T, GENERATE_S = 0, 1, 2
BT_EMPTY, BT_BOUNCE, BT_CHAIN = 0, 1, 2  # shade's BounceTable argument: BounceTable{}, btab, chain[round - 1]
WALK_BINARY, WALK_COUNTING, WALK_WIDE4, WALK_LISTED, WALK_WIDE8 = 0, 1, 2, 3, 4


def derived(batch):
    """(bounce, chainDepth, direct)"""
    table, bounce_current, chain, bounce_knob, round0_entries, sampler, fisheye, rounds = batch
    bounce = bounce_current and bounce_knob and not sampler  # :520
    chain_depth = chain if bounce and rounds > 2 else 1  # :522
    direct = table and not sampler and not fisheye and round0_entries != 1  # :525
    return bool(bounce), chain_depth, bool(direct)


def generate(batch):
    _, _, direct = derived(batch)
    if direct:  # :527
        return GENERATE_C
    if batch[0]:  # :528
        return GENERATE_T
    return GENERATE_S  # :529


def shade(batch, rnd):
    """(branch, template bits, fresh, BounceTable argument, mask handed over, PrimaryTable handed over) of shade(rnd)"""
    sampler, rounds = batch[5], batch[7]
    bounce, chain_depth, direct = derived(batch)
    last = rnd + 1 == rounds
    if sampler:  # :559
        return 1, QL, int(rnd == 0), BT_EMPTY, 0, 0
    if direct and rnd == 0 and chain_depth > 1:  # :560
        return 2, BOUNCE | TABLE0 | CHAIN, 1, BT_BOUNCE, 1, 1
    if rnd == 0 and chain_depth > 1:  # :561
        return 3, BOUNCE | CHAIN, 1, BT_BOUNCE, 1, 0
    if rnd > 0 and rnd < chain_depth and not last:  # :562-564
        return 4, CHAIN, 0, BT_CHAIN, 1, 0
    if direct and rnd == 0 and bounce and not last:  # :565
        return 5, BOUNCE | TABLE0, 1, BT_BOUNCE, 1, 1
    if direct and rnd == 0:  # :566
        return 6, TABLE0, 1, BT_EMPTY, 0, 1
    if bounce and rnd == 0 and not last:  # :567
        return 7, BOUNCE, 1, BT_BOUNCE, 1, 0
    return 8, 0, int(rnd == 0), BT_EMPTY, 0, 0  # :568


def light_mixed(batch, rnd):
    """k_light_s's TABLE0 at the head of mixed round rnd > 0, over the shadow records of round rnd - 1"""
    _, _, direct = derived(batch)
    if direct and rnd == 1:  # :552
        return 1
    return 0  # :553


def light_after_connect(batch, rnd):
    """k_light_s's TABLE0 behind connect(rnd)"""
    _, _, direct = derived(batch)
    if direct and rnd == 0:  # :579
        return 1
    return 0  # :580


def light_launches(batch, mixed):
    """every k_light_s launch of the batch as (site, round of the loop, TABLE0), in launch order (:550-555, :570, :578-581)"""
    rounds = batch[7]
    out = []
    for rnd in range(rounds):
        last = rnd + 1 == rounds
        if mixed and rnd > 0:
            out.append(("mixed", rnd, light_mixed(batch, rnd)))
        if mixed and not last:
            continue
        out.append(("connect", rnd, light_after_connect(batch, rnd)))
    return out


def walk_connect(counting, wide):
    """launch_connect, :81-87"""
    if counting:
        return WALK_COUNTING
    if not wide:
        return WALK_BINARY
    return WALK_WIDE4


def walk_connect_s(counting, wide, wide8):
    """launch_connect_s, :365-376"""
    if counting:
        return WALK_COUNTING
    if wide8:
        return WALK_WIDE8
    if not wide:
        return WALK_BINARY
    return WALK_WIDE4


def walk_occluded_scope(counting, wide, wide8):
    """rt_occluded_scope, csrc/rt_api_query.inc:108-109 and :121-130 (wide: the context's 4-wide nodes, wide8: the scope's 8-wide ones)"""
    wide8_walk = not counting and wide8
    wide_walk = not counting and (wide or wide8_walk)
    if counting:
        return WALK_COUNTING
    if not wide_walk:
        return WALK_BINARY
    if wide8_walk:
        return WALK_WIDE8
    return WALK_WIDE4
