"""CPU tier of the start-depth tests: on the oracle alone, the inputs of tests/test_gpu_depths.py tell neighbouring depths apart.  A
device that answered depth d with the result of depth d - 1 or d + 1 (one round too few in a round loop, a 'depth < 5' off by one) must
miss the radiance bar on many rays, not on one ray that happens to be non-finite: for every scene, function and pair of neighbouring
tested depths, the share of the caller rays that are finite at both depths and differ is held above the thresholds of
tests/depth_cases.py.  Where a share falls short the input changes (camera, ray set), never the threshold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cases as dc  # noqa: E402

# Sample and Trace as Tick calls them (parts A and C) next to the general kernels' cases (part B)
CASES = [(name, dc.SAMPLE, False, dc.PATH_DEPTHS) for name in dc.PATH_SCENES] \
    + [(name, dc.TRACE, True, depths) for name, (_, _, depths) in dc.WHITTED_CASES.items()] + dc.GENERAL_CASES


def _id(case):
    name, mode, flag, _ = case
    return "%s-%s-flag_%s" % (name, "Sample" if mode == dc.SAMPLE else "Trace", "set" if flag else "clear")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_neighbouring_depths_differ(case, scenes, oracle_api):
    name, mode, flag, depths = case
    ref = dc.oracle_values(scenes, oracle_api, name, mode, flag, depths)
    for d in depths:
        fin = np.isfinite(ref[d])
        assert fin.all(1).mean() > 0.75 and np.abs(ref[d][fin]).sum() > 0, (name, d)  # (a light met head-on is +inf: a few dozen rays; 'hall' at depth 12: 13 %)
        if mode == dc.SAMPLE and d < 0:
            assert np.all(ref[d] == np.float32(0.05))
    for lo, hi in zip(depths, depths[1:]):
        share = dc.changed_share(ref[lo], ref[hi])
        need = dc.MIN_SHARE_DEEP if hi >= dc.DEEP_FROM else dc.MIN_SHARE
        if (lo, hi) == (4, 5) and dc.roulette_case(mode, flag):
            need = dc.MIN_SHARE_ROULETTE
        if name == "hall":
            need = dc.MIN_SHARE_HALL
            if hi - lo > 1:
                # 7 -> 12 is no step of one level.  A call tree of depth 12 has up to 4096 leaves, and in 13 % of the trees one of them meets
                # the light's disk head-on (+inf): no more than 87 % of the rays are finite at both depths (83 % differ).  The 90 % are asked of those
                need *= float((np.isfinite(ref[lo]).all(1) & np.isfinite(ref[hi]).all(1)).mean())
        print("%s %s flag %d: %d -> %d differs on %.2f %% of the rays (needs %.1f %%)" % (name, "Sample" if mode else "Trace", flag, lo, hi, 100 * share, 100 * need))
        assert share >= need, (name, mode, flag, lo, hi, share)


def test_the_cases_are_the_issue_s():
    """the lists the device is held to: nothing dropped from them without this file noticing"""
    assert dc.PATH_DEPTHS == tuple(range(-1, 8)) and len(dc.PATH_ENVS) == 7 and dc.PATH_SCENES == ("mixed_small", "pretty_tlas")
    by = {(n, m, f): d for n, m, f, d in dc.GENERAL_CASES}
    for name in ("mixed_small_rt0", "pretty_tlas_rt0"):
        assert by[(name, dc.TRACE, False)] == by[(name, dc.SAMPLE, True)] == tuple(range(1, 8))
    assert by[("shiny", dc.TRACE, False)] == tuple(range(1, 8)) and by[("shiny", dc.SAMPLE, False)] == tuple(range(-1, 8))
    assert by[("hall", dc.SAMPLE, False)] == tuple(range(0, 6)) and by[("hall", dc.TRACE, False)] == tuple(range(1, 8)) + (12,)
    assert dc.WHITTED_CASES["mixed_small"] == (97, 61, (1, 2, 3, 5, 7)) and dc.WHITTED_CASES["pretty_tlas"] == (120, 67, (1, 2, 3, 5, 7))
    assert dc.WHITTED_CASES["shiny_rt"][2] == (1, 2, 3) and len(dc.WHITTED_ENVS) == 3


def test_materials_wrapper_builds_the_same_scene(scenes, oracle_api):
    """'shiny_rt' is 'shiny' with another materials flag and nothing else: the same nearest hits, and Trace with the flag set sees
    the flag of the materials (diffuse::scatter draws only when it is clear), so its values are those of no other scene here"""
    o0, r0 = dc.oracle_pair(scenes, oracle_api, "shiny")
    o1, r1 = dc.oracle_pair(scenes, oracle_api, "shiny_rt")
    O, D = r0.primary_rays()
    a, b = o0.find_nearest(O, D), o1.find_nearest(O, D)
    assert np.array_equal(a["obj"], b["obj"]) and np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)) and (a["obj"] != -1).mean() > 0.3
    for r in (r0, r1):
        r.close()
    for o in (o0, o1):
        o.close()
