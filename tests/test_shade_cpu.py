"""CPU tier of the shade-step tests: on the oracle alone, no case of tests/shade_cases.py is vacuous.
  - Twins.  Every case names the scene, energy or depth just across its branch.  On the same rays and the same random streams the oracle's
    values differ from the twin's, by bits or by non-finite class, on at least half of the case's rays -- in every pipeline that shades it.
  - Random choices.  Where a path pipeline chooses at random (the child of a glass hit, a light's sampled position, the roulette) the
    repeats of one ray show both outcomes; each child of a glass hit is taken by at least two repeats.
  - Not compared against the floor.  The largest channel of at least half of a case's finite rays is 0.02 or more (in magnitude: Trace
    with the flag clear weighs its indirect child with a sum of either sign): an error of the bar's size (1e-4) is measured against the
    value, not against the 1e-3 floor of conftest.rel_err.
  - Non-finite expectations.  A light seen directly is (+inf, NaN, +inf) where its colour has a zero channel.
And a few inputs are shown to sit on the edge they are named for (dis == radius, cosi within 1e-3 of 0, exp underflowing to 0).
Where a condition falls short the input changes (tests/shade_cases.py), never the condition."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_cases as sc  # noqa: E402

PAIRS = [(c, p) for c in sc.CASES for p in c.pipelines]


def _id(pair):
    return "%s-%s" % (pair[0].name, pair[1])


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_twin_differs_and_values_are_above_the_floor(pair, oracle_api):
    case, pipeline = pair
    ref, twin = sc.twin_values(oracle_api, case, pipeline)
    assert ref.shape == (len(case.rays) * case.reps, 3)
    share = sc.changed_share(ref, twin)
    fin = np.isfinite(ref).all(1)
    big = float((np.abs(ref[fin]).max(1) >= sc.MIN_VALUE).mean()) if fin.any() else 1.0
    print("%s %s: twin differs on %.0f %% of %d rays; %d finite, %.0f %% of them >= %g" % (case.name, pipeline, 100 * share, len(ref), int(fin.sum()), 100 * big, sc.MIN_VALUE))
    assert share >= sc.MIN_SHARE, (case.name, pipeline, share)
    assert big >= 0.5, (case.name, pipeline, big)
    assert not np.isneginf(ref).any()
    if case.expect == "direct":
        assert not fin.any()  # a light met head-on: relStr = 1 / (0 * PI) * strength
    else:
        assert fin.any()


def _per_ray(case, values):
    return values.reshape(len(case.rays), case.reps, 3)


def _distinct(v):
    return np.unique(np.ascontiguousarray(v).view(np.uint32).reshape(len(v), 3), axis=0, return_counts=True)


MAKES = {"glass": ("sample", "sample_g0"), "light": sc.PATHS, "roulette": sc.ROULETTE}  # the pipelines that make each random choice (sample_g's glass child plays the roulette first)


@pytest.mark.parametrize("pair", [(c, p) for c, p in PAIRS if c.random and p in MAKES[c.random]], ids=_id)
def test_random_choices_go_both_ways(pair, oracle_api):
    case, pipeline = pair
    mode, flag, rt = sc.PIPELINES[pipeline]
    makes = MAKES[case.random]
    assert pipeline in makes
    ref, _ = sc.twin_values(oracle_api, case, pipeline)
    for k, v in enumerate(_per_ray(case, ref)):
        vals, counts = _distinct(v)
        print("%s %s ray %d: %d distinct values over %d repeats, counts %s" % (case.name, pipeline, k, len(vals), case.reps, sorted(counts.tolist(), reverse=True)[:4]))
        assert len(vals) >= 2, (case.name, pipeline, k)
        if case.random == "glass":
            # The refracted child leaves for the sky (one value); the reflected one stays inside (one or two more).  The values do not
            # say which child a repeat took: what is asserted is that the two most frequent values occur twice or more each, and two
            # repeats of one ray can only differ by the child taken at the first hit (or, after a reflection, at the second).
            assert np.sort(counts)[-2] >= 2, (case.name, pipeline, counts)
        if case.random == "roulette":
            dead = (v == 0).all(1).sum()
            assert 2 <= dead <= case.reps - 2, (case.name, pipeline, dead)


def test_direct_lights_have_the_class_pattern(oracle_api):
    """(+inf, NaN, +inf): the coloured light seen from the front, from behind and obliquely, and the lower of two stacked disks where it
    is the later in the table; the upper one where that is (Q6: the last light that passes the test wins, whatever its t)"""
    want = [2, 1, 2]
    for pipeline in sc.ALL:
        ref, twin = sc.twin_values(oracle_api, sc.BY_NAME["light_direct"], pipeline)
        assert (sc.classes(ref) == want).all(), pipeline
        assert (sc.classes(twin) == [2, 2, 2]).all(), pipeline
        ref, twin = sc.twin_values(oracle_api, sc.BY_NAME["light_stacked"], pipeline)
        c = _per_ray(sc.BY_NAME["light_stacked"], sc.classes(ref))
        assert (c[0] == [1, 2, 2]).all() and (c[1] == want).all(), pipeline   # x = 6: the upper disk is the later one; x = 9: the lower
        c = _per_ray(sc.BY_NAME["light_stacked"], sc.classes(twin))
        assert (c[0] == want).all() and (c[1] == [1, 2, 2]).all(), pipeline


def test_inputs_sit_on_their_edges(oracle_api):
    o, _ = sc.oracle_scene(oracle_api, "lamps", True)
    # the rim of the in-plane light: the hit point is exact and its distance to the light's centre is the radius, to the bit
    case = sc.BY_NAME["light_in_plane"]
    O, D = np.stack([r[0] for r in case.rays]), np.stack([r[1] for r in case.rays])
    hit = o.find_nearest(O, D, t_min=1e-6)
    assert (hit["obj"] == 0).all() and (hit["t"] == 2).all()
    P = O + hit["t"][:, None] * D
    dis = np.sqrt(((P - np.float32([18, 0, 0])) ** 2).sum(1, dtype=np.float32))
    assert dis[0] == dis[1] == np.float32(0.5) and (dis[2:] < 0.5).all()
    # the other lamps cases shade what they say: the floor, or the sphere in front of the disk
    for name, objs in (("light_behind_sphere", {3}), ("light_below", {0}), ("light_occluder", {0}), ("dir_cone", {0, 6}), ("light_parallel", {-1})):
        c = sc.BY_NAME[name]
        got = o.find_nearest(np.stack([r[0] for r in c.rays]), np.stack([r[1] for r in c.rays]), t_min=1e-6)
        assert set(got["obj"].tolist()) == objs, (name, got["obj"])
    # the shadow rays of 'light_occluder': blocked half-way, and free where the occluder starts just past the light (tmax is the light's distance)
    up = np.float32([[0, 1, 0]] * 2)
    at = np.float32([[36, 1e-4, 0], [42, 1e-4, 0]])
    assert o.is_occluded(at, up, np.float32([3, 3]))["occluded"].tolist() == [1, 0]
    assert o.is_occluded(at, up, np.float32([3, 3.2]))["occluded"].tolist() == [1, 1]
    # glass: grazing incidence within 1e-3 of 0; the critical angles on the side the cases say
    o, _ = sc.oracle_scene(oracle_api, "spec", True)
    c = sc.BY_NAME["glass_grazing"]
    hit = o.find_nearest(c.rays[0][0][None], c.rays[0][1][None], t_min=0.001)
    cosi = float((hit["normal"][0] * c.rays[0][1]).sum())
    assert hit["obj"][0] == 0 and 0 < -cosi < 1e-3
    # the wall of ir 1: sint = 1 / 1 * sqrt(1 - cosi * cosi) is 1 to the bit, so glass::fresnel's 'sint >= 1' answers with its equality
    c = sc.BY_NAME["glass_sint_1"]
    hit = o.find_nearest(c.rays[0][0][None], c.rays[0][1][None], t_min=0.001)
    d = c.rays[0][1]
    cosi = np.float32(d[0] * (np.float32(1) / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))   # dot(normalize(D), (1, 0, 0))
    assert hit["obj"][0] == 8 and (hit["normal"][0] == [1, 0, 0]).all() and cosi < 0
    assert np.sqrt(np.maximum(np.float32(0), np.float32(1) - cosi * cosi)) == np.float32(1)
    for name, ir, beyond in (("glass_ir1.5_inside_beyond", 1.5, True), ("glass_ir2.4_inside_beyond", 2.4, True), ("glass_ir1.5_inside_below", 1.5, False),
                             ("glass_ir2.4_inside_below", 2.4, False), ("glass_ir0.8_outside_beyond", 1 / 0.8, True)):
        c = sc.BY_NAME[name]
        hit = o.find_nearest(c.rays[0][0][None], c.rays[0][1][None], t_min=0.001)
        cosi = float((hit["normal"][0].astype(np.float64) * c.rays[0][1]).sum())
        assert (cosi > 0) == ("inside" in name)
        assert (ir * np.sqrt(1 - cosi * cosi) >= 1) == beyond, name
    c = sc.BY_NAME["glass_absorption_underflow"]
    hit = o.find_nearest(np.stack([r[0] for r in c.rays]), np.stack([r[1] for r in c.rays]), t_min=0.001)
    assert (hit["obj"] == 5).all() and (np.exp(np.float64(sc.DENSE[0]) * -hit["t"]).astype(np.float32) == 0).all()
    assert (np.exp(np.float64(sc.DENSE_TWIN[0]) * -hit["t"]).astype(np.float32) > 0).all()
    # the back side of a triangle: the ray and the normal point the same way
    c = sc.BY_NAME["glass_ir1.5_triangle_back"]
    hit = o.find_nearest(np.stack([r[0] for r in c.rays]), np.stack([r[1] for r in c.rays]), t_min=0.001)
    assert (hit["obj"] == 3000).all() and ((hit["normal"] * np.stack([r[1] for r in c.rays])).sum(1) > 0).all()


def test_no_light_is_black_under_trace(oracle_api):
    """count_0 runs in the path functions alone: both Trace functions give exactly 0 on its rays at every depth.  With the flag set the
    light loop is empty; with it clear it is empty too, so diffuse::scatter never writes scatteredDir and the indirect child is weighed
    with dot((0, 0, 0), (1, 1, 1)) = 0.  (Not run on the device: the child is a ray of direction (0, 0, 0).)"""
    case = sc.BY_NAME["count_0"]
    assert not {"trace", "trace_g"} & set(case.pipelines)
    O, D = np.stack([r[0] for r in case.rays] * 8), np.stack([r[1] for r in case.rays] * 8)
    for pipeline in ("trace", "trace_g"):
        hit = sc.oracle_scene(oracle_api, "spec", sc.PIPELINES[pipeline][2])[0].find_nearest(O, D, t_min=1e-6)
        assert (hit["obj"] == 7).all()
        for depth in (1, 2, 3):
            assert (sc.oracle_batch(oracle_api, "spec", pipeline, depth, O, D) == 0).all(), (pipeline, depth)


def test_the_cases_are_the_issue_s():
    """the families and what each must hold: nothing dropped without this file noticing"""
    names = set(sc.BY_NAME)
    for ir in ("0.8", "1", "1.5", "2.4"):
        assert {"glass_ir%s_%s" % (ir, k) for k in ("outside_normal", "inside_below", "triangle_front", "triangle_back")} <= names
    assert {"glass_ir1.5_inside_beyond", "glass_ir2.4_inside_beyond", "glass_ir0.8_outside_beyond", "glass_grazing", "glass_sint_1", "glass_absorption_underflow"} <= names
    assert {"diffuse_N0", "diffuse_N1", "diffuse_N200", "diffuse_pow_0_0", "diffuse_fmax_floor", "diffuse_retention", "diffuse_shininess", "metal_energy"} <= names
    assert {"light_direct", "light_parallel", "light_stacked", "light_behind_sphere", "light_in_plane", "light_normal_z", "light_normal_x", "light_below", "light_occluder"} <= names
    assert {"dir_cone", "dir_outside", "dir_sin_angle_1", "count_0", "count_1", "count_31", "count_32", "instance_glass", "instance_diffuse"} <= names
    assert {"roulette_ends", "roulette_ends_no_gate", "roulette_depth_4", "roulette_depth_5", "roulette_channel"} <= names
    assert sc.LAMPS == 31 and sc.MANY == 32 and sc.IRS == (0.8, 1.0, 1.5, 2.4) and sc.INST_SCALES == (0.5, 2.0)
    assert {"glass_ir1.5_triangle_back_beyond", "glass_ir2.4_triangle_back_beyond"} <= names   # where Trace meets kr == 1
    for c in sc.CASES:
        assert 8 <= len(c.rays) * c.reps <= 64 and c.reps >= 16
        if c.family == 7:
            assert set(c.pipelines) == set(sc.ROULETTE), c.name
        elif c.name.endswith("_inside_beyond"):   # black in Trace at any depth (shade_cases._cases)
            assert set(c.pipelines) == {"sample", "sample_g", "sample_g0"}, c.name
        elif c.name == "count_0":                 # black in both Trace functions (test_no_light_is_black_under_trace)
            assert set(c.pipelines) == {"sample", "sample_g", "sample_g0"}, c.name
        elif c.name == "diffuse_shininess":       # the path wavefront cannot replay a shiny material: Sample runs k_sample_general ('sample_g0')
            assert set(c.pipelines) == set(sc.ALL) - {"sample"}, c.name
        else:
            assert set(c.pipelines) == set(sc.ALL), c.name
    assert all(e != 1 for e in sc.ENERGY) and sc.MATTE_ENERGY[0] - (1 - sc.RETAIN["zero"][1][0]) == 0
