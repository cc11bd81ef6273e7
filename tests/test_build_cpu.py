"""CPU tier for the crafted builder and refit inputs of tests/build_cases.py: every input reaches the branch it is listed for, shown with the
oracle (oracle/orc_bvh.h), the plain restatement of tlas::build and the host-only layout builder.  tests/test_gpu_build.py holds the device
to the same inputs; with this tier it cannot pass because an input turned out harmless."""
import numpy as np
import pytest

import build_cases as bc
import instances_ref as ir

ROOT_CASES = ["root%d" % n for n in (255, 256, 257, 511, 512, 513, 1025)]
EQUAL_CASES = ["equal40", "equal30_outlier_hi", "equal30_outlier_lo"]


@pytest.fixture(scope="module")
def dumps(oracle_api):
    """the oracle's tree of every (case, split) that is run: built once, read by every test"""
    return {(name, s): bc.oracle_bvh(oracle_api, name, s) for name, s in bc.bvh_runs()}


def leaves(ref):
    nd = ref["nodes"]
    return [i for i in range(ref["nodes_used"]) if i != 1 and nd[i, 7] > 0]


def permuted_leaves(ref):
    """leaves whose primitiveIdx range is not ascending: the partition loop ran over them (bvh.cpp:296-313)"""
    nd, prim = ref["nodes"], ref["prim_idx"].astype(np.int64)
    return [i for i in leaves(ref) if np.any(np.diff(prim[nd[i, 3]:nd[i, 3] + nd[i, 7]]) < 0)]


def root_left(ref):
    """(the primitives of the root's left child in their original numbering, the root's count) of a tree whose root was split"""
    first, count = bc.tree_ranges(ref)
    assert ref["nodes"][0, 7] == 0, "the root was split"
    lc = int(ref["nodes"][0, 3])
    return np.sort(ref["prim_idx"][first[lc]:first[lc] + count[lc]].astype(np.int64)), int(count[0])


def test_case_table():
    """the inputs are the ones listed: sizes, dtypes, finiteness, which splits run"""
    want = {"equal40": (40, 0, 0), "equal30_outlier_hi": (31, 0, 0), "equal30_outlier_lo": (31, 0, 0), "random1": (1, 0, 0), "random2": (2, 0, 0),
            "random3": (3, 0, 0), "presorted": (600, 0, 0), "ascending": (600, 0, 0), "duplicate_keys": (300, 0, 0), "lattice": (512, 0, 0),
            "lattice_flat": (512, 0, 0), "chain": (40, 0, 0), "staircase": (1023, 0, 0), "mixed_plane": (257, 70, 1), "mixed": (257, 70, 0),
            "spheres1": (0, 1, 0), "spheres2": (0, 2, 0), "spheres65": (0, 65, 0), "mixed_sparse": (257, 70, 0), "signed_zeros": (96, 0, 0), "lattice_zero_signs": (64, 0, 0)}
    want.update({"root%d" % n: (n, 0, 0) for n in (255, 256, 257, 511, 512, 513, 1025)})
    assert {k: bc.sizes(k) for k in bc.BVH_CASES} == want
    for name, arrays in bc.BVH_CASES.items():
        for a, width in zip(arrays, (9, 4, 4)):
            assert a is None or (a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == width and np.isfinite(a).all()), name
    runs = bc.bvh_runs()
    assert len(set(runs)) == len(runs)
    for name in bc.BVH_CASES:
        n = sum(bc.sizes(name)[:2])
        assert [s for c, s in runs if c == name] == ([0, 1, 2, 3] if n <= bc.SAH_MAX else [0, 1, 2]), name
    assert max(sum(bc.sizes(k)) for k in bc.BVH_CASES) == 1025 and max(sum(bc.sizes(c)) for c, s in runs if s == 3) <= bc.SAH_MAX
    # the keys the cases are named for
    k = bc.keys("duplicate_keys")
    assert sorted(np.unique(k[:, 0], return_counts=True)[1]) == [75] * 4 and len(np.unique(k[:, 1])) > 290  # (y, z: random)
    assert len(np.unique(bc.keys("lattice_flat")[:, 2])) == 1 and len(np.unique(bc.keys("lattice")[:, 2])) == 8
    assert np.all(np.diff(bc.keys("presorted")[:, 0]) < 0) and np.all(np.diff(bc.keys("ascending")[:, 0]) > 0)
    s = bc.BVH_CASES["mixed"][1]
    assert s[:, 3].min() >= 0.05 and s[:, 3].max() <= 1.5 and bc.BVH_CASES["mixed_plane"][0] is bc.BVH_CASES["mixed"][0]


@pytest.mark.parametrize("case,split", bc.bvh_runs(), ids=lambda v: str(v))
def test_oracle_builds_every_case(case, split, dumps):
    """the oracle builds a whole tree over the intended primitives: the counts, a permutation in primitiveIdx, every primitive in one leaf"""
    ref = dumps[(case, split)]
    nt, ns, npl = bc.sizes(case)
    assert (ref["NTri"], ref["NSph"], ref["NPla"], ref["N"]) == (nt, ns, npl, nt + ns + npl)
    assert ref["nodes_used"] % 2 == 0 and np.array_equal(np.sort(ref["prim_idx"]), np.arange(ref["N"]))
    first, count = bc.tree_ranges(ref)
    assert (first[0], count[0]) == (0, ref["N"])
    sub = 2 if npl and nt + ns else 0  # separatePlanes: node 2 is what Subdivide starts from
    assert count[sub] == nt + ns, "the subdivided root holds every triangle and sphere"
    lv = leaves(ref)
    assert sum(int(ref["nodes"][i, 7]) for i in lv) == ref["N"] and 1 <= ref["max_depth"] <= ref["N"] + 1


def test_depth_crosses_the_launch_groups(dumps):
    """rt_build_bvh_split launches LEVEL_GROUP levels, then reads the open count back: the chain under LONGESTAXIS crosses two group
    boundaries, and every other method has a case that crosses one"""
    assert dumps[("chain", 2)]["max_depth"] > 2 * bc.LEVEL_GROUP
    assert dumps[("chain", 2)]["max_depth"] == 40  # one triangle per level
    for s in (0, 1, 3):
        deep = [c for (c, sp), ref in dumps.items() if sp == s and ref["max_depth"] > bc.LEVEL_GROUP]
        assert deep, "no case deeper than one launch group under split %d" % s
    assert dumps[("staircase", 1)]["max_depth"] == 19  # two levels per halving of 1023 (build_cases._staircase)
    for c in ROOT_CASES[:6]:
        assert dumps[(c, 0)]["max_depth"] > bc.LEVEL_GROUP and dumps[(c, 3)]["max_depth"] >= bc.LEVEL_GROUP, c


def test_root_counts_sit_at_the_block(dumps):
    """the partition of the root runs over 255 .. 1025 positions under every method that is run: chunks of BUILD_THREADS with one lane to
    spare, exactly full, and one lane into the next chunk"""
    sizes = sorted(bc.sizes(c)[0] for c in ROOT_CASES)
    assert sizes == [bc.BUILD_THREADS - 1, bc.BUILD_THREADS, bc.BUILD_THREADS + 1, 2 * bc.BUILD_THREADS - 1, 2 * bc.BUILD_THREADS,
                     2 * bc.BUILD_THREADS + 1, 4 * bc.BUILD_THREADS + 1]
    for (c, s), ref in dumps.items():
        if c in ROOT_CASES:
            left, n = root_left(ref)
            assert n == bc.sizes(c)[0] and 0 < len(left) < n, (c, s)


def test_presorted_and_ascending_partitions(dumps):
    """descending keys: the root's left side is the primitives at the back of the range, so every position below min(nL, n - nL) is a hole
    and its partner a filler, and there are more of them than one chunk of the block: the holesSeen / fillersSeen carries are used.
    ascending keys: the left side already sits in front, K = 0."""
    for s in bc.SPLITS:
        left, n = root_left(dumps[("presorted", s)])
        nL = len(left)
        assert np.array_equal(left, np.arange(n - nL, n)), s
        assert min(nL, n - nL) > bc.BUILD_THREADS, (s, nL)
        left, n = root_left(dumps[("ascending", s)])
        assert np.array_equal(left, np.arange(len(left))), s


def samesize_repeats(case, ref):
    """nodes of a SAMESIZE tree (count >= 2) whose median key (bvh.cpp:240-252) more than one of their primitives has"""
    k = bc.keys(case)
    first, count = bc.tree_ranges(ref)
    nf = ref["nodes"].view(np.float32)
    out = []
    for i in range(ref["nodes_used"]):
        if i == 1 or count[i] < 2:
            continue
        prims = ref["prim_idx"][first[i]:first[i] + count[i]]
        if prims.max() >= len(k):
            continue  # a node that holds planes is never subdivided
        a = bc.longest_axis(nf[i, 0:3], nf[i, 4:7])
        ks = np.sort(k[prims, a])
        if (ks == ks[count[i] // 2]).sum() > 1:
            out.append(i)
    return out


def test_samesize_median_is_repeated(dumps):
    for case in ("duplicate_keys", "staircase", "lattice", "equal40"):
        assert samesize_repeats(case, dumps[(case, 1)]), case
    # the root of duplicate_keys: 75 copies of the median key; the staircase: the median is repeated on every second level
    ref = dumps[("duplicate_keys", 1)]
    assert 0 in samesize_repeats("duplicate_keys", ref) and len(root_left(ref)[0]) == 150
    assert len(samesize_repeats("staircase", dumps[("staircase", 1)])) >= 9
    # ... and with distinct keys it never is
    assert not samesize_repeats("root513", dumps[("root513", 1)])


def test_leaves_with_permuted_ranges(dumps):
    """'a leaf after all, with its range permuted' (bvh.cpp:315): the partition ran, one side stayed empty"""
    for s in (1, 2, 3):
        assert any(permuted_leaves(dumps[(c, s)]) for c in EQUAL_CASES), s
    assert permuted_leaves(dumps[("equal40", 1)]) == [0] and permuted_leaves(dumps[("equal40", 2)]) == [0]  # the root itself
    # LONGESTAXIS leaves empty sides wherever the keys repeat
    assert any(dumps[("duplicate_keys", 2)]["nodes"][i, 7] > 1 for i in leaves(dumps[("duplicate_keys", 2)]))


def split_nodes_with_spheres(case, ref):
    """how many nodes that Subdivide split hold a sphere"""
    nt, ns, npl = bc.sizes(case)
    first, count = bc.tree_ranges(ref)
    found = 0
    for i in range(2 if npl else 0, ref["nodes_used"]):  # (with a plane the root is separatePlanes' node, not a split)
        if ref["nodes"][i, 7] == 0:
            prims = ref["prim_idx"][first[i]:first[i] + count[i]]
            found += int(np.any((prims >= nt) & (prims < nt + ns)))
    return found


def test_splits_of_nodes_with_spheres(dumps):
    """EvaluateSAH's sphere quirk (pos[axis] -+ r on all three axes, bvh.cpp:533-544) decides splits of the mixed cases under SAH; under
    binned SAH the bins of mixed_sparse grow by 2 r (Q3), while the large primitives of mixed are cheaper unsplit"""
    for case in ("mixed", "mixed_plane", "mixed_sparse"):
        assert split_nodes_with_spheres(case, dumps[(case, 3)]) >= 10, case
    assert split_nodes_with_spheres("mixed_sparse", dumps[("mixed_sparse", 0)]) >= 10
    assert dumps[("mixed", 0)]["nodes_used"] == 2 and dumps[("mixed_plane", 0)]["nodes_used"] == 4
    assert dumps[("spheres65", 3)]["nodes_used"] == 130


def test_zero_bounds_carry_both_signs(dumps):
    """signed_zeros, lattice_zero_signs: under every method the oracle's tree has zero bounds of both signs, and nodes whose lower bound is
    +0 although a corner below them is -0 there (the last zero the ternary met was +0), or whose upper bound is -0 over a +0 corner: an
    order-free hardware minimum / maximum gives other bits for these nodes"""
    for case in ("signed_zeros", "lattice_zero_signs"):
        tv = bc.BVH_CASES[case][0].reshape(-1, 3, 3)
        bits = tv.view(np.uint32)
        neg, pos = (bits == 0x80000000).any(axis=1), (bits == 0).any(axis=1)  # [primitive][axis]: a -0.0 / +0.0 among the corners
        assert neg.any() and pos.any(), case
        for s in bc.SPLITS:
            ref = dumps[(case, s)]
            first, count = bc.tree_ranges(ref)
            used = [i for i in range(ref["nodes_used"]) if i != 1]
            box = ref["nodes"][used][:, [0, 1, 2, 4, 5, 6]]
            assert (box == 0).any() and (box == 0x80000000).any(), (case, s)
            found = 0
            for i in used:
                prims = ref["prim_idx"][first[i]:first[i] + count[i]]
                for k in range(3):
                    found += int(ref["nodes"][i, k] == 0 and neg[prims, k].any()) + int(ref["nodes"][i, 4 + k] == 0x80000000 and pos[prims, k].any())
            assert found >= 1, (case, s)
    # the lattice: both z bounds of every node are zeros, leaves, inner nodes and the root alike
    ref = dumps[("lattice_zero_signs", 0)]
    nf = ref["nodes"].view(np.float32)
    used = [i for i in range(ref["nodes_used"]) if i != 1]
    assert ref["nodes"][0, 7] == 0 and np.all(nf[used][:, [2, 6]] == 0)


# ---- TLAS -----------------------------------------------------------------------------------------------------------------------------
def test_tlas_set_table():
    want = {"grid4x4x4": 64, "grid16x16x1": 256, "grid256x1x1": 256, "line63": 63, "line64": 64, "line65": 65, "line129": 129, "grid6x6x6_permuted": 216,
            "identical5": 5, "identical256": 256, "points4x4x4": 64, "concentric40": 40, "huge3x3": 9, "beyond2x2": 4}
    assert {k: len(v) for k, v in bc.TLAS_SETS.items()} == want
    for name, b6 in bc.TLAS_SETS.items():
        assert b6.dtype == np.float32 and b6.shape[1] == 6 and np.isfinite(b6).all() and np.all(b6[:, :3] <= b6[:, 3:]) and np.abs(b6).max() < 1e30, name
    g = bc.TLAS_SETS["grid4x4x4"]
    assert np.all(g[:, 3:] - g[:, :3] == 1) and set(np.unique(g[:, :3])) == {0, 2, 4, 6}
    assert sorted(map(tuple, bc.TLAS_SETS["grid6x6x6_permuted"])) == sorted(map(tuple, bc._grid(6, 6, 6)))
    assert not np.array_equal(bc.TLAS_SETS["grid6x6x6_permuted"], bc._grid(6, 6, 6))
    assert np.all(bc.TLAS_SETS["points4x4x4"][:, :3] == bc.TLAS_SETS["points4x4x4"][:, 3:])
    c = bc.TLAS_SETS["concentric40"]
    assert np.all(c[1:, :3] < c[:-1, :3]) and np.all(c[1:, 3:] > c[:-1, 3:])
    assert set(bc.TLAS_TIED) == set(want) - {"concentric40", "beyond2x2"}


@pytest.mark.parametrize("name", list(bc.TLAS_SETS))
def test_tlas_restatement_terminates_and_ties(name):
    b6 = bc.TLAS_SETS[name]
    n = len(b6)
    stats = {}
    nodes = bc.tlas_reference(b6, stats)  # (raises after 4 n^2 + 16 rounds)
    if name in bc.TLAS_NO_MATCH:
        assert nodes is None and stats["calls"] == 1, "no union area below 1e30 at the first step"
        return
    ir.check_numbering(nodes, n)
    assert stats["calls"] >= 2 * n - 3
    if name in bc.TLAS_TIED:
        assert stats["tied"] > 0, "no FindBestMatch call met equal smallest areas"
    if n <= 65:  # the other restatement of the suite (scalar f32 arithmetic, one candidate at a time): the same nodes
        assert np.array_equal(nodes, ir.tlas_build(b6))


def test_tlas_huge_areas_stay_below_the_sentinel():
    """huge3x3: every union area FindBestMatch can meet is far above anything a scene has and below its 1e30; beyond2x2: none is below"""
    def areas(b6):
        lo = np.minimum(b6[:, None, :3], b6[None, :, :3])
        hi = np.maximum(b6[:, None, 3:], b6[None, :, 3:])
        e = (hi - lo).astype(np.float32)
        a = (e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2]) + e[..., 2] * e[..., 0]
        return a[~np.eye(len(b6), dtype=bool)]
    h = bc.TLAS_SETS["huge3x3"]
    whole = np.concatenate([h[:, :3].min(0), h[:, 3:].max(0)])[None]
    assert areas(h).min() > 1e28 and areas(np.concatenate([h, whole])).max() < np.float32(1e30)
    assert areas(bc.TLAS_SETS["beyond2x2"]).min() >= np.float32(1e30) and np.isfinite(areas(bc.TLAS_SETS["beyond2x2"])).all()


# ---- the refit scene --------------------------------------------------------------------------------------------------------------------
def test_refit_scene_profile(host_api, oracle_api):
    """rt_set_time's launch plan on the refit scene: going up from the deepest level wide, narrow, wide, narrow -- the narrow levels between
    two wide ones are the branch that launches them one by one -- and the pair records are the oracle's nodes, two per record"""
    tv = bc.refit_triangles()
    assert len(tv) < 20000 and np.isfinite(tv).all()
    h = host_api.HostScene()
    bc.refit_scene(h)
    L = host_api.layout(h.describe(), 1, 0, 1)
    counts, profile = bc.refit_profile(L["refitLevelStart"])
    assert profile == "WnWn", (profile, list(counts))
    assert L["refitLevels"] == len(counts) and counts.sum() == len(L["refitOrder"]) and np.all(counts > 0)
    wide = np.flatnonzero(counts >= bc.REFIT_WIDE)
    gap = np.arange(wide.min(), wide.max() + 1)
    between = [l for l in gap if counts[l] < bc.REFIT_WIDE]
    assert len(between) >= 2 and wide.min() > 0, "several narrow levels between the wide ones, and a narrow top for the single-workgroup kernel"
    assert L["wideOK"] and L["animSlots"] == len(tv)
    o = oracle_api.OracleScene()
    bc.refit_scene(o)
    ref, got = o.bvh_dump(-1), h.bvh_dump(-1)
    assert ref["nodes_used"] == got["nodes_used"] == 2 * len(L["pairs"]) // 16 and np.array_equal(ref["prim_idx"], got["prim_idx"])
    lo, hi = bc.pair_boxes(L["pairs"])
    used = ref["nodes_used"]
    assert np.array_equal(lo[2:used], ref["nodes"][2:used, 0:3]) and np.array_equal(hi[2:used], ref["nodes"][2:used, 4:7])
    # the animation moves the boxes: the oracle's refit at t = 0.6 differs from the uploaded tree, and t = 0 restores it
    o.set_time(0.6)
    moved = o.bvh_dump(-1)["nodes"]
    assert (moved[2:used] != ref["nodes"][2:used]).any(axis=1).mean() > 0.5
    o.set_time(0.0)
    assert np.array_equal(o.bvh_dump(-1)["nodes"][2:used], ref["nodes"][2:used])
    # the rays of the GPU tier meet the clusters
    O, D = bc.refit_rays(4000, 7)
    hit = o.find_nearest(O, D)["obj"] != -1
    assert 400 < hit.sum() < 3600
    far = O[:, 2] > 100
    assert hit[far].sum() > 200 and hit[~far].sum() > 200
    o.close()
    h.close()
