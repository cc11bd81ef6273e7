"""The device builders and the refit on the crafted inputs of tests/build_cases.py, bit for bit against the oracle: k_build_level under all
four split methods (equal keys, equal costs, empty sides, node sizes at the block, trees deeper than two launch groups), k_build_tlas on boxes
whose union areas tie, and the boxes k_animate / k_refit / k_refit_level / k_wide_sync leave behind rt_set_time, read back as pair records.
tests/test_build_cpu.py shows on the CPU that every input reaches the branch it is here for."""
import ctypes as C

import numpy as np
import pytest

import build_cases as bc
import instances_ref as ir
import support as sp
from conftest import random_rays

pytestmark = pytest.mark.gpu
TIMES = (0.6, 2.9, 7.5, 0.0)


@pytest.fixture(scope="module")
def dev(host_api):
    """one context for the builder calls of this module (they need no scene)"""
    r = host_api.HostRenderer(8, 8)
    yield r
    r.close()


# ---- bvh::Build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,split", bc.bvh_runs(), ids=lambda v: str(v))
def test_bvh_builder_equals_oracle(case, split, dev, oracle_api):
    tv, sph, pla = bc.BVH_CASES[case]
    bc.same_tree(dev.build_bvh(tv, sph, pla, split=split), bc.oracle_bvh(oracle_api, case, split))


@pytest.mark.parametrize("split", bc.SPLITS)
def test_bvh_builder_refusals(split, dev, host_api, oracle_api):
    tv, sph, _ = bc.BVH_CASES["mixed"]
    unsupported, arg = "rt_amd error %d:" % host_api.RT_E_UNSUPPORTED, "rt_amd error %d:" % host_api.RT_E_ARG
    for col, value in ((3, np.inf), (3, np.nan), (0, np.inf), (1, -np.inf), (2, np.nan)):  # radius, centre
        bad = sph.copy()
        bad[17, col] = value
        with pytest.raises(RuntimeError, match=unsupported):
            dev.build_bvh(tv, bad, split=split)
        with pytest.raises(RuntimeError, match=unsupported):
            dev.build_bvh(None, bad, split=split)
    with pytest.raises(RuntimeError, match=unsupported):
        dev.build_bvh(None, None, [[0, 1, 0, 1]], split=split)  # planes only
    for s in (4, -1):
        with pytest.raises(RuntimeError, match=arg):
            dev.build_bvh(tv, sph, split=s)
    # the context builds the next input as if nothing had been refused
    bc.same_tree(dev.build_bvh(tv, sph, split=split), bc.oracle_bvh(oracle_api, "mixed", split))


# ---- tlas::build ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bc.TLAS_SETS))
def test_tlas_builder_equals_restatement(name, dev, host_api):
    b6 = bc.TLAS_SETS[name]
    ref = bc.tlas_reference(b6)
    if name in bc.TLAS_NO_MATCH:
        assert ref is None
        with pytest.raises(RuntimeError, match="rt_amd error %d:" % host_api.RT_E_UNSUPPORTED):
            dev.build_tlas(b6)
        b6 = bc.TLAS_SETS["grid4x4x4"]  # ... and the next set is built correctly
        ref = bc.tlas_reference(b6)
    got = dev.build_tlas(b6)
    assert got.dtype == np.uint32 and np.array_equal(got, ref)


def test_tlas_ties_through_set_instances(host_api):
    """the real path of a tie-heavy set: 64 instances of one one-triangle mesh, moved onto the 4 x 4 x 4 grid with that set's boxes"""
    b6 = bc.TLAS_SETS["grid4x4x4"]
    n = len(b6)
    r = host_api.HostRenderer(16, 8)
    s = r.scene
    ir.triangles_scene(s, ir.grid_transforms(s, n), two_meshes=False)
    r.commit()
    rec = np.zeros(n, dtype=host_api.RT_INSTANCE_DTYPE)
    L = host_api.host_lib()
    for i in range(n):
        T = np.ascontiguousarray(s.trs(b6[i, :3] + np.float32(0.5), 1, 0.0, 0.0, 0.0), dtype=np.float32)
        inv = np.zeros(16, dtype=np.float32)
        L.rth_mat4_inverse(T.ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p))
        rec[i] = (s.instance_dump(i)["blas"], T, inv)
    assert r.set_instances(0, rec, b6) == 0
    got = r.download_tlas()
    assert np.array_equal(got, bc.tlas_reference(b6))
    assert np.array_equal(got, r.build_tlas(b6))
    r.close()


# ---- Scene::SetTime + bvh::Refit ------------------------------------------------------------------------------------------------------------
def _builders(scenes):
    return {"refit_scene": bc.refit_scene, "mixed_small": scenes.REGISTRY["mixed_small"], "tower": scenes.REGISTRY["tower"]}


@pytest.fixture(scope="module")
def refit_refs(scenes, oracle_api):
    """per scene the oracle's scene (built once) and its node boxes after set_time(t), filled in as the tests ask for them"""
    refs = {}

    def get(name):
        if name not in refs:
            o = oracle_api.OracleScene()
            _builders(scenes)[name](o)
            refs[name] = dict(o=o, nodes={}, uploaded=o.bvh_dump(-1))
        return refs[name]

    yield get
    for v in refs.values():
        v["o"].close()


def _oracle_at(ref, t):
    """the oracle's scene at time t (it stays there), and its nodes then"""
    ref["o"].set_time(t)
    if t not in ref["nodes"]:
        ref["nodes"][t] = ref["o"].bvh_dump(-1)["nodes"]
    return ref["nodes"][t]


def _rays(name):
    if name == "refit_scene":
        return bc.refit_rays(4000, 7)
    return random_rays(4000, 13, center=(0.0, 1.0, 3.0), spread=6.0) if name == "tower" else random_rays(4000, 13)


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", ["refit_scene", "mixed_small", "tower"])
def test_refit_boxes_equal_oracle(name, wide, scenes, host_api, refit_refs, monkeypatch):
    """After rt_set_time(t) pair record p holds the boxes of the oracle's nodes 2 p and 2 p + 1 after its SetTime(t) + Refit, for every pair
    of the tree; at t = 0 they are the uploaded ones again.  The queries at every t give the oracle's hits and flags: with RT_WIDE=1 through
    the 4-wide nodes k_wide_sync rewrote (the occlusion walk of clean rays) and the binary pairs, with RT_WIDE=0 through the pairs alone."""
    sp.clean_env(monkeypatch, {"RT_WIDE": wide, "RT_WIDE8": "0"})
    ref = refit_refs(name)
    used = ref["uploaded"]["nodes_used"]
    r = host_api.HostRenderer(16, 8)
    _builders(scenes)[name](r.scene)
    r.commit()
    uploaded = r.scene_array("pairs")
    assert len(uploaded) == 16 * (used // 2)
    lo0, hi0 = bc.pair_boxes(uploaded)
    assert np.array_equal(lo0[2:used], ref["uploaded"]["nodes"][2:used, 0:3]) and np.array_equal(hi0[2:used], ref["uploaded"]["nodes"][2:used, 4:7])
    O, D = _rays(name)
    tmax = np.random.default_rng(5).uniform(0.5, 8.0, len(O)).astype(np.float32)
    for t in TIMES:
        nodes = _oracle_at(ref, t)
        r.set_time(t)
        pairs = r.scene_array("pairs")
        lo, hi = bc.pair_boxes(pairs)
        assert np.array_equal(lo[2:used], nodes[2:used, 0:3]), (t, "aabbMin")
        assert np.array_equal(hi[2:used], nodes[2:used, 4:7]), (t, "aabbMax")
        if t == 0.0:
            assert np.array_equal(lo[2:used], lo0[2:used]) and np.array_equal(hi[2:used], hi0[2:used])
        else:
            assert (lo[2:used] != lo0[2:used]).any(), "the boxes moved"
        want = ref["o"].find_nearest(O, D)
        got = r.find_nearest(O, D)
        assert np.array_equal(got["obj"], want["obj"]) and np.array_equal(got["t"].view(np.uint32), want["t"].view(np.uint32)), t
        assert (want["obj"] != -1).sum() > len(O) // 20
        for tm in (None, tmax):
            assert np.array_equal(r.is_occluded(O, D, tm), ref["o"].is_occluded(O, D, tm)["occluded"]), t
        # the queries changed nothing
        assert np.array_equal(r.scene_array("pairs").view(np.uint32), pairs.view(np.uint32))
    r.close()
