"""CPU tier for rt_set_instance_list (include/rt_amd.h): the GPU cases of tests/test_gpu_instance_list.py are not vacuous.  Every step of
the walk of lists changes every array the call rewrites; the ray sets of the behaviour test meet, on the oracle, the instances whose
records are new in the step; and the host mirror's description after Scene::SetInstanceList is the one the tests assemble by hand."""
import numpy as np
import pytest

import instance_list_ref as il
import instances_ref as ir
import support as sp
import triangles_desc as td

f32 = np.float32


def _uploaded(host_api):
    h = host_api.HostScene()
    ir.triangles_scene(h, ir.grid_transforms(h, len(il.UPLOADED)))
    return h


def test_every_step_of_the_walk_changes_what_the_call_rewrites(host_api):
    """rt_layout_build of the updated description after each step differs from the step before in inst, scalars and reach, and in pairs
    unless both have no TLAS pair record; nInst and tlasPairs follow n; the TLAS copy in LDS is off at 38 and back at 37; the 256-instance
    list leaves BLAS 1 without an instance and the layout keeps its records."""
    h = _uploaded(h_api := host_api)
    d = td.Desc(h_api, h)
    assert [int(b) for b in d.inst["blas"]] == list(il.UPLOADED)
    prev = h_api.layout(d.desc())
    blas_pairs = len(prev["pairs"]) // 16 - prev["tlasPairs"]
    lds = {}
    for k, st in enumerate(il.WALK):
        rec, b6 = il.walk_step(h_api, d, h, k)
        assert (b6 is not None) == st["given"] and len(rec) == st["n"] == d.n
        L = h_api.layout(d.desc())
        n = st["n"]
        assert L["nInst"] == n and L["tlasPairs"] == (n if n >= 2 else 0) and len(L["inst"]) == n * 32
        assert L["root"] == (0x40000000 if n == 1 else L["tlasBase"]) and L["tlasBase"] == (blas_pairs if n >= 2 else 0)
        assert len(L["pairs"]) // 16 == blas_pairs + L["tlasPairs"], "no BLAS is laid out again, with or without an instance"
        for a in ("inst", "scalars", "reach"):
            assert not sp.same(L[a], prev[a]), (k, a)
        assert not sp.same(L["pairs"], prev["pairs"]) or (L["tlasPairs"] == 0 and prev["tlasPairs"] == 0), (k, "pairs")
        assert sp.same(L["pairs"][:16 * blas_pairs], prev["pairs"][:16 * blas_pairs]) and sp.same(L["prims"], prev["prims"])
        lds[n] = L["tlasLds"]
        prev = L
    assert lds[il.N_SPLIT] == 0 and lds[il.N_SPLIT - 1] == 1 and lds[17] == 1 and lds[256] == 0 and il.N_SPLIT == 38
    assert il.WALK[0]["blas"][:2] == [1 - b for b in il.UPLOADED[:2]], "3 -> 5 re-points entries 0 and 1"
    assert set(il.WALK[6]["blas"]) == {0}
    h.close()


@pytest.mark.parametrize("n", [5, 2])
def test_the_behaviour_rays_meet_the_new_instances(n, host_api, oracle_api):
    """On the oracle, for each ray set of the behaviour test: at least one ray in four ends on an instance whose record is new in that step
    (il.BEHAVIOUR_NEW: the BLAS or the matrices differ from the list before at that index, or the index is new)."""
    h = host_api.HostScene()
    before = {5: 3, 2: 5}[n]
    Ts0, Ts = il.behaviour_transforms(h, before), il.behaviour_transforms(h, n)
    new = [i for i in range(n) if i >= before or il.BEHAVIOUR_LISTS[n][i] != il.BEHAVIOUR_LISTS[before][i] or not np.array_equal(Ts[i], Ts0[i])]
    assert new == il.BEHAVIOUR_NEW[n], "5 keeps instance 2 of the 3"
    o = oracle_api.OracleScene()
    il.list_scene(o, il.BEHAVIOUR_LISTS[n], il.behaviour_transforms(o, n))
    O, D = il.behaviour_rays(Ts, new, 50 + n)
    assert len(O) == il.BEHAVIOUR_RAYS
    ref, on = il.hits_on(o, O, D, new)
    assert 4 * int(on.sum()) >= len(O), "%d of %d rays end on a new instance" % (on.sum(), len(O))
    assert (ref["obj"] == -1).any() or (~on).any()
    h.close(), o.close()


def test_list_scene_restates_triangles_scene(host_api):
    a, b = host_api.HostScene(), host_api.HostScene()
    Ts = ir.grid_transforms(a, 5)
    ir.triangles_scene(a, Ts)
    il.list_scene(b, [0, 1, 0, 1, 0], Ts)
    La, Lb = host_api.layout(a.describe()), host_api.layout(b.describe())
    for arr, _ in host_api.LAYOUT_ARRAYS:
        assert sp.same(La[arr], Lb[arr]), arr
    a.close(), b.close()


@pytest.mark.parametrize("k", [2, 3, 7], ids=lambda k: "n%d" % il.WALK[k]["n"])
def test_host_mirror_describes_the_list_the_test_assembles(k, host_api):
    """Scene::SetInstanceList (what a caller does before CommitInstanceList) leaves the description the tests assemble by hand on
    triangles_desc.Desc: the records, the boxes of fresh instances, tlas::build over them -- for lists that keep the BLASes' order of
    first use.  Without a committed scene CommitInstanceList refuses; a list edit needs a TLAS and a mesh the build gave a bvh."""
    h = _uploaded(host_api)
    d = td.Desc(host_api, h)
    st = il.WALK[k]
    assert st["blas"][:2] == [0, 1]
    Ts = il.walk_transforms(h, k)
    il.set_list(d, ir.records(host_api, st["blas"], Ts))  # a fresh bvhInstance's box: what the mirror's new instances hold
    h.set_instance_list([(st["blas"][i], Ts[i]) for i in range(st["n"])])
    assert np.array_equal(h.tlas_dump(), d.tlas) and len(d.tlas) == 2 * st["n"]
    for i in (0, st["n"] - 1):
        x = h.instance_dump(i)
        assert x["blas"] == st["blas"][i] and sp.same(x["bounds"], d.bounds[i]) and sp.same(x["T"], Ts[i])
    Lh, Ld = host_api.layout(h.describe()), host_api.layout(d.desc())
    for arr, _ in host_api.LAYOUT_ARRAYS:
        assert sp.same(Lh[arr], Ld[arr]), arr
    with pytest.raises(RuntimeError, match="Commit"):
        h.commit_instance_list()
    with pytest.raises(RuntimeError, match="mesh"):
        h.set_instance_list([(5, Ts[0])])
    h.close()
    g = host_api.HostScene()
    __import__("importlib").import_module("ray-and-pathtracer_amd.scenes").mixed_small(g)
    with pytest.raises(RuntimeError, match="no TLAS"):
        g.set_instance_list([(0, Ts[0])])
    g.close()
