"""The device's walks held to a scan of all primitives (tests/scan_ref.py: rules A, B and the two occlusion rules), read without the oracle's
walk in between: the answers of rt_intersect_scope / rt_occluded_scope at scopes 1 to 3, rt_intersect_batch / rt_occluded_batch and
rt_primary_hits go straight to the rule.  The primitives are the context's own records (rt_blas_array 'prims', rt_scene_array 'brute' and
'inst', the leaf boxes of rt_download_tlas); only the leaf functions and the slab test come from oracle/ (orc_scan_*, pinned by
tests/test_ref_leaf_cpu.py).  The rule fixes no visiting order, so it holds for the reference walk (counting on), the timed walks with
their clean slab forms, reach cull and TLAS copy in LDS (counting off), and the wide walks alike.  Cases and ray sets: tests/scan_cases.py
(their figures are held in tests/test_scan_cpu.py)."""
import numpy as np
import pytest

import instances_ref as ir
import scan_cases as sc
import scan_ref as sr
import support as sp
import triangles_ref as tr
import vertices_ref as vr

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = {"default": ({}, False), "counting": ({}, True), "tlas_in_global": ({"RT_TLAS_LDS": "0"}, False), "wide4": ({"RT_WIDE": "1"}, False),
         "wide8": ({"RT_WIDE8": "1"}, False), "binary": ({"RT_WIDE": "0"}, False)}
MODE_CASES = [(m, n) for n in sc.CASES for m in ("default", "counting")] + \
             [("tlas_in_global", n) for n in ("tlas_test2_BigB", "pretty_tlas_8", "two_prims", "moving")] + \
             [("wide4", n) for n in ("mixed_small_s0", "deep_tree", "deep_chain", "tlas_test2_BigB", "two_prims", "one_leaf")] + \
             [("wide8", n) for n in ("deep_tree", "deep_chain", "tlas_test2_BigB", "two_prims", "one_leaf")] + \
             [("binary", "deep_chain")]  # (no 8-wide layout with spheres or planes in the tree; binary: a scene BVH's any-hit walk is 4-wide by
                                         # default, and on the chain only the binary one goes deep enough to spill)


def _renderer(host_api, monkeypatch, scenes, name, env=None, w=16, h=8, device_build=False):
    sp.clean_env(monkeypatch, env)
    r = host_api.HostRenderer(w, h)
    if device_build:
        r.scene.device_build(r.ctx)
    rec = sc.fill(name, r.scene, scenes)
    r.commit()
    return r, rec


def device_parts(oa, r, rec, scope, index, blas_of, t_min=1e-6):
    """the parts (tests/scan_ref.py) of a query, from the arrays the context holds"""
    P = lambda a: sr.prims_from_records(oa, a)
    if not rec.tlas:
        part = dict(prims=P(r.blas_array(0, "prims")), t_min=sr.BVH_T_MIN)
        return [part], [part]
    if scope == 2:
        part = dict(prims=P(r.blas_array(index, "prims")), t_min=sr.BVH_T_MIN)
        return [part], [part]
    inst = np.asarray(r.scene_array("inst")).view(F32).reshape(-1, 32)
    assert len(inst) == len(blas_of)
    tl = r.download_tlas()
    leaves = tl[1:][tl[1:, 3] == 0] if len(tl) > 1 else tl
    box = {int(nd[7]): np.concatenate([nd[0:3], nd[4:7]]).view(F32) for nd in leaves}
    prims = {b: P(r.blas_array(b, "prims")) for b in set(blas_of)}
    parts = [dict(prims=prims[blas_of[i]], t_min=sr.BVH_T_MIN, inv_t=sr.mat16(inst[i, 0:12]), nrm_m=sr.mat16(inst[i, 12:24]),
                  bounds=None if scope == 3 else box[i]) for i in ([index] if scope == 3 else range(len(inst)))]
    if scope == "world":
        b = P(r.scene_array("brute"))
        b.nobox = True
        return [dict(prims=b, t_min=t_min)] + parts, parts
    return parts, parts


def _count(v):
    return "%d of %d rays, first %s" % (int(v.sum()), len(v), np.flatnonzero(v)[:5].tolist())


def check_device(oa, r, rec, O, D, tmax, what, blas_of=None, scopes=("world", 1, 2, 3), min_hits=0.2):
    """the context's queries against the scan; in a TLAS scene scope 2 of every BLAS and scope 3 of the first and the last instance"""
    blas_of = blas_of if blas_of is not None else ([rec.mesh_of_blas().index(m) for m, _ in rec.instances] if rec.tlas else [])
    queries = []
    for scope in scopes:
        if scope == "world":
            queries.append(("world", 0, O, D, tmax, lambda: r.find_nearest(O, D, tmax), lambda: r.is_occluded(O, D, tmax)))
        elif scope == 2 and rec.tlas:
            inst = np.asarray(r.scene_array("inst")).view(F32).reshape(-1, 32)
            for b in sorted(set(blas_of)):
                bO, bD = oa.instance_ray(O, D, sr.mat16(inst[blas_of.index(b), 0:12]))
                keep = sr.in_scope(bO, bD)
                queries.append((2, b, bO[keep], bD[keep], None if tmax is None else tmax[keep], None, None))
        elif scope == 3 and rec.tlas:
            for i in sorted({0, len(blas_of) - 1}):
                queries.append((3, i, O, D, tmax, None, None))
        elif scope in (1, 2):
            queries.append((scope, 0, O, D, tmax, None, None))
    for scope, index, qO, qD, qt, near, occ in queries:
        got = near() if near else r.scope_nearest(scope, index, qO, qD, qt)
        flag = occ() if occ else r.scope_occluded(scope, index, qO, qD, qt)
        parts, occ_parts = device_parts(oa, r, rec, scope, index, blas_of)
        A, B = sr.nearest_violations(oa, parts, qO, qD, qt, got, rec.light_table() if scope == "world" else None)
        where = "%s, scope %s index %d" % (what, scope, index)
        assert not A.any(), "%s: rule A (a hit no primitive gives): %s" % (where, _count(A))
        assert not B.any(), "%s: rule B (a nearer primitive inside its own box): %s" % (where, _count(B))
        inv, over = sr.occluded_violations(oa, occ_parts, qO, qD, qt, flag)
        assert not inv.any(), "%s: occluded with no occluder: %s" % (where, _count(inv))
        assert not over.any(), "%s: an occluder inside its own box overlooked: %s" % (where, _count(over))
        if scope in ("world", 1):
            assert (got["obj"] != -1).mean() >= min_hits and 0.05 <= flag.mean() <= 0.95, "%s: the rays must meet the scene, and miss it" % where


@pytest.mark.parametrize("mode,name", MODE_CASES)
def test_walks_obey_the_scan(mode, name, oracle_api, host_api, scenes, monkeypatch):
    """every query at every scope under every tmax set: the timed walks (default), the reference walk (counting on), the TLAS in global
    memory and the two wide walks; the three large scenes leave the constant tmax to the default knobs"""
    env, counting = MODES[mode]
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    r, rec = _renderer(host_api, monkeypatch, scenes, name, env)
    r.set_counting(counting)
    if mode in ("wide4", "wide8"):  # the layout the knob asks for exists, so the wide walk is the one that answers
        assert dict(zip(host_api.LAYOUT_SCALARS, r.scene_array("scalars")))["wideOK" if mode == "wide4" else "wide8OK"] == 1
    for k in (sc.TMAX_SETS if mode == "default" or name not in sc.LARGE else ("none", "hit_ulp")):
        check_device(oracle_api, r, rec, O, D, tms[k], "%s, %s, tmax %s" % (name, mode, k))
    r.close()


@pytest.mark.parametrize("name", ["mixed_small_s0", "tlas_test2_BigB", "moving"])
def test_primary_hits_obey_the_scan(name, oracle_api, host_api, scenes, monkeypatch):
    """rt_primary_hits at 64 x 48 (it reports t and obj): the camera's in-scope rays, at both t_min values the renderer uses"""
    r, rec = _renderer(host_api, monkeypatch, scenes, name, w=64, h=48)
    cam = ((0.1, 1.0, -2.5), (-1.2, 2.0, -0.6), (1.5, 1.9, -0.5), (-1.3, 0.0, -0.4))
    r.set_camera(*cam)
    o = oracle_api.OracleScene()  # ray generation only (Camera::GetPrimaryRay is pinned by tests/test_ref_leaf_cpu.py and tests/test_gpu_ref_leaf.py)
    sc.fill(name, o, scenes)
    orr = oracle_api.OracleRenderer(o, 64, 48)
    orr.set_camera(*cam)
    O, D = orr.primary_rays()
    keep = sr.in_scope(O, D)
    assert keep.mean() > 0.9
    blas_of = [rec.mesh_of_blas().index(m) for m, _ in rec.instances] if rec.tlas else []
    for t_min in (1e-6, 0.001):
        obj, t = r.primary_hits(t_min)
        got = dict(obj=obj.reshape(-1)[keep], t=t.reshape(-1)[keep])
        parts, _ = device_parts(oracle_api, r, rec, "world", 0, blas_of, t_min)
        A, B = sr.nearest_violations(oracle_api, parts, O[keep], D[keep], None, got, rec.light_table(), t_min)
        assert not A.any(), "t_min %g: rule A: %s" % (t_min, _count(A))
        assert not B.any(), "t_min %g: rule B: %s" % (t_min, _count(B))
        assert (got["obj"] != -1).mean() > 0.3
    orr.close(), o.close(), r.close()


@pytest.mark.parametrize("name", ["mixed_small_s0", "mixed_small_s1", "mixed_small_s2", "mixed_small_s3", "two_prims", "moving"])
@pytest.mark.parametrize("counting", [False, True], ids=["timed", "reference"])
def test_device_built_trees_obey_the_scan(name, counting, oracle_api, host_api, scenes, monkeypatch):
    """the trees rt_build_bvh_split makes on the device, by each split method"""
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    r, rec = _renderer(host_api, monkeypatch, scenes, name, device_build=True)
    r.set_counting(counting)
    check_device(oracle_api, r, rec, O, D, tms["hit_ulp"], "%s, built on the device" % name)
    r.close()


@pytest.mark.parametrize("name", ["mixed_small_s0", "mixed_small_s3", "deep_tree", "one_leaf"])
@pytest.mark.parametrize("t", sc.TIMES)
def test_after_set_time(name, t, oracle_api, host_api, scenes, monkeypatch):
    """rt_set_time deforms and refits on the device; the primitives are the records it left"""
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    r, rec = _renderer(host_api, monkeypatch, scenes, name)
    before = r.blas_array(0, "prims")
    r.set_time(t)
    assert not sp.same(before, r.blas_array(0, "prims"))
    for counting in (False, True):
        r.set_counting(counting)
        check_device(oracle_api, r, rec, O, D, tms["hit_ulp"], "%s at time %s, counting %s" % (name, t, counting), min_hits=0.05)
    r.close()


@pytest.mark.parametrize("name,k", [("mixed_small_s0", 0), ("moving", 0), ("moving", 1), ("two_prims", 0)])
@pytest.mark.parametrize("how", ["triangles", "vertices"])
def test_after_a_twist(name, k, how, oracle_api, host_api, scenes, monkeypatch):
    """rt_set_triangles / rt_set_vertices with a twist of BLAS k's triangles; the primitives are read back from rt_blas_array"""
    import triangles_desc as td
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    r, rec = _renderer(host_api, monkeypatch, scenes, name)
    old = td.Desc(host_api, r.scene).tris[k]
    before = r.blas_array(k, "prims")
    if how == "triangles":
        assert r.set_triangles(k, tr.triangles(old, tr.twist(tr.v9_of(old), 1.5))) == 0
    else:
        xyz, idx = vr.weld(tr.v9_of(old))
        assert r.set_mesh_indices(k, idx, len(xyz)) == 0
        assert r.set_vertices(k, vr.deformed(xyz, "twist")) == 0
    assert not sp.same(before, r.blas_array(k, "prims"))
    for counting in (False, True):
        r.set_counting(counting)
        check_device(oracle_api, r, rec, O, D, tms["hit_ulp"], "%s, BLAS %d twisted by %s, counting %s" % (name, k, how, counting), min_hits=0.05)
    r.close()


@pytest.mark.parametrize("env", [{}, {"RT_TLAS_LDS": "0"}], ids=sp.env_id)
def test_after_moving_instances(env, oracle_api, host_api, scenes, monkeypatch):
    """rt_set_instances, then rt_set_instance_list with one instance more and two re-pointed; the records are read back from rt_scene_array"""
    O, D, tms = sc.ray_sets("moving", oracle_api, scenes)
    r, rec = _renderer(host_api, monkeypatch, scenes, "moving", env)
    s = r.scene
    before = r.scene_array("inst")
    assert r.set_instances(1, ir.records(host_api, [1, 0], [s.trs((0.1, 0.9, 3.2), 1.3, 0.2, 2.6, 0.0), s.trs((1.6, 0.4, 4.4), 1.2, 0.0, 0.3, 0.1)])) == 0
    assert not sp.same(before, r.scene_array("inst"))
    for counting in (False, True):
        r.set_counting(counting)
        check_device(oracle_api, r, rec, O, D, tms["hit_ulp"], "moved, counting %s" % counting, blas_of=[0, 1, 0], min_hits=0.05)
    blas_of = [1, 1, 0, 0]
    Ts = [s.trs((-1.0, 0.4, 3.1), 0.9, 0.0, 0.7, 0.0), s.trs((0.5, 0.5, 3.4), 0.7, 0.3, 1.1, 0.0), s.trs((1.9, 0.8, 4.0), 1.0, 0.0, 2.0, 0.5),
          s.trs((0.0, 1.6, 5.0), 2.0, 0.5, 0.1, 0.2)]
    assert r.set_instance_list(ir.records(host_api, blas_of, Ts)) == 0
    assert len(np.asarray(r.scene_array("inst")).reshape(-1, 32)) == 4
    for counting in (False, True):
        r.set_counting(counting)
        check_device(oracle_api, r, rec, O, D, tms["hit_ulp"], "new list, counting %s" % counting, blas_of=blas_of, min_hits=0.05)
    r.close()
