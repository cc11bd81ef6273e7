"""The oracle's walks (oracle/orc_bvh.h: bvh, bvhInstance, tlas; Scene::FindNearest / IsOccluded) held to a scan of all primitives:
rules A, B and the two occlusion rules of tests/scan_ref.py on the cases of tests/scan_cases.py, at scopes 1, 2, 3 and world level, under
every tmax set and after set_time.  Also here: the C loop of the scan against its numpy statement, the instance-ray helper against an f64
product, the three figures every ray set is held to (printed, then asserted), and the checker itself on spoiled answers."""
import numpy as np
import pytest

import scan_cases as sc
import scan_ref as sr

F32 = np.float32


def _small_prims(oa, nobox):
    rng = np.random.default_rng(5)
    v9 = rng.uniform(-1, 1, (6, 9)).astype(F32)
    v9[5] = [0, 0, 0.5, 1, 0, 0.5, 0, 1, 0.5]  # a box without thickness
    sph = np.array([[0.2, 0.1, -0.3, 0.4], [-0.6, 0.5, 0.2, 0.25]], F32)
    pla = np.array([[0, 1, 0, 0.3], [0.6, 0.0, 0.8, 0.1], [1, 0, 0, -0.2]], F32)
    return oa.ScanPrims(v9=v9, spheres=sph, planes=pla, ids=np.arange(22).reshape(11, 2), nobox=nobox)


@pytest.mark.parametrize("nobox", [False, True])
def test_c_loop_equals_the_numpy_statement(nobox, oracle_api):
    """orc_scan_nearest / orc_scan_occluded against tests/scan_ref.py's numpy loop over the one-call-per-case leaf entry points, bit for
    bit: every kind of primitive, an axis plane (Q1's slab at 0, here off the plane itself: d = 0.3) and a tilted one, with and without boxes"""
    P = _small_prims(oracle_api, nobox)
    rng = np.random.default_rng(9)
    n = 600
    O = rng.uniform(-2, 2, (n, 3)).astype(F32)
    D = (rng.normal(size=(n, 3)) * rng.choice([1.0, 1e-3, 37.0], (n, 1))).astype(F32)
    D[: n // 2] = (rng.uniform(-1, 1, (n // 2, 3)) - O[: n // 2]).astype(F32)
    assert sr.in_scope(O, D).all()
    for tmax in (np.full(n, 1e34, F32), rng.uniform(0.5, 4.0, n).astype(F32)):
        free = oracle_api.scan_nearest(P, O, D, tmax, sr.BVH_T_MIN, tmax)
        T = np.where(free["t_all"] < sr.NONE, free["t_all"], tmax).astype(F32)
        T[::3] = tmax[::3]
        got, ref = oracle_api.scan_nearest(P, O, D, tmax, sr.BVH_T_MIN, T), sr.scan_nearest_np(oracle_api, P, O, D, tmax, sr.BVH_T_MIN, T)
        assert (got["t_all"] < sr.NONE).mean() > 0.5
        if not nobox:
            assert (got["t_flt"] != got["t_all"]).any(), "the filter must matter somewhere, or nothing is compared"
        for k in ("t_all", "t_flt"):
            assert np.array_equal(sr.bits(got[k]), sr.bits(ref[k])), k
        assert np.array_equal(got["wit_t"], ref["wit_t"]) and (got["wit_t"] >= 0).any()
        go, ro = oracle_api.scan_occluded(P, O, D, tmax, sr.BVH_T_MIN), sr.scan_occluded_np(oracle_api, P, O, D, tmax, sr.BVH_T_MIN)
        assert np.array_equal(go["occ_all"], ro["occ_all"]) and np.array_equal(go["occ_flt"], ro["occ_flt"])
        box = oracle_api.slab(O, D, T, np.array([-0.5, -0.2, -0.1, 0.7, 0.9, 0.4], F32))
        assert np.array_equal(sr.bits(box), sr.bits(sr.slab_np(O, D, T, np.array([[-0.5, -0.2, -0.1]], F32), np.array([[0.7, 0.9, 0.4]], F32))))


def test_instance_ray_against_f64(oracle_api):
    """orc_leaf_instance_ray (TransformPosition / TransformVector of the inverse transform): each component within 4 ulp of the largest
    operand (the products and the translation) of the f64 value -- three f32 products and three f32 sums, half an ulp each at most"""
    o = oracle_api.OracleScene()
    rng = np.random.default_rng(3)
    for T in (o.trs((0.3, -0.2, 1.0), 2.5, 0.3, 0.7, 0.0), o.trs((-3.0, 0.25, 7.0), 0.8, 0.0, 2.3, 0.0), o.trs((100.0, 5.0, -40.0), 0.01, 1.0, 2.0, 3.0)):
        inv = np.zeros(16, F32)
        oracle_api.lib().orc_mat4_inverse(oracle_api._p(T), oracle_api._p(inv))
        O = (rng.normal(size=(500, 3)) * rng.choice([1.0, 30.0, 1e3], (500, 1))).astype(F32)
        D = (rng.normal(size=(500, 3)) * rng.choice([1.0, 1e-3, 37.0], (500, 1))).astype(F32)
        gO, gD = oracle_api.instance_ray(O, D, inv)
        M = inv.reshape(4, 4).astype(np.float64)
        for got, v, w in ((gO, O, 1.0), (gD, D, 0.0)):
            terms = np.concatenate([M[None, :3, :3] * v.astype(np.float64)[:, None, :], np.broadcast_to(M[None, :3, 3:] * w, (len(v), 3, 1))], 2)
            big = np.abs(terms).max(2).astype(F32)
            assert (np.abs(got.astype(np.float64) - terms.sum(2)) <= 4 * np.spacing(big).astype(np.float64)).all()
    o.close()


def _shares(oa, scenes, name):
    O, D, tms = sc.ray_sets(name, oa, scenes)
    o = oa.OracleScene()
    rec = sc.fill(name, o, scenes)
    parts, _ = sc.oracle_parts(oa, o, rec, 1)
    out = {k: sr.shares(oa, parts, O, D, tm) for k, tm in tms.items()}
    o.close()
    return out


@pytest.mark.parametrize("name", list(sc.CASES))
def test_caps(name, oracle_api, scenes):
    """how tight the rule is on each ray set, from the leaf functions and the slab test alone: undecided share, hit share, occluded share"""
    O, D, _ = sc.ray_sets(name, oracle_api, scenes)
    assert sr.in_scope(O, D).all() and len(O) <= 8192
    got = _shares(oracle_api, scenes, name)
    for k in sc.TMAX_SETS:
        s = got[k]
        print("%-16s %-8s undecided %.4f  hit %.3f  occluded %.3f" % (name, k, s["undecided"], s["hit"], s["occluded"]))
    for k in sc.TMAX_SETS:
        s = got[k]
        assert s["undecided"] <= sc.CAPS["undecided_max"], (k, s)
        assert s["hit"] >= sc.CAPS["hit_min"], (k, s)
        assert sc.CAPS["occluded"][0] <= s["occluded"] <= sc.CAPS["occluded"][1], (k, s)


def _count(v):
    return "%d of %d rays, first %s" % (int(v.sum()), len(v), np.flatnonzero(v)[:5].tolist())


def check_oracle(oa, o, rec, O, D, tmax, what, scopes=("world", 1, 2, 3)):
    """every query of the oracle scene o against the scan: world level, scope 1, scope 2 of every BLAS, scope 3 of every instance"""
    nearest = [("world", 0, lambda: o.find_nearest(O, D, tmax), lambda: o.is_occluded(O, D, tmax)["occluded"], O, D),
               (1, 0, lambda: o.scope_nearest(1, 0, O, D, tmax), lambda: o.scope_occluded(1, 0, O, D, tmax), O, D)]
    if rec.tlas:
        mob = rec.mesh_of_blas()
        for b in range(len(mob)):
            first = [i for i in range(len(rec.instances)) if o.instance_dump(i)["blas"] == b][0]
            bO, bD = oa.instance_ray(O, D, o.instance_dump(first)["invT"])
            keep = sr.in_scope(bO, bD)
            bO, bD, bt = bO[keep], bD[keep], None if tmax is None else tmax[keep]
            nearest.append((2, b, lambda b=b, bO=bO, bD=bD, bt=bt: o.scope_nearest(2, b, bO, bD, bt),
                            lambda b=b, bO=bO, bD=bD, bt=bt: o.scope_occluded(2, b, bO, bD, bt), bO, bD, bt))
        for i in range(len(rec.instances)):
            nearest.append((3, i, lambda i=i: o.scope_nearest(3, i, O, D, tmax), lambda i=i: o.scope_occluded(3, i, O, D, tmax), O, D))
    else:
        nearest.append((2, 0, lambda: o.scope_nearest(2, 0, O, D, tmax), lambda: o.scope_occluded(2, 0, O, D, tmax), O, D))
    for q in nearest:
        if q[0] not in scopes:
            continue
        scope, index, near, occ, qO, qD = q[:6]
        qt = q[6] if len(q) > 6 else tmax
        parts, occ_parts = sc.oracle_parts(oa, o, rec, scope, index)
        A, B = sr.nearest_violations(oa, parts, qO, qD, qt, near(), rec.light_table() if scope == "world" else None)
        assert not A.any(), "%s, scope %s index %d: rule A (a hit no primitive gives): %s" % (what, scope, index, _count(A))
        assert not B.any(), "%s, scope %s index %d: rule B (a nearer primitive inside its own box): %s" % (what, scope, index, _count(B))
        inv, over = sr.occluded_violations(oa, occ_parts, qO, qD, qt, occ())
        assert not inv.any(), "%s, scope %s index %d: occluded with no occluder: %s" % (what, scope, index, _count(inv))
        assert not over.any(), "%s, scope %s index %d: an occluder inside its own box overlooked: %s" % (what, scope, index, _count(over))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_oracle_obeys_the_scan(name, oracle_api, scenes):
    """every scope under every tmax set; the three large scenes keep scopes 2 and 3 (a BLAS, an instance alone: the same primitives
    again) to the set with distances one ulp around the hit"""
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    o = oracle_api.OracleScene()
    rec = sc.fill(name, o, scenes)
    for k, tm in tms.items():
        check_oracle(oracle_api, o, rec, O, D, tm, "%s, tmax %s" % (name, k), ("world", 1) if name in sc.LARGE and k != "hit_ulp" else ("world", 1, 2, 3))
    o.close()


@pytest.mark.parametrize("t", sc.TIMES)
@pytest.mark.parametrize("name", [n for n in sc.SMALL if n not in ("two_prims",)])
def test_oracle_obeys_the_scan_after_set_time(name, t, oracle_api, scenes):
    """Scene::SetTime deforms the meshes and refits the scene's BVH (not a TLAS scene's BLASes, which it leaves stale: those stay out);
    the rays stay the undeformed scene's, the primitives are read after the deformation"""
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    o = oracle_api.OracleScene()
    rec = sc.fill(name, o, scenes)
    before = o.mesh_tris(0)[0].copy()
    o.set_time(t)
    assert not np.array_equal(before, o.mesh_tris(0)[0])
    for k in ("none", "hit_ulp"):
        check_oracle(oracle_api, o, rec, O, D, tms[k], "%s at time %s, tmax %s" % (name, t, k))
    o.close()


@pytest.mark.parametrize("name", ["mixed_small_s0", "moving", "deep_tree"])
def test_the_rule_catches_tampered_answers(name, oracle_api, scenes):
    """the checker itself: the oracle's scope-1 answers, spoiled four ways, break the rule on every ray where it can tell -- a t one ulp
    off (A), a hit turned into a miss (B, on every ray whose nearest primitive lies inside its own box), both occlusion flags flipped"""
    O, D, tms = sc.ray_sets(name, oracle_api, scenes)
    o = oracle_api.OracleScene()
    rec = sc.fill(name, o, scenes)
    parts, occ_parts = sc.oracle_parts(oracle_api, o, rec, 1)
    got = o.scope_nearest(1, 0, O, D)
    hit = got["obj"] != -1
    off = dict(got, t=np.where(hit, (sr.bits(got["t"]) + 1).view(F32), got["t"]))
    A, _ = sr.nearest_violations(oracle_api, parts, O, D, None, off)
    assert hit.mean() > 0.5 and (A[hit]).mean() > 0.99 and not A[~hit].any()
    miss = dict(got, t=np.full(len(O), 1e34, F32), obj=np.full(len(O), -1, np.int32))
    A, B = sr.nearest_violations(oracle_api, parts, O, D, None, miss)
    tm = np.full(len(O), 1e34, F32)
    inside = sr.scan_query(oracle_api, parts, O, D, tm, tm)["t_flt"] != sr.NONE
    assert not A.any() and np.array_equal(B, inside) and B[hit].mean() > 0.95 and not B[~hit].any()
    flag = o.scope_occluded(1, 0, O, D).astype(bool)
    s = sr.occluded_query(oracle_api, occ_parts, O, D, tm)
    inv, over = sr.occluded_violations(oracle_api, occ_parts, O, D, None, ~flag)
    assert np.array_equal(inv, ~flag & ~s["occ_all"]) and inv[~flag].mean() > 0.95 and np.array_equal(over, flag & s["occ_flt"]) and over[flag].mean() > 0.95
    o.close()
