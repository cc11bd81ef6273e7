"""A second statement of FindNearest / IsOccluded that knows no tree, no stack and no visiting order: every primitive the query can reach
is tested with its leaf function (oracle/oracle_capi.cpp orc_leaf_* bodies, pinned to the reference's compiled code by
tests/test_ref_leaf_cpu.py), and the only box fact used is the one a tree may use.  Whatever walks a BVH over these primitives -- the
oracle's restatement of bvh.cpp / tlas.cpp, or a device kernel in any order, width or with any extra cull -- must obey it.

For a ray with answer T (a hit's t; for a miss the ray.t the walk ran with, i.e. the caller's tmax, which is what '1e30' stands for when
no tmax is given), over all primitives p the query can reach:

  A (nothing invented)   a hit's t bits are the leaf function's t bits for some primitive (leaf called with tmax = the caller's, t_min =
                         the level's); obj, mat and normal bits are those of ONE such primitive.  Ties between primitives are allowed.
                         A miss needs no witness.
  B (nothing overlooked) no primitive has leaf t < T while the reference's slab test (bvh::IntersectAABB, bvh.cpp:819-828 as
                         oracle/orc_bvh.h:21-30 states it) of that primitive's OWN box passes with ray.t = T.  Own boxes: a triangle's
                         min / max of its vertices, a sphere's pos -/+ r in f32, a plane's slab at coordinate 0 (orc_bvh.h:89-105, Q1;
                         any other plane: the +-1e30 box).
  occlusion              flag set   => some primitive's IsOccluding is true;
                         flag clear => no primitive is occluding while its own box passes the slab test with ray.t = tmax.
                         (Triangle::IsOccluding where the reference is undefined: the oracle's 'false', as ref_leaf.npz marks it.)

Why B is sound for any correct walk.  Node boxes are nested: a leaf's box is the componentwise min / max over its primitives' own boxes
and an inner node's the min / max of its children's (UpdateNodeBounds, Refit), so every ancestor's bmin <= own bmin and bmax >= own bmax
per component, exactly, in f32.  The slab arithmetic is monotone: (b - O) * rD rounds monotonically in b, so widening a box can only lower
the entry tmin = max of mins and raise the exit tmax = min of maxes; 'tmax >= tmin && tmin < ray.t && tmax > 0' that holds for the own
box therefore holds for every ancestor at the same ray.t, and raising ray.t keeps it.  A walk's ray.t never drops below its final answer
T.  So a ray that passes a primitive's own box with ray.t = T passes every ancestor whenever the walk could test it: the walk must reach
the leaf, and the leaf function with ray.t >= T > t accepts the hit.  Rays are restricted to finite origins and finite non-zero direction
components, where no slab product is NaN and the argument holds.

At world level in a TLAS scene an instance's primitives are scanned with the ray taken into the instance's space (orc_leaf_instance_ray:
TransformPosition / TransformVector, no normalisation, so t keeps its meaning) and filtered by their own box AND by the instance's world
bounds with the world ray (the TLAS leaf box; TLAS inner boxes are unions of these).  Lights come first and are not gated by ray.t (Q6):
the LAST area light the ray meets sets ray.t for everything after it, which is Scene::FindNearest's own order (template/scene.h:1248-1267)
and no tree's; the scan takes that value as the caller's tmax.  Brute-force spheres and planes are always tested and have no box.

'Undecided' measures how tight the rule is on a ray, with no walk involved.  The unfiltered scan's nearest t always satisfies both rules;
the ray is undecided when the next answer A allows (the next farther leaf t, or a miss) satisfies B too, i.e. no primitive at the nearest
t passes its own box with ray.t = that next answer -- the nearest t of the unfiltered scan is then not the nearest t among the primitives
passing B's filter, and the rules accept both.  For occlusion: an occluder exists, but only outside its box.

A part of a query is a dict(prims=ScanPrims, t_min=float, inv_t=None or 16 floats, nrm_m=None or 16 floats, bounds=None or 6 floats)."""
import numpy as np

F32 = np.float32
NONE = F32(1e30)
BVH_T_MIN = 0.0001  # bvh::BIntersect / BIsOccluded (bvh.cpp:608, :765)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def in_scope(O, D):
    """finite origins, finite non-zero direction components"""
    return np.isfinite(O).all(1) & np.isfinite(D).all(1) & (D != 0).all(1)


# ---- numpy statement of the box test and of the scan (held to the C loop bit for bit on a small case) ------------------------------------
def slab_np(O, D, t, bmin, bmax):
    """IntersectAABB (orc_bvh.h:21-30) in f32, one rounding per operation, for in-scope rays: tmin, or 1e30"""
    O, D = np.asarray(O, F32), np.asarray(D, F32)
    rD = (F32(1) / D).astype(F32)
    lo = hi = None
    with np.errstate(all="ignore"):
        for a in range(3):
            t1 = ((bmin[..., a] - O[:, a]).astype(F32) * rD[:, a]).astype(F32)
            t2 = ((bmax[..., a] - O[:, a]).astype(F32) * rD[:, a]).astype(F32)
            mn, mx = np.minimum(t1, t2), np.maximum(t1, t2)
            lo, hi = (mn, mx) if lo is None else (np.maximum(lo, mn), np.minimum(hi, mx))
    ok = (hi >= lo) & (lo < np.asarray(t, F32)) & (hi > 0)
    return np.where(ok, lo, NONE).astype(F32)


def own_boxes(prims):
    """(n, 3) bmin, bmax of every primitive, in ScanPrims order"""
    v = prims.v9.reshape(-1, 3, 3)
    lo, hi = [v.min(1)], [v.max(1)]
    s = prims.spheres
    lo.append((s[:, :3] - s[:, 3:4]).astype(F32)), hi.append((s[:, :3] + s[:, 3:4]).astype(F32))
    for q in prims.planes:
        # Q1: normalize(N) is exactly +X, +Y or +Z only for a normal with one positive component and two zeros whose length rounds to 1;
        # this statement takes the unit axes themselves and calls every other plane unbounded (the C loop normalises as the oracle does)
        l, h = np.full(3, -1e30, F32), np.full(3, 1e30, F32)
        axis = [a for a in range(3) if q[a] == 1 and q[(a + 1) % 3] == 0 and q[(a + 2) % 3] == 0]
        if axis:
            l[axis[0]] = h[axis[0]] = 0
        lo.append(l[None]), hi.append(h[None])
    return np.concatenate(lo).astype(F32), np.concatenate(hi).astype(F32)


def _leaf_np(oa, prims, p, O, D, tmax, t_min, occluding=False):
    """primitive p's leaf function on every ray, through the one-call-per-case leaf entry points: (hit, t) or occluding"""
    import ctypes as C
    L, n = oa.lib(), len(O)
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    tm, tn = np.ascontiguousarray(tmax, F32), np.full(n, t_min, F32)
    hit, t, nrm, occ = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros(n, np.int32)
    nt, ns = len(prims.v9), len(prims.spheres)
    if p < nt:
        v = np.ascontiguousarray(np.tile(prims.v9[p], (n, 1)))
        if occluding:
            L.orc_leaf_tri_occluding(n, P(v), P(O), P(D), P(tm), P(tn), P(occ))
        else:
            L.orc_leaf_tri_intersect(n, P(v), P(O), P(D), P(tm), P(tn), P(hit), P(t), P(nrm))
    elif p < nt + ns:
        s = prims.spheres[p - nt]
        pos, rad = np.ascontiguousarray(np.tile(s[:3], (n, 1))), np.full(n, s[3], F32)
        if occluding:
            L.orc_leaf_sphere_occluding(n, P(pos), P(rad), P(O), P(D), P(tm), P(tn), P(occ))
        else:
            L.orc_leaf_sphere_intersect(n, P(pos), P(rad), P(O), P(D), P(tm), P(tn), P(hit), P(t), P(nrm))
    else:
        q = prims.planes[p - nt - ns]
        N, d = np.ascontiguousarray(np.tile(q[:3], (n, 1))), np.full(n, q[3], F32)
        if occluding:
            L.orc_leaf_plane_occluding(n, P(N), P(d), P(O), P(D), P(tm), P(tn), P(occ))
        else:
            L.orc_leaf_plane_intersect(n, P(N), P(d), P(O), P(D), P(tm), P(tn), P(hit), P(t), P(nrm))
    return occ != 0 if occluding else (t < tm, t)


def scan_nearest_np(oa, prims, O, D, tmax, t_min, T):
    """the loop of orc_scan_nearest in numpy, one primitive at a time: t_all, t_flt, wit_t"""
    O, D = np.ascontiguousarray(O, F32), np.ascontiguousarray(D, F32)
    n = len(O)
    lo, hi = own_boxes(prims)
    t_all, t_flt, wit = np.full(n, NONE, F32), np.full(n, NONE, F32), np.full(n, -1, np.int32)
    for p in range(prims.n):
        hit, t = _leaf_np(oa, prims, p, O, D, tmax, t_min)
        box = np.ones(n, bool) if prims.nobox and p >= len(prims.v9) else slab_np(O, D, T, lo[p][None], hi[p][None]) != NONE
        t_all = np.where(hit & (t < t_all), t, t_all)
        t_flt = np.where(hit & box & (t < t_flt), t, t_flt)
        wit = np.where(hit & (bits(t) == bits(T)) & (wit < 0), p, wit)
    return dict(t_all=t_all, t_flt=t_flt, wit_t=wit)


def scan_occluded_np(oa, prims, O, D, tmax, t_min):
    O, D = np.ascontiguousarray(O, F32), np.ascontiguousarray(D, F32)
    n = len(O)
    lo, hi = own_boxes(prims)
    occ_all, occ_flt = np.zeros(n, bool), np.zeros(n, bool)
    for p in range(prims.n):
        occ = _leaf_np(oa, prims, p, O, D, tmax, t_min, occluding=True)
        box = np.ones(n, bool) if prims.nobox and p >= len(prims.v9) else slab_np(O, D, tmax, lo[p][None], hi[p][None]) != NONE
        occ_all |= occ
        occ_flt |= occ & box
    return dict(occ_all=occ_all, occ_flt=occ_flt)


# ---- a query: parts, and for Scene::FindNearest the lights in front ----------------------------------------------------------------------
def light_stage(oa, lights, O, D, tmax, t_min):
    """Scene::FindNearest's light loop (template/scene.h:1251-1252) through orc_leaf_area_intersect: AreaLight::Intersect does not look at
    ray.t (Q6), so the LAST light the ray meets sets it.  lights: (k, 12) as orc_leaf_area_intersect takes them plus their objIdx list.
    Returns (ray.t after the loop, met, obj, normal)."""
    import ctypes as C
    n = len(O)
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    t_now = np.ascontiguousarray(tmax, F32).copy()
    met, obj, nrm = np.zeros(n, bool), np.full(n, -1, np.int32), np.zeros((n, 3), F32)
    for rec, idx in zip(*lights):
        L12 = np.ascontiguousarray(np.tile(np.asarray(rec, F32), (n, 1)))
        hit, t, nn = np.zeros(n, np.int32), np.zeros(n, F32), np.zeros((n, 3), F32)
        sentinel = np.full(n, np.nan, F32)  # the leaf entry point reports through ray.t; a NaN tmax tells a meeting from none
        oa.lib().orc_leaf_area_intersect(n, P(L12), P(O), P(D), P(sentinel), P(np.full(n, t_min, F32)), P(hit), P(t), P(nn))
        m = ~np.isnan(t)
        t_now = np.where(m, t, t_now).astype(F32)
        met |= m
        obj = np.where(m, idx, obj).astype(np.int32)
        nrm = np.where(m[:, None], nn, nrm).astype(F32)
    return t_now, met, obj, nrm


def _part_rays(oa, part, O, D):
    return oa.instance_ray(O, D, part["inv_t"]) if part.get("inv_t") is not None else (O, D)


def _gate(oa, part, O, D, T):
    return None if part.get("bounds") is None else (oa.slab(O, D, T, np.asarray(part["bounds"], F32)) != NONE).astype(np.uint8)


def scan_query(oa, parts, O, D, tmax, T, got=None):
    """orc_scan_nearest over every part, combined: t_all, t_flt (minima), wit_t, wit_full (any)"""
    n = len(O)
    out = dict(t_all=np.full(n, NONE, F32), t_flt=np.full(n, NONE, F32), wit_t=np.zeros(n, bool), wit_full=np.zeros(n, bool))
    cand = []
    for part in parts:
        pO, pD = _part_rays(oa, part, O, D)
        s = oa.scan_nearest(part["prims"], pO, pD, tmax, part["t_min"], T, _gate(oa, part, O, D, T), got, part.get("nrm_m"))
        out["t_all"], out["t_flt"] = np.minimum(out["t_all"], s["t_all"]), np.minimum(out["t_flt"], s["t_flt"])
        out["wit_t"] |= s["wit_t"] >= 0
        out["wit_full"] |= s["wit_full"] >= 0
        cand += [s["t_all"], s["t_next"]]
    out["t_next"] = np.min([np.where(c > out["t_all"], c, NONE) for c in cand], 0).astype(F32)  # the nearest t farther than t_all
    return out


def nearest_violations(oa, parts, O, D, tmax, got, lights=None, t_min=1e-6):
    """(A, B): a bool per ray, set where the answer 'got' (dict t, obj, mat, normal) breaks the rule.  lights: Scene::FindNearest's
    light loop goes first, at the caller's t_min."""
    O, D = np.ascontiguousarray(O, F32).reshape(-1, 3), np.ascontiguousarray(D, F32).reshape(-1, 3)
    assert in_scope(O, D).all()
    n = len(O)
    tm = np.full(n, 1e34, F32) if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F32), (n,)))
    by_light = overlooked_light = np.zeros(n, bool)
    if lights is not None and len(lights[0]):
        tm, met, lobj, lnrm = light_stage(oa, lights, O, D, tm, t_min)
        by_light = met & (bits(got["t"]) == bits(tm)) & (got["obj"] == lobj)
        if "normal" in got:
            by_light &= (bits(got["normal"]) == bits(lnrm)).all(1)
        overlooked_light = met & (got["obj"] == -1)
    hit = got["obj"] != -1
    T = np.where(hit, got["t"], tm).astype(F32)
    s = scan_query(oa, parts, O, D, tm, T, got)
    A = hit & ~s["wit_full"] & ~by_light
    B = ((s["t_flt"] != NONE) & (s["t_flt"] < T)) | overlooked_light  # (NONE: no primitive inside its box was hit at all)
    return A, B


def occluded_query(oa, parts, O, D, tmax):
    n = len(O)
    out = dict(occ_all=np.zeros(n, bool), occ_flt=np.zeros(n, bool))
    for part in parts:
        pO, pD = _part_rays(oa, part, O, D)
        s = oa.scan_occluded(part["prims"], pO, pD, tmax, part["t_min"], _gate(oa, part, O, D, tmax))
        out["occ_all"] |= s["occ_all"]
        out["occ_flt"] |= s["occ_flt"]
    return out


def occluded_violations(oa, parts, O, D, tmax, flag):
    """(invented, overlooked): flag set with no occluder at all; flag clear with an occluder inside its own box"""
    O, D = np.ascontiguousarray(O, F32).reshape(-1, 3), np.ascontiguousarray(D, F32).reshape(-1, 3)
    assert in_scope(O, D).all()
    tm = np.full(len(O), 1e34, F32) if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F32), (len(O),)))
    s = occluded_query(oa, parts, O, D, tm)
    flag = np.asarray(flag).astype(bool)
    return flag & ~s["occ_all"], ~flag & s["occ_flt"]


def shares(oa, parts, O, D, tmax, occ_parts=None):
    """dict(undecided, hit, occluded): the three figures a ray set is held to; leaf functions and slab test alone"""
    O, D = np.ascontiguousarray(O, F32).reshape(-1, 3), np.ascontiguousarray(D, F32).reshape(-1, 3)
    n = len(O)
    tm = np.full(n, 1e34, F32) if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F32), (n,)))
    first = scan_query(oa, parts, O, D, tm, tm)
    t_all = first["t_all"]
    hit = t_all < np.minimum(tm, NONE)
    T = np.where(first["t_next"] < NONE, first["t_next"], tm).astype(F32)  # the next answer A would allow: the next leaf t, or a miss
    und_near = hit & (bits(scan_query(oa, parts, O, D, tm, T)["t_flt"]) != bits(t_all))
    o = occluded_query(oa, parts if occ_parts is None else occ_parts, O, D, tm)
    und = und_near | (o["occ_all"] & ~o["occ_flt"])
    return dict(undecided=float(und.mean()), hit=float(hit.mean()), occluded=float(o["occ_all"].mean()))


# ---- primitives from what a scene holds ---------------------------------------------------------------------------------------------------
def prims_from_records(oa, rec):
    """ScanPrims of device primitive records (rt_blas_array 'prims': 16 words each, {v0, N.x} {v1, N.y} {v2, N.z} {d, obj, mat, kind};
    sphere {pos, r2} {invr, r}; plane {N, d}).  A zero record (a padded slot) is a triangle of three equal points, which nothing hits."""
    r = np.ascontiguousarray(rec, F32).reshape(-1, 16)
    w = r.view(np.uint32)
    kind = w[:, 15] & 3
    ids = w[:, 13:15].view(np.int32)
    t, s, q = r[kind == 0], r[kind == 1], r[kind == 2]
    return oa.ScanPrims(v9=t[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], tri_n=t[:, [3, 7, 11]], spheres=np.concatenate([s[:, :3], s[:, 5:6]], 1),
                        planes=q[:, :4], ids=np.concatenate([ids[kind == 0], ids[kind == 1], ids[kind == 2]]))


def mat16(rows12):
    """a 3 x 4 row-major block (12 words) as the 16 cells of a mat4"""
    return np.concatenate([np.asarray(rows12, F32).reshape(12), np.array([0, 0, 0, 1], F32)])
