"""Restatements for rt_set_triangles (include/rt_amd.h), in NumPy: bvh::Refit over a node array, bvh::bounds, Triangle::update's normal, the
seeded deformations, the pieces of the updated description and the small scenes the CPU and GPU tests of the call share.  Nothing here
loads the library under test."""
import numpy as np

import instances_ref as ir

f32 = np.float32
BVH_NODE = np.dtype([("aabb_min", np.float32, 3), ("left_first", np.uint32), ("aabb_max", np.float32, 3), ("prim_count", np.uint32)])
TRIANGLE = np.dtype([("v0", np.float32, 3), ("v1", np.float32, 3), ("v2", np.float32, 3), ("N", np.float32, 3), ("obj_idx", np.int32), ("material", np.int32)])
SPHERE = np.dtype([("pos", np.float32, 3), ("r2", np.float32), ("invr", np.float32), ("r", np.float32), ("obj_idx", np.int32), ("material", np.int32)])
PLANE = np.dtype([("N", np.float32, 3), ("d", np.float32), ("obj_idx", np.int32), ("material", np.int32)])
BIG = f32(1e30)


def tmin(a, b):
    """fminf(float3, float3) of the reference: a < b ? a : b per component (b where they compare equal: the sign of a zero is b's)"""
    return np.where(a < b, a, b).astype(f32)


def tmax(a, b):
    return np.where(a > b, a, b).astype(f32)


# ---- Triangle::update (template/scene.h:238-246) ------------------------------------------------------------------------------------
def normals(v9):
    """N = normalize(cross(v1 - v0, v2 - v0)), every operation rounded to f32: cross as a.y * b.z - a.z * b.y ..., dot as (xx + yy) + zz,
    invLen = 1 / sqrtf(dot), N = v * invLen.  A degenerate triangle gets NaNs, as in the reference."""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3, 3)
    a, b = (v[:, 1] - v[:, 0]).astype(f32), (v[:, 2] - v[:, 0]).astype(f32)
    with np.errstate(all="ignore"):
        c = np.stack([f32(a[:, 1] * b[:, 2]) - f32(a[:, 2] * b[:, 1]), f32(a[:, 2] * b[:, 0]) - f32(a[:, 0] * b[:, 2]),
                      f32(a[:, 0] * b[:, 1]) - f32(a[:, 1] * b[:, 0])], -1).astype(f32)
        d = ((c[:, 0] * c[:, 0]).astype(f32) + (c[:, 1] * c[:, 1]).astype(f32)).astype(f32)
        d = (d + (c[:, 2] * c[:, 2]).astype(f32)).astype(f32)
        inv = (f32(1.0) / np.sqrt(d, dtype=f32)).astype(f32)
        return (c * inv[:, None]).astype(f32)


def triangles(old, v9, N=None):
    """the records sent to rt_set_triangles: 'old' (the uploaded ones: obj_idx and material stay) under the vertices v9 and their normals"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 9)
    t = np.array(old, dtype=TRIANGLE).copy()
    assert len(t) == len(v)
    t["v0"], t["v1"], t["v2"] = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    t["N"] = normals(v) if N is None else N
    return t


def v9_of(tris):
    return np.concatenate([tris["v0"], tris["v1"], tris["v2"]], -1).astype(f32)


# ---- the seeded deformations ---------------------------------------------------------------------------------------------------------
def twist(v9, rate=2.5):
    """a twist about y: every vertex turned about the y axis by rate * y radians (cos / sin in f64, rounded once)"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3).astype(np.float64)
    a = rate * v[:, 1]
    out = np.stack([v[:, 0] * np.cos(a) + v[:, 2] * np.sin(a), v[:, 1], -v[:, 0] * np.sin(a) + v[:, 2] * np.cos(a)], -1)
    return out.astype(f32).reshape(-1, 9)


def scale(v9, s=100.0):
    return (np.ascontiguousarray(v9, dtype=f32) * f32(s)).astype(f32).reshape(-1, 9)


def collapse(v9, axis=2, at=0.0):
    """every vertex onto the plane axis = at: flat boxes, zeros of either sign stay out (at is +0 or a number)"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3).copy()
    v[:, axis] = f32(at)
    return v.reshape(-1, 9)


DEFORMS = {"twist": twist, "scale": scale, "collapse": collapse}


# ---- bvh::Refit (bvh.cpp:556-594) and bvh::bounds (:48-49) -----------------------------------------------------------------------------
def _leaf_bounds(node, prim_idx, tris, spheres, planes):
    """bvh::UpdateNodeBounds (bvh.cpp:67-114): the primitives in prim_idx order, v0 v1 v2 each folded into lo then into hi"""
    lo, hi = np.full(3, BIG, f32), np.full(3, -BIG, f32)
    nt, ns = len(tris), len(spheres)
    for j in range(int(node["prim_count"])):
        p = int(prim_idx[int(node["left_first"]) + j])
        if p < nt:
            for k in ("v0", "v1", "v2"):
                lo = tmin(lo, tris[k][p])
            for k in ("v0", "v1", "v2"):
                hi = tmax(hi, tris[k][p])
        elif p < nt + ns:
            s = spheres[p - nt]
            lo, hi = tmin(lo, (s["pos"] - s["r"]).astype(f32)), tmax(hi, (s["pos"] + s["r"]).astype(f32))
        else:
            n = planes[p - nt - ns]["N"].astype(f32)
            inv = f32(1.0) / np.sqrt(f32(f32(f32(n[0] * n[0]) + f32(n[1] * n[1])) + f32(n[2] * n[2])), dtype=f32)
            n = (n * inv).astype(f32)
            if f32(f32(n[0] + n[1]) + n[2]) == 1 and (n[0] == 1 or n[1] == 1 or n[2] == 1):
                ax = 0 if n[0] == 1 else (1 if n[1] == 1 else 2)
                slo, shi = np.full(3, -BIG, f32), np.full(3, BIG, f32)
                slo[ax] = shi[ax] = 0
                lo, hi = tmin(lo, slo), tmax(hi, shi)
            else:
                return np.full(3, -BIG, f32), np.full(3, BIG, f32)
    return lo, hi


def refit(nodes, prim_idx, tris, spheres=None, planes=None):
    """bvh::Refit: the nodes (BVH_NODE array, nodes_used of them) with every box recomputed bottom-up from the primitives; node 1 does not
    exist.  An inner node is fminf(l, r) / fmaxf(l, r) of its children, a leaf its primitives' bounds."""
    out = np.array(nodes, dtype=BVH_NODE).copy()
    spheres = np.zeros(0, SPHERE) if spheres is None else spheres
    planes = np.zeros(0, PLANE) if planes is None else planes
    for i in range(len(out) - 1, -1, -1):
        if i == 1:
            continue
        nd = out[i]
        if nd["prim_count"] > 0:
            lo, hi = _leaf_bounds(nd, prim_idx, tris, spheres, planes)
        else:
            l, r = out[int(nd["left_first"])], out[int(nd["left_first"]) + 1]
            lo, hi = tmin(l["aabb_min"], r["aabb_min"]), tmax(l["aabb_max"], r["aabb_max"])
        out[i]["aabb_min"], out[i]["aabb_max"] = lo, hi
    return out


def local_box(nodes):
    """bvh::bounds: the empty box grown by node 0's two corners, as (min.xyz, max.xyz)"""
    lo, hi = np.full(3, BIG, f32), np.full(3, -BIG, f32)
    for c in (nodes[0]["aabb_min"], nodes[0]["aabb_max"]):
        lo, hi = tmin(lo, c), tmax(hi, c)
    return np.concatenate([lo, hi]).astype(f32)


# ---- the updated description's pieces ----------------------------------------------------------------------------------------------------
def updated_bounds(bounds, blas_of, blas, nodes, transforms):
    """every instance's box after the call: the instances of 'blas' get the box of a fresh instance under their transform (the refitted
    node 0's box as the local one), every other instance keeps the box it had"""
    out = np.array(bounds, dtype=f32).reshape(-1, 6).copy()
    local = local_box(nodes)
    for i, k in enumerate(blas_of):
        if int(k) == int(blas):
            out[i] = ir.fresh_bounds(local, transforms[i])
    return out


def blas_ranges(blas):
    """per BLAS of a description (a list of dicts with nodes and n_prims) its pair and primitive record ranges in the layout's arrays"""
    out, po, so = [], 0, 0
    for b in blas:
        out.append((po, po + len(b["nodes"]) // 2, so, so + int(b["n_prims"])))
        po, so = out[-1][1], out[-1][3]
    return out


# ---- meshes and scenes ----------------------------------------------------------------------------------------------------------------------
def random_mesh(n=300, seed=5, extent=0.35, size=0.12):
    """n seeded triangles in a box of half-width 'extent' around (0, 0.4, 0): leaves of several triangles under every split method"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, (n, 1, 3)) + np.array([0.0, 0.4, 0.0])
    return (c + rng.uniform(-size, size, (n, 3, 3))).astype(f32).reshape(n, 9)


def grid_mesh(nx=12, nz=12, seed=8, extent=0.35):
    """a height field over the xz square of half-width 'extent': 2 nx nz triangles that share edges and never overlap when looked at along
    y -- so that collapsing it onto a plane y = const leaves no two triangles on top of one another (no two hits at one t)"""
    rng = np.random.default_rng(seed)
    x, z = np.linspace(-extent, extent, nx + 1), np.linspace(-extent, extent, nz + 1)
    y = 0.4 + rng.uniform(-0.1, 0.1, (nx + 1, nz + 1))
    P = lambda i, j: (x[i], y[i, j], z[j])
    out = []
    for i in range(nx):
        for j in range(nz):
            out.append(P(i, j) + P(i + 1, j) + P(i + 1, j + 1))
            out.append(P(i, j) + P(i + 1, j + 1) + P(i, j + 1))
    return np.array(out, dtype=f32)


def sentinel_mesh(n=40, seed=6):
    """a mesh as a .tri file leaves it: real triangles, then the two sentinel triangles with every vertex at 999"""
    return np.concatenate([random_mesh(n, seed), np.full((2, 9), 999.0, f32)])


def sentinel_normals(v9):
    """the normals sent for a sentinel mesh: N = 0 for the two closing triangles (Triangle::Intersect rejects them), computed for the rest"""
    N = normals(v9)
    N[-2:] = 0
    return N


SMALL = np.array([[-0.2, 0, 0, 0.2, 0, 0, 0, 0.4, 0.05]], dtype=f32)  # the one-triangle BLAS 0 in front of a mesh under test


def mesh_scene(b, meshes, transforms, split=0):
    """raw meshes (a list of (n, 9) vertex arrays) under len(transforms) instances, instance i of mesh i mod len(meshes); a floor plane and a
    sphere tested by brute force, one light.  The same call builds the oracle's scene from deformed vertices."""
    b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
    mats = [b.diffuse(0.8, (1, 0.2, 0.2), 0.0, 1, 1), b.diffuse(0.8, (0.2, 0.2, 1), 0.0, 1, 1)]
    floor = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    ids = [b.mesh_raw(1 + k, mats[k & 1], np.ascontiguousarray(m, dtype=f32)) for k, m in enumerate(meshes)]
    b.plane(0, floor, (0, 1, 0), 0)
    b.sphere(7, mats[1], (1.8, 0.5, 2.0), 0.5)
    b.build_tlas(split, [(ids[i % len(ids)], T) for i, T in enumerate(transforms)])
    return dict(name="deform_mesh_scene", tlas=True)


def spread_transforms(scene, n):
    """n placements well apart, in front of the default camera: Translate * RotateY(0.3 i)"""
    return [scene.trs((f32(-1.5 + 1.0 * (i % 4)), f32(0.1 + 0.9 * (i // 4)), f32(3.0 + 0.2 * i)), f32(1.0), 0.0, f32(0.3 * i), 0.0) for i in range(n)]


def aimed_rays(n, seed, transforms, v9, spread=5.0, jitter=0.004):
    """n seeded rays: three in four aimed at the centroid of a triangle of the mesh v9 under one of the transforms (jittered by much less
    than a triangle's size: away from the edges, where a folded surface is met twice at nearly one distance), the rest anywhere"""
    rng = np.random.default_rng(seed)
    tri = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3, 3).astype(np.float64)
    tri = tri[np.abs(tri).max((1, 2)) < 900]  # (not the sentinels)
    O = (rng.uniform(-1, 1, (n, 3)) * spread + np.array([0.0, 1.5, 1.0])).astype(f32)
    D = rng.normal(size=(n, 3))
    k = 3 * n // 4
    T = np.stack([np.asarray(t, dtype=np.float64).reshape(4, 4) for t in transforms])[rng.integers(0, len(transforms), k)]
    p = tri[rng.integers(0, len(tri), k)].mean(1)
    world = np.einsum("kij,kj->ki", T[:, :3, :3], p) + T[:, :3, 3]
    D[:k] = world + rng.normal(size=(k, 3)) * jitter - O[:k]
    D = (D / np.maximum(np.sqrt((D ** 2).sum(1, keepdims=True)), 1e-20)).astype(f32)
    return O, D


# the behaviour tests' scene: mesh_scene over [SMALL, grid_mesh()] under this many spread_transforms (the odd instances are the mesh)
BEHAVIOUR_INSTANCES, BEHAVIOUR_RAYS = 4, 2048
# ... and its deformations: the height field is flattened along y, the direction in which none of its triangles lies above another
BEHAVIOUR_DEFORMS = {"twist": twist, "scale": scale, "collapse": lambda v9: collapse(v9, axis=1, at=0.4)}
