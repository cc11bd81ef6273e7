"""Scenes and seeded ray sets for the scan rule (tests/scan_ref.py), shared by tests/test_scan_cpu.py and tests/test_gpu_scan.py.

A case is a scene filled through the builder protocol (a Recorder keeps what the scan needs and the builders do not give back: spheres,
planes, lights, the material of each mesh, the instance list) and one ray set of at most 8,192 in-scope rays (finite origins, finite
non-zero direction components), used under three tmax sets: none, a constant, and the nearest leaf distance +-1 ulp on two rays of every four (tmax_sets).  The ray set
mixes, seeded: random rays through the content box; rays aimed at vertices, edge midpoints and centroids from 0.5, 3, 30 and 1e3 units with
unit and non-unit directions (x1e-3, x37); the same with +-1 to 3 ulp nudges of the direction; rays that start on a primitive's surface.

Figures of each set (tests/test_scan_cpu.py::test_caps prints and asserts them: undecided <= 5 %, hit >= 0.5, occluded in 0.1 .. 0.9),
scope 1, as 'undecided / hit / occluded' per tmax set (none | constant | hit +-1 ulp):

case             none                    |  const                   |  hit_ulp
mixed_small_s0   0.0127 / 0.842 / 0.842  |  0.0123 / 0.835 / 0.835  |  0.0299 / 0.603 / 0.603
mixed_small_s1   0.0144 / 0.847 / 0.847  |  0.0144 / 0.842 / 0.842  |  0.0273 / 0.609 / 0.609
mixed_small_s2   0.0140 / 0.848 / 0.848  |  0.0140 / 0.841 / 0.841  |  0.0303 / 0.611 / 0.611
mixed_small_s3   0.0160 / 0.849 / 0.849  |  0.0160 / 0.843 / 0.843  |  0.0289 / 0.613 / 0.613
tlas_test2_BigB  0.0044 / 0.836 / 0.836  |  0.0034 / 0.712 / 0.712  |  0.0186 / 0.614 / 0.614
pretty_tlas_1    0.0010 / 0.748 / 0.748  |  0.0010 / 0.623 / 0.623  |  0.0010 / 0.562 / 0.562
pretty_tlas_8    0.0010 / 0.763 / 0.763  |  0.0000 / 0.643 / 0.643  |  0.0010 / 0.569 / 0.569
deep_tree        0.0078 / 0.731 / 0.731  |  0.0066 / 0.602 / 0.602  |  0.0322 / 0.638 / 0.638
deep_chain       0.0000 / 0.821 / 0.821  |  0.0000 / 0.696 / 0.696  |  0.0000 / 0.618 / 0.618
two_prims        0.0039 / 0.706 / 0.706  |  0.0029 / 0.599 / 0.599  |  0.0049 / 0.524 / 0.524
one_leaf         0.0015 / 0.681 / 0.681  |  0.0010 / 0.564 / 0.564  |  0.0015 / 0.504 / 0.504
moving           0.0034 / 0.725 / 0.725  |  0.0029 / 0.604 / 0.604  |  0.0083 / 0.536 / 0.536
"""
import numpy as np

F32 = np.float32
CAPS = dict(undecided_max=0.05, hit_min=0.5, occluded=(0.1, 0.9))
TMAX_SETS = ("none", "const", "hit_ulp")
TIMES = (0.7, 3.1)  # set_time


class Recorder:
    """forwards the builder protocol to a builder and keeps what the scan needs"""

    def __init__(self, b):
        self.b = b
        self.spheres, self.planes, self.lights, self.light_idx, self.mesh_mat, self.instances, self.tlas, self.split = [], [], [], [], [], [], False, 0

    def __getattr__(self, k):
        return getattr(self.b, k)

    def sphere(self, idx, mat, pos, r):
        self.spheres.append((idx, mat, tuple(pos) + (r,)))
        return self.b.sphere(idx, mat, pos, r)

    def plane(self, idx, mat, N, d):
        self.planes.append((idx, mat, tuple(N) + (d,)))
        return self.b.plane(idx, mat, N, d)

    def area_light(self, idx, pos, strength, col, radius, normal):
        self.lights.append(tuple(pos) + (strength,) + tuple(col) + (radius,) + tuple(normal) + (1.0,))
        self.light_idx.append(idx)
        return self.b.area_light(idx, pos, strength, col, radius, normal)

    def mesh_raw(self, group, mat, v9):
        self.mesh_mat.append(mat)
        return self.b.mesh_raw(group, mat, v9)

    def mesh_obj(self, group, path, mat, pos, scale):
        self.mesh_mat.append(mat)
        return self.b.mesh_obj(group, path, mat, pos, scale)

    def mesh_tri(self, group, path, mat):
        self.mesh_mat.append(mat)
        return self.b.mesh_tri(group, path, mat)

    def build(self, split=0):
        self.tlas, self.split = False, split
        return self.b.build(split)

    def build_tlas(self, split, instances):
        self.tlas, self.split, self.instances = True, split, [(int(m), np.asarray(T, F32).reshape(16)) for m, T in instances]
        return self.b.build_tlas(split, instances)

    # what the scan takes
    def mesh_of_blas(self):
        """mesh index of each BLAS: BLASes are made in the order the instance list first names their mesh"""
        out = []
        for m, _ in self.instances:
            if m not in out:
                out.append(m)
        return out

    def light_table(self):
        return (np.array(self.lights, F32).reshape(-1, 12), list(self.light_idx))

    def sphere_plane_arrays(self):
        s = np.array([x[2] for x in self.spheres], F32).reshape(-1, 4)
        q = np.array([x[2] for x in self.planes], F32).reshape(-1, 4)
        ids = np.array([x[:2] for x in self.spheres] + [x[:2] for x in self.planes], np.int32).reshape(-1, 2)
        return s, q, ids


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def _deep_tree(b, scenes):
    """the degenerate LONGESTAXIS tree of tests/test_gpu_parity.py::test_deep_tree_uses_the_spill_stack"""
    tris = np.array([[x, 0, 1, x, 1, 1, x * 1.1, 0, 1] for x in (2.0 ** i * 1e-6 for i in range(40))], F32)
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), tris)
    b.build(2)


def _deep_chain(b, scenes):
    """the 24-triangle chain of tests/spill_cases.py with wider triangles (base -0.45 .. 1.45, apex at 1.25: four rays in five of the set
    below hit one): under LONGESTAXIS a tree 24 levels deep that a ray along +x walks to the bottom, pushing the far leaf at every
    level -- the walk's stack pointer peaks at 23, past the rows kept in LDS, and the deep walks are held to the tree-free rule too"""
    import spill_cases
    t = spill_cases.chain_tris(24)
    t[:, 1], t[:, 4], t[:, 8] = -0.45, 1.45, 1.25
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), t)
    b.build(2)


def _chain_rays(name, o, rec):
    """three in four along +x from in front of the chain (direction (1, +-1e-21, +-1e-21): finite, non-zero, no drift to speak of), the
    others from between the last triangles and back along -x from beyond the far end, interleaved"""
    import spill_cases
    n = CASES[name]["n"]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + 1)
    c = dict(spill_cases.CASES["chain_p23"])
    O, D, _, _ = spill_cases._mix(rng, spill_cases._chain_parts(rng, c, n - 1 - 2 * (n // 8), n // 8))
    return O, D


def _two_prims(b, scenes):
    """a BLAS of two triangles under one instance that scales (x2.5), turns and moves it: the instance ray's direction is not unit"""
    m = b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0.25], [0.2, 0.1, 0.5, 1.1, 0.3, 0.6, 0.1, 1.2, 0.4]], F32))
    b.build_tlas(0, [(m, b.trs((0.3, -0.2, 1.0), 2.5, 0.3, 0.7, 0.0))])


def _one_leaf(b, scenes):
    """a root that is a leaf: one triangle"""
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), np.array([[0, 0, 1, 1, 0.1, 1.2, 0.2, 1, 0.9]], F32))
    b.build(0)


def _moving(b, scenes):
    """two small meshes under three instances, a brute-force sphere and floor, one light: the scene tests/test_gpu_scan.py moves"""
    from conftest import pkg
    assets = pkg("assets")
    b.area_light(11, (0.0, 5.0, 2.0), 10.0, (1, 1, 1), 1.0, (0, -1, 0))
    df, me = b.diffuse(0.8, (0, 1, 0), 0.6, 0.4, 10), b.metal(0.7, (1, 1, 1))
    m0 = b.mesh_obj(1, assets.obj_path("ico"), df, (0.0, 0.0, 0.0), 0.5)
    m1 = b.mesh_obj(2, assets.obj_path("stellatedDode"), me, (0.0, 0.0, 0.0), 0.5)
    b.plane(0, df, (0, 1, 0), 1)
    b.sphere(7, me, (1.8, -0.5, 2.0), 0.5)
    b.build_tlas(0, [(m0, b.trs((-1.2, 0.3, 3.0), 1.5, 0.0, 0.4, 0.0)), (m1, b.trs((0.4, 0.5, 3.5), 0.7, 0.3, 1.1, 0.0)), (m0, b.trs((1.9, 0.8, 4.0), 1.0, 0.0, 2.0, 0.5))])


# name -> fill(b, scenes), rays, share of random rays, share of non-unit directions, weights of vertex / edge midpoint / centroid targets.
# Sphere::Intersect takes the direction for a unit vector (template/scene.h:351-371): with any other length its t lies off the sphere and
# mostly outside the sphere's box, which leaves the ray undecided, so scenes with spheres in the tree get few such rays; the flat boxes of
# the deep tree's coplanar triangles leave a ray aimed at a vertex or an edge undecided more often than a mesh's, so it aims at centroids.
# A ray stopped one ulp behind a hit in a box without thickness is undecided about one time in three (the plane's t is a quotient, the
# slab's a product with the reciprocal), so the deep tree's 'hit_ulp' set places such a tmax on one ray of eight, not of four.
def _case(fill, n, random=0.15, nonunit=0.5, targets=(1, 1, 1), ulp_every=4, make=None):
    return dict(fill=fill, n=n, random=random, nonunit=nonunit, targets=targets, ulp_every=ulp_every, make=make)


CASES = {
    "mixed_small_s0": _case(lambda b, s: s.mixed_small(b, split=0), 8192, 0.5, 0.04),
    "mixed_small_s1": _case(lambda b, s: s.mixed_small(b, split=1), 8192, 0.5, 0.04),
    "mixed_small_s2": _case(lambda b, s: s.mixed_small(b, split=2), 8192, 0.5, 0.04),
    "mixed_small_s3": _case(lambda b, s: s.mixed_small(b, split=3), 8192, 0.5, 0.04),
    "tlas_test2_BigB": _case(lambda b, s: s.tlas_test2(b, mesh="BigB"), 2048),
    "pretty_tlas_1": _case(lambda b, s: s.pretty_tlas(b, 1), 2048),
    "pretty_tlas_8": _case(lambda b, s: s.pretty_tlas(b, 8), 1024),
    "deep_tree": _case(_deep_tree, 4096, 0.05, targets=(1, 1, 30), ulp_every=8),
    "deep_chain": _case(_deep_chain, 4096, make=_chain_rays),  # its own rays: the mix below aims from every side and never walks deep
    "two_prims": _case(_two_prims, 2048, 0.05, targets=(1, 1, 4)),
    "one_leaf": _case(_one_leaf, 2048, 0.05, targets=(1, 1, 4)),
    "moving": _case(_moving, 4096),
}
LARGE = ("tlas_test2_BigB", "pretty_tlas_1", "pretty_tlas_8")  # 12 to 100 thousand triangles: fewer rays, and fewer repeats in the tests
SMALL = ("mixed_small_s0", "mixed_small_s1", "mixed_small_s2", "mixed_small_s3", "deep_tree", "two_prims", "one_leaf")
DEEP_WALKS = ("deep_chain",)  # (apart from SMALL: set_time would turn the chain about z, and its rays are made for the chain as it is)


def fill(name, b, scenes):
    """fills the builder b with the case's scene; returns the Recorder"""
    rec = Recorder(b)
    CASES[name]["fill"](rec, scenes)
    return rec


# ---- the scan's parts from an oracle-side scene (tests/test_gpu_scan.py reads the device's own arrays instead) -----------------------------
def mesh_prims(oa, o, rec, meshes, with_scene_prims):
    v, ids = [], []
    for m in meshes:
        t, obj = o.mesh_tris(m)
        v.append(t)
        ids.append(np.stack([obj, np.full(len(obj), rec.mesh_mat[m], np.int32)], 1))
    v = np.concatenate(v) if v else np.zeros((0, 15), F32)
    s, q, pid = rec.sphere_plane_arrays() if with_scene_prims else (None, None, np.zeros((0, 2), np.int32))
    return oa.ScanPrims(v9=v[:, :9], tri_n=v[:, 9:12], spheres=s, planes=q, ids=np.concatenate(ids + [pid]))


def oracle_parts(oa, o, rec, scope, index=0, t_min=1e-6):
    """the parts (tests/scan_ref.py) of a query of the oracle scene o: scope 'world' (Scene::FindNearest / IsOccluded(Ray&)), 1, 2 or 3.
    Returns (parts for the nearest hit, parts for occlusion): in a TLAS scene the brute-force primitives cast no shadows."""
    from scan_ref import BVH_T_MIN
    if not rec.tlas:
        part = dict(prims=mesh_prims(oa, o, rec, range(len(rec.mesh_mat)), True), t_min=BVH_T_MIN)
        return [part], [part]
    mob = rec.mesh_of_blas()
    if scope == 2:
        part = dict(prims=mesh_prims(oa, o, rec, [mob[index]], False), t_min=BVH_T_MIN)
        return [part], [part]
    parts = []
    for i in ([index] if scope == 3 else range(len(rec.instances))):
        I = o.instance_dump(i)
        parts.append(dict(prims=mesh_prims(oa, o, rec, [mob[I["blas"]]], False), t_min=BVH_T_MIN, inv_t=I["invT"], nrm_m=I["T"],
                          bounds=None if scope == 3 else I["bounds"]))
    if scope == "world":
        s, q, pid = rec.sphere_plane_arrays()
        return [dict(prims=oa.ScanPrims(spheres=s, planes=q, ids=pid, nobox=True), t_min=t_min)] + parts, parts
    return parts, parts


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------
def world_geometry(o, rec):
    """(k, 3, 3) f64 world-space triangles and (m, 4) spheres of the scene, for aiming"""
    out = []
    if rec.tlas:
        mob = rec.mesh_of_blas()
        for i in range(len(rec.instances)):
            I = o.instance_dump(i)
            T = I["T"].reshape(4, 4).astype(np.float64)
            v = o.mesh_tris(mob[I["blas"]])[0][:, :9].reshape(-1, 3).astype(np.float64)
            out.append((v @ T[:3, :3].T + T[:3, 3]).reshape(-1, 3, 3))
    else:
        for m in range(len(rec.mesh_mat)):
            out.append(o.mesh_tris(m)[0][:, :9].reshape(-1, 3, 3).astype(np.float64))
    tris = np.concatenate(out)
    return tris[np.isfinite(tris).all((1, 2))], np.array([x[2] for x in rec.spheres], np.float64).reshape(-1, 4)


def _nudge(d, rng):
    """+-1 to 3 ulp on every component"""
    k = rng.integers(1, 4, d.shape).astype(np.int32) * rng.choice(np.array([-1, 1], np.int32), d.shape)
    d = np.ascontiguousarray(d, F32)
    return np.where(np.abs(d) > 1e-30, (d.view(np.int32) + k).view(F32), d)  # (integer steps from a zero would leave the numbers)


def make_rays(name, o, rec):
    """the case's ray set (O, D), seeded by its name"""
    case = CASES[name]
    if case["make"]:
        O, D = case["make"](name, o, rec)
        assert np.isfinite(O).all() and np.isfinite(D).all() and (D != 0).all() and len(O) <= 8192, name
        return O, D
    n, random_share = case["n"], case["random"]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + 1)
    tris, sph = world_geometry(o, rec)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = np.maximum(hi - lo, 1e-3)
    n_rand, n_surf = int(n * random_share), n // 16
    n_aim = n - n_rand - n_surf
    # random rays through the content box: from a point around it towards a point inside it; every other one in any direction
    tgt = rng.uniform(lo, hi, (n_rand, 3))
    org = (lo + hi) / 2 + rng.normal(size=(n_rand, 3)) * ext * 1.5
    d = tgt - org
    d[::2] = rng.normal(size=d[::2].shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    O, D = [org.astype(F32)], [d.astype(F32)]
    # aimed: vertices, edge midpoints, centroids (and sphere silhouette points), four distances, three direction lengths, nudges on half
    t = tris[rng.integers(0, len(tris), n_aim)]
    kind = rng.choice(3, n_aim, p=np.array(case["targets"], np.float64) / sum(case["targets"]))
    a, b = rng.integers(0, 3, n_aim), rng.integers(1, 3, n_aim)
    ar = np.arange(n_aim)
    vert, mid, cen = t[ar, a], (t[ar, a] + t[ar, (a + b) % 3]) / 2, t.mean(1)
    tgt = np.where((kind == 0)[:, None], vert, np.where((kind == 1)[:, None], mid, cen))
    if len(sph):
        k = rng.uniform(size=n_aim) < 0.1
        s = sph[rng.integers(0, len(sph), n_aim)]
        u = rng.normal(size=(n_aim, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        tgt = np.where(k[:, None], s[:, :3] + u * s[:, 3:4], tgt)
    dirs = rng.normal(size=(n_aim, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dist = rng.choice([0.5, 3.0, 30.0, 1e3], n_aim)
    org = (tgt - dirs * dist[:, None]).astype(F32)
    d = tgt - org.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = (d * np.where(rng.uniform(size=n_aim) < case["nonunit"], rng.choice([1e-3, 37.0], n_aim), 1.0)[:, None]).astype(F32)
    d[::2] = _nudge(d[::2], rng)
    O.append(org), D.append(d)
    # starting on a surface: a triangle's centroid rounded to f32, any direction (the self-hit against the level's t_min)
    c = tris[rng.integers(0, len(tris), n_surf)].mean(1)
    d = rng.normal(size=(n_surf, 3))
    O.append(c.astype(F32)), D.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32))
    O, D = np.concatenate(O), np.concatenate(D)
    D[D == 0] = F32(1e-7)
    assert np.isfinite(O).all() and np.isfinite(D).all() and len(O) <= 8192, name
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


def tmax_sets(t_all, every=4):
    """name -> tmax: none; a constant; per ray the nearest leaf distance (scope 1, no tmax) one ulp farther (ray 0 of every 'every') or
    nearer (ray 1), none for the other rays"""
    hit = t_all < F32(1e30)
    b = np.ascontiguousarray(t_all, F32).view(np.int32)
    k = np.arange(len(b)) % every
    near = np.where(k < 2, (b + np.where(k == 0, 1, -1).astype(np.int32)).view(F32), F32(1e34))
    return {"none": None, "const": np.full(len(t_all), 2000.0, F32), "hit_ulp": np.where(hit | (k >= 2), near, F32(5.0)).astype(F32)}


_SETS = {}


def ray_sets(name, oa, scenes):
    """(O, D, {tmax set name: tmax}) of a case, made once with an oracle-side scene and shared, never changed"""
    if name not in _SETS:
        import scan_ref as sr
        o = oa.OracleScene()
        rec = fill(name, o, scenes)
        O, D = make_rays(name, o, rec)
        parts, _ = oracle_parts(oa, o, rec, 1)
        tm = np.full(len(O), 1e34, F32)
        t_all = sr.scan_query(oa, parts, O, D, tm, tm)["t_all"]
        o.close()
        _SETS[name] = (O, D, tmax_sets(t_all, CASES[name]["ulp_every"]))
    return _SETS[name]
