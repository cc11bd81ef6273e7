"""Support for the tests of rt_set_mesh_indices / rt_set_vertices (include/rt_amd.h), in NumPy: indexed meshes made from triangle soups and
back, the shared-vertex meshes the tests deform, the meshes that put each extreme of a box on one chosen triangle (the device's reduction
must not drop a lane, a wave or a block), the expected description on top of tests/triangles_desc.py, and the comparison under the one
rule that is not bitwise: a degenerate triangle's normal is a NaN whose sign and payload are the device's.  Nothing here loads the library
under test."""
import numpy as np

import triangles_ref as tr

f32, u32 = np.float32, np.uint32


# ---- indexed meshes ------------------------------------------------------------------------------------------------------------------------
def weld(v9):
    """(n, 9) triangles -> (xyz, idx): the distinct vertices in order of first use (distinct BIT PATTERNS: -0 is not +0, and a NaN is
    itself) and, per triangle, the three 0-based indices into them"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3)
    keys = np.ascontiguousarray(v).view(u32).reshape(-1, 3)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # unique row -> its rank by first use
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    xyz = v[np.sort(first)].copy()
    idx = rank[np.asarray(inverse).reshape(-1)].astype(u32).reshape(-1, 3)
    return xyz, idx


def assemble(xyz, idx):
    """the inverse: triangle p is xyz[idx[p, 0]], xyz[idx[p, 1]], xyz[idx[p, 2]], as (n, 9)"""
    xyz = np.ascontiguousarray(xyz, dtype=f32).reshape(-1, 3)
    return xyz[np.asarray(idx, dtype=np.int64).reshape(-1, 3)].reshape(-1, 9).copy()


def grid(m, n, seed=8, extent=0.35):
    """a shared-vertex height field of m x n cells around (0, 0.4, 0): (m + 1)(n + 1) vertices, 2 m n triangles in strips, as (xyz, idx)"""
    rng = np.random.default_rng(seed)
    x, z = np.linspace(-extent, extent, m + 1), np.linspace(-extent, extent, n + 1)
    y = 0.4 + rng.uniform(-0.1, 0.1, (m + 1, n + 1))
    X, Z = np.meshgrid(x, z, indexing="ij")
    xyz = np.stack([X, y, Z], -1).reshape(-1, 3).astype(f32)
    at = lambda i, j: i * (n + 1) + j
    idx = []
    for i in range(m):
        for j in range(n):
            idx.append((at(i, j), at(i + 1, j), at(i + 1, j + 1)))
            idx.append((at(i, j), at(i + 1, j + 1), at(i, j + 1)))
    return xyz, np.array(idx, dtype=u32)


def asset(name):
    """an indexed fixture of the product's assets (ico, lowBigB, three, stellatedDode), scaled into the test scenes' size, 0-based"""
    import conftest
    v, f = conftest.pkg("assets").obj_arrays(name)
    v = np.asarray(v, dtype=f32)
    span = float(np.abs(v).max())
    xyz = (v * f32(0.35 / span) + np.array([0, 0.4, 0], f32)).astype(f32)
    return xyz, (np.asarray(f, dtype=np.int64) - 1).astype(u32)


SHARED = {"ico": lambda: asset("ico"), "lowBigB": lambda: asset("lowBigB"), "three": lambda: asset("three"), "stellatedDode": lambda: asset("stellatedDode"),
          "grid16": lambda: grid(16, 16)}
SHARED_COUNTS = {"ico": (12, 20), "lowBigB": (9, 14), "three": (21, 38), "stellatedDode": (112, 200), "grid16": (289, 512)}  # (vertices, triangles)


# ---- the reduction's boundaries --------------------------------------------------------------------------------------------------------------
BOUNDARY_SIZES = (1, 63, 64, 65, 255, 256, 257, 769)
EXTREME = (-1.0, -0.5, -1.0, 1.0, 1.5, 1.0)  # x y z low, x y z high: outside every other coordinate of a boundary mesh


def boundary_targets(n):
    """the triangles an extreme is moved to: the first, the last, and either side of every multiple of 64 (so of 256) below n"""
    t = {0, n - 1}
    for b in range(64, n, 64):
        t |= {b - 1, b}
    return sorted(t)


def boundary_mesh(n):
    """n triangles in a strip along x: triangle p is (r[p // 2], a[p], b[p]) -- a rail vertex it shares with its neighbour and two vertices
    of its own, a[p] below and behind the rail vertex in every coordinate, b[p] above and in front of it.  As (xyz, idx); a[p] is vertex
    R + 2 p and b[p] vertex R + 2 p + 1 with R = (n + 1) // 2 rail vertices"""
    R = (n + 1) // 2
    r = np.stack([-0.3 + 0.6 * (np.arange(R) + 0.5) / R, np.full(R, 0.4), np.zeros(R)], -1)
    own = np.empty((2 * n, 3))
    own[0::2] = r[np.arange(n) // 2] - np.array([0.02, 0.02, 0.02])
    own[1::2] = r[np.arange(n) // 2] + np.array([0.02, 0.03, 0.025])
    idx = np.stack([np.arange(n) // 2, R + 2 * np.arange(n), R + 2 * np.arange(n) + 1], -1)
    return np.concatenate([r, own]).astype(f32), idx.astype(u32)


def boundary_vertices(n, extreme, t):
    """boundary_mesh(n)'s vertices with box extreme 'extreme' (0-2: x y z low, 3-5: high) on triangle t alone and the five others on
    triangle (t + n // 2) % n alone; returns (xyz, intended) with intended[e] the triangle meant to attain extreme e"""
    xyz, _ = boundary_mesh(n)
    R = (n + 1) // 2
    home = (t + n // 2) % n
    intended = [t if e == extreme else home for e in range(6)]
    for e, p in enumerate(intended):
        xyz[R + 2 * p + (e >= 3), e % 3] = f32(EXTREME[e])
    return xyz, intended


def extreme_holders(v9):
    """per box extreme (x y z low, x y z high) the triangles with a corner on it"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3, 3)
    out = []
    for a in range(3):
        out.append(np.flatnonzero((v[:, :, a] == v[:, :, a].min()).any(1)))
    for a in range(3):
        out.append(np.flatnonzero((v[:, :, a] == v[:, :, a].max()).any(1)))
    return out


# ---- deformations of a vertex array, refusal inputs -----------------------------------------------------------------------------------------
def collapse(xyz, lean=(0.31, 0.17)):
    """every vertex onto the plane z = +0, along the direction (lean, 1) and not along z: flat boxes like triangles_ref.collapse's, but no
    face of a closed mesh is projected onto a line (a face degenerates only if it holds that direction).  f64, rounded once"""
    v = np.ascontiguousarray(xyz, dtype=f32).reshape(-1, 3).astype(np.float64)
    out = np.stack([v[:, 0] - lean[0] * v[:, 2], v[:, 1] - lean[1] * v[:, 2], np.zeros(len(v))], -1)
    return out.astype(f32)


def _per_vertex(f):
    def g(xyz):
        v = np.ascontiguousarray(xyz, dtype=f32).reshape(-1, 3)
        pad = (-len(v)) % 3
        return f(np.concatenate([v, np.zeros((pad, 3), f32)]).reshape(-1, 9)).reshape(-1, 3)[:len(v)].copy()
    return g


DEFORMS = {"twist": _per_vertex(tr.twist), "scale": _per_vertex(tr.scale), "collapse": collapse}  # triangles_ref's, on (n, 3) vertex arrays


def deformed(xyz, how, keep=None):
    """xyz under DEFORMS[how]; the vertices keep (a boolean mask: a .tri mesh's sentinel vertex) stay where they are"""
    out = DEFORMS[how](xyz)
    if keep is not None:
        out[keep] = np.ascontiguousarray(xyz, dtype=f32).reshape(-1, 3)[keep]
    return out


def coincident_faces(xyz, idx):
    """the triangles with two corners at one position: degenerate by construction, and under every deformation of the vertices"""
    v = assemble(xyz, idx).reshape(-1, 3, 3)
    return np.flatnonzero((v[:, 0] == v[:, 1]).all(1) | (v[:, 1] == v[:, 2]).all(1) | (v[:, 0] == v[:, 2]).all(1))


def with_spare_vertex(xyz, idx):
    """the mesh with one more vertex that no triangle names (the last one)"""
    return np.concatenate([np.ascontiguousarray(xyz, dtype=f32).reshape(-1, 3), np.array([[0.1, 0.4, 0.1]], f32)]), np.asarray(idx, dtype=u32)


def refusal_inputs(xyz, idx):
    """name -> (vertices, the spoiled vertex, is it referenced): a NaN and a 2e29 in a vertex a triangle names (refused) and in the spare
    vertex of with_spare_vertex (accepted)"""
    n = len(xyz)
    used = int(np.asarray(idx).reshape(-1)[len(np.asarray(idx).reshape(-1)) // 2])
    out = {}
    for what, value in (("nan", np.nan), ("2e29", 2e29)):
        for where, vtx in (("referenced", used), ("spare", n - 1)):
            v = np.array(xyz, dtype=f32)
            v[vtx, 1] = f32(value)
            out["%s_%s" % (what, where)] = (v, vtx, where == "referenced")
    return out


# ---- the expected description and the NaN rule ------------------------------------------------------------------------------------------------
def nan_triangles(v9):
    """the triangles Triangle::update gives a NaN normal (degenerate ones: the reference's 0 * inf)"""
    return np.flatnonzero(np.isnan(tr.normals(v9)).any(1))


def deform(d, k, xyz, idx):
    """the description d (triangles_desc.Desc) after rt_set_vertices(k, xyz) with idx bound: the assembled triangles under
    Triangle::update's normals, obj_idx and material kept; returns the records rt_set_triangles would be sent"""
    return d.deform(k, assemble(xyz, idx), None)


def referenced(idx, n_vertices):
    out = np.zeros(n_vertices, bool)
    out[np.asarray(idx, dtype=np.int64).reshape(-1)] = True
    return out


def same_prims(got, want, prim_idx, nan_tris):
    """primitive records (16 words each, in slot order) equal bit for bit, but for N.x N.y N.z and d (words 3, 7, 11, 12) of the records
    of the triangles nan_tris, which must hold NaNs in both"""
    g = np.ascontiguousarray(got).view(u32).reshape(-1, 16).copy()
    w = np.ascontiguousarray(want).view(u32).reshape(-1, 16).copy()
    if g.shape != w.shape:
        return False
    slots = np.flatnonzero(np.isin(np.asarray(prim_idx, dtype=np.int64), np.asarray(nan_tris, dtype=np.int64)))
    free = [3, 7, 11, 12]
    for x in (g, w):
        if len(slots) and not np.isnan(x[np.ix_(slots, free)].view(f32)).all():
            return False
        x[np.ix_(slots, free)] = 0
    return np.array_equal(g, w)
