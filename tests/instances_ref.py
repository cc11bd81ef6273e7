"""Restatements for rt_set_instances (include/rt_amd.h), in NumPy: the box of a fresh instance, tlas::build, the numbering its nodes always
have, and the small scenes the CPU and GPU tests of the call share.  Nothing here loads the library under test; records() takes the host mirror from its caller."""
import numpy as np

f32 = np.float32
TLAS_NODE = np.dtype([("aabb_min", np.float32, 3), ("left_right", np.uint32), ("aabb_max", np.float32, 3), ("blas", np.uint32)])
# csrc/rt_scene_dev.h: RT_LDS_WORDS, RT_BLOCK, RT_STACK_ROWS_MIN (tests/test_layout_cpu.py lds_rows)
LDS_WORDS, BLOCK, ROWS_MIN = 5120, 256, 8


def lds_rows(pairs, instances):
    words = pairs * 28 + instances * 13
    return (LDS_WORDS - ((words + 3) & ~3)) // BLOCK - 6


def smallest_n_without_lds():
    """the smallest instance count whose tlas::build-shaped TLAS (n pairs) no longer fits a traversal block's LDS"""
    n = 2
    while lds_rows(n, n) >= ROWS_MIN:
        n += 1
    return n


def transform_position(p, T):
    """TransformPosition(p, M): ((c0 * x + c1 * y) + c2 * z) + c3 * 1.0f per row, every operation rounded to f32"""
    T = np.asarray(T, dtype=f32).reshape(4, 4)
    x, y, z = f32(p[0]), f32(p[1]), f32(p[2])
    out = np.zeros(3, dtype=f32)
    for r in range(3):
        c = T[r]
        s = f32(f32(c[0] * x) + f32(c[1] * y))
        s = f32(s + f32(c[2] * z))
        out[r] = f32(s + f32(c[3] * f32(1.0)))
    return out


def fresh_bounds(local6, T):
    """bvhInstance(blas) followed by one SetTransform(T): the BLAS's local box grown by its 8 corners under T; corner i takes max.x /
    max.y / max.z where bits 0 / 1 / 2 of i are set.  min / max are the ternaries a < b ? a : b and a > b ? a : b."""
    local6 = np.asarray(local6, dtype=f32)
    lo, hi = local6[:3].copy(), local6[3:].copy()
    mn, mx = lo.copy(), hi.copy()
    for i in range(8):
        p = transform_position([hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]], T)
        for a in range(3):
            mn[a] = mn[a] if mn[a] < p[a] else p[a]
            mx[a] = mx[a] if mx[a] > p[a] else p[a]
    return np.concatenate([mn, mx]).astype(f32)


def tlas_build(b6):
    """tlas::build (tlas.cpp:13-48) with FindBestMatch (:50-63) over (n, 6) boxes: the nodes as (2 n, 8) uint32"""
    b6 = np.asarray(b6, dtype=f32).reshape(-1, 6)
    n = len(b6)
    node = np.zeros(2 * n + 1, dtype=TLAS_NODE)
    idx = []
    used = 1
    for i in range(n):
        node[used]["aabb_min"], node[used]["aabb_max"], node[used]["blas"] = b6[i, :3], b6[i, 3:], i
        idx.append(used)
        used += 1

    def best(A, live):
        a, smallest, bb = node[idx[A]], f32(1e30), -1
        for B in range(live):
            if B == A:
                continue
            b = node[idx[B]]
            e = np.maximum(a["aabb_max"], b["aabb_max"]) - np.minimum(a["aabb_min"], b["aabb_min"])
            area = f32(f32(f32(e[0] * e[1]) + f32(e[1] * e[2])) + f32(e[2] * e[0]))
            if area < smallest:
                smallest, bb = area, B
        return bb

    live, A = n, 0
    B = best(A, live)
    while live > 1:
        Cc = best(B, live)
        if A != Cc:
            A, B = B, Cc
            continue
        ia, ib = idx[A], idx[B]
        node[used]["left_right"] = ia + (ib << 16)
        node[used]["aabb_min"] = np.minimum(node[ia]["aabb_min"], node[ib]["aabb_min"])
        node[used]["aabb_max"] = np.maximum(node[ia]["aabb_max"], node[ib]["aabb_max"])
        idx[A] = used
        used += 1
        idx[B] = idx[live - 1]
        live -= 1
        B = best(A, live)
    node[0] = node[idx[A]]
    return node[:used].view(np.uint32).reshape(-1, 8).copy()


def check_numbering(nodes, n):
    """fact 1 of csrc/rt_instances.h on a (2 n, 8) uint32 node array: leaves 1..n (leaf i holds instance i - 1), inner nodes n+1..2n-1 with
    children below them, node 0 a copy of the last node"""
    nodes = np.asarray(nodes).reshape(-1, 8)
    assert len(nodes) == 2 * n
    lr, blas = nodes[:, 3].astype(np.int64), nodes[:, 7]
    assert np.all(lr[1:n + 1] == 0) and np.array_equal(blas[1:n + 1], np.arange(n, dtype=np.uint32))
    for i in range(n + 1, 2 * n):
        a, b = lr[i] & 0xFFFF, lr[i] >> 16
        assert lr[i] != 0 and 1 <= a < i and 1 <= b < i and a != b
    assert np.array_equal(nodes[0], nodes[2 * n - 1])
    inner_children = sorted(int(c) for i in range(n + 1, 2 * n) for c in (lr[i] & 0xFFFF, lr[i] >> 16))
    assert inner_children == list(range(1, 2 * n - 1)), "every node but the root is the child of exactly one inner node"


def aimed_rays(n, seed, transforms, spread=4.0):
    """n seeded rays, three in four aimed at points near the instances' places (the rest anywhere, some axis-aligned): origins in a box
    around the scene, so that a good share meets the instanced geometry however small it is"""
    rng = np.random.default_rng(seed)
    at = np.stack([np.asarray(T, dtype=np.float64).reshape(4, 4)[:3, 3] for T in transforms])
    O = (rng.uniform(-1, 1, (n, 3)) * spread + np.array([0.0, 1.5, 1.0])).astype(f32)
    D = rng.normal(size=(n, 3))
    k = 3 * n // 4
    tgt = at[rng.integers(0, len(at), k)] + rng.normal(size=(k, 3)) * 0.15 + np.array([0.0, 0.2, 0.0])
    D[:k] = tgt - O[:k]
    D[k:k + 6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)[:max(0, min(6, n - k))]
    D = (D / np.maximum(np.sqrt((D ** 2).sum(1, keepdims=True)), 1e-20)).astype(f32)
    return O, D


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def grid_transforms(scene, n, turn=0.0, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """n instance transforms on a 16-wide grid in front of the default camera: Translate * Scale * RotateY(turn + 0.1 i)"""
    return [scene.trs((f32(-3.0 + 0.45 * (i % 16) + shift[0]), f32(0.2 + 0.3 * (i // 16) + shift[1]), f32(2.0 + 0.05 * i + shift[2])), f32(scale), 0.0,
                      f32(turn + 0.1 * i), 0.0) for i in range(n)]


def triangles_scene(b, transforms, two_meshes=True):
    """one-triangle BLASes (two of them, alternating, when two_meshes) under len(transforms) instances, a floor plane and a sphere tested by
    brute force, one light: the smallest scene with every part of a TLAS scene"""
    b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
    red = b.diffuse(0.8, (1, 0.2, 0.2), 0.0, 1, 1)
    blue = b.diffuse(0.8, (0.2, 0.2, 1), 0.0, 1, 1)
    floor = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    m0 = b.mesh_raw(1, red, np.array([[-0.2, 0, 0, 0.2, 0, 0, 0, 0.4, 0.05]], dtype=f32))
    m1 = b.mesh_raw(2, blue, np.array([[-0.15, 0, 0.1, 0.15, 0, -0.1, 0, 0.3, 0], [-0.15, 0, 0.1, 0, 0.3, 0, 0, 0.1, 0.3]], dtype=f32)) if two_meshes else m0
    b.plane(0, floor, (0, 1, 0), 0)
    b.sphere(7, blue, (1.8, 0.5, 2.0), 0.5)
    b.build_tlas(0, [((m0, m1)[i & 1], T) for i, T in enumerate(transforms)])
    return dict(name="triangles", tlas=True, meshes=(m0, m1))


def mesh_scene(b, transforms, mesh="lowBigB"):
    """scenes.tlas_test2's contents (TLASSceneTest2, template/scene.h:941-972) under the given instance transforms"""
    import importlib
    assets = importlib.import_module("ray-and-pathtracer_amd.assets")
    red = b.diffuse(0.8, (1, 0, 0), 0.0, 1, 1)
    gold = b.diffuse(0.8, (1, 0.84, 0), 0.8, 0.2, 1)
    floor = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
    m = b.mesh_obj(1, assets.obj_path(mesh), red, (0, 0.5, 0), 1)
    b.plane(0, floor, (0, 1, 0), 0)
    b.sphere(7, gold, (1.8, -0.5, 2.0), 0.5)
    b.build_tlas(0, [(m, T) for T in transforms])
    return dict(name="mesh_scene", tlas=True)


def mesh_transforms(scene, turn):
    """three placements like tlas_test2's, each turned by 'turn' more"""
    return [scene.trs((0, 0, 3), 4, 0.0, f32(1.5707964 + turn), 0.0), scene.trs((f32(2 + 0.3 * turn), 0, 3), 4, 0.0, f32(3.1415927 - turn), 0.0),
            scene.trs((f32(-2.3), f32(0.2 * turn), 3), 4, 0.0, f32(1.5707964 + 2 * turn), 0.0)]


def records(host_api, blas, Ts):
    """rt_instance records: the transforms with the host mirror's inverse (mat4::Inverted, as SetTransform takes it)"""
    import ctypes as C
    L = host_api.host_lib()
    rec = np.zeros(len(Ts), dtype=host_api.RT_INSTANCE_DTYPE)
    for k, T in enumerate(Ts):
        T = np.ascontiguousarray(T, dtype=f32).reshape(16)
        inv = np.zeros(16, dtype=f32)
        L.rth_mat4_inverse(T.ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p))
        rec[k] = (blas[k], T, inv)
    return rec


def mat_mul(A, B):
    """rapt::operator*(mat4, mat4): ((a0 b0 + a1 b4) + a2 b8) + a3 b12 per entry, every operation rounded to f32"""
    A, B = np.asarray(A, dtype=f32).reshape(4, 4), np.asarray(B, dtype=f32).reshape(4, 4)
    s = A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]
    s = s + A[:, 2:3] * B[2:3, :]
    return (s + A[:, 3:4] * B[3:4, :]).astype(f32).reshape(16)
