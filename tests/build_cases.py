"""Crafted inputs for the device builders (csrc/rt_build.h k_build_level, k_build_tlas) and the refit behind rt_set_time (csrc/rt_kernels.h
k_animate, k_refit, k_refit_level, k_wide_sync).  A plain helper module of the test suite, numpy only, seeded: tests/test_gpu_build.py drives the
device with these inputs, tests/test_build_cpu.py checks on a machine without a device that every input reaches the branch it is listed for.

The constants restate the library's: RT_BUILD_THREADS (the stride of every loop of k_build_level's closed-form partition), the levels
rt_build_bvh_split launches before it reads the open count back, the record count from which rt_set_time gives a refit level a launch of its
own.  A change to one of them in the library makes the CPU tier say that the inputs no longer reach the edges."""
import numpy as np

f32 = np.float32
BUILD_THREADS = 256  # RT_BUILD_THREADS
LEVEL_GROUP = 16     # csrc/rt_api_build.inc: levels per launch group
REFIT_WIDE = 2048    # csrc/rt_api_build.inc rt_set_time: records from which a level is launched on its own
SPLITS = (0, 1, 2, 3)  # BINNEDSAH, SAMESIZE, LONGESTAXIS, SAH (bvh.h:38-43)
SAH_MAX = 600        # full-sweep SAH is quadratic per node: split 3 runs only up to this many primitives


def same_tree(got, ref):
    """(nodes, prim_idx) of HostRenderer.build_bvh against an oracle bvh_dump: numbering, boxes, primitiveIdx, bit for bit"""
    nodes, prim = got
    assert len(nodes) == ref["nodes_used"]
    assert np.array_equal(prim, ref["prim_idx"])
    keep = np.ones(len(nodes), dtype=bool)
    keep[1] = False  # node 1 is never allocated (Q4)
    assert np.array_equal(nodes[keep], ref["nodes"][:ref["nodes_used"]][keep])


# ---- BVH inputs --------------------------------------------------------------------------------------------------------------------
def small_tris(centres, s=0.004):
    """one small triangle per centre (n, 3): the same shape everywhere, so equal centres give equal triangles and equal coordinates equal keys"""
    c = np.asarray(centres, dtype=f32).reshape(-1, 3)
    off = np.array([[-s, -s, 0], [s, -s, 0], [0, s, s / 2]], dtype=f32)
    return (c[:, None, :] + off[None]).astype(f32).reshape(-1, 9)


def _boxed(rng, n):
    """random triangles in a box: every corner anywhere in [-3, 3]^3, so the triangles are large and overlap (the SAH trees get deep)"""
    return rng.uniform(-3, 3, (n, 9)).astype(f32)


def _lattice(flat):
    g = np.arange(8, dtype=f32)
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    if flat:
        c[:, 2] = 0
    return small_tris(c, s=0.1)


def _staircase(n):
    """SAMESIZE's deepest tree over n = 2^k - 1 primitives on one axis.  A node of 2 p + 1 keys is [a, p copies of d, p larger keys]: the
    median key is d, only a is below it, the right child holds the p copies first, its median is the first larger key, its left child is the p
    copies (equal keys: a leaf) and its right child the same shape over p keys.  Two levels per halving: 19 levels over 1023 primitives,
    where distinct keys give 11."""
    x, at = [], 0.0
    while n > 1:
        p = n // 2
        x += [at] + [at + 1.0] * p
        at, n = at + 2.0, p
    x.append(at)
    c = np.zeros((len(x), 3), dtype=f32)
    c[:, 0] = x
    return small_tris(c)


def _spheres(rng, n):
    return np.concatenate([rng.uniform(-4, 4, (n, 3)), rng.uniform(0.05, 1.5, (n, 1))], 1).astype(f32)


def _bvh_cases():
    rng = np.random.default_rng(20)
    one = np.array([[0, 0, 0, 1, 0.2, 0.1, 0.9, 0.7, 0.3]], dtype=f32)  # centroid above the middle of its box on every axis: "all right"
    out = {}
    out["equal40"] = (np.tile(one, (40, 1)), None, None)
    out["equal30_outlier_hi"] = (np.concatenate([np.tile(one, (30, 1)), rng.uniform(5, 6, (1, 9)).astype(f32)]), None, None)
    out["equal30_outlier_lo"] = (np.concatenate([np.tile(one, (30, 1)), rng.uniform(-6, -5, (1, 9)).astype(f32)]), None, None)  # the copies go right: their range is permuted
    for n in (1, 2, 3):
        out["random%d" % n] = (rng.uniform(-1, 1, (n, 9)).astype(f32), None, None)
    for n in (255, 256, 257, 511, 512, 513, 1025):  # the root's count around one and two chunks of the block, and four chunks plus one
        out["root%d" % n] = (_boxed(rng, n), None, None)
    desc = np.zeros((600, 3), dtype=f32)
    desc[:, 0] = f32(0.01) * np.arange(600, 0, -1, dtype=f32)
    out["presorted"] = (small_tris(desc, s=0.002), None, None)      # descending: every partition is all holes, then all fillers
    out["ascending"] = (small_tris(desc[::-1], s=0.002), None, None)  # K = 0: no hole, no filler
    # y, z random in [100, 101]: a centroid is 0.999 of the mean, so in a node narrower than ~0.2 every centroid lies below the spatial middle
    dup = rng.uniform(100, 101, (300, 3)).astype(f32)
    dup[:, 0] = np.repeat(np.array([0, 10, 20, 30], dtype=f32), 75)[rng.permutation(300)]
    out["duplicate_keys"] = (small_tris(dup), None, None)
    out["lattice"] = (_lattice(False), None, None)
    out["lattice_flat"] = (_lattice(True), None, None)
    chain = np.zeros((40, 3), dtype=f32)
    chain[:, 0] = np.ldexp(f32(1), np.arange(40)).astype(f32)
    out["chain"] = (small_tris(chain), None, None)
    out["staircase"] = (_staircase(1023), None, None)
    mixed_t, mixed_s = _boxed(rng, 257), _spheres(rng, 70)
    out["mixed_plane"] = (mixed_t, mixed_s, np.array([[0, 1, 0, 1]], dtype=f32))
    out["mixed"] = (mixed_t, mixed_s, None)
    for n in (1, 2, 65):
        out["spheres%d" % n] = (None, _spheres(rng, n), None)
    # the large primitives above stay one leaf under binned SAH; small ones far apart are split, with spheres in the bins (grown by 2 r, Q3)
    small = _spheres(rng, 70)
    small[:, 3] = (small[:, 3] * f32(0.2)).astype(f32)
    out["mixed_sparse"] = (small_tris(rng.uniform(-4, 4, (257, 3)), s=0.1), small, None)
    # +0.0 and -0.0 among the corners: a zero bound has the sign of the last zero the reference's a < b ? a : b met, in primitiveIdx
    # order (leaves) and left-then-right (inner nodes), while a hardware minimum prefers -0 and a hardware maximum +0.
    # signed_zeros: coordinates in [0, 1), three in ten of them a zero of either sign
    rz = np.random.default_rng(22)
    zeros, m = rz.uniform(0, 1, (96, 9)).astype(f32), rz.random((96, 9))
    zeros[m < 0.15], zeros[(m >= 0.15) & (m < 0.3)] = f32(0.0), f32(-0.0)
    out["signed_zeros"] = (zeros, None, None)
    # lattice_zero_signs: an 8 x 8 lattice of triangles that lie in the plane z = 0, each with z = +0 or z = -0 at all three corners:
    # both z bounds of the root, of every inner node and of every leaf are zeros
    g = np.arange(8, dtype=f32)
    c = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    flat = np.zeros((64, 3, 3), dtype=f32)
    flat[:, :, :2] = c[:, None, :] + np.array([[-0.1, -0.1], [0.1, -0.1], [0, 0.1]], dtype=f32)[None]
    flat[rz.random(64) < 0.5, :, 2] = f32(-0.0)
    out["lattice_zero_signs"] = (flat.reshape(64, 9), None, None)
    return out


BVH_CASES = _bvh_cases()  # name -> (triangles (n, 9) | None, spheres (n, 4) | None, planes (n, 4) | None)


def sizes(case):
    """(triangles, spheres, planes) of a case"""
    return tuple(0 if a is None else len(a) for a in BVH_CASES[case])


def bvh_runs():
    """every (case, split) that is run: split 3 only where triangles + spheres <= SAH_MAX"""
    return [(name, s) for name in BVH_CASES for s in SPLITS if s != 3 or sum(sizes(name)[:2]) <= SAH_MAX]


def oracle_bvh(oracle_api, case, split):
    """bvh_dump(-1) of the oracle's bvh::Build over a case (a scene of one raw mesh, the spheres, the planes)"""
    tv, sph, pla = BVH_CASES[case]
    o = oracle_api.OracleScene()
    mat = o.diffuse(0.8, (1, 1, 1))
    if tv is not None:
        o.mesh_raw(1, mat, tv)
    for i, s in enumerate(sph if sph is not None else ()):
        o.sphere(100 + i, mat, s[:3], s[3])
    for i, p in enumerate(pla if pla is not None else ()):
        o.plane(200 + i, mat, p[:3], p[3])
    o.build(split)
    ref = o.bvh_dump(-1)
    o.close()
    return ref


def tree_ranges(ref):
    """per used node of a dump the range [first, first + count) of primitiveIdx below it (node 1: (0, 0)); children have larger numbers"""
    nodes, used = ref["nodes"], ref["nodes_used"]
    first, count = np.zeros(used, np.int64), np.zeros(used, np.int64)
    for i in range(used - 1, -1, -1):
        if i == 1:
            continue
        lf, pc = int(nodes[i, 3]), int(nodes[i, 7])
        if pc:
            first[i], count[i] = lf, pc
        else:
            first[i], count[i] = min(first[lf], first[lf + 1]), count[lf] + count[lf + 1]
    return first, count


def keys(case):
    """the split keys (n, 3) of a case's triangles and spheres: Triangle::centroid = (v0 + v1 + v2) * 0.333f, Sphere::pos"""
    tv, sph, _ = BVH_CASES[case]
    k = []
    if tv is not None:
        v = tv.reshape(-1, 3, 3)
        k.append(((v[:, 0] + v[:, 1]) + v[:, 2]) * f32(0.333))
    if sph is not None:
        k.append(sph[:, :3])
    return np.concatenate(k).astype(f32)


def longest_axis(lo, hi):
    """the axis bvh::Subdivide picks for SAMESIZE and LONGESTAXIS (bvh.cpp:228-231)"""
    e = hi - lo
    a = 1 if e[1] > e[0] else 0
    return 2 if e[2] > e[a] else a


# ---- TLAS box sets --------------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, nz, extent=1.0, spacing=2.0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64) * spacing
    return np.concatenate([g, g + extent], 1).astype(f32)


def _tlas_sets():
    out = {"grid4x4x4": _grid(4, 4, 4), "grid16x16x1": _grid(16, 16, 1), "grid256x1x1": _grid(256, 1, 1)}
    for n in (63, 64, 65, 129):  # tlas_best_match gives lane l the candidates l, l + 64, l + 128, l + 192
        out["line%d" % n] = _grid(n, 1, 1)
    out["grid6x6x6_permuted"] = _grid(6, 6, 6)[np.random.default_rng(21).permutation(216)]
    one = np.array([[-1, 0, 2, 1.5, 3, 2.5]], dtype=f32)
    out["identical5"], out["identical256"] = np.tile(one, (5, 1)), np.tile(one, (256, 1))
    out["points4x4x4"] = _grid(4, 4, 4, extent=0.0, spacing=1.0)  # zero-extent boxes: every union area is 0 or a small integer
    k = np.arange(1, 41, dtype=f32)[:, None]
    out["concentric40"] = np.concatenate([-k * f32(0.25) * np.ones((1, 3), f32), k * f32(0.25) * np.ones((1, 3), f32)], 1).astype(f32)
    out["huge3x3"] = _grid(3, 3, 1, extent=1e14, spacing=1e14)  # areas up to ~2e29: below FindBestMatch's 1e30
    out["beyond2x2"] = _grid(2, 2, 1, extent=1e15, spacing=1e15)  # every union area >= 2e30: no match at the first step
    return out


TLAS_SETS = _tlas_sets()  # name -> (n, 6) f32 boxes (min.xyz, max.xyz)
TLAS_NO_MATCH = ("beyond2x2",)
# the sets in which FindBestMatch meets equal smallest areas (grids and repeated boxes)
TLAS_TIED = tuple(k for k in TLAS_SETS if k.startswith(("grid", "line", "identical", "points", "huge")))


def tlas_reference(b6, stats=None):
    """tlas::build (tlas.cpp:13-48) with FindBestMatch (:50-63) over (n, 6) boxes, a plain restatement: the nodes as (used, 8) uint32, or None
    where FindBestMatch finds no union area below 1e30 (the reference would index nodeIdx[-1]).  stats (a dict) receives 'calls' and 'tied':
    FindBestMatch calls, and those whose smallest area more than one candidate has.  The loop is cut after 4 n^2 + 16 rounds (k_build_tlas's own
    guard is 4 * 256^2): a cycle raises instead of hanging."""
    b6 = np.asarray(b6, dtype=f32).reshape(-1, 6)
    n = len(b6)
    node = np.zeros((2 * n + 1, 8), np.uint32)
    nf = node.view(np.float32)
    idx = list(range(1, n + 1))
    for i in range(n):
        nf[1 + i, 0:3], nf[1 + i, 4:7] = b6[i, :3], b6[i, 3:]
        node[1 + i, 7] = i
    used = n + 1
    live = n
    count = stats if stats is not None else {}
    count.update(calls=0, tied=0)
    def best(A):
        ids = np.array(idx[:live])
        e = np.maximum(nf[idx[A], 4:7][None], nf[ids, 4:7]) - np.minimum(nf[idx[A], 0:3][None], nf[ids, 0:3])  # float32 throughout
        area = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
        if A < live:
            area[A] = np.inf
        B = int(np.argmin(area))  # the first minimum, like the strict '<' of FindBestMatch
        count["calls"] += 1
        count["tied"] += int(area[B] < np.float32(1e30) and (area == area[B]).sum() > 1)
        return B if area[B] < np.float32(1e30) else -1
    A, B = 0, best(0) if n > 1 else 0
    rounds = 0
    while live > 1:
        rounds += 1
        if rounds > 4 * n * n + 16:
            raise RuntimeError("tlas::build does not terminate on these boxes")
        if B < 0:
            return None
        Cc = best(B)
        if Cc < 0:
            return None
        if A != Cc:
            A, B = B, Cc
            continue
        ia, ib = idx[A], idx[B]
        node[used, 3] = ia + (ib << 16)
        nf[used, 0:3] = np.minimum(nf[ia, 0:3], nf[ib, 0:3])
        nf[used, 4:7] = np.maximum(nf[ia, 4:7], nf[ib, 4:7])
        idx[A] = used
        used += 1
        idx[B] = idx[live - 1]  # the list only shrinks logically: A may now sit past its end, as in the reference
        live -= 1
        B = best(A)
    node[0] = node[idx[A]]
    return node[:used]


# ---- the refit scene ----------------------------------------------------------------------------------------------------------------
REFIT_CLUSTER = (64, 128)  # a cluster: this many cells in x and y, one small triangle each, flat in z
REFIT_CHAIN = range(2, 14)  # chain triangles at z = 2^2 .. 2^13
REFIT_FAR = 12              # the second cluster lies at z = 2^12, ten chain steps beyond the first one's z = 0


def refit_triangles():
    """Two flat clusters of 64 x 128 small triangles (cell 1/64, x in [0, 1), y in [0, 2)) at z = 0 and z = 2^12, and a chain of small
    triangles at z = 2^2 .. 2^13 on the z axis.  Under LONGESTAXIS the chain is peeled off one triangle per level from the far end; the far
    cluster leaves the chain at depth 2, the near one at depth 12, and each is then halved down to single triangles (y, x alternating: z is
    never their longest axis, which matters because a centroid is 0.999 of the mean and at z = 4096 lies outside its own triangle).  The pair
    records per depth are then wide (>= REFIT_WIDE) at depths 13-14 (far cluster) and 23-24 (near cluster) with only narrow levels between.
    Scene::SetTime turns x, y about z and leaves z alone, so the boxes move while the tree keeps this shape."""
    nx, ny = REFIT_CLUSTER
    gx, gy = np.meshgrid(np.arange(nx, dtype=f32) / f32(64) + f32(1 / 128), np.arange(ny, dtype=f32) / f32(64) + f32(1 / 128), indexing="ij")
    cell = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(nx * ny, f32)], -1)
    far = cell.copy()
    far[:, 2] = f32(2.0 ** REFIT_FAR)
    chain = np.zeros((len(REFIT_CHAIN), 3), dtype=f32)
    chain[:, 0], chain[:, 1], chain[:, 2] = 0.01, 0.01, [2.0 ** k for k in REFIT_CHAIN]
    return np.concatenate([small_tris(cell, s=0.006), small_tris(far, s=0.006), small_tris(chain, s=0.006)])


def refit_scene(b):
    """the refit scene through the scene-builder protocol (scenes.py): one raw mesh, LONGESTAXIS, no TLAS"""
    b.area_light(11, (0.5, 1.0, -6.0), 10.0, (1, 1, 1), 1.0, (0, 0, 1))
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), refit_triangles())
    b.build(2)
    return dict(name="refit_scene", tlas=False)


def refit_rays(n, seed):
    """n seeded rays aimed at the two clusters from both sides of their planes (a cluster covers about a third of its rectangle)"""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random(n) < 0.5, 0.0, 2.0 ** REFIT_FAR)
    side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    O = np.stack([rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 2.2, n), z + side * rng.uniform(0.5, 3.0, n)], -1)
    T = np.stack([rng.uniform(0, 1, n), rng.uniform(0, 2, n), z], -1)
    D = T - O
    D /= np.sqrt((D ** 2).sum(1, keepdims=True))
    return O.astype(f32), D.astype(f32)


def refit_profile(level_start):
    """records per refit level from refitLevelStart, and the levels going up from the deepest as a string of 'W' (>= REFIT_WIDE) and 'n',
    runs collapsed: 'WnWn' is wide, narrow, wide, narrow top"""
    counts = np.diff(np.asarray(level_start, dtype=np.int64))
    s = "".join("W" if c >= REFIT_WIDE else "n" for c in counts[::-1])
    return counts, "".join(ch for i, ch in enumerate(s) if i == 0 or s[i - 1] != ch)


def pair_boxes(pairs):
    """the box words of pair records (-1, 16): record p as the boxes of nodes 2 p and 2 p + 1, shaped (2 records, 2, 3) uint32 for lo and hi"""
    w = np.ascontiguousarray(pairs).view(np.uint32).reshape(-1, 16)
    lo = np.stack([w[:, 0:3], w[:, 8:11]], 1).reshape(-1, 3)
    hi = np.stack([w[:, 4:7], w[:, 12:15]], 1).reshape(-1, 3)
    return lo, hi
