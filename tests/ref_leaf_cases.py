"""Crafted inputs for the leaf functions of the path -- every primitive test, both lights, the material functions, the camera and the sky
lookup (template/scene.h, camera.h) -- which oracle/ref/ref_leaf.cpp runs through the reference's own compiled code.  A plain helper module of
the test suite, numpy only, seeded: tests/golden/make_ref_leaf_golden.py records the reference's answers to these inputs in
tests/golden/ref_leaf.npz, tests/test_ref_leaf_cpu.py holds the oracle and the host mirror to the record and tests/test_gpu_ref_leaf.py the device.

Every group of inputs ("family") is a named range of cases with the property the RECORD must show for it: 'hit' (every case hits), 'miss'
(every case misses), 'mixed' (at least a fifth of the cases on either side), or None where the test states the property itself.  A family that
never takes its branch is a failure of the inputs, not a pass.

The crafted triangles lie in axis planes with corners at small binary fractions, so that the plane distance, the hit point and the three edge
functions of template/scene.h:190-215 are exact in f32 and 'exactly on the edge' / 'one ulp outside' mean what they say:
  T1 = (1,1,0) (2,1,0) (1,2,0): N = (0,0,1); a ray (x, y, h) + t (0,0,-1) has t = h, edge functions y - 1, 3 - x - y, x - 1
  TX = (2,1,1) (2,1,3) (2,3,1): N = (-1,0,0); a ray (3, y, z) + t (-1,0,0) has t = 1, edge functions 2 (y - 1), 2 (4 - y - z), 2 (z - 1)"""
import numpy as np

f32 = np.float32
BVH_TMIN = f32(0.0001)          # what bvh::BIntersect / BIsOccluded hand every leaf test, whatever the caller's t_min (bvh.cpp:606-656, 763-806)
TMINS = (f32(1e-6), BVH_TMIN, f32(1e-3))  # the two t_min values of Renderer::Trace / Sample and the shadow rays, and the BVH's own
AREA_TMINS = (TMINS[0], TMINS[2])         # lights are tested by Scene::FindNearest itself, with the caller's t_min
FAR = f32(1e34)                 # Ray's default distance (template/scene.h:42)
CAM_W, CAM_H = 600, 400         # camera.h:4-5


def nx(x, k=1):
    """the f32 k steps above (k > 0) or below (k < 0) x"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf if k > 0 else -np.inf), dtype=f32)
    return x


def random_rays(n, seed, center=(0.5, 0.8, 1.0), spread=4.0):
    """the recipe of conftest.random_rays: origins in a box, unit directions, some axis-aligned"""
    rng = np.random.default_rng(seed)
    O = (rng.uniform(-1, 1, (n, 3)) * spread + np.array(center)).astype(f32)
    D = rng.normal(size=(n, 3)).astype(f32)
    k = n // 16
    D[:k, 0] = 0
    D[k:2 * k, 1] = 0
    D[2 * k:3 * k, 2] = 0
    D[3 * k:3 * k + 8] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, 0, 1]], dtype=f32)[: max(0, min(8, n - 3 * k))]
    nrm = np.sqrt((D.astype(np.float64) ** 2).sum(1, keepdims=True))
    return O, (D / np.maximum(nrm, 1e-20)).astype(f32)


def aimed_rays(n, seed, target, reach, center, spread=4.0):
    """seeded rays from a box towards points within 'reach' of 'target': about half of them meet a primitive of that size there"""
    rng = np.random.default_rng(seed)
    O = (rng.uniform(-1, 1, (n, 3)) * spread + np.array(center)).astype(f32)
    P = np.asarray(target, np.float64) + rng.uniform(-1, 1, (n, 3)) * reach
    D = P - O
    D /= np.sqrt((D ** 2).sum(1, keepdims=True))
    return O, D.astype(f32)


class Cases:
    """rows of per-case inputs, collected family by family"""

    def __init__(self, fields):
        self.fields = fields
        self.rows = {k: [] for k in fields}
        self.fam = []  # (name, start, stop, expect)
        self.n = 0

    def add(self, name, expect, **cols):
        assert set(cols) == set(self.fields), set(cols) ^ set(self.fields)
        arrs = {k: np.asarray(cols[k], np.float64).reshape(-1, w) for k, w in self.fields.items()}
        m = max(len(a) for a in arrs.values())
        for k, w in self.fields.items():
            self.rows[k].append(np.array(np.broadcast_to(arrs[k], (m, w))))
        self.fam.append((name, self.n, self.n + m, expect))
        self.n += m

    def done(self, dtypes=None):
        out = {}
        for k, w in self.fields.items():
            a = np.concatenate(self.rows[k]).astype((dtypes or {}).get(k, f32))
            out[k] = np.ascontiguousarray(a[:, 0] if w == 1 else a)
        out["fam"] = self.fam
        return out


# ---- Triangle -------------------------------------------------------------------------------------------------------------------------
T1 = f32([1, 1, 0, 2, 1, 0, 1, 2, 0])
TX = f32([2, 1, 1, 2, 1, 3, 2, 3, 1])
TG = f32([0.3, -0.2, 1.1, 1.7, 0.4, 0.9, 0.2, 1.5, 1.6])  # a general triangle: nothing about it is exact
DEGENERATE = f32([[1, 1, 0, 1, 1, 0, 1, 2, 0],    # v0 == v1
                  [1, 1, 0, 2, 1, 0, 2, 1, 0],    # v1 == v2
                  [0.5, 0.25, 2, 0.5, 0.25, 2, 0.5, 0.25, 2],
                  [999] * 9])                     # what a .tri mesh ends with, twice (template/scene.h:266-282)
TRI_PRIMS = np.concatenate([[T1, TX, TG], DEGENERATE]).astype(f32)


def _t1_ray(xy, h=1.0):
    xy = np.asarray(xy, f32).reshape(-1, 2)
    O = np.concatenate([xy, np.full((len(xy), 1), h, f32)], 1)
    return O, np.broadcast_to(f32([0, 0, -1]), O.shape)


def _tx_ray(yz):
    yz = np.asarray(yz, f32).reshape(-1, 2)
    O = np.concatenate([np.full((len(yz), 1), 3, f32), yz], 1)
    return O, np.broadcast_to(f32([-1, 0, 0]), O.shape)


def triangle_cases():
    c = Cases(dict(prim=1, O=3, D=3, tmax=1, tmin=1))

    def add(name, expect, prim, O, D, tmax=FAR, tmins=TMINS):
        for tm in tmins:
            c.add("%s@%g" % (name, tm), expect, prim=prim, O=O, D=D, tmax=tmax, tmin=tm)

    # interior
    O, D = _t1_ray([[1.25, 1.25], [1.1, 1.7], [1.6, 1.3], [1.01, 1.01]])
    add("interior_t1", "hit", 0, O, D)
    O, D = _tx_ray([[1.5, 1.5], [1.1, 2.7], [2.6, 1.2]])
    add("interior_tx", "hit", 1, O, D)
    a, b, cc = TG[:3].astype(np.float64), TG[3:6].astype(np.float64), TG[6:].astype(np.float64)
    inner = np.array([u * a + v * b + (1 - u - v) * cc for u, v in [(0.3, 0.3), (0.1, 0.2), (0.6, 0.2), (0.2, 0.7), (1 / 3, 1 / 3)]])
    Or = random_rays(len(inner) * 4, 5)[0]
    Dr = np.repeat(inner, 4, 0) - Or
    Dr /= np.sqrt((Dr ** 2).sum(1, keepdims=True))
    add("interior_general", "hit", 2, Or, Dr.astype(f32))
    # exactly on each edge and each corner, and one ulp outside each
    on1 = [[1.5, 1], [1.25, 1], [1, 1.5], [1, 1.75], [1.5, 1.5], [1.25, 1.75], [1.75, 1.25], [1, 1], [2, 1], [1, 2]]
    out1 = [[1.5, nx(1, -1)], [1.25, nx(1, -1)], [nx(1, -1), 1.5], [nx(1, -1), 1.75], [1.5, nx(1.5)], [nx(1.25), 1.75], [1.75, nx(1.25)],
            [nx(1, -1), 1], [1, nx(1, -1)], [nx(2), 1], [2, nx(1, -1)], [1, nx(2)], [nx(1, -1), 2]]
    add("edge_on_t1", "hit", 0, *_t1_ray(on1))
    add("edge_out_t1", "miss", 0, *_t1_ray(out1))
    onx = [[1, 2], [1, 1.5], [2, 1], [2.5, 1], [2, 2], [1.5, 2.5], [2.5, 1.5], [1, 1], [1, 3], [3, 1]]
    outx = [[nx(1, -1), 2], [2, nx(1, -1)], [2, nx(2)], [nx(1.5), 2.5], [nx(1, -1), 1], [1, nx(1, -1)], [1, nx(3)], [nx(3), 1], [nx(1, -1), 3], [3, nx(1, -1)]]
    add("edge_on_tx", "hit", 1, *_tx_ray(onx))
    add("edge_out_tx", "miss", 1, *_tx_ray(outx))
    # dot(N, D) == 0: the ray runs in a plane parallel to the triangle's (and in the triangle's own plane)
    Dp = f32([[1, 0, 0], [0, 1, 0], [0.6, 0.8, 0], [-1, 0, 0], [1, 0, 0], [0.6, 0.8, 0]])
    Op = f32([[0, 1.2, 0.5], [1.2, 0, 0.5], [0, 0, -0.25], [3, 1.2, 0.5], [0, 1.2, 0], [0.6, 0.8, 0]])
    add("parallel", "miss", 0, Op, Dp)
    # |dot(N, D)| just below t_min (the early-out of :192), equal to it and just above it; the hit is at t = 0.25, well inside
    for tm in TMINS:
        for name, dz, expect in (("ndot_below", nx(tm, -1), "miss"), ("ndot_equal", tm, "hit"), ("ndot_above", nx(tm), "hit")):
            h = f32(0.25) * dz
            c.add("%s@%g" % (name, tm), expect, prim=0, O=f32([[1.1, 1.2, h], [1.1, 1.2, -h]]), D=f32([[1, 0, -dz], [1, 0, dz]]), tmax=FAR, tmin=tm)
    # the plane is behind the origin (t < 0), and exactly at it (t == 0: every edge test passes, the range test fails)
    add("behind", "miss", 0, f32([[1.2, 1.2, -1], [1.2, 1.2, -1e-3], [1.3, 1.1, 2]]), f32([[0, 0, -1], [0, 0, -1], [0, 0, 1]]))
    add("t_zero", "miss", 0, f32([[1.2, 1.2, 0], [1, 1, 0]]), f32([[0, 0, -1], [0, 0, -1]]))
    # t against ray.t: equal, one ulp below, one ulp above (t = 1 exactly)
    O, D = _t1_ray([[1.2, 1.2], [1.5, 1.5]])
    add("tmax_at", "miss", 0, O, D, tmax=f32(1))
    add("tmax_below", "miss", 0, O, D, tmax=nx(1, -1))
    add("tmax_above", "hit", 0, O, D, tmax=nx(1))
    add("tmax_at_tx", "miss", 1, *_tx_ray([[1.5, 1.5]]), tmax=f32(1))
    add("tmax_above_tx", "hit", 1, *_tx_ray([[1.5, 1.5]]), tmax=nx(1))
    # t around t_min (t = the origin's height exactly)
    for tm in TMINS:
        c.add("tmin_at@%g" % tm, "miss", prim=0, O=_t1_ray([[1.2, 1.2]], tm)[0], D=f32([0, 0, -1]), tmax=FAR, tmin=tm)
        c.add("tmin_below@%g" % tm, "miss", prim=0, O=_t1_ray([[1.2, 1.2]], nx(tm, -1))[0], D=f32([0, 0, -1]), tmax=FAR, tmin=tm)
        c.add("tmin_above@%g" % tm, "hit", prim=0, O=_t1_ray([[1.2, 1.2]], nx(tm))[0], D=f32([0, 0, -1]), tmax=FAR, tmin=tm)
    # degenerate triangles: N is NaN, every comparison fails, nothing is hit
    for k in range(len(DEGENERATE)):
        O, D = random_rays(4, 30 + k)  # few: every one of them runs off the end of IsOccluding, and those cases are capped
        aim = DEGENERATE[k, :3].astype(np.float64) - O[:2]
        D[:2] = (aim / np.sqrt((aim ** 2).sum(1, keepdims=True))).astype(f32)
        add("degenerate%d" % k, "miss", 3 + k, O, D)
    # the floor under the crafted cases: seeded rays, about half of them aimed at the triangle
    for prim, seed in ((2, 40), (0, 41), (1, 42)):
        ctr = TRI_PRIMS[prim].reshape(3, 3).mean(0)
        O, D = aimed_rays(400, seed, ctr, 0.55, ctr)
        add("random%d" % prim, "mixed", prim, O, D)
    O, D = random_rays(200, 43)
    add("random_unaimed", None, 2, O, D)
    r = c.done(dict(prim=np.int32))
    r["prims"] = TRI_PRIMS
    return r


# ---- Sphere ---------------------------------------------------------------------------------------------------------------------------
SPH_PRIMS = f32([[0, 0, 0, 1], [1, 2, 3, 0.5], [-0.7, -0.5, 2, 0.5], [0, 2.5, -3.07, 8]])  # unit; exact halves; two of the reference's scenes'


def sphere_cases():
    c = Cases(dict(prim=1, O=3, D=3, tmax=1, tmin=1))

    def add(name, expect, prim, O, D, tmax=FAR, tmins=TMINS):
        for tm in tmins:
            c.add("%s@%g" % (name, tm), expect, prim=prim, O=O, D=D, tmax=tmax, tmin=tm)

    axes = f32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, -0.6, 0.8]])
    for p in (0, 1):
        pos, r = SPH_PRIMS[p, :3], SPH_PRIMS[p, 3]
        add("outside%d" % p, "hit", p, pos - 3 * axes, axes)                      # two roots, the first is taken
        add("inside%d" % p, "hit", p, pos + f32(0.25) * r * axes[::-1], axes)      # the first root is negative, the second is taken
        add("centre%d" % p, "hit", p, np.broadcast_to(pos, axes.shape), axes)
        add("surface_in%d" % p, "hit", p, pos - r * axes[:6], axes[:6])           # on the surface looking in: t = 0 is refused, the far root taken
        add("surface_out%d" % p, "miss", p, pos + r * axes[:6], axes[:6])          # on the surface looking out: roots -2r and 0
        add("behind%d" % p, "miss", p, pos + 3 * axes, axes)
    # the discriminant exactly 0 (a tangent ray from the tangent point), one ulp either side
    add("disc_zero", "miss", 0, f32([[1, 0, 0], [0, 1, 0], [0, -1, 0]]), f32([[0, 0, 1], [1, 0, 0], [0, 0, -1]]))
    add("disc_negative", "miss", 0, f32([[nx(1), 0, 0], [0, nx(1), 0]]), f32([[0, 0, 1], [1, 0, 0]]))
    add("disc_positive", "hit", 0, f32([[nx(1, -1), 0, 0], [0, nx(1, -1), 0]]), f32([[0, 0, 1], [1, 0, 0]]), tmins=TMINS[:2])  # roots +-3.5e-4
    add("disc_positive_small_roots", "miss", 0, f32([[nx(1, -1), 0, 0]]), f32([[0, 0, 1]]), tmins=TMINS[2:])                  # both under 1e-3
    add("tangent_far", None, 0, f32([[1, 0, -2], [1, -2, 0], [nx(1, -1), 0, -2], [nx(1), 0, -2]]), f32([[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 0, 1]]))
    # the first root under t_min, the second accepted
    add("first_root_small", "hit", 0, f32([[0, 0, -1.0005], [0, 1.0002, 0]]), f32([[0, 0, 1], [0, -1, 0]]))
    # roots at and past ray.t (roots 2 and 4 from outside; -1 and 1 from the centre)
    O, D = f32([[0, 0, -3]]), f32([[0, 0, 1]])
    add("tmax_at_first", "miss", 0, O, D, tmax=f32(2))
    add("tmax_above_first", "hit", 0, O, D, tmax=nx(2))
    add("tmax_under", "miss", 0, O, D, tmax=f32(1))
    add("tmax_between", "hit", 0, O, D, tmax=f32(3))
    add("tmax_at_second", "miss", 0, f32([[0, 0, 0]]), D, tmax=f32(1))
    add("tmax_above_second", "hit", 0, f32([[0, 0, 0]]), D, tmax=nx(1))
    for p, seed in ((0, 50), (1, 51), (2, 52), (3, 53)):
        pos, r = SPH_PRIMS[p, :3], SPH_PRIMS[p, 3]
        O, D = aimed_rays(300, seed, pos, 1.6 * r, pos, spread=4.0 if p < 3 else 12.0)
        add("random%d" % p, "mixed", p, O, D)
    r = c.done(dict(prim=np.int32))
    r["prims"] = SPH_PRIMS
    return r


# ---- Plane ----------------------------------------------------------------------------------------------------------------------------
PLA_PRIMS = f32([[0, 1, 0, 1], [0, 1, 0, 0], [0, 0, -1, 3.99], [0.6, 0.8, 0, 0.5], [-1, 0, 0, 2.99]])


def plane_cases():
    c = Cases(dict(prim=1, O=3, D=3, tmax=1, tmin=1))

    def add(name, expect, prim, O, D, tmax=FAR, tmins=TMINS):
        for tm in tmins:
            c.add("%s@%g" % (name, tm), expect, prim=prim, O=O, D=D, tmax=tmax, tmin=tm)

    par = f32([[1, 0, 0], [0, 0, 1], [0.6, 0, 0.8], [1, -0.0, 0]])
    add("parallel_above", "miss", 0, f32([0, 2, 0]), par)       # t = -inf
    add("parallel_below", "miss", 0, f32([0, -3, 0]), par)      # t = +inf, refused by t < ray.t
    add("parallel_on", "miss", 0, f32([0.5, -1, 2]), par)       # t = 0 / 0
    add("facing", "hit", 0, f32([[0, 0, 0], [3, 2, -1], [0, 0.5, 0]]), f32([[0, -1, 0], [0.6, -0.8, 0], [0.8, -0.6, 0]]))
    add("from_below", "hit", 0, f32([[0, -3, 0], [1, -1.5, 2]]), f32([[0, 1, 0], [0, 0.6, 0.8]]))
    add("facing_away", "miss", 0, f32([[0, 0, 0], [0, -3, 0]]), f32([[0, 1, 0], [0, -1, 0]]))
    add("tmax_at", "miss", 0, f32([0, 0, 0]), f32([0, -1, 0]), tmax=f32(1))
    add("tmax_above", "hit", 0, f32([0, 0, 0]), f32([0, -1, 0]), tmax=nx(1))
    for tm in TMINS:
        c.add("tmin_at@%g" % tm, "miss", prim=1, O=f32([0, tm, 0]), D=f32([0, -1, 0]), tmax=FAR, tmin=tm)
        c.add("tmin_above@%g" % tm, "hit", prim=1, O=f32([0, nx(tm), 0]), D=f32([0, -1, 0]), tmax=FAR, tmin=tm)
    for p in range(len(PLA_PRIMS)):
        O, D = random_rays(200, 60 + p)
        add("random%d" % p, "mixed", p, O, D)
    r = c.done(dict(prim=np.int32))
    r["prims"] = PLA_PRIMS
    return r


# ---- AreaLight ------------------------------------------------------------------------------------------------------------------------
# pos(3) strength col(3) radius normal(3) raytracer
AREA_LIGHTS = f32([[0, 2, 0, 4, 1, 1, 1, 1, 0, -1, 0, 1],
                   [4.5, 5, 7, 19, 1, 1, 1, 2, 0, -1, 0, 1],       # the default scene's (template/scene.h:793)
                   [1.8, 2, 5.5, 10, 1, 0.5, 0.25, 2, 0, 1, 0, 0],  # facing up, coloured, sampled
                   [0, 2, 0, 4, 1, 1, 1, 0.5, 0, -1, 0, 0],
                   [0, 0, 0, 4, 1, 1, 1, 1, 0, -1, 0, 1]])             # at the origin: distances to its plane are exact


def area_intersect_cases():
    c = Cases(dict(prim=1, O=3, D=3, tmax=1, tmin=1))

    def add(name, expect, prim, O, D, tmax=FAR, tmins=AREA_TMINS):
        for tm in tmins:
            c.add("%s@%g" % (name, tm), expect, prim=prim, O=O, D=D, tmax=tmax, tmin=tm)

    # d == 0: t is -inf (origin below), +inf (above: the hit point is NaN) or 0 / 0 (in the plane)
    add("d_zero", "miss", 0, f32([[0, 0, 0], [0, 3, 0], [0, 2, 0], [0.5, 2, 0]]), f32([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]]))
    # the rim: sqrtf(dis2) == radius is a hit, one ulp further out is not; ray.t < t does not matter (:109 has no such test)
    add("rim_on", "hit", 0, f32([[1, 0, 0], [0, 0, -1], [0.6, 1, 0.8]]), f32([0, 1, 0]))
    add("rim_on_short_ray", "hit", 0, f32([[1, 0, 0], [0.5, 0, 0]]), f32([0, 1, 0]), tmax=f32(1))
    add("rim_out", "miss", 0, f32([[nx(1), 0, 0], [0, 0, nx(-1, -1)]]), f32([0, 1, 0]))
    # the store t - 1e-6 (a double subtraction rounded to float) at several magnitudes of t, t_min itself included
    for tm in AREA_TMINS:
        hs = f32([2 - 0.5, 0, 2 - 100, 2 - 1e-3, 2 - 1e-2, 2 - 0.125]).tolist()
        c.add("store@%g" % tm, "hit", prim=0, O=f32([[0.25, h, 0.25] for h in hs]), D=f32([0, 1, 0]), tmax=FAR, tmin=tm)
        c.add("t_equals_tmin@%g" % tm, "hit", prim=4, O=f32([[0.25, -tm, 0.25]]), D=f32([0, 1, 0]), tmax=FAR, tmin=tm)  # t >= t_min (:109)
        c.add("t_below_tmin@%g" % tm, "miss", prim=4, O=f32([[0.25, -nx(tm, -1), 0.25]]), D=f32([0, 1, 0]), tmax=FAR, tmin=tm)
    add("under_tmin", "miss", 0, f32([[0, 2 - 1e-7, 0], [0, 3, 0]]), f32([0, 1, 0]))
    add("from_behind", "hit", 0, f32([[0.2, 4, 0.1]]), f32([0, -1, 0]))   # a light has no back: it is hit from above as well
    for p, seed in ((0, 70), (1, 71), (2, 72)):
        pos, r = AREA_LIGHTS[p, :3], AREA_LIGHTS[p, 7]
        O, D = aimed_rays(350, seed, pos, 1.5 * r, pos)
        add("random%d" % p, "mixed", p, O, D)
    r = c.done(dict(prim=np.int32))
    r["prims"] = AREA_LIGHTS
    return r


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _normalize(v):
    v = f32(v)
    return v * f32(f32(1) / np.sqrt(_dot(v, v), dtype=f32))


def cos_ang_f32(n, d):
    """dot(normalize(n), normalize(d)) in the reference's f32 operation order (template/precomp.h:835, scene.h:124)"""
    return _dot(_normalize(n), _normalize(d))


def area_intensity_cases():
    c = Cases(dict(prim=1, p=3, n=3, frm=3))
    # dis == 0: the light seen directly (+inf for a white light)
    c.add("direct_view", None, prim=[0, 1, 3], p=f32([[0, 2, 0], [4, 5, 7.5], [0.1, 2, 0.2]]), n=f32([0, 1, 0]), frm=f32([[0, 2, 0], [4, 5, 7.5], [0.1, 2, 0.2]]))
    # dis <= radius on both sides of isZero's 1e-4, a double-precision comparison of the float cosine: the float nearest 1e-4 is below it
    ys, cs = [], []
    y0 = f32(0.5e-4)
    for k in range(-40, 41):
        y = nx(y0, k)
        ys.append(y), cs.append(cos_ang_f32(f32([0, 1, 0]), f32([0.5, y, 0])))
    ys, cs = f32(ys), f32(cs)
    assert (cs == f32(1e-4)).any() and (cs > f32(1e-4)).any() and (cs < f32(1e-4)).any()
    frm = np.stack([np.full_like(ys, 0.5), ys, np.zeros_like(ys)], 1)
    c.add("near_zero_cos_at", None, prim=0, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=frm[cs == f32(1e-4)])
    c.add("near_zero_cos_below", None, prim=0, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=frm[cs < f32(1e-4)])
    c.add("near_zero_cos_above", None, prim=0, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=frm[cs > f32(1e-4)])
    c.add("near_negative_cos", None, prim=0, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=f32([[0.5, -0.2, 0], [0, -0.9, 0.1], [0.3, -1e-3, 0.3]]))
    # the same directions further away than the radius: never the flat branch
    c.add("far_zero_cos", None, prim=3, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=f32([[0.75, -0.2, 0], [2, 0, 0], [0.6, 1e-5, 0]]))
    c.add("at_radius", None, prim=0, p=f32([0, 0, 0]), n=f32([0, 1, 0]), frm=f32([[1, 0, 0], [nx(1), 0, 0], [0, -1, 0], [0, nx(-1, -1), 0]]))
    rng = np.random.default_rng(75)
    m = 600
    c.add("random", None, prim=rng.integers(0, 4, m), p=rng.uniform(-3, 3, (m, 3)), n=rng.normal(size=(m, 3)), frm=rng.uniform(-3, 3, (m, 3)))
    m = 300
    p = rng.uniform(-1, 1, (m, 3))
    c.add("random_near", None, prim=rng.integers(0, 4, m), p=p, n=rng.normal(size=(m, 3)), frm=p + rng.normal(size=(m, 3)) * 0.4)
    r = c.done(dict(prim=np.int32))
    r["prims"] = AREA_LIGHTS
    return r


def area_position_cases():
    rng = np.random.default_rng(76)
    m = 256
    seeds = rng.integers(1, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = [1, 0xFFFFFFFF, 0x12345678, 0x80000000]
    return dict(prim=(np.arange(m) % len(AREA_LIGHTS)).astype(np.int32), seed=seeds, prims=AREA_LIGHTS)


# ---- DirectionalLight -----------------------------------------------------------------------------------------------------------------
# pos(3) strength normal(3) r
DIR_LIGHTS = f32([[0, 4, 0, 3, 0, -1, 0, 0.5], [1, 3, -2, 5, 0.6, -0.8, 0, 0.25], [0, 4, 0, 2, 0, -2, 0, 0.9], [0, 0, 0, 1, 0, 0, 1, 1]]
                 + [[0, 1, 0, 1, 0, -1, 0, r] for r in (0, 0.1, 1.5, 2, -0.5, 1e-4)])


def dir_intensity_cases():
    c = Cases(dict(prim=1, p=3))
    c.add("behind", None, prim=0, p=f32([[0, 5, 0], [1, 4.5, 2], [3, 4.0001, 0]]))
    c.add("at_pos", None, prim=[0, 1], p=f32([[0, 4, 0], [1, 3, -2]]))
    # sinAngle - sTheta across 0: points on the cone of half-angle asin(sin(r PI / 2)) = 45 degrees below light 0, a few steps either side
    xs = f32([nx(2, k) for k in range(-6, 7)] + [1.9, 2.1])
    c.add("cone_edge", None, prim=0, p=np.stack([xs, np.full_like(xs, 2), np.zeros_like(xs)], 1))
    c.add("inside", None, prim=0, p=f32([[0, 0, 0], [0.5, 1, 0.5], [0, 3.5, 0.1]]))
    c.add("outside", None, prim=0, p=f32([[5, 3, 0], [0, 3.9, 3]]))
    rng = np.random.default_rng(77)
    m = 500
    c.add("random", None, prim=rng.integers(0, 4, m), p=rng.uniform(-4, 4, (m, 3)) + f32([0, 1, 0]))
    r = c.done(dict(prim=np.int32))
    r["prims"] = DIR_LIGHTS
    return r


# ---- glass ----------------------------------------------------------------------------------------------------------------------------
IORS = f32([0.8, 1.0, 1.5, 2.4])


def fresnel_cases():
    c = Cases(dict(I=3, N=3, ior=1))
    N = f32([0, 1, 0])
    for ior in IORS:
        c.add("cosi_-1_0_1@%g" % ior, None, I=f32([[0, -1, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1], [0, -2, 0], [0, 3, 0]]), N=N, ior=ior)
        for side in (-1, 1):  # cosi < 0: entering; cosi > 0: leaving
            th = np.linspace(0.01, np.pi / 2 - 0.01, 24)
            eta = (1 / float(ior)) if side < 0 else float(ior)  # etai / etat
            crit = np.arcsin(1 / eta) if eta > 1 else None
            if crit is not None:
                th = np.concatenate([th, crit + np.linspace(-2e-6, 2e-6, 33), crit + np.array([-1e-3, 1e-3, -0.1, 0.1])])
            I = np.stack([np.sin(th), side * np.cos(th), np.zeros_like(th)], 1).astype(f32)
            c.add("sweep%+d@%g" % (side, ior), "mixed" if crit is not None else "miss", I=I, N=N, ior=ior)  # 'hit' here: total internal reflection, kr == 1
    rng = np.random.default_rng(80)
    m = 800
    I = rng.normal(size=(m, 3))
    Nn = rng.normal(size=(m, 3))
    c.add("random", None, I=I / np.sqrt((I ** 2).sum(1, keepdims=True)), N=Nn / np.sqrt((Nn ** 2).sum(1, keepdims=True)), ior=IORS[rng.integers(0, 4, m)])
    return c.done()


def refract_cases():
    c = Cases(dict(D=3, N=3, ratio=1))
    N = f32([0, 1, 0])
    # dot(-D, N) above 1: the fmin clamp
    c.add("clamp", None, D=f32([[0, -1.5, 0], [0.1, -2, 0], [0, nx(-1, -1), 0], [0, -1, 0]]), N=N, ratio=f32([1 / 1.5, 1.5, 1, 0.8]))
    # |perpendicular| = ratio sin(theta) near 1: the fabs(1 - len^2) under the root changes sign
    for ratio in (f32(1.5), f32(2.4), f32(1.25), f32(1.0)):
        crit = np.arcsin(min(1.0, 1 / float(ratio)))
        th = np.concatenate([crit + np.linspace(-4e-6, 4e-6, 33), crit + np.array([-1e-2, -1e-3, 1e-3, 1e-2])])
        th = th[(th > 0) & (th < np.pi / 2)]
        D = np.stack([np.sin(th), -np.cos(th), np.zeros_like(th)], 1).astype(f32)
        c.add("len_near_1@%g" % ratio, None, D=D, N=N, ratio=ratio)
    rng = np.random.default_rng(81)
    m = 800
    D = rng.normal(size=(m, 3))
    Nn = rng.normal(size=(m, 3))
    c.add("random", None, D=D / np.sqrt((D ** 2).sum(1, keepdims=True)), N=Nn / np.sqrt((Nn ** 2).sum(1, keepdims=True)),
          ratio=np.concatenate([IORS, 1 / IORS]).astype(f32)[rng.integers(0, 8, m)])
    return c.done()


# ---- diffuse::scatter, metal::scatter -------------------------------------------------------------------------------------------------
def diffuse_cases():
    rng = np.random.default_rng(82)
    m = 600
    unit = lambda a: a / np.sqrt((a ** 2).sum(1, keepdims=True))
    mat = np.concatenate([rng.choice([0.0, 0.3, 0.7, 0.8, 1.0], (m, 3)), rng.uniform(0, 1, (m, 2)), rng.choice([0, 1, 2, 4, 10, 50, 1200], (m, 1))], 1)
    nrm = unit(rng.normal(size=(m, 3)))
    D = unit(rng.normal(size=(m, 3)))
    light = unit(nrm + rng.normal(size=(m, 3)) * 0.7)
    light[::3] = (D - 2 * nrm * (D * nrm).sum(1, keepdims=True))[::3]  # the mirror direction: the specular lobe's peak
    energy = rng.choice([1.0, 0.8, 0.5, 0.2, 0.1, 0.0], (m, 1)) * np.ones((m, 3))
    return dict(mat=mat.astype(f32), O=rng.uniform(-2, 2, (m, 3)).astype(f32), D=D.astype(f32), t=rng.uniform(0.1, 9, m).astype(f32),
                lightDir=light.astype(f32), lightInt=rng.uniform(0, 6, (m, 3)).astype(f32), nrm=nrm.astype(f32), energy=energy.astype(f32))


def metal_cases():
    rng = np.random.default_rng(83)
    m = 400
    unit = lambda a: a / np.sqrt((a ** 2).sum(1, keepdims=True))
    nrm = unit(rng.normal(size=(m, 3)))
    D = unit(rng.normal(size=(m, 3)))
    D[:8] = -nrm[:8]                                   # head on
    D[8:16] = unit(np.cross(nrm[8:16], [0.3, 0.5, 0.8]))  # grazing: dot(reflected, normal) near 0
    return dict(O=rng.uniform(-2, 2, (m, 3)).astype(f32), D=D.astype(f32), t=rng.uniform(0.1, 9, m).astype(f32), nrm=nrm.astype(f32))


# ---- Camera ---------------------------------------------------------------------------------------------------------------------------
def camera_pixels():
    px = [(0, 0), (CAM_W - 1, 0), (0, CAM_H - 1), (CAM_W - 1, CAM_H - 1), (CAM_W // 2, CAM_H // 2), (CAM_W // 2, CAM_W // 2 % CAM_H)]
    for y in (0, 199, 300, 399):
        px += [(x, y) for x in range(0, CAM_W, 8)]
    px += [(x, y) for y in range(17, CAM_H, 40) for x in range(13, CAM_W, 40)]
    px = np.unique(np.array(px, np.int32), axis=0)
    assert len(px) <= 4096
    return np.ascontiguousarray(px[:, 0]), np.ascontiguousarray(px[:, 1])


def cameras():
    """rows of camPos(3) topLeft(3) topRight(3) bottomLeft(3) fishEye viewAngle yAngle"""
    asp = f32(CAM_W) / f32(CAM_H)
    default = [0, 1, -2, -asp, 2, 0, asp, 2, 0, -asp, 0, 0]
    skewed = [0.7, 1.9, -3.1, -1.2, 2.6, 0.4, 1.9, 2.2, -0.3, -1.5, 0.3, 0.9]  # off-axis: the screen is neither centred on nor square to the view axis
    cams = [default + [0, 0.25, 0], skewed + [0, 0.25, 0]]
    for va in (0.11, 0.25, 0.4, 0.99):
        for ya in (0, 0.3, -1.2):
            cams.append(default + [1, va, ya])
    cams.append(skewed + [1, 0.4, 0.3])
    return f32(cams)


# ---- Scene::GetSkyColor ---------------------------------------------------------------------------------------------------------------
def sky_cases():
    rng = np.random.default_rng(90)
    img = rng.integers(0, 256, (9, 16, 3)).astype(np.uint8)
    D = random_rays(700, 91)[1]
    extra = f32([[0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 0.6, 0.8], [0, -0.6, -0.8], [1e-20, -1, 0], [0, -1, 1e-20]])  # unit length only: a longer D indexes past the image (:1321-1322)
    return dict(img=img, D=np.concatenate([extra, D]).astype(f32), n_straight=2)


def expect_ok(hit, fam):
    """the property each family was listed for, checked on a record of hits (bool per case): the names of the families that miss it"""
    bad = []
    for name, a, b, expect in fam:
        h = np.asarray(hit[a:b], bool)
        ok = {"hit": h.all(), "miss": not h.any(), "mixed": min(h.mean(), 1 - h.mean()) >= 0.2 if expect == "mixed" else True, None: True}[expect]
        if not ok:
            bad.append("%s: %d of %d hit, listed as %s" % (name, h.sum(), b - a, expect))
    return bad


# ---- one caller for both libraries ---------------------------------------------------------------------------------------------------
def all_cases():
    return dict(tri=triangle_cases(), sph=sphere_cases(), pla=plane_cases(), area=area_intersect_cases(), area_int=area_intensity_cases(),
                area_pos=area_position_cases(), dirl=dir_intensity_cases(), fresnel=fresnel_cases(), refract=refract_cases(),
                diffuse=diffuse_cases(), metal=metal_cases(), sky=sky_cases())


def answers(L, prefix, cs=None, sky=True):
    """Every leaf function's answer to every case, from a library that exports the entry points of oracle/ref/ref_leaf.cpp under 'prefix'
    ('ref_' for the reference's compiled code, 'orc_leaf_' for the oracle's own functions): a flat dict of arrays, float outputs as f32."""
    import ctypes as C
    cs = cs or all_cases()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = lambda name: getattr(L, prefix + name)
    out = {}

    def rays(kind, name, c, prims):
        n = len(c["O"])
        pr = np.ascontiguousarray(prims[c["prim"]])
        hit, t, nrm, occ = np.zeros(n, np.int32), np.zeros(n, f32), np.zeros((n, 3), f32), np.zeros(n, np.int32)
        args = ([P(np.ascontiguousarray(pr[:, :3])), P(np.ascontiguousarray(pr[:, 3]))] if kind in ("sphere", "plane") else [P(pr)]) + [P(c["O"]), P(c["D"]), P(c["tmax"]), P(c["tmin"])]
        fn(kind + "_intersect")(n, *args, P(hit), P(t), P(nrm))
        out[name + "_hit"], out[name + "_t"], out[name + "_nrm"] = hit != -1, t, nrm
        if kind != "area":
            fn(kind + "_occluding")(n, *args, P(occ))
            out[name + "_occ"] = occ != 0

    c = cs["tri"]
    rays("tri", "tri", c, c["prims"])
    k = len(c["prims"])
    N, cen = np.zeros((k, 3), f32), np.zeros((k, 3), f32)
    fn("tri_ctor")(k, P(c["prims"]), P(N), P(cen))
    out["tri_N"], out["tri_centroid"] = N, cen
    c = cs["sph"]
    rays("sphere", "sph", c, c["prims"])
    pr = np.ascontiguousarray(c["prims"][c["prim"]])
    I = np.ascontiguousarray(c["O"] + c["D"] * f32(1.5))  # any points will do: GetNormal asks nothing of them
    nrm = np.zeros_like(I)
    fn("sphere_normal")(len(I), P(np.ascontiguousarray(pr[:, :3])), P(np.ascontiguousarray(pr[:, 3])), P(I), P(nrm))
    out["sph_getnormal"] = nrm
    c = cs["pla"]
    rays("plane", "pla", c, c["prims"])
    c = cs["area"]
    rays("area", "area", c, c["prims"])
    c = cs["area_int"]
    rgb = np.zeros((len(c["p"]), 3), f32)
    fn("area_intensity")(len(rgb), P(np.ascontiguousarray(c["prims"][c["prim"]])), P(c["p"]), P(c["n"]), P(c["frm"]), P(rgb))
    out["area_int"] = rgb
    c = cs["area_pos"]
    pos, after = np.zeros((len(c["seed"]), 3), f32), np.zeros(len(c["seed"]), np.uint32)
    fn("area_position")(len(after), P(np.ascontiguousarray(c["prims"][c["prim"]])), P(c["seed"]), P(pos), P(after))
    out["area_pos"], out["area_pos_seed"] = pos, after
    c = cs["dirl"]
    sa = np.zeros(len(c["prims"]), f32)
    fn("dir_ctor")(len(sa), P(c["prims"]), P(sa))
    rgb = np.zeros((len(c["p"]), 3), f32)
    fn("dir_intensity")(len(rgb), P(np.ascontiguousarray(c["prims"][c["prim"]])), P(c["p"]), P(rgb))
    out["dir_sin"], out["dir_int"] = sa, rgb
    c = cs["fresnel"]
    kr = np.zeros(len(c["ior"]), f32)
    fn("glass_fresnel")(len(kr), P(c["I"]), P(c["N"]), P(c["ior"]), P(kr))
    out["fresnel_kr"] = kr
    c = cs["refract"]
    v = np.zeros_like(c["D"])
    fn("glass_refract")(len(v), P(c["D"]), P(c["N"]), P(c["ratio"]), P(v))
    out["refract"] = v
    c = cs["diffuse"]
    att, en, so = np.zeros_like(c["O"]), np.zeros_like(c["O"]), np.zeros_like(c["O"])
    fn("diffuse_scatter")(len(att), P(c["mat"]), P(c["O"]), P(c["D"]), P(c["t"]), P(c["lightDir"]), P(c["lightInt"]), P(c["nrm"]), P(c["energy"]), P(att), P(en), P(so))
    out["diffuse_att"], out["diffuse_energy"], out["diffuse_O"] = att, en, so
    c = cs["metal"]
    mo, md, ret = np.zeros_like(c["O"]), np.zeros_like(c["O"]), np.zeros(len(c["O"]), np.int32)
    fn("metal_scatter")(len(ret), P(c["O"]), P(c["D"]), P(c["t"]), P(c["nrm"]), P(mo), P(md), P(ret))
    out["metal_O"], out["metal_D"], out["metal_ret"] = mo, md, ret != 0
    xs, ys = camera_pixels()
    cams = cameras()
    D = np.zeros((len(cams), len(xs), 3), f32)
    for i, cam in enumerate(cams):
        O = np.zeros((len(xs), 3), f32)
        fn("camera_rays")(P(np.ascontiguousarray(cam)), len(xs), P(xs), P(ys), P(O), P(D[i]))
        assert np.array_equal(O, np.broadcast_to(cam[:3], O.shape))
    out["cam_D"] = D
    if sky:
        c = cs["sky"]
        rgb = np.zeros_like(c["D"])
        h, w, nch = c["img"].shape
        fn("sky_color")(w, h, nch, P(c["img"]), len(rgb), P(c["D"]), P(rgb))
        out["sky_rgb"] = rgb
    return out


def same_bits(a, b):
    """per element: equal bits, or NaN on both sides (NaNs compare by class, as conftest.rel_err defines class)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a == b
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def flat_inputs(cs):
    """the inputs of all_cases() as a flat dict of arrays (what the golden file keeps beside the answers)"""
    out = {}
    for kind, c in cs.items():
        for k, v in c.items():
            if k != "fam" and not np.isscalar(v):
                out["in_%s_%s" % (kind, k)] = np.asarray(v)
    out["in_cam_xs"], out["in_cam_ys"] = camera_pixels()
    out["in_cam_rows"] = cameras()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- scenes that hand a ray to one leaf test ------------------------------------------------------------------------------------------
FAR_TRIANGLE = f32([[5000, 5000, 5000, 5001, 5000, 5000, 5000, 5001, 5000]])  # something for an accelerator to hold that no ray of the cases meets


def one_primitive(scene, kind, prim):
    """One triangle (as a mesh), sphere or plane behind a BVH: the root is a leaf, so bvh::Intersect / IsOccluded are the leaf test alone, at
    the BVH's own t_min (BVH_TMIN).  'scene' follows the builder protocol of the oracle's and the host's scene wrappers."""
    m = scene.diffuse(0.8, (1, 1, 1))
    if kind == "tri":
        scene.mesh_raw(1, m, np.asarray(prim, f32).reshape(1, 9))
    elif kind == "sph":
        scene.sphere(5, m, prim[:3], float(prim[3]))
    else:
        scene.plane(3, m, prim[:3], float(prim[3]))
    scene.build(0)


def callers_t_min(scene, kind, prim):
    """One sphere or plane tested by brute force beside a TLAS (template/scene.h:1260-1261), or one area light before a BVH (:1257): the two
    places where Scene::FindNearest hands the caller's t_min to a leaf test.  The accelerator holds FAR_TRIANGLE."""
    m = scene.diffuse(0.8, (1, 1, 1))
    mesh = scene.mesh_raw(1, m, FAR_TRIANGLE)
    if kind == "area":
        scene.area_light(11, prim[:3], float(prim[3]), prim[4:7], float(prim[7]), prim[8:11])
        scene.build(0)
        return
    if kind == "sph":
        scene.sphere(5, m, prim[:3], float(prim[3]))
    else:
        scene.plane(3, m, prim[:3], float(prim[3]))
    scene.build_tlas(0, [(mesh, scene.trs((0, 0, 0), 1.0, 0.0, 0.0, 0.0)), (mesh, scene.trs((3, 0, 0), 1.0, 0.0, 0.0, 0.0)), (mesh, scene.trs((0, 0, 7), 2.0, 0.0, 0.0, 0.0))])


def check_callers_t_min(new_scene, gold, kinds=("sph", "pla", "area")):
    """new_scene(build) -> (find_nearest(O, D, tmax, t_min) -> dict(t, obj, normal), close): every row of the record for these kinds, at the
    t_min the row names, through Scene::FindNearest of a callers_t_min scene; returns how many rows went through"""
    seen = 0
    for kind in kinds:
        g = lambda k: gold["out_%s_%s" % (kind, k)]
        i_ = lambda k: gold["in_%s_%s" % (kind, k)]
        for p in range(len(i_("prims"))):
            find, close = new_scene(lambda sc: callers_t_min(sc, kind, i_("prims")[p]))
            for tm in (AREA_TMINS if kind == "area" else TMINS):
                rows = np.where((i_("prim") == p) & (i_("tmin") == tm))[0]
                if not len(rows):
                    continue
                got = find(i_("O")[rows], i_("D")[rows], i_("tmax")[rows], float(tm))
                hit = g("hit")[rows]
                assert np.array_equal(got["obj"] != -1, hit), (kind, p, tm)
                assert same_bits(got["t"], g("t")[rows]).all(), (kind, p, tm)
                assert same_bits(got["normal"][hit], g("nrm")[rows][hit]).all(), (kind, p, tm)
                seen += len(rows)
            close()
    return seen
