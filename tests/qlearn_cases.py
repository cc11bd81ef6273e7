"""Crafted tables, cells and hits for the Q-learning guided sampler (csrc/rt_qlearn.h, the QL branch of k_shade_s).  A plain helper module
of the test suite, numpy only: tests/test_qlearn_cpu.py shows on the oracle alone that every input reaches the cell and the branch it is
listed for and that its twin pays other rewards; tests/test_gpu_qlearn.py holds the device to the oracle, and to the restatement
tests/qlearn_ref.py, on the same inputs.

Rays go through rt_trace_batch: ray i of a batch draws from StreamSeed(SEED_BASE + i) and learns iff that state & learn_mask == 0.
A primary ray goes straight down onto the plane y = 0, so t and the hit point are exact; every ray is repeated REPS times, as the shade
tier repeats its rays (other streams: other picks).

Boxes have a power of two as the cell size on every axis -- (1/2, 1/4, 1): not a cube -- so (x - lo) * inv is exact and a hit point on a
cell face belongs to the upper cell by the definition, with no rounding to hide behind.  'face': y = 0 is a cell face inside the grid
(grid 1 has none: there it is lo); 'lo': the box starts at y = 0."""
import numpy as np

import qlearn_ref as qr
from shade_cases import sky_pixels

f32 = np.float32
SEED_BASE = 4242
REPS = 16
CELL = (0.5, 0.25, 1.0)
GRIDS = (1, 3, 64)
MASKS = (0, 3, 0xFFFFFFFF)
EPS, Q_INIT = 0.2, 1.0
FLOOR_ALBEDO, FLOOR_COL = 0.8, (1.0, 0.8, 0.7)


def box(grid, kind):
    """(lo, hi) of the 'face' or the 'lo' box of a grid"""
    k = grid // 2
    # (x: two cells further down, so that x - lo is exact next to the first inner face: |x - lo| < |x| there)
    lo = np.array([-(k + 2) * CELL[0], 0.0 if kind == "lo" else -k * CELL[1], -k * CELL[2]], f32)
    return lo, (lo + f32(grid) * np.array(CELL, f32)).astype(f32)


def _down(x, z, y=2.0):
    return (np.array([x, y, z], f32), np.array([0, -1, 0], f32))


def _ulp(x, up):
    return float(np.nextafter(f32(x), f32(np.inf if up else -np.inf)))


def floor_points(grid, kind):
    """{name: (x, z)} on the floor: on a cell face in x, one ulp to either side of it, at lo and at hi (and one ulp inside hi), and outside
    the box on all four sides; z is inside a cell unless it is the coordinate that leaves the box"""
    lo, hi = box(grid, kind)
    face = float(lo[0]) + CELL[0]   # the first face inside the grid (grid 1: hi itself)
    zin = float(lo[2]) + 0.25 * CELL[2]
    xin = float(lo[0]) + 0.25 * CELL[0]
    pts = {"face": (face, zin), "face-": (_ulp(face, False), zin), "face+": (_ulp(face, True), zin),
            "lo": (float(lo[0]), zin), "lo-": (_ulp(lo[0], False), zin), "hi": (float(hi[0]), zin), "hi-": (_ulp(hi[0], False), zin),
            "out-x": (float(lo[0]) - 3.0, zin), "out+x": (float(hi[0]) + 3.0, zin),
            "out-z": (xin, float(lo[2]) - 3.0), "out+z": (xin, float(hi[2]) + 3.0), "z-hi": (xin, float(hi[2]))}
    if lo[0] < 0 < hi[0]:   # the face x = 0 from one ulp below: x - lo rounds onto the face, and the point belongs to the upper cell
        pts["round"] = (_ulp(0.0, False), zin)
    return pts


def expected_cell_xz(grid, kind, name):
    """the (ix, iz) the definition gives the point 'name' -- written down by hand, not computed: what floor_points is for"""
    g = grid - 1
    return {"face": (min(1, g), 0), "face-": (0, 0), "face+": (min(1, g), 0), "round": (grid // 2 + 2, 0), "lo": (0, 0), "lo-": (0, 0), "hi": (g, 0), "hi-": (g, 0),
            "out-x": (0, 0), "out+x": (g, 0), "out-z": (0, 0), "out+z": (0, g), "z-hi": (0, g)}[name]


def expected_cell_y(grid, kind):
    """the iy of the floor y = 0: the cell above the face, or the first one"""
    return 0 if kind == "lo" else grid // 2


def rays_of(points, reps=REPS):
    O, D, where, at = [], [], {}, 0
    for name, (x, z) in points.items():
        o, d = _down(x, z)
        O += [o] * reps
        D += [d] * reps
        where[name] = slice(at, at + reps)
        at += reps
    return np.stack(O).astype(f32), np.stack(D).astype(f32), where


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def floor(b, rt=True, twin=None):
    """one diffuse floor under the sky, no lights: a guided pick is the only thing that draws"""
    b.sky(sky_pixels())
    b.plane(0, b.diffuse(FLOOR_ALBEDO, (0.5, 0.8, 0.7) if twin == "col" else FLOOR_COL, rt=rt), (0, 1, 0), 0)
    b.build(0)
    return dict(name="floor", tlas=False)


R2 = float(f32(np.sqrt(0.5)))
# (normal, d, the patch the definition gives the normal -- by hand): planes around the origin whose normals sit on the sector
# boundaries and at both poles.  Plane::Intersect reports N as given, from either side.
TILT_PLANES = [
    ((0.0, 0.0, -1.0), 1.5, 0),            # the lower pole: band 0, sector 0
    ((0.0, 0.0, 1.0), 1.5, 56),            # the upper pole: band 7 (z = 1 is held inside), sector 0
    ((-0.5, -0.5, -R2), 3.0, 8 * 1 + 5),   # |x| = |y| below: the tie goes to the later sector
    ((0.5, -0.5, R2), 3.0, 8 * 6 + 7),
    ((0.0, -1.0, 0.0), 4.0, 8 * 4 + 6),    # x = 0 below: the quadrant on its right
    ((-0.6, -0.0, -0.8), 2.0, 8 * 0 + 3),  # y = -0.0: the upper half-plane
    ((0.5, 0.5, -R2), -3.0, 8 * 1 + 1),    # |x| = |y| above
    ((-0.5, 0.5, R2), -3.0, 8 * 6 + 3),
    ((0.0, 0.6, 0.8), -3.0, 8 * 7 + 2),    # x = 0 above: the later sector again; z = 0.8: the last band's lower edge is 0.75
]
TILT_BOX = (np.array([-4, -1, -4], f32), np.array([4, 7, 4], f32))   # grid 4: cells of 2 -- the planes cross many of them
TILT_GRID = 4
TILT_POINTS = {"a": (0.25, 0.5), "b": (-1.5, 0.25), "c": (1.25, -1.0), "d": (-0.5, -1.25), "e": (0.75, 1.0), "f": (-0.25, -0.5)}
TILT_REPS = 48


def tilt(b, rt=True, twin=None):
    """the floor inside tilted diffuse planes: every guided child that leaves the floor meets one of them (or the sky), and its reward
    is the V row of the hit's cell at the patch of the plane's normal.  Twin 'nudge': every normal moved off its boundary."""
    b.sky(sky_pixels())
    b.plane(0, b.diffuse(FLOOR_ALBEDO, FLOOR_COL, rt=rt), (0, 1, 0), 0)
    m = b.diffuse(0.9, (0.9, 1.0, 0.6), rt=rt)
    for k, (N, d, _) in enumerate(TILT_PLANES):
        if twin == "nudge":
            N = (N[0] + 0.05, N[1] - 0.03, N[2] * 0.9)
        b.plane(1 + k, m, N, d)
    b.build(0)
    return dict(name="tilt", tlas=False)


TILT_MATS = {0: (FLOOR_ALBEDO, FLOOR_COL)}
TILT_MATS.update({1 + k: (0.9, (0.9, 1.0, 0.6)) for k in range(len(TILT_PLANES))})

KIND_X = {"sky": 40.0, "light": 0.0, "glass": 10.0, "metal": 20.0, "diffuse": 30.0}
KIND_BOX = (np.array([-4, -1, -4], f32), np.array([44, 5, 4], f32))
KIND_GRID = 6


def kinds(b, rt=True, twin=None):
    """what a guided child can hit, each above its own stretch of the floor: nothing (the sky), an area light's disk, a glass sphere, a
    metal sphere, a diffuse sphere.  The primary ray starts below the object.  Twin 'away': every object lifted out of reach."""
    up = 50.0 if twin == "away" else 0.0
    b.sky(sky_pixels())
    b.area_light(11, (KIND_X["light"] + 20 * up, 0.5 + up, 0.0), 6.0, (1, 1, 1), 3.0, (0, -1, 0))
    b.plane(0, b.diffuse(FLOOR_ALBEDO, FLOOR_COL, rt=rt), (0, 1, 0), 0)
    b.sphere(1, b.glass(1.5, (0.9, 0.8, 1.0), (0.3, 0.0, 0.6), rt=rt), (KIND_X["glass"], 2.0 + up, 0.0), 1.5)
    b.sphere(2, b.metal(0.7, (1.0, 0.6, 0.3), rt=rt), (KIND_X["metal"], 2.0 + up, 0.0), 1.5)
    b.sphere(3, b.diffuse(0.7, (0.6, 1.0, 0.9), rt=rt), (KIND_X["diffuse"], 2.0 + up, 0.0), 1.5)
    b.build(0)
    return dict(name="kinds", tlas=False)


def kind_rays(reps=2 * REPS):
    pts = {k: (x + 0.125, 0.25) for k, x in KIND_X.items()}
    O, D, where, at = [], [], {}, 0
    for name, (x, z) in pts.items():
        o, d = _down(x, z, 0.25)   # from below the object: t = 1/4 and the hit point are exact
        O += [o] * reps
        D += [d] * reps
        where[name] = slice(at, at + reps)
        at += reps
    return np.stack(O).astype(f32), np.stack(D).astype(f32), where


SCENES = {"floor": floor, "tilt": tilt, "kinds": kinds}


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def table_sums(name, cells, seed=7):
    """(sums, counts) whose fold with alpha = 1 into any table gives the crafted table 'name': a value v (a multiple of 2^-16) is the sum
    v * 65536 with count 1, Q_MIN is the sum 0 with count 1 (the floor)"""
    rng = np.random.default_rng(seed)
    sums = np.zeros((cells, 64), np.int64)
    if name == "peak":      # one patch at 64 -- another one in every cell -- and the rest at Q_MIN
        sums[np.arange(cells), (np.arange(cells) * 11 + 37) % 64] = 64 << 16
    elif name == "band":    # one band entirely at Q_MIN, the rest between 1/4 and 4
        sums[:] = rng.integers(1 << 14, 1 << 18, (cells, 64))
        for c in range(cells):
            sums[c, 8 * (c % 8): 8 * (c % 8) + 8] = 0
    elif name == "equal":
        sums[:] = 2 << 16
    elif name == "random":  # every value its own, between 2^-16 and 8
        sums[:] = rng.integers(1, 1 << 19, (cells, 64))
    else:
        raise KeyError(name)
    return sums, np.ones((cells, 64), np.uint32)


TABLES = ("peak", "band", "equal", "random")


_TABLES = {}


def table(name, cells):
    """the crafted table (made once, never written to)"""
    if (name, cells) not in _TABLES:
        s, c = table_sums(name, cells)
        _TABLES[name, cells] = qr.apply(np.full((cells, 64), f32(Q_INIT)), s, c, 1.0)[0]
        _TABLES[name, cells].setflags(write=False)
    return _TABLES[name, cells]


# ---- part A: crafted pending sums -------------------------------------------------------------------------------------------------------
APPLY_GRIDS = (1, 2, 5, 64)
ALPHAS = (1.0, 0.3, 2.0 ** -20)
ENTRIES = {  # name: (sum, count)
    "unpaid": (12345, 0),                       # count 0 with a sum: the table untouched, the pending sum stays
    "zero": (0, 1),                             # towards 0: repeated, it ends on the floor
    "full": (5 * 64 * 65536, 5),                # sum = count * 64 * 65536
    "third": (1, 3),
    "huge": (1 << 62, 0xFFFFFFFF),
    "negative": (-(1 << 62), 1),               # the floor
}


def crafted_sums(cells, seed=3):
    """every entry of ENTRIES at a seeded place of every cell (the first six patches of a permutation), seeded sums elsewhere with
    counts 0 .. 3"""
    rng = np.random.default_rng(seed)
    sums = rng.integers(0, 1 << 24, (cells, 64)).astype(np.int64)
    counts = rng.integers(0, 4, (cells, 64)).astype(np.uint32)
    at = {}
    for k, (name, (s, n)) in enumerate(ENTRIES.items()):
        p = (np.arange(cells) * 5 + 9 * k) % 64   # (9 k mod 64 for k < 6 are all different)
        sums[np.arange(cells), p], counts[np.arange(cells), p] = s, n
        at[name] = p
    return sums, counts, at


# ---- the prediction: diffuse surfaces, no lights ----------------------------------------------------------------------------------------
def predict(q, grid, lo, hi, mask, oscene, mats, O, D, depth, eps=EPS):
    """(sums, counts, the per-ray record of the first pick) a batch leaves behind on a scene of diffuse surfaces without lights, from
    tests/qlearn_ref.py and the oracle's geometry alone (find_nearest, sky_color): what Sample pays, restated as a loop over hit levels.
    mats: objIdx -> (albedo, col)."""
    n = len(O)
    q = np.asarray(q, f32)
    sums, counts = np.zeros((grid ** 3, 64), np.int64), np.zeros((grid ** 3, 64), np.uint32)
    state = qr.stream_seed((SEED_BASE + np.arange(n)).astype(np.uint32))
    learner = (state & np.uint32(mask)) == 0
    alive = np.ones(n, bool)
    key = np.full(n, -1, np.int64)   # cell * 64 + patch of the pick that sent the ray
    O, D = np.array(O, f32), np.array(D, f32)
    first = None

    def pay(who, keys, fixed):
        np.add.at(sums.reshape(-1), keys[who], fixed[who] if np.ndim(fixed) else fixed)
        np.add.at(counts.reshape(-1), keys[who], 1)
    for level in range(depth, -1, -1):
        hit = oscene.find_nearest(O, D, t_min=0.001)
        sky = alive & (hit["obj"] == -1)
        owes = learner & (key >= 0)
        if sky.any():
            R = qr.lum(oscene.sky_color(D))
            pay(sky & owes, key, qr.reward_fixed(R))
        alive = alive & ~sky
        I = (O + hit["t"][:, None] * D).astype(f32)
        cells = qr.cell(grid, lo, hi, I)
        rho = np.zeros(n, f32)
        for obj, (albedo, col) in mats.items():
            rho[hit["obj"] == obj] = qr.lum(np.array(col, f32) * f32(albedo))
        met, back = np.unique(cells, return_inverse=True)   # (the V rows of the cells that were met: a grid of 64 has 262144 of them)
        v = qr.derive(q[met])[1][back.reshape(-1), qr.patch_of(hit["normal"])]
        R = rho * (v * f32(1.0 / 16))
        pay(alive & owes, key, qr.reward_fixed(R))
        pick = qr.sample(q[cells], eps, state)
        state = pick["state"]
        N = hit["normal"]
        c = (pick["dir"][:, 0] * N[:, 0] + pick["dir"][:, 1] * N[:, 1]) + pick["dir"][:, 2] * N[:, 2]
        dead = ~(c > 0)
        key = cells * 64 + pick["patch"]
        if first is None:
            first = dict(cell=cells, patch=pick["patch"], dead=dead, branch=pick["branch"], last_band=pick["last_band"],
                         last_sector=pick["last_sector"], learner=learner.copy(), dir=pick["dir"], P=pick["P"])
        pay(alive & dead & learner, key, 0)
        alive = alive & ~dead
        O, D = I, pick["dir"]
    return sums, counts, first
