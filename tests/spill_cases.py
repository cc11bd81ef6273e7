"""Scenes and seeded ray sets that drive the traversal stack (csrc/rt_scene_dev.h Stack) through its LDS rows into the spill buffer, shared
by tests/test_spill_cpu.py (conditions on these inputs, on the oracle alone) and tests/test_gpu_spill.py (the device against the oracle on
the same rays).  A plain helper module of the test suite, numpy only; the row counts come from the host-only layout builder
(host_api.layout), the peaks from the oracle's tally (OracleScene.stack_peaks), nothing here is read from a device.

The chain mesh: triangle i has the vertices (x, 0, 0), (x, w, 0), (1.1 x, w / 2, w) with x = x0 * 2^i.  Built with split method 2
(LONGESTAXIS) the tree peels the LARGEST triangle per level: depth n for n triangles.  A ray along +x from in front of the first triangle
passes every box; at every level it descends into the near child and pushes the far leaf: its stack pointer peaks at n - 1, for the
nearest-hit and the any-hit walk alike (the descent to the bottom comes before the first leaf test).  Started between triangles k - 1 and
k it peaks at n - 1 - k.  Directions are (1, +-tilt, +-tilt): every component finite and non-zero, no slab product is 0 x inf, and the
drift over the whole chain stays far below the triangles' extent.  55 % of such rays hit a triangle, the others pop every entry and miss.

Groups of a set (interleaved by a seeded permutation, so lanes of one wave refill while their neighbours are deep; no set's size is a
multiple of 64).  'peak' is the stacked peak (the TLAS pointer at an instance's entry + 1 + the pointer inside the BLAS: what the device's
one stack holds), equal for both walks, measured on the oracle and asserted by tests/test_spill_cpu.py:

  chains without a TLAS (rows = 14, general kernels 16); n triangles, x0 = 2, w = 1
    case        n    deep   shallow (starts before the last two triangles)   reversed (-x, from beyond the last triangle)
    chain_p13   14   13     1                                                1
    chain_p14   15   14     1      (the last LDS row, no spill)              1
    chain_p15   16   15     1      (the first spill entry)                   1
    chain_p17   18   17     1      (past the general kernels' 16 rows)       1
    chain_p23   24   23     1                                                1
    chain_p61   62   61     1                                                38  (2^62 apart the boxes' entry distances tie, and a tie
                                                                                  descends into the inner node first)
    twin_p23    48   23     0 / 1 by column                                  11 / 12 by column
  twin_p23 is two chains side by side (triangle i in column i % 2, the columns 2 w apart along y, rays in either column): a ray passes
  the inner boxes, which span both columns, and the leaves of its own column only, so at the same stack position the lanes of a wave
  hold DIFFERENT links.  On the one-column chains every deep ray pushes the same link at the same position, and a walk that read a
  neighbour lane's spill column would still answer right; here it does not.
  chains of instances: m instances, instance i translated by (e0 * 2^i, 0, 0) with e0 twice the deep mesh's largest x.  The first m - 3 hold
  the deep chain mesh (BLAS 0, n triangles), the last three a short one (BLAS 1, rows - 1 triangles).  An instance's box is the union of
  the BLAS's own box and the moved one (the reference never resets it), so every box reaches back to the origin: a ray from in front of
  everything passes all m boxes, reaches instance 0 with m - 1 TLAS entries pushed and walks its BLAS above them.  A ray that starts
  behind instance k passes only the later ones: behind m - 4, m - 3, m - 2 (three, two, one short meshes ahead) it peaks at rows + 1,
  rows, rows - 1.
    case        m    n    rows (layout)        deep   over      edge   under
    tlas_first  6    40   13  LDS copy, max    45     14        13     12
    tlas_mid    20   40   10  LDS copy         59     11        10     9
    tlas_last   37   40   8   LDS copy, min    76     9         8      7      (37 = instances_ref.smallest_n_without_lds() - 1)
    tlas_global 52   56   14  TLAS in memory   107    15        14     13     (x0 = 2^-11, w = 2^-12: every coordinate below 1.6e29)
  107 = 51 + 1 + 55 is the largest stacked depth: more than either of the reference's stack[64] arrays holds alone, 23 below RT_STACK_MAX.
  With m + n - 1 entries the largest coordinate is x0 * 2^(m + n + 1); tlas::build compares areas with 1e30 and the device calls a ray
  clean below 1e30, so x0 * w * 2^(m + n + 2) < 1e30 bounds the depth: 107 with triangles of 2^-12.  The over / edge / under rays of
  tlas_global start up to 2^98 from their instances and are axis-parallel (tilt 0: no drift, no box bound equals a ray's y or z, so no
  slab product is NaN either; such rays are not 'clean' and take the walks' literal slab test).

  large: 256 * 8 * 256 + 12,345 rays on chain_p23's scene, more than a full grid of the persistent kernels has lanes (8 blocks of 256 lanes
  on each of 256 CUs), so every block's spill columns are written: deep / shallow / reversed as above, peaks 23 / 1 / 1.
  render: 24 triangles, triangle 0 as above, the others flipped ((x, 0, 1), (x, 1, 1), (1.1 x, 0.5, 0)), a diffuse material, an area light
  beyond the far end that faces -x.  Both modes at depths 1 and 4 peak at 23.  20 % of the rays miss every triangle, see the light and
  come back +inf; of the finite ones 31 to 32 % are lit (their shadow ray passes the other 23 triangles: O(1) by the light's strength)
  and the rest dark (the shadow ray is occluded after a descent to the bottom).
  overflow: 136 triangles from x0 = 2^-40 with w = 2^-42 (the extents below the smallest x; the largest x is 1.1 * 2^95 < 1e30), rays
  along +x exactly (any tilt an f32 holds would leave the chain before its far end): the walk would peak at 135 > RT_STACK_MAX = 130.
  For the device's builder and walks alone: the oracle's stack[64] cannot hold it.

Measured on an MI355X by tests/test_gpu_spill.py ('The traversal stack under test'): every query of every case bit
for bit under the default walk, RT_WIDE=0 / 1, RT_WIDE8=1 and RT_TLAS_LDS=0, every counting-mode tally the oracle's; on the render chain the
largest relative error (floor 1e-3, bar 1e-4) is 1.4e-7 for Sample -- one set of bits under all twelve wavefront schedules, 1.4e-7 through
k_sample_general -- and 0 for Trace under the four Whitted schedules and through k_trace_general.  No kernel or host sizing had to change."""
import numpy as np

F32 = np.float32
SPLIT = 2                      # LONGESTAXIS
STACK_MAX = 130                # csrc/rt_scene_dev.h RT_STACK_MAX
GENERAL_ROWS = 16              # RT_STACK_LDS
GRID_LANES = 256 * 8 * 256     # lanes of a full grid: RT_BLOCK x 8 resident blocks x 256 CUs (rt_create: gridBlocks * RT_BLOCK)
LARGE_EXTRA = 12345
N_DEEP, N_OTHER, N_TLAS_OTHER = 1201, 401, 267
SEED_BASE, ENERGY = 4242, (0.9, 0.8, 0.7)
SHORT_INSTANCES = 3            # the last instances of an instance chain hold the short mesh


def chain_tris(n, x0=2.0, w=1.0, flipped_from=None, columns=1):
    """(n, 9) f32: the chain mesh; from triangle 'flipped_from' on with the apex at z = 0 and the base at z = w; triangle i stands in
    column i % columns, 2 w further along y per column"""
    x = x0 * 2.0 ** np.arange(n)
    o = 2.0 * w * (np.arange(n) % columns)
    z = np.zeros(n)
    t = np.stack([x, o, z, x, o + w, z, 1.1 * x, o + 0.5 * w, z + w], 1)
    if flipped_from is not None:
        t[flipped_from:, [2, 5]], t[flipped_from:, 8] = w, 0.0
    return t.astype(F32)


def translation(x):
    m = np.eye(4, dtype=F32)
    m[0, 3] = x
    return m.reshape(16)


def _chain(n, reversed_peak=1, columns=1, shallow_peak=1):
    return dict(kind="chain", n=n, x0=2.0, w=1.0, tilt=1e-21, columns=columns,
                peaks=dict(deep=n // columns - 1, shallow=shallow_peak, reversed=reversed_peak))


def _tlas(m, n, x0=2.0, w=1.0, tilt=1e-24, far_tilt=True):
    return dict(kind="tlas", m=m, n=n, x0=x0, w=w, tilt=tilt, far_tilt=far_tilt)


def last_count_with_a_copy():
    from instances_ref import smallest_n_without_lds
    return smallest_n_without_lds() - 1


CASES = {
    "chain_p13": _chain(14), "chain_p14": _chain(15), "chain_p15": _chain(16), "chain_p17": _chain(18), "chain_p23": _chain(24),
    "chain_p61": _chain(62, reversed_peak=38),
    "twin_p23": _chain(48, columns=2, shallow_peak=(0, 1), reversed_peak=(11, 12)),
    "tlas_first": _tlas(6, 40), "tlas_mid": _tlas(20, 40), "tlas_last": _tlas(last_count_with_a_copy(), 40),
    "tlas_global": _tlas(52, 56, x0=2.0 ** -11, w=2.0 ** -12, tilt=2.0 ** -70, far_tilt=False),
}
CHAINS = tuple(k for k, c in CASES.items() if c["kind"] == "chain")
TLAS = tuple(k for k, c in CASES.items() if c["kind"] == "tlas")
LARGE_SCENE = "chain_p23"
DEEPEST = "tlas_global"

_ROWS = {}


def rows_of(name, host_api):
    """(stackRows, tlasLds) of the case's scene under the default knobs, from the host-only layout builder; they follow from the
    instance count alone, so the short mesh (whose size follows from the rows) is taken with 3 triangles for this"""
    if name not in _ROWS:
        h = host_api.HostScene()
        fill(name, h, short=3)
        L = host_api.layout(h.describe())
        h.close()
        _ROWS[name] = (L["stackRows"], L["tlasLds"])
    return _ROWS[name]


def fill(name, b, host_api=None, short=None):
    """fills the builder b (OracleScene or HostScene) with the case's scene; an instance chain's short mesh has rows - 1 triangles"""
    c = CASES[name]
    mat = b.diffuse(0.8, (1, 1, 1))
    deep = b.mesh_raw(1, mat, chain_tris(c["n"], c["x0"], c["w"], columns=c.get("columns", 1)))
    if c["kind"] == "chain":
        b.build(SPLIT)
        return
    nb = short if short is not None else rows_of(name, host_api)[0] - 1
    low = b.mesh_raw(2, mat, chain_tris(nb, c["x0"], c["w"]))
    b.build_tlas(SPLIT, [(deep if i < c["m"] - SHORT_INSTANCES else low, translation(_e0(c) * 2.0 ** i)) for i in range(c["m"])])


def _e0(c):
    return c["x0"] * 2.0 ** (c["n"] + 1)


def expected_peaks(name, host_api):
    """group -> the stacked peak every ray of the group must reach"""
    c = CASES[name]
    if c["kind"] == "chain":
        return dict(c["peaks"])
    rows = rows_of(name, host_api)[0]
    return dict(deep=c["m"] + c["n"] - 1, over=rows + 1, edge=rows, under=rows - 1)


def _group(rng, n, x_start, sign, tilt, w, columns=1):
    col = rng.integers(0, columns, n) if columns > 1 else np.zeros(n)
    O = np.stack([np.full(n, x_start), (2.0 * col + rng.uniform(0.05, 0.95, n)) * w, rng.uniform(0.05, 0.95, n) * w], 1).astype(F32)
    D = np.stack([np.full(n, sign), tilt * rng.choice([-1.0, 1.0], n), tilt * rng.choice([-1.0, 1.0], n)], 1).astype(F32)
    return O, D


def _mix(rng, parts):
    """(O, D, group index per ray, group names) of the parts name -> (O, D), interleaved at random"""
    names = list(parts)
    O = np.concatenate([parts[k][0] for k in names])
    D = np.concatenate([parts[k][1] for k in names])
    g = np.concatenate([np.full(len(parts[k][0]), i, np.int32) for i, k in enumerate(names)])
    p = rng.permutation(len(O))
    assert len(O) % 64 != 0 and np.isfinite(O).all() and np.isfinite(D).all()
    return np.ascontiguousarray(O[p]), np.ascontiguousarray(D[p]), g[p], names


def _chain_parts(rng, c, n_deep, n_other):
    x0, w, n, t, k = c["x0"], c["w"], c["n"], c["tilt"], c.get("columns", 1)
    return {"deep": _group(rng, n_deep, -x0 / 2, 1.0, t, w, k),
            "shallow": _group(rng, n_other, 1.5 * x0 * 2.0 ** (n - 3), 1.0, t, w, k),
            "reversed": _group(rng, n_other, 1.5 * x0 * 2.0 ** n, -1.0, t, w, k)}


_RAYS = {}


def rays(name):
    """dict(O, D, group (index per ray), names): the case's ray set, seeded by its name, made once and never changed"""
    if name not in _RAYS:
        c = CASES[name]
        rng = np.random.default_rng(sum(name.encode()) * 7919 + 5)
        if c["kind"] == "chain":
            parts = _chain_parts(rng, c, N_DEEP, N_OTHER)
        else:
            parts = {"deep": _group(rng, N_DEEP, -c["x0"] / 2, 1.0, c["tilt"], c["w"])}
            for k, label in ((c["m"] - 4, "over"), (c["m"] - 3, "edge"), (c["m"] - 2, "under")):
                start = 1.5 * _e0(c) * 2.0 ** k   # behind instance k and its mesh, in front of instance k + 1
                parts[label] = _group(rng, N_TLAS_OTHER, start, 1.0, 2.0 ** -10 * c["w"] / start if c["far_tilt"] else 0.0, c["w"])
        O, D, g, names = _mix(rng, parts)
        for a in (O, D, g):
            a.setflags(write=False)
        _RAYS[name] = dict(O=O, D=D, group=g, names=names)
    return _RAYS[name]


def large_rays():
    """the large set on LARGE_SCENE: more rays than a full grid has lanes, plus a ragged remainder; half of them deep"""
    if "large" not in _RAYS:
        c = CASES[LARGE_SCENE]
        n = GRID_LANES + LARGE_EXTRA
        rng = np.random.default_rng(20261)
        O, D, g, names = _mix(rng, _chain_parts(rng, c, n - 2 * (n // 4), n // 4))
        for a in (O, D, g):
            a.setflags(write=False)
        _RAYS["large"] = dict(O=O, D=D, group=g, names=names)
    return _RAYS["large"]


# ---- the render chain ----------------------------------------------------------------------------------------------------------------------
RENDER_N, RENDER_PEAK, RENDER_RAYS = 24, 23, 2003
RENDER_DEPTHS = (1, 4)
LIGHT_X, LIGHT_STRENGTH = 2.0 ** 26, 2.0 ** 30   # 2^26 from the triangles: the strength brings a lit hit to O(1)


def render_chain(b, rt=True):
    """24 triangles of which all but the first are flipped, so together they cover 80 % of the rays' cross-section, and a light beyond the
    far end facing back along -x: a hit's shadow ray runs the whole chain"""
    b.area_light(11, (LIGHT_X, 0.5, 0.5), LIGHT_STRENGTH, (1, 1, 1), 2.0, (-1, 0, 0))
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1), rt=rt), chain_tris(RENDER_N, flipped_from=1))
    b.build(SPLIT)
    return dict(name="render_chain", tlas=False)


def render_rays():
    if "render" not in _RAYS:
        O, D = _group(np.random.default_rng(77), RENDER_RAYS, -1.0, 1.0, 1e-21, 1.0)
        O.setflags(write=False), D.setflags(write=False)
        _RAYS["render"] = (O, D)
    return _RAYS["render"]


# ---- past the limit ------------------------------------------------------------------------------------------------------------------------
OVERFLOW_N, OVERFLOW_X0, OVERFLOW_W = 136, 2.0 ** -40, 2.0 ** -42


def overflow_chain(b):
    """136 triangles: a +x ray would push 135 entries.  For the device's builder and walks ONLY -- the oracle's walks keep stack[64]."""
    assert not hasattr(b, "stack_peaks"), "never hand this chain to the oracle's walk"
    assert OVERFLOW_N - 1 > STACK_MAX and OVERFLOW_W < OVERFLOW_X0 and np.isfinite(chain_tris(OVERFLOW_N, OVERFLOW_X0, OVERFLOW_W)).all()
    b.mesh_raw(1, b.diffuse(0.8, (1, 1, 1)), chain_tris(OVERFLOW_N, OVERFLOW_X0, OVERFLOW_W))
    b.build(SPLIT)


def overflow_rays(n=777):
    return _group(np.random.default_rng(136), n, -OVERFLOW_X0 / 2, 1.0, 0.0, OVERFLOW_W)
