"""Crafted hits for the shade step (csrc/rt_shade.h: the lights, diffuse::scatter, the glass, metal and diffuse bounces, the shadow ray, the
roulette).  A plain helper module of the test suite, numpy only: tests/test_shade_cpu.py shows on the oracle alone that every case reaches
the branch it is listed for, tests/test_gpu_shade.py holds every pipeline of the device to the oracle on the same rays.

A scene is a function of a scene builder (the protocol OracleScene and HostScene share) with keyword arguments: 'rt', the flag its
materials are built with, and 'twin', the name of ONE variation just across a branch (another index of refraction, a light moved out of
the plane, two stacked disks swapped, ...).  A case is a handful of rays on one scene, each repeated REPS times or more, with the depth
each of Renderer::Trace and Renderer::Sample starts at (the smallest at which the case's branch contributes), the pipelines that shade
it, and its twin: the same rays, the same random streams, on the varied scene (or with another energy, or another depth).

A pipeline is a function (mode, flag) -- see tests/depth_cases.py -- and the flag the scene's materials are built with:
  'trace'      Trace, flag set, materials rt=True       the Whitted schedules (WHITTED_ENVS)
  'sample'     Sample, flag clear, materials rt=True    the dense and the slot wavefront (PATH_ENVS and OWN_ENVS)
  'trace_g'    Trace, flag clear, materials rt=False    k_trace_general: roulette, sampled lights, the indirect child
  'sample_g'   Sample, flag set, materials rt=False     k_sample_general: roulette, lights at their position
  'sample_g0'  Sample, flag clear, materials rt=False   k_sample_general as path mode runs it where the wavefront cannot replay the scene
All cases of one scene that share a pipeline and a depth make ONE batch; ray i of a batch draws from StreamSeed(SEED_BASE + i), so the
repeats of a ray are different streams, and a case's streams are its position in the batch on the oracle and on the device alike.

Measured on an MI355X (largest relative error against the oracle, floor 1e-3, bar 1e-4; tests/test_gpu_shade.py prints them):
  family               trace    sample   trace_g  sample_g  sample_g0
  1 glass             1.1e-7    1.8e-7    1.1e-7    1.8e-7    1.8e-7
  2 diffuse           8.1e-8    1.6e-7    4.8e-7    1.6e-7    1.5e-7
  3 metal                  0    8.6e-8         0    9.3e-8    8.6e-8
  4 area lights            0         0    4.0e-7    2.5e-7    3.2e-7
  5 directional            0         0    2.6e-7    1.8e-7    3.0e-7
  6 counts                 0    1.3e-7    3.4e-7    2.4e-7    2.9e-7
  7 roulette               -         -    8.6e-7    2.2e-7         -
  8 instances         1.9e-7    2.0e-7    1.9e-7    2.0e-7    2.0e-7
0: the device's bits are the oracle's in every case of the family (the light families under both wavefront functions, metal under
Trace).  The ten schedules of 'sample', the 24-slot one among them, give one set of bits, and so do the three of 'trace'.  A later change can pin the zeros."""
import numpy as np

f32 = np.float32
TRACE, SAMPLE = 0, 1
SEED_BASE = 4242
ENERGY = (0.9, 0.8, 0.7)
REPS = 16
MIN_VALUE = 0.02     # tests/test_shade_cpu.py: the largest channel of at least half of a case's finite rays
MIN_SHARE = 0.5      # ... and the share of a case's rays the twin changes

# pipeline -> (mode, flag, the materials' flag)
PIPELINES = {"trace": (TRACE, True, True), "sample": (SAMPLE, False, True),
             "trace_g": (TRACE, False, False), "sample_g": (SAMPLE, True, False), "sample_g0": (SAMPLE, False, False)}
ALL = ("trace", "sample", "trace_g", "sample_g", "sample_g0")
PATHS = ("sample", "trace_g", "sample_g0")   # the pipelines that sample a light's position (the lights' flag is clear)
ROULETTE = ("trace_g", "sample_g")

# the schedules of the two wavefront functions: tests/depth_cases.py PATH_ENVS / WHITTED_ENVS, and for Sample three of this tier's own.
# RT_SHADE_LDS is a switch of the dense wavefront alone (k_shade_s / k_light_s read the material and light tables from memory instead of
# LDS); the slot kernels have no such tables, so with RT_STREAM=0 it is the plain slot run once more.  depth_cases' RT_SLOTS=777 is above
# every batch of this tier (528 rays at most): the slot wavefront then has a slot per sample and finishes each where it ends.  SLOT_BUDGET
# is below every batch: slots are refilled as samples finish, and k_finish stores the finished ones.
SLOT_BUDGET = 24
OWN_ENVS = [{"RT_SHADE_LDS": "0"}, {"RT_SHADE_LDS": "0", "RT_STREAM": "0"}, {"RT_STREAM": "0", "RT_SLOTS": str(SLOT_BUDGET)}]


def sky_pixels():
    """a small bright sky: every texel between 0.31 and 0.94, no two neighbours alike"""
    i = np.arange(4 * 8 * 3, dtype=np.int64).reshape(4, 8, 3)
    return ((i * 37) % 160 + 80).astype(np.uint8)


def _unit(d):
    d = np.asarray(d, dtype=np.float64)
    return (d / np.sqrt((d * d).sum())).astype(f32)


def _to(o, p):
    """the ray from o through p"""
    o, p = np.asarray(o, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return (o.astype(f32), _unit(p - o))


def _down(x, z, y=2.0):
    """straight down onto (x, 0, z): t = y and the hit point are exact"""
    return (np.array([x, y, z], dtype=f32), np.array([0, -1, 0], dtype=f32))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
IRS = (0.8, 1.0, 1.5, 2.4)
IRS_TWIN = (0.95, 1.05, 1.2, 1.1)   # every total reflection of IRS is below its critical angle here
GLASS_COL = (0.9, 0.8, 1.0)           # (outside family 7 every colour has a channel of 1: the roulette draws, and nothing dies)
ABSORB = (0.3, 0.0, 0.6)            # one component zero: exp is skipped there (glass_hit)
DENSE, DENSE_TWIN = (400.0, 0.0, 0.5), (1.0, 0.0, 0.5)  # exp(-400 * 4) underflows to 0 in x; exp(-4) does not
SPEC_X = (10.0, 14.0, 18.0, 22.0)    # sphere k of IRS at (SPEC_X[k], SPEC_Y, 0), triangle k above it in the plane z = 6
DENSE_X, METAL_X, MATTE_X, GRAZE_X = 26.0, 30.0, 34.0, 12.0
SPEC_Y = 2.0   # the floor is the plane y = 0: a +Y plane has its BVH slab at coordinate 0 whatever its d (quirk Q1); so has the wall x = 0
WALL_COS = 1e-4   # an incidence on the ir = 1 wall for which sqrt(1 - cosi * cosi) is 1 to the bit: sint == 1, the '>=' of glass::fresnel


def spec(b, rt=True, twin=None):
    """family 1 (glass by ir), 3 (metal) and the light count 0: four glass spheres and four glass triangles, a glass sphere that absorbs
    x away, a metal and a diffuse sphere over a glass floor and beside a glass wall of ir 1, under the sky alone"""
    b.sky(sky_pixels())
    irs = IRS_TWIN if twin == "ir" else IRS
    for k, ir in enumerate(irs):
        g = b.glass(ir, GLASS_COL, ABSORB, rt=rt)
        x = SPEC_X[k]
        b.sphere(1 + k, g, (x, SPEC_Y, 0), 1.0)
        b.mesh_raw(1 + k, g, [x - 1.5, 9, 6, x + 1.5, 9, 6, x, 12, 6])  # N = (0, 0, 1): a ray towards -z arrives from outside
    b.sphere(5, b.glass(1.5, GLASS_COL, DENSE_TWIN if twin == "absorb" else DENSE, rt=rt), (DENSE_X, SPEC_Y, 0), 1.0)
    b.sphere(6, b.metal(0.7, (0.6, 1.0, 0.3) if twin == "metal" else (1.0, 0.6, 0.3), rt=rt), (METAL_X, SPEC_Y, 0), 1.0)
    b.sphere(7, b.diffuse(0.8, (1.0, 0.7, 0.5), rt=rt), (MATTE_X, SPEC_Y, 0), 1.0)
    b.plane(0, b.glass(1.25 if twin == "ir" else 1.5, GLASS_COL, ABSORB, rt=rt), (0, 1, 0), 0)
    b.plane(8, b.glass(1.05 if twin == "ir" else 1.0, GLASS_COL, ABSORB, rt=rt), (1, 0, 0), 0)
    if twin == "light":
        b.area_light(11, (MATTE_X, 7, -3), 8.0, (1, 1, 1), 0.5, (0, -1, 0))
    b.build(0)
    return dict(name="spec", tlas=False)


MATTE_ENERGY = (0.5, 0.9, 0.9)            # energy.x - (1 - albedo.x) is exactly 0 at albedo.x = 0.5
MATTE_ENERGY_TWIN = (0.5 + 2.0 ** -20, 0.9, 0.9)
MATTE_LIGHT = (0.0, 6.0, 0.0)
N_X = {200: 3.0, 1: 6.0, 0: 9.0}          # the specular spheres by exponent
RETAIN = {"pos": (-3.0, (0.75, 0.5, 0.5)), "zero": (-6.0, (0.5, 0.5, 0.5)), "neg": (-9.0, (0.25, 0.5, 0.5)), "mixed": (-12.0, (0.75, 0.05, 0.5))}


def matte(b, rt=True, twin=None):
    """family 2 and the light count 1: spheres of one diffuse material each under one light"""
    b.sky(sky_pixels())
    b.area_light(11, (N_X[1], 6.0, 0.0) if twin == "light_up" else MATTE_LIGHT, 40.0, (1, 1, 1), 0.5, (0, -1, 0))
    if twin == "second":
        b.area_light(12, (0.0, 6.0, 4.0), 20.0, (1, 1, 1), 0.5, (0, -1, 0))
    for k, (n, x) in enumerate(N_X.items()):
        m = b.diffuse(0.8, (1.0, 0.8, 0.7), 0.7, 0.3, {200: 100, 1: 2, 0: 1}[n] if twin == "N" else n, rt=rt)
        b.sphere(1 + k, m, (x, 0, 0), 1.0)
    for k, (x, albedo) in enumerate(RETAIN.values()):
        b.sphere(5 + k, b.diffuse(albedo, (1.0, 0.8, 0.7), rt=rt), (x, 0, 0), 1.0)
    b.build(0)
    return dict(name="matte", tlas=False)


def shiny(b, rt=True, twin=None):
    """family 2, the mirror branch of a diffuse hit: a floor of shininess 0.25 and a sphere of shininess 1 (no direct term at all)"""
    b.sky(sky_pixels())
    b.area_light(11, (0.0, 6.0, 0.0), 20.0, (1, 1, 1), 0.5, (0, -1, 0))
    lo, hi = (0.5, 0.75) if twin == "sh" else (0.25, 1.0)
    b.plane(0, b.diffuse(0.8, (1.0, 0.8, 0.7), 0.3, 0.7, 4, shininess=lo, rt=rt), (0, 1, 0), 0)
    b.sphere(1, b.diffuse(0.8, (0.7, 0.8, 1.0), 0.3, 0.7, 4, shininess=hi, rt=rt), (4, 1, 0), 1.0)
    b.build(0)
    return dict(name="shiny", tlas=False)


LAMPS = 31   # a ragged table: one short of rt_upload_scene's limit


def lamps(b, rt=True, twin=None):
    """families 4 and 5 and the light count 31: a white floor (albedo 1: diffuse::scatter keeps the energy, every light counts) under
    crafted area and directional lights, each far enough from the others' rays, and plain ones along z = 10 up to the count"""
    b.sky(sky_pixels())
    fl = b.diffuse(1.0, (1.0, 0.9, 0.8), rt=rt)
    b.plane(0, fl, (0, 1, 0), 0)
    L = []
    # 0: coloured, one channel zero; seen directly it is (inf, NaN, inf)
    L.append(("a", (0, 4, 0), 8.0, (1, 1, 0.5) if twin == "col" else (1, 0, 0.5), 0.5, (-0.6, -0.8, 0) if twin == "tilt" else (0, -1, 0)))
    # 1 .. 4: two pairs of disks stacked on one vertical ray, the upper one later in the table at x = 6 and earlier at x = 9 (Q6: the last wins)
    lo, up = (4.0, (1, 0, 1)), (5.0, (0, 1, 1))   # the lower disk has no green, the upper one no red
    for x, pair in ((6, (lo, up)), (9, (up, lo))):
        for y, col in (pair[::-1] if twin == "swap" else pair):
            L.append(("a", (x, y, 0), 5.0, col, 0.5, (0, -1, 0)))
    # 5: a disk behind a sphere: the light test sets ray.t, the sphere in front of it still wins
    L.append(("a", (12, 4, 0), 5.0, (1, 0, 1), 0.5, (0, -1, 0)))
    b.sphere(3, fl, (11, 2.5, 5.0 if twin == "sphere_away" else 0.0), 0.5)
    # 6: an upright disk centred in the floor: from a floor point within its radius cos is 0 (< 1e-4): strength * col, not relStr * col
    L.append(("a", (18, 0.3 if twin == "out_of_plane" else 0.0, 0), 3.0, (1, 0.9, 0.8), 0.5, (1, 0, 0)))
    # 7: normal (0, 0, 1); a sampled position moves in x and y whatever the normal
    L.append(("a", (24, 3, 1.5 if twin == "move_z" else 0), 6.0, (0.9, 1, 0.8), 1.0, (0, 0, 1)))
    # 8: below the floor: cos < 0, and no term of the shade step minds
    L.append(("a", (30, -1, 0), 4.0, (0.8, 0.9, 1), 1.5 if twin == "below_r" else 0.5, (0, 1, 0)))
    # 9, 10: an occluder between the floor and the light, and one just past the light (the shadow ray ends at the light)
    L.append(("a", (36, 3, 0), 6.0, (1, 1, 1), 0.2, (0, -1, 0)))
    L.append(("a", (42, 3, 0), 6.0, (1, 1, 1), 0.2, (0, -1, 0)))
    past = twin == "occl_past"
    b.sphere(4, fl, (36, 3.5 if past else 1.5, 0), 0.25)
    b.sphere(5, fl, (42, 2.9 if past else 3.4, 0), 0.3)
    # 11, 12: directional: a cone of 45 degrees around (0, -1, 0) and one of 90 degrees (sin_angle = 1)
    L.append(("d", (48, 5, 0), 10.0, (0, 1, 0) if twin == "dir_flip" else (0, -1, 0), 1.0 if twin == "dir_wide" else 0.5))
    L.append(("d", (60, 5, 0), 10.0, (0, -1, 0), 0.5 if twin == "dir_narrow" else 1.0))
    b.sphere(6, fl, (48, 8, 0), 1.0)   # a surface behind light 11
    # the rest: plain lights of both kinds along z = 10, every one of them in reach of every floor point
    while len(L) < (LAMPS - 1 if twin == "one_less" else LAMPS):
        k = len(L) - 13
        x = 3.5 * k
        if k % 2 == 0:
            L.append(("a", (x, 5, 10), 3.0, (1, 1, 1), 0.3, (0, -1, 0)))
        else:
            L.append(("d", (x, 5, 10), 6.0, tuple(_unit((0, -1, -2))), 1.0))
    for i, l in enumerate(L):
        if l[0] == "a":
            b.area_light(11 + i, *l[1:])
        else:
            b.dir_light(11 + i, l[1], l[2], (1, 1, 1), l[3], l[4])
    b.build(0)
    return dict(name="lamps", tlas=False)


MANY = 32   # rt_upload_scene's limit


def many(b, rt=True, twin=None):
    """family 6: 32 lights of both kinds on a ring around a sphere on a floor (the twin has 31: the last one counts)"""
    b.sky(sky_pixels())
    fl = b.diffuse(1.0, (1.0, 0.9, 0.8), rt=rt)
    b.plane(0, fl, (0, 1, 0), 0)
    b.sphere(1, fl, (0, 1, 0), 1.0)
    n = MANY - 1 if twin == "one_less" else MANY
    for i in range(n):
        a = 2 * np.pi * i / MANY
        pos = (float(f32(4 * np.cos(a))), 3.0, float(f32(4 * np.sin(a))))
        if i % 2 == 0:
            b.area_light(11 + i, pos, 4.0, (1, 0.5 + 0.5 * (i % 3) / 2, 1 - 0.25 * (i % 4) / 3), 0.3, (0, -1, 0))
        else:
            b.dir_light(11 + i, pos, 6.0, (1, 1, 1), tuple(_unit([-pos[0], -pos[1], -pos[2]])), 1.0)
    b.build(0)
    return dict(name="many", tlas=False)


def _octahedron():
    tris = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                v = [(sx, 0, 0), (0, sy, 0), (0, 0, sz)]
                if sx * sy * sz < 0:
                    v[1], v[2] = v[2], v[1]  # outward normals
                tris.append(np.array(v, dtype=f32).reshape(9))
    return np.stack(tris)


INST_SCALES, INST_SCALES_TWIN = (0.5, 2.0), (0.625, 1.75)


def inst(b, rt=True, twin=None):
    """family 8: a glass octahedron and a diffuse triangle, each a BLAS placed with trs at scales 0.5 and 2 under a TLAS (a sphere is no
    BLAS member here: under a TLAS spheres and planes are tested by brute force, template/scene.h:1260-1261, so the glass is a mesh).
    The instance's normal is normalised on its way back to world space (bvhInstance::Intersect, oracle/orc_bvh.h), so what the family
    holds is the scale in t, in the hit point, in the glass bias and in the distance to the light, not an un-normalised normal."""
    b.sky(sky_pixels())
    b.area_light(11, (0, 8, 2), 10.0, (1, 1, 1), 0.5, (0, -1, 0))
    b.plane(0, b.diffuse(0.8, (1.0, 0.8, 0.8), rt=rt), (0, 1, 0), 3)
    g = b.mesh_raw(1, b.glass(1.5, GLASS_COL, ABSORB, rt=rt), _octahedron())
    d = b.mesh_raw(2, b.diffuse(0.8, (1.0, 0.8, 0.7), 0.5, 0.5, 3, rt=rt), [-1, 0.4, -1, 0, 0.4, 1.5, 1, 0.4, -1])  # N = (0, 1, 0), off the origin: the scale moves it
    s = INST_SCALES_TWIN if twin == "scale" else INST_SCALES
    b.build_tlas(0, [(g, b.trs((-3, 1, 0), f32(s[0]), 0.0, f32(0.3), 0.0)), (g, b.trs((3, 1, 0), f32(s[1]), 0.0, 0.0, 0.0)),
                     (d, b.trs((-3, -1, 4), f32(s[0]), 0.0, 0.0, 0.0)), (d, b.trs((3, -1, 4), f32(s[1]), 0.0, f32(0.3), 0.0))])
    return dict(name="inst", tlas=True)


ROUL_COLS = {"grey": (0.7, 0.7, 0.7), "x": (0.8, 0.3, 0.2), "y": (0.3, 0.8, 0.2), "z": (0.2, 0.3, 0.8)}
ROUL_COLS_TWIN = {"grey": (0.7, 0.7, 0.7), "x": (0.5, 0.3, 0.2), "y": (0.3, 0.5, 0.2), "z": (0.2, 0.3, 0.5)}
ROUL_X = {"grey": 0.0, "x": 3.0, "y": 6.0, "z": 9.0, "black": -3.0, "white": -6.0}


def roul(b, rt=False, twin=None):
    """family 7, the general kernels only: the roulette plays on the largest channel of the material's colour; black (p == 0) always
    dies, at any depth, white (p == 1) never"""
    b.sky(sky_pixels())
    b.area_light(11, (0.0, 6.0, 0.0), 30.0, (1, 1, 1), 0.5, (0, -1, 0))
    cols = dict(ROUL_COLS_TWIN if twin == "p" else ROUL_COLS)
    cols["black"], cols["white"] = ((1, 1, 1), (0, 0, 0)) if twin == "ends" else ((0, 0, 0), (1, 1, 1))
    for k, (name, x) in enumerate(ROUL_X.items()):
        b.sphere(1 + k, b.diffuse(0.8, cols[name], rt=rt), (x, 0, 0), 1.0)
    b.build(0)
    return dict(name="roul", tlas=False)


SCENES = {"spec": spec, "matte": matte, "shiny": shiny, "lamps": lamps, "many": many, "inst": inst, "roul": roul}
SCENE_ENERGY = {"matte": MATTE_ENERGY}
# the scenes of each test of tests/test_gpu_shade.py
SAMPLE_SCENES = ("spec", "matte", "lamps", "many", "inst")
TRACE_SCENES = SAMPLE_SCENES + ("shiny",)
GENERAL_SCENES = ("spec", "matte", "shiny", "lamps", "many", "inst", "roul")


def energy_of(scene):
    return SCENE_ENERGY.get(scene, ENERGY)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, scene, rays, depth, twin, pipelines=ALL, reps=REPS, random=None, expect=None):
        """depth: (Trace's, Sample's); twin: {'twin': scene variation} or {'energy': ...} or {'depth': (Trace's, Sample's)};
        random: None, or the random choice whose both outcomes the repeats must show in the pipelines tests/test_shade_cpu.py MAKES lists
        for it ('glass': sample and sample_g0 -- sample_g plays the roulette before it --, 'light': PATHS, 'roulette': ROULETTE); expect: 'direct' for a light seen directly"""
        self.name, self.family, self.scene, self.rays, self.depth, self.twin = name, family, scene, rays, depth, twin
        self.pipelines, self.reps, self.random, self.expect = tuple(pipelines), reps, random, expect
        assert 8 <= len(rays) * reps <= 64, name

    def __repr__(self):
        return self.name


def _mirror_view(x, tilt):
    """the ray that meets the top of the sphere at (x, 0, 0) 'tilt' off the mirror direction of matte's light"""
    P = np.array([x, 1.0, 0.0])
    L = np.array(MATTE_LIGHT) - P
    L /= np.sqrt((L * L).sum())
    d = np.array([L[0], -L[1], L[2] + tilt])
    d /= np.sqrt((d * d).sum())
    return ((P - 4 * d).astype(f32), d.astype(f32))


def _from_light(x):
    """the ray that meets the top of the sphere at (x, 0, 0) coming from the light's side: -dot(reflection, rayD) < 0 where the light is low"""
    P = np.array([x, 1.0, 0.0])
    L = np.array(MATTE_LIGHT) - P
    L /= np.sqrt((L * L).sum())
    return ((P + 3 * L + np.array([0, 0, 0.3])).astype(f32), _unit(-(3 * L + np.array([0, 0, 0.3]))))


def _cases():
    C = []
    z = lambda x, y, zz, d=(0, 0, 1): (np.array([x, y, zz], dtype=f32), np.array(d, dtype=f32))
    s = lambda x, y, zz, d=(0, 0, 1): z(x, y + SPEC_Y, zz, d)   # in the spec scene, relative to the spheres' height
    # ---- 1: glass ----
    inside = {0.8: 0.5, 1.0: 0.5, 1.5: 0.62, 2.4: 0.4}   # sin of the angle at the inner surface, below the critical angle (the ray starts this far below the centre, above it for ir < 1: its refracted child leaves upwards, past every neighbour)
    beyond = {1.5: 0.8, 2.4: 0.5}                        # ... and beyond it: ir * sin >= 1
    for k, ir in enumerate(IRS):
        x, tag = SPEC_X[k], "ir%g" % ir
        C.append(Case("glass_%s_outside_normal" % tag, 1, "spec", [s(x, 0, -5)], (3, 2), {"twin": "ir"}))
        C.append(Case("glass_%s_inside_below" % tag, 1, "spec", [s(x, inside[ir] if ir < 1 else -inside[ir], 0)], (2, 1), {"twin": "ir"}, reps=32, random="glass" if ir > 1 else None))
        if ir in beyond:
            # (the reflection stays inside the sphere at the same angle for ever: Trace gives black at any depth, so the path functions alone;
            # the back side of the triangle below is where Trace meets kr == 1)
            C.append(Case("glass_%s_inside_beyond" % tag, 1, "spec", [s(x, -beyond[ir], 0)], (2, 1), {"twin": "ir"}, pipelines=("sample", "sample_g", "sample_g0")))
        # the triangle: from outside head-on and at 37 degrees, from its back side head-on and at 53 degrees (beyond the critical angle from ir 1.25 on)
        C.append(Case("glass_%s_triangle_front" % tag, 1, "spec", [s(x, 8, 9, (0, 0, -1)), s(x - 1.8, 8, 8.4, (0.6, 0, -0.8))], (2, 1), {"twin": "ir"}))
        C.append(Case("glass_%s_triangle_back" % tag, 1, "spec", [s(x, 8, 4)], (2, 1), {"twin": "ir"}))
        C.append(Case("glass_%s_triangle_back_%s" % (tag, "beyond" if ir in beyond else "oblique"), 1, "spec", [s(x - 1.6, 8, 4.8, (0.8, 0, 0.6))], (2, 1), {"twin": "ir"}))
    C.append(Case("glass_ir0.8_outside_beyond", 1, "spec", [s(SPEC_X[0] + 0.9, 0, -5)], (2, 1), {"twin": "ir"}))
    C.append(Case("glass_grazing", 1, "spec", [(np.array([GRAZE_X, 0.01, -3], dtype=f32), _unit((0, -5e-4, 1)))], (2, 1), {"twin": "ir"}))
    C.append(Case("glass_sint_1", 1, "spec", [(np.array([1e-3, 14, -3], dtype=f32), _unit((-WALL_COS, 0, 1)))], (2, 1), {"twin": "ir"}))
    C.append(Case("glass_absorption_underflow", 1, "spec", [s(DENSE_X, 0, -5), s(DENSE_X + 0.1, 0.1, -5)], (3, 2), {"twin": "absorb"}))
    # ---- 3: metal, energy != 1 ----
    C.append(Case("metal_energy", 3, "spec", [s(METAL_X + 0.3, 0.2, -5), s(METAL_X - 0.4, -0.3, -5)], (2, 1), {"twin": "metal"}))
    # ---- 6: no light: the path functions alone.  Trace shades it black with the flag set (an empty light loop) and with it clear (no light,
    # so diffuse::scatter never runs and scatteredDir stays 0: the indirect child is weighed with 0); tests/test_shade_cpu.py shows both ----
    C.append(Case("count_0", 6, "spec", [s(MATTE_X + 0.2, 5, 0.3, (0, -1, 0)), s(MATTE_X - 0.3, 5, -0.2, (0, -1, 0))], (2, 1), {"twin": "light"}, pipelines=("sample", "sample_g0", "sample_g")))
    # ---- 2: diffuse ----
    for n in (0, 1, 200):
        C.append(Case("diffuse_N%d" % n, 2, "matte", [_mirror_view(N_X[n], 0.1), _mirror_view(N_X[n], 0.3)], (1, 0), {"twin": "N"}))
    C.append(Case("diffuse_pow_0_0", 2, "matte", [_from_light(N_X[0])], (1, 0), {"twin": "N"}))   # fmax's floor under N = 0: pow(0, 0) = 1
    C.append(Case("diffuse_fmax_floor", 2, "matte", [_from_light(N_X[1])], (1, 0), {"twin": "light_up"}))  # ... under N = 1: 0; with the light overhead the dot is positive
    C.append(Case("diffuse_retention", 2, "matte", [(np.array([x + 0.1, 5, 0.1], dtype=f32), np.array([0, -1, 0], dtype=f32)) for x, _ in RETAIN.values()],
                  (1, 0), {"energy": MATTE_ENERGY_TWIN}))
    C.append(Case("count_1", 6, "matte", [(np.array([N_X[200] - 0.2, 5, 0.3], dtype=f32), np.array([0, -1, 0], dtype=f32))], (1, 0), {"twin": "second"}))
    sh = [_to((-3, 2, -1), (1.5, 0, 0.5)), _to((6, 4, -2), (4.2, 1.9, -0.3))]   # the floor (0.25), the sphere (1.0)
    C.append(Case("diffuse_shininess", 2, "shiny", sh, (2, 1), {"twin": "sh"}, pipelines=("trace", "sample_g0", "trace_g", "sample_g")))
    # ---- 4: area lights ----
    direct = [((0, 1, 0), (0, 1, 0)), ((0, 7, 0), (0, -1, 0))]
    direct = [(np.array(o, dtype=f32), np.array(d, dtype=f32)) for o, d in direct] + [_to((-2, 1, 0), (0.1, 4, 0))]
    C.append(Case("light_direct", 4, "lamps", direct, (1, 0), {"twin": "col"}, expect="direct"))
    C.append(Case("light_parallel", 4, "lamps", [z(-3, y, 0, (1, 0, 0)) for y in (3.9, 4.0, 4.1)], (1, 0), {"twin": "tilt"}))
    C.append(Case("light_stacked", 4, "lamps", [z(6, 1, 0, (0, 1, 0)), z(9, 1, 0, (0, 1, 0))], (1, 0), {"twin": "swap"}, expect="direct"))
    C.append(Case("light_behind_sphere", 4, "lamps", [_to((10, 1, 0), (12, 4, 0))], (1, 0), {"twin": "sphere_away"}))
    C.append(Case("light_in_plane", 4, "lamps", [_down(18.5, 0), _down(17.5, 0), _down(18.25, 0), _down(18, 0.25)], (1, 0), {"twin": "out_of_plane"}))  # the first two on the rim: dis == radius
    C.append(Case("light_normal_z", 4, "lamps", [_down(24.3, 0.4), _down(23.5, -0.3)], (1, 0), {"twin": "move_z"}, random="light"))
    C.append(Case("light_normal_x", 4, "lamps", [_down(18.75, 0.5), _down(19.5, -0.25)], (1, 0), {"twin": "out_of_plane"}, random="light"))
    C.append(Case("light_below", 4, "lamps", [_down(30.25, 0), _down(30.5, 0.25)], (1, 0), {"twin": "below_r"}))
    C.append(Case("light_occluder", 4, "lamps", [_to((34, 1, 0), (36, 0, 0)), _to((40, 1, 0), (42, 0, 0))], (1, 0), {"twin": "occl_past"}))
    # ---- 5: directional lights ----
    C.append(Case("dir_cone", 5, "lamps", [_down(48, 0), _down(50, 0), z(48, 6, 0, (0, 1, 0))], (1, 0), {"twin": "dir_flip"}))   # on the axis, inside, behind
    C.append(Case("dir_outside", 5, "lamps", [_down(56, 0)], (1, 0), {"twin": "dir_wide"}))
    C.append(Case("dir_sin_angle_1", 5, "lamps", [_down(63, 0), _down(60, 1)], (1, 0), {"twin": "dir_narrow"}))
    # ---- 6: counts ----
    C.append(Case("count_31", 6, "lamps", [_down(27, 2), _down(45, 3)], (1, 0), {"twin": "one_less"}))
    C.append(Case("count_32", 6, "many", [_down(2, 0.5), _down(-1.5, 2), _down(0.25, 0.125, 6.0), _to((3, 4, -3), (0.5, 1.2, -0.6))], (1, 0), {"twin": "one_less"}))
    # ---- 8: scaled instances ----
    C.append(Case("instance_glass", 8, "inst", [z(-2.9, 1.05, -5), z(3.3, 1.2, -6)], (3, 2), {"twin": "scale"}))
    C.append(Case("instance_diffuse", 8, "inst", [(np.array([-3, 3, 4.1], dtype=f32), np.array([0, -1, 0], dtype=f32)), (np.array([3.2, 3, 4.3], dtype=f32), np.array([0, -1, 0], dtype=f32))],
                  (1, 0), {"twin": "scale"}))
    # ---- 7: roulette ----
    top = lambda name: (np.array([ROUL_X[name] + 0.1, 5, 0.1], dtype=f32), np.array([0, -1, 0], dtype=f32))
    C.append(Case("roulette_ends", 7, "roul", [top("black"), top("white")], (3, 3), {"twin": "ends"}, pipelines=ROULETTE, reps=32))
    C.append(Case("roulette_ends_no_gate", 7, "roul", [top("black"), top("white")], (6, 6), {"twin": "ends"}, pipelines=ROULETTE, reps=32))  # depth >= 5: only '!p' plays
    C.append(Case("roulette_depth_4", 7, "roul", [top("grey")], (4, 4), {"depth": (5, 5)}, pipelines=ROULETTE, reps=64, random="roulette"))
    C.append(Case("roulette_depth_5", 7, "roul", [top("grey")], (5, 5), {"depth": (4, 4)}, pipelines=ROULETTE, reps=64))
    C.append(Case("roulette_channel", 7, "roul", [top("x"), top("y"), top("z")], (2, 2), {"twin": "p"}, pipelines=ROULETTE, random="roulette"))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def depth_of(case, pipeline, depth=None):
    return (depth or case.depth)[PIPELINES[pipeline][0]]


def batches(scene, pipeline):
    """[(depth, O, D, {case name: slice})]: the cases of 'scene' that 'pipeline' shades, one batch per start depth, in CASES' order"""
    out = {}
    for c in CASES:
        if c.scene == scene and pipeline in c.pipelines:
            out.setdefault(depth_of(c, pipeline), []).append(c)
    res = []
    for depth in sorted(out):
        O, D, where, at = [], [], {}, 0
        for c in out[depth]:
            for o, d in c.rays:
                O += [o] * c.reps
                D += [d] * c.reps
            where[c.name] = slice(at, at + len(c.rays) * c.reps)
            at += len(c.rays) * c.reps
        res.append((depth, np.stack(O).astype(f32), np.stack(D).astype(f32), where))
    return res


_SCENE_CACHE, _REFS = {}, {}


def oracle_scene(oracle_api, scene, rt, twin=None):
    key = (scene, rt, twin)
    if key not in _SCENE_CACHE:
        o = oracle_api.OracleScene()
        SCENES[scene](o, rt=rt, twin=twin)
        _SCENE_CACHE[key] = (o, oracle_api.OracleRenderer(o, 8, 8))
    return _SCENE_CACHE[key]


def oracle_batch(oracle_api, scene, pipeline, depth, O, D, twin=None, energy=None):
    """the oracle's values of one batch (computed once per session, never written to)"""
    mode, flag, rt = PIPELINES[pipeline]
    energy = tuple(energy or energy_of(scene))
    key = (scene, pipeline, depth, twin, energy, O.tobytes(), D.tobytes())
    if key not in _REFS:
        o, orr = oracle_scene(oracle_api, scene, rt, twin)
        o.set_raytracer(flag)
        _REFS[key] = orr.trace_rays(mode, O, D, depth, energy, seed_base=SEED_BASE)
        _REFS[key].setflags(write=False)
    return _REFS[key]


def reference(oracle_api, scene, pipeline):
    """[(depth, O, D, where, the oracle's values)] of batches(scene, pipeline)"""
    return [(depth, O, D, where, oracle_batch(oracle_api, scene, pipeline, depth, O, D)) for depth, O, D, where in batches(scene, pipeline)]


def twin_values(oracle_api, case, pipeline):
    """(the case's values, its twin's): the twin runs the case's whole batch -- the same rays at the same places, so the same streams"""
    for depth, O, D, where in batches(case.scene, pipeline):
        if case.name in where:
            ref = oracle_batch(oracle_api, case.scene, pipeline, depth, O, D)
            t = case.twin
            other = oracle_batch(oracle_api, case.scene, pipeline, depth_of(case, pipeline, t.get("depth")), O, D, twin=t.get("twin"), energy=t.get("energy"))
            return ref[where[case.name]], other[where[case.name]]
    raise KeyError((case.name, pipeline))


def classes(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, per value"""
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def changed_share(a, b):
    """depth_cases.changed_share with classes: the share of rays whose value differs by bits where both are finite, or by class"""
    ca, cb = classes(a), classes(b)
    fin = (ca == 0) & (cb == 0)
    bits = np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)
    return float(((ca != cb) | (fin & bits)).any(1).mean())
