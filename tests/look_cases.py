"""What the tests of rt_set_lights, rt_set_materials and rt_set_sky share: a small scene whose lights, materials and sky are arguments, so
that the same builder makes the scene as uploaded, the edited scene built from scratch (the host mirror's and the oracle's) and -- through
its description -- the records the three calls send; the list of edits; and the patching of a tests/triangles_desc.py Desc, the updated
description of a scene that rt_set_triangles / rt_set_instances / rt_set_time have changed as well.  A plain helper module: numpy only."""
import ctypes as C

import numpy as np

from test_layout_cpu import LIGHT, MATERIAL, RtSceneDesc, desc_array

f32 = np.float32
W, H = 16, 8  # the frame of the GPU tests
TYPE_SHIFT, TYPE_MASK = 4, 3 << 4  # csrc/rt_scene_dev.h RT_TYPE_SHIFT: bits 4-5 of a primitive record's word 15
DIFFUSE, METAL, GLASS = 1, 2, 3

# ---- materials, lights and skies as data -------------------------------------------------------------------------------------------------
# (kind, arguments of the builder protocol's diffuse / metal / glass)
FLOOR = ("diffuse", dict(albedo=0.8, col=(1.0, 1.0, 1.0), ks=0.0, kd=1.0, n=4))
GREEN = ("diffuse", dict(albedo=0.8, col=(0.1, 0.9, 0.2), ks=0.3, kd=0.7, n=6))
RED = ("diffuse", dict(albedo=0.8, col=(0.9, 0.1, 0.1), ks=0.3, kd=0.7, n=6))
SHINY = ("diffuse", dict(albedo=0.8, col=(0.1, 0.9, 0.2), ks=0.3, kd=0.7, n=6, shininess=0.5))
GOLD = ("metal", dict(fuzzy=0.3, col=(0.85, 0.65, 0.13)))
STEEL = ("metal", dict(fuzzy=0.1, col=(0.7, 0.7, 0.8)))
BLUEGLASS = ("glass", dict(ir=1.5, col=(0.6, 0.6, 1.0), absorption=(0.1, 0.2, 0.05)))
GREY = ("diffuse", dict(albedo=0.8, col=(0.5, 0.5, 0.5), ks=0.0, kd=1.0, n=2))
# the table of the scene: 0 the floor's, 1 X: a mesh's, a sphere's and a wall plane's (the material the edits change), 2 Y: another mesh's
# and sphere's, 3 one no primitive names
MATS = (FLOOR, GREEN, GOLD, GREY)


def lights(n):
    """n lights over the scene, area and directional by turns, objIdx 11 .. 11 + n - 1 (template/scene.h: a light's objIdx is 11 + its index)"""
    out = []
    for i in range(n):
        x, z = f32(-2.0 + 0.5 * (i % 8)), f32(0.5 + 0.8 * (i // 8))
        if i % 2 == 0:
            out.append(("area", dict(idx=11 + i, pos=(float(x), 3.5, float(z)), strength=12.0 / max(n, 1) + 2.0, col=(1.0, 1.0, 0.9), radius=0.4, normal=(0, -1, 0))))
        else:
            out.append(("dir", dict(idx=11 + i, pos=(float(x), 4.0, float(z)), strength=6.0 / max(n, 1) + 1.0, col=(0.9, 0.9, 1.0), normal=(0.2, -1, 0.3), r=1)))
    return tuple(out)


LIGHTS = lights(2)


def sky_image(w, h, seed):
    """an 8-bit RGB image with structure at every scale (a gradient plus seeded noise)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([40 + 180 * x / max(w - 1, 1), 60 + 150 * y / max(h - 1, 1), 200 - 120 * x / max(w - 1, 1)], -1)
    return np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


SKY = (32, 16, 1)  # sky_image's arguments; None: no sky


def add_material(b, spec):
    return getattr(b, spec[0])(**spec[1])


def add_light(b, spec):
    return (b.area_light if spec[0] == "area" else b.dir_light)(**spec[1])


PANEL = np.array([[-0.9, 0.1, 1.6, 0.1, 0.1, 1.9, -0.5, 1.3, 1.8], [0.1, 0.1, 1.9, 0.3, 1.2, 2.0, -0.5, 1.3, 1.8]], dtype=f32)
WEDGE = np.array([[0.5, 0.0, 1.0, 1.3, 0.0, 1.2, 0.9, 0.9, 1.1]], dtype=f32)


def look_scene(b, tlas=False, mats=MATS, lights=LIGHTS, sky=SKY):
    """A panel (material X), a wedge (Y), two spheres (X, Y), the floor plane and a wall plane (X) in front of the default camera.  Without
    a TLAS all of it is the scene BVH (triangle, sphere and plane records in leaves); with one the two meshes are instanced twice each
    and the spheres and planes are the brute-force primitives."""
    if sky is not None:
        b.sky(sky_image(*sky))
    for l in lights:
        add_light(b, l)
    m = [add_material(b, s) for s in mats]
    panel = b.mesh_raw(1, m[1], PANEL)
    wedge = b.mesh_raw(2, m[2], WEDGE)
    b.sphere(3, m[1], (-0.2, 0.35, 0.6), 0.35)
    b.sphere(4, m[2], (0.9, 0.3, 0.4), 0.3)
    b.plane(0, m[0], (0, 1, 0), 0)
    b.plane(5, m[1], (1, 0, 0), 2.5)  # a wall on the left: the sky stays in view on the right
    if tlas:
        T = [b.trs((0, 0, 0), 1, 0.0, 0.0, 0.0), b.trs((0.2, 0, 0.5), 1, 0.0, 0.3, 0.0), b.trs((-1.2, 0.0, 1.0), 0.8, 0.0, -0.4, 0.0), b.trs((0.3, 0.6, 0.8), 0.7, 0.0, 0.8, 0.0)]
        b.build_tlas(0, [(panel, T[0]), (wedge, T[1]), (panel, T[2]), (wedge, T[3])])
    else:
        b.build(0)
    return dict(name="look", tlas=tlas)


def strip_scene(b, n, mats=MATS, lights=LIGHTS, sky=None):
    """n small triangles of material X in one scene BVH: n primitive records (n = 1: the root is a leaf)"""
    for l in lights:
        add_light(b, l)
    m = [add_material(b, s) for s in mats]
    i = np.arange(n, dtype=f32)
    x, z = f32(-1.5) + f32(0.012) * i, f32(1.0) + f32(0.003) * i
    v9 = np.stack([x, 0 * i, z, x + f32(0.01), 0 * i, z, x, 0 * i + f32(0.5), z + f32(0.1)], 1).astype(f32)
    b.mesh_raw(1, m[1], v9)
    b.build(0)
    return dict(name="strip%d" % n, tlas=False)


STRIP_SIZES = (1, 255, 256, 257)  # records around the 256-thread block of k_retype_prims


def with_mat(mats, index, spec):
    out = list(mats)
    out[index] = spec
    return tuple(out)


# ---- the edits: name -> (arguments of look_scene before, after, what changed) ------------------------------------------------------------
# 'first' / 'count': the range rt_set_materials is given; 'type': the edit changes a type (k_retype_prims runs); 'unsupported': the value
# of pathUnsupported (RT_LAYOUT_SCALARS word 11) before and after
MATERIAL_EDITS = {
    "colour": dict(before=MATS, after=with_mat(MATS, 1, RED), first=1, count=1, type=False, unsupported=(0, 0)),
    "diffuse_to_metal": dict(before=MATS, after=with_mat(MATS, 1, STEEL), first=1, count=1, type=True, unsupported=(0, 0)),
    "metal_to_glass": dict(before=with_mat(MATS, 1, STEEL), after=with_mat(MATS, 1, BLUEGLASS), first=1, count=1, type=True, unsupported=(0, 0)),
    # X is the only glass or metal material before: the edit removes the last specular material (no bounce table afterwards)
    "glass_to_diffuse": dict(before=with_mat(with_mat(MATS, 1, BLUEGLASS), 2, GREY), after=with_mat(with_mat(MATS, 1, GREEN), 2, GREY), first=1, count=1, type=True, unsupported=(0, 0)),
    "shiny_on": dict(before=MATS, after=with_mat(MATS, 1, SHINY), first=1, count=1, type=False, unsupported=(0, 1)),
    "shiny_off": dict(before=with_mat(MATS, 1, SHINY), after=MATS, first=1, count=1, type=False, unsupported=(1, 0)),
    # materials 1 and 2 of four, both changing type and colour: a range that is not the whole table
    "range": dict(before=MATS, after=with_mat(with_mat(MATS, 1, BLUEGLASS), 2, RED), first=1, count=2, type=True, unsupported=(0, 0)),
}
TYPE_EDITS = tuple(k for k, e in MATERIAL_EDITS.items() if e["type"])
LIGHT_TABLES = (0, 1, 31, 32)
LIGHT_TRANSITIONS = ((0, 1), (1, 32), (32, 0))
SKY_EDITS = {"same_size": (32, 16, 2), "larger": (64, 32, 3), "smaller": (8, 4, 4), "none": None}


# ---- records out of a description --------------------------------------------------------------------------------------------------------
def tables(ptr):
    """(materials, lights, sky) behind an rt_scene_desc pointer: MATERIAL and LIGHT records and the (h, w, n) texels or None"""
    d = RtSceneDesc.from_address(ptr.value)
    sky = None
    if d.sky_pixels and d.sky_w > 0 and d.sky_h > 0:
        sky = np.frombuffer(C.string_at(d.sky_pixels, d.sky_w * d.sky_h * d.sky_n), dtype=np.uint8).reshape(d.sky_h, d.sky_w, d.sky_n).copy()
    return desc_array(d.materials, d.n_materials, MATERIAL), desc_array(d.lights, d.n_lights, LIGHT), sky


def scene_tables(host_api, **kw):
    """the three tables of look_scene(**kw), from the host mirror's own flattening (no device)"""
    s = host_api.HostScene()
    look_scene(s, **kw)
    out = tables(s.describe())
    s.close()
    return out


def retyped(mats, shift=1):
    """every material's type rotated diffuse -> metal -> glass -> diffuse: an edit for scenes whose materials the tests did not choose"""
    out = mats.copy()
    out["type"] = (mats["type"] - 1 + shift) % 3 + 1
    out["shinieness"] = 0
    out["raytracer"] = 1
    out["ir"] = np.where(out["type"] == GLASS, f32(1.5), out["ir"])
    return out


def patch(d, mats=None, lights=None, sky=False):
    """a tests/triangles_desc.py Desc with its material table, its light table or its sky replaced (sky: texels or None; False: as it is)"""
    own = lambda a: C.create_string_buffer(np.ascontiguousarray(a).tobytes(), max(a.nbytes, 1)) if a is not None and a.nbytes else None
    if mats is not None:
        assert len(mats) == d.raw.n_materials
        d.own["materials"] = own(np.ascontiguousarray(mats, dtype=MATERIAL))
    if lights is not None:
        d.own["lights"], d.raw.n_lights = own(np.ascontiguousarray(lights, dtype=LIGHT)), len(lights)
    if sky is not False:
        d.own["sky_pixels"] = own(sky)
        d.raw.sky_w, d.raw.sky_h, d.raw.sky_n = (sky.shape[1], sky.shape[0], sky.shape[2]) if sky is not None else (0, 0, 3)
    return d


def kind_words(prims):
    """word 15 of every 64-byte record of a PRIMS / BRUTE array (its spare words dropped), and the records with that word cleared"""
    w = np.ascontiguousarray(prims).view(np.uint32)
    w = w[:len(w) // 16 * 16].reshape(-1, 16).copy()
    kind = w[:, 15].copy()
    w[:, 15] = 0
    return kind, w
