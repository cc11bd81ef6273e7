"""What the CPU and GPU tests of rt_set_instance_list (include/rt_amd.h) share: the two-mesh scene under an explicit list of BLASes, the walk
of lists the layout test takes, the lists and ray sets of the behaviour test, and the UPDATED description after a list edit on top of
tests/triangles_desc.py's Desc (instances / n_instances replaced, tlas_nodes the restated tlas::build over the n boxes).  Nothing here
loads the library under test; the host mirror (for mat4::Inverted and trs) comes from the caller."""
import numpy as np

import instances_ref as ir
import triangles_ref as tr
from conftest import random_rays

f32 = np.float32
UPLOADED = (0, 1, 0)  # ir.triangles_scene's three instances: the meshes alternate
N_SPLIT = ir.smallest_n_without_lds()  # 38


def _alt(n):
    return [i & 1 for i in range(n)]


# the walk of the layout test: uploaded 3 -> 5 -> 1 -> 2 -> 17 -> 38 -> 37 -> 256 -> 3.  blas: the mesh of every instance (3 -> 5 re-points
# entries 0 and 1 to the other mesh; 256 leaves mesh 1 without an instance); given: bounds6 is sent (False: NULL, the device computes them)
WALK = (dict(n=5, blas=[1, 0, 0, 1, 0], given=False), dict(n=1, blas=[1], given=True), dict(n=2, blas=[0, 1], given=False),
        dict(n=17, blas=_alt(17), given=True), dict(n=N_SPLIT, blas=_alt(N_SPLIT), given=False), dict(n=N_SPLIT - 1, blas=_alt(N_SPLIT - 1), given=True),
        dict(n=256, blas=[0] * 256, given=False), dict(n=3, blas=[0, 1, 1], given=True))


def walk_transforms(scene, k):
    """the transforms of step k of WALK: a grid of their own per step, so that every record changes"""
    return ir.grid_transforms(scene, WALK[k]["n"], turn=0.2 * (k + 1), scale=1.0 + 0.1 * (k % 3), shift=(0.05 * k, 0.02 * k, -0.03 * k))


def list_scene(b, blas, transforms):
    """ir.triangles_scene with the mesh of every instance named by 'blas' (ir.triangles_scene alternates them): the scene a fresh build of a
    list makes.  The BLASes are numbered by first use, as Scene::Describe numbers them."""
    b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
    red = b.diffuse(0.8, (1, 0.2, 0.2), 0.0, 1, 1)
    blue = b.diffuse(0.8, (0.2, 0.2, 1), 0.0, 1, 1)
    floor = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    m0 = b.mesh_raw(1, red, np.array([[-0.2, 0, 0, 0.2, 0, 0, 0, 0.4, 0.05]], dtype=f32))
    m1 = b.mesh_raw(2, blue, np.array([[-0.15, 0, 0.1, 0.15, 0, -0.1, 0, 0.3, 0], [-0.15, 0, 0.1, 0, 0.3, 0, 0, 0.1, 0.3]], dtype=f32))
    b.plane(0, floor, (0, 1, 0), 0)
    b.sphere(7, blue, (1.8, 0.5, 2.0), 0.5)
    b.build_tlas(0, [((m0, m1)[k], T) for k, T in zip(blas, transforms)])
    return dict(name="list_scene", tlas=True, meshes=(m0, m1))


def given_bounds(d, blas, Ts):
    """boxes a caller might send: each a fresh instance's, grown by a margin of its own (so that they are not what NULL would compute)"""
    out = []
    for i, (k, T) in enumerate(zip(blas, Ts)):
        b = ir.fresh_bounds(tr.local_box(d.nodes[int(k)]), T)
        out.append(np.concatenate([b[:3] - f32(0.05 * (i % 3)), b[3:] + f32(0.1 + 0.02 * (i % 5))]))
    return np.stack(out).astype(f32)


def set_list(d, rec, bounds=None):
    """rt_set_instance_list(rec, bounds) on a triangles_desc.Desc: the list replaced, the boxes given or a fresh instance's over the BLAS's
    current nodes, tlas_nodes = tlas::build over them"""
    n = len(rec)
    inst = np.zeros(n, dtype=d.inst.dtype)
    for i in range(n):
        inst[i] = (rec["blas"][i], rec["transform"][i], rec["inv_transform"][i])
    d.inst, d.n = inst, n
    d.raw.n_instances = n
    d.bounds = np.stack([bounds[i] if bounds is not None else ir.fresh_bounds(tr.local_box(d.nodes[int(inst["blas"][i])]), inst["transform"][i]) for i in range(n)]).astype(f32)
    d.tlas = ir.tlas_build(d.bounds)


def walk_step(host_api, d, scene, k):
    """step k of WALK applied to the description d: (records, bounds6 or None) as the call takes them"""
    st = WALK[k]
    Ts = walk_transforms(scene, k)
    rec = ir.records(host_api, st["blas"], Ts)
    b6 = given_bounds(d, st["blas"], Ts) if st["given"] else None
    set_list(d, rec, b6)
    return rec, b6


# ---- the behaviour test: uploaded 3 -> 5 -> 2 ----------------------------------------------------------------------------------------------
BEHAVIOUR_RAYS = 2048
BEHAVIOUR_SPREAD = 2.0  # aimed_rays' origin box: chosen on the oracle so that one ray in four ends on an instance that is new in the step


def behaviour_transforms(scene, n):
    """placements in front of the default camera, large enough to be met: 3 are the upload's, 5 keeps instance 2 of them, 2 moves both"""
    place = lambda i, turn: scene.trs((f32(-2.0 + 1.0 * i), f32(0.1 * i), f32(3.0 + 0.2 * i)), f32(2.5), 0.0, f32(turn + 0.3 * i), 0.0)
    if n == 3:
        return [place(i, 0.0) for i in range(3)]
    if n == 5:
        return [place(0, 0.5), place(1, 0.7), place(2, 0.0), place(3, 0.2), place(4, -0.4)]
    return [place(1, -0.6), place(3, 0.9)]


BEHAVIOUR_LISTS = {3: list(UPLOADED), 5: [1, 0, 0, 1, 0], 2: [0, 1]}
# the instances whose record (BLAS or matrices) is not the one the list before held at that index
BEHAVIOUR_NEW = {5: [0, 1, 3, 4], 2: [0, 1]}


def behaviour_rays(Ts, new, seed):
    """BEHAVIOUR_RAYS rays: one in eight anywhere (conftest.random_rays), the rest ir.aimed_rays at the instances that are new in the step"""
    k = BEHAVIOUR_RAYS // 8
    O0, D0 = random_rays(k, seed)
    O1, D1 = ir.aimed_rays(BEHAVIOUR_RAYS - k, seed + 1, [Ts[i] for i in new], spread=BEHAVIOUR_SPREAD)
    return np.concatenate([O0, O1]).astype(f32), np.concatenate([D0, D1]).astype(f32)


def hits_on(oracle_scene, O, D, instances):
    """on the oracle: which rays' nearest hit lies on one of 'instances' -- the scene's hit is that instance's own (RT_SCOPE_INSTANCE = 3)"""
    ref = oracle_scene.find_nearest(O, D)
    on = np.zeros(len(O), bool)
    for i in instances:
        own = oracle_scene.scope_nearest(3, i, O, D)
        on |= (ref["obj"] != -1) & (own["obj"] == ref["obj"]) & (own["t"].view(np.uint32) == ref["t"].view(np.uint32))
    return ref, on
