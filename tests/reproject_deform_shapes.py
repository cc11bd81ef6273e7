"""What tests/test_gpu_reproject_deform.py, tests/test_reproject_deform_cpu.py and profiles/reproject_deform_bench.py share: the scenes of the
motion tests (tests/reproject_motion_shapes.py) and one without a TLAS, the deformations of one of their BLASes, how they are sent to a
context, and the experiment that says what a carry across a deformation is worth.  Nothing here needs a device until a renderer is handed in."""
import importlib

import numpy as np

import reproject_motion_shapes as ms
import triangles_desc as td
import triangles_ref as tr

F32 = np.float32
CAMERA, COUNTS, build = ms.CAMERA, ms.COUNTS, ms.build
NO_TLAS = 0          # the 'instance count' of the scene without a TLAS (scenes.mixed_small, through triangles_desc.build_case)
NO_TLAS_CAMERA = ms.look_at((0.3, 1.4, 0.0), (0.0, 0.6, 1.8))  # nearer than CAMERA: mixed_small's diffuse mesh is a tenth of a small frame


def camera(n):
    return NO_TLAS_CAMERA if n == NO_TLAS else CAMERA


# The small amplitude of triangles_ref.DEFORMS["scale"] (whose own default, 100, is the layout tests'): every vertex 5 % nearer to the
# mesh's local origin, and in a second call 10 % more.  A silhouette moves by up to some three pixels of a 97 x 41 frame: the floor a
# shrunken mesh uncovers has no history (the capture saw the mesh there), which is what the rejection bar of the tests needs, and the
# mesh itself is carried through bu, bv.  (A growing mesh uncovers nothing: tests/test_reproject_deform_cpu.py, where the figures were
# chosen, fails the rejection bar with a second factor of 1.1.)
SCALE, SCALE_AGAIN = 0.95, 0.9
TIME = 1.5           # rt_set_time's t on the scene without a TLAS: a = sinf(t) / 2, a vertex turns by 0.2 a y about z (k_animate)


def scenes_module():
    return importlib.import_module("ray-and-pathtracer_amd.scenes")


def build_scene(scene, n):
    """reproject_motion_shapes.build's scenes for n in COUNTS; n == NO_TLAS: mixed_small, whose BLAS 0 is the scene BVH"""
    if n == NO_TLAS:
        return td.build_case(scene, "mixed_small", scenes_module())
    return build(scene, n)


def target(n):
    """the BLAS the tests deform and the instance of it they move with it.  1, 3: the one mesh, instance 0; 70: the two-triangle mesh
    (BLAS 1: half of it can be deformed, one triangle of it collapsed with the other still in view), instance 7 beside the middle of the view"""
    if n == NO_TLAS:
        return dict(blas=0, inst=None)
    return dict(blas=0, inst=0) if n <= 3 else dict(blas=1, inst=7)


def small(v9, s=SCALE):
    return tr.DEFORMS["scale"](v9, s)


def deformations(v9, n, base=None):
    """name -> the steps of a deformation of the target BLAS away from the uploaded vertices v9 (n, 9): ("tris", vertices) is one
    rt_set_triangles call, ("move", first, transforms) one rt_set_instances call, ("time", t) one rt_set_time call"""
    tgt = target(n)
    v9 = np.ascontiguousarray(v9, F32).reshape(-1, 9)
    every = small(v9)
    half = v9.copy()
    some = np.isin(np.arange(len(v9)) % 4, (1, 2))  # about half the triangles, the rest bit-identical: of the two of the lowBigB mesh that CAMERA
    half[some] = every[some]                        # sees (1 and 11) and of the two of the 70's mesh (0 and 1) one each
    line = every.copy()
    line[-1, 6:9] = line[-1, 3:6]          # the last triangle's v2 = v1: e2 = e1, so d11 = d12 = d22 and den == 0 exactly
    out = {"all": [("tris", every)], "half": [("tris", half)], "there_and_back": [("tris", every), ("tris", v9)],
           "two_calls": [("tris", every), ("tris", small(every, SCALE_AGAIN))], "collapsed": [("tris", line)]}
    if tgt["inst"] is not None:
        out["with_move"] = [("tris", every), ("move", tgt["inst"], [ms.translated(base[tgt["inst"]], (0.3, 0.0, 0.1))])]
    else:
        out["time"] = [("time", TIME)]     # (last: rt_set_time(0) afterwards recomputes the normals, it does not bring the uploaded bits back)
    return out


REAL = ("all", "half", "two_calls", "collapsed", "with_move", "time")  # the deformations that leave something deformed


def send(host_api, r, d, n, steps, blas_of=None):
    """the steps on the renderer's context; d: the triangles_desc.Desc of the uploaded scene (the triangles keep its obj_idx and material)"""
    k = target(n)["blas"]
    for step in steps:
        if step[0] == "tris":
            v9 = np.ascontiguousarray(step[1], F32).reshape(-1, 9)
            back = np.array_equal(v9.view(np.uint32), tr.v9_of(d.tris[k]).view(np.uint32))  # the uploaded vertices: under the uploaded normals' bits
            assert r.set_triangles(k, d.tris[k] if back else tr.triangles(d.tris[k], v9)) == 0
        elif step[0] == "move":
            _, first, Ts = step
            assert r.set_instances(first, ms.records(host_api, blas_of[first:first + len(Ts)], Ts)) == 0
        else:
            r.set_time(step[1])


def restore(host_api, r, d, n, blas_of=None, base=None):
    """the target BLAS back to the uploaded triangles (their own normals: the uploaded bits), every instance back at its base transform"""
    k = target(n)["blas"]
    assert r.set_triangles(k, d.tris[k]) == 0
    if n != NO_TLAS:
        assert r.set_instances(0, ms.records(host_api, blas_of, base)) == 0


def prims(r, n_blas):
    """the primitive records the context holds now, every BLAS in order: (slots, 16) f32, the array the G-buffer's prim indexes"""
    return np.concatenate([np.asarray(r.blas_array(b, "prims")).view(F32).reshape(-1, 16) for b in range(n_blas)])


def gbuffer(r):
    """the current G-buffer as the device holds it, instance and primitive indices included"""
    a = r.aovs()
    return dict(pos=r.aov_positions(), normal=a["normal"], t=a["t"], obj=a["obj"], mat=a["mat"], inst=r.aov_instances(), prim=r.aov_prims())


# ---- what the carry is worth -----------------------------------------------------------------------------------------------------------
QUALITY = dict(ms.QUALITY, scale=0.9)  # reproject_motion_shapes.quality's experiment; the 'three' mesh shrunk by a tenth instead of moved
del QUALITY["move"]


def quality(host_api, r):
    """reproject_motion_shapes.quality with a deformation in place of the move, on a renderer that holds ms.quality_scene under the default
    camera with statistics on: 32 samples per pixel, the mesh deformed through rt_set_triangles, the samples carried (rt_reproject_deform)
    and 4 more added -- against clearing and taking the 4 alone, both measured on the library's own 256-sample render of the deformed
    scene.  The zones are that experiment's: 'safe' pixels are carried ones on the mesh, or on the floor outside the box around the mesh
    and its shadow (before and after); 'shadow' pixels the carried floor pixels inside it."""
    q = QUALITY
    PATH = host_api.RT_MODE_PATH
    d = td.Desc(host_api, r.scene)
    r.clear()
    r.render(PATH, 0, q["history_frames"])
    r.render_aovs(0.001)
    before = dict(pos=r.aov_positions(), inst=r.aov_instances())
    r.history_capture()
    assert r.set_triangles(0, tr.triangles(d.tris[0], small(tr.v9_of(d.tris[0]), q["scale"]))) == 0
    r.render_aovs(0.001)
    a, pos, inst = r.aovs(), r.aov_positions(), r.aov_instances()
    n = r.reproject_deform()
    carried = r.stats()[0] > 0
    f0 = q["history_frames"]
    r.render(PATH, f0, q["fresh_frames"])
    acc, cnt = r.accumulator()[..., :3].astype(np.float64), r.stats()[0]
    mean_carried = acc / cnt[..., None]
    r.clear()
    r.render(PATH, f0, q["fresh_frames"])
    mean_fresh = r.accumulator()[..., :3].astype(np.float64) / q["fresh_frames"]
    r.clear()
    r.render(PATH, q["reference_frame0"], q["reference_frames"])
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
    P = np.concatenate([before["pos"][before["inst"] == 0], pos[inst == 0]]).astype(np.float64)
    L = np.array(q["light"])
    P = P[P[:, 1] < L[1] - 0.1]
    S = L + (P - L) * ((L[1] - q["floor_y"]) / (L[1] - P[:, 1]))[:, None]
    obj_xz = np.concatenate([P[:, [0, 2]], S[:, [0, 2]]])
    lo, hi = obj_xz.min(0) - q["margin"], obj_xz.max(0) + q["margin"]
    floor = (inst == -1) & (a["obj"] == 0)
    near = floor & np.all((pos[..., [0, 2]] >= lo) & (pos[..., [0, 2]] <= hi), -1)
    fin = np.isfinite(ref).all(-1) & np.isfinite(mean_fresh).all(-1) & np.isfinite(mean_carried).all(-1)
    safe = carried & fin & ((inst == 0) | (floor & ~near))
    shadow = carried & fin & near
    out = dict(q, carried_pixels=int(n), deformed_mesh_pixels_carried=int((carried & (inst == 0)).sum()), safe_pixels=int(safe.sum()),
               shadow_zone_pixels=int(shadow.sum()), floor_pixels=int(floor.sum()), finite_pixels=int(fin.sum()),
               mse_carried=ms._mse(mean_carried, ref, safe), mse_fresh=ms._mse(mean_fresh, ref, safe),
               shadow_zone_mse_carried=ms._mse(mean_carried, ref, shadow), shadow_zone_mse_fresh=ms._mse(mean_fresh, ref, shadow))
    out["mse_ratio"] = out["mse_carried"] / out["mse_fresh"]
    out["shadow_zone_mse_ratio"] = out["shadow_zone_mse_carried"] / out["shadow_zone_mse_fresh"] if shadow.any() else None
    return out
