"""The shading kernels of this checkout against another checkout's library, bit for bit: a SHA-256 of every accumulator and every
rt_trace_batch result of a fixed list.
  python3 profiles/shade_fold_ab.py --parent <checkout> [--json out.json]          (GPU box, repository root; both checkouts built)
csrc/rt_shade.h holds the shade step that six pipelines used to restate; this renders through every one of them.  Each library runs
in a fresh child process of its own, one after the other (this script with --dump), and prints one digest per entry; the parent
process puts the two lists side by side.  Per scene (mixed_small, scene3 with its own materials, pretty_tlas with 4 instances, the
shiny-floor scene of tests/test_gpu_parity.py with shininess 0.25), at 96 x 64:
  whitted RT_MEGA=0 / =1      one Whitted frame by wavefront rounds (k_shade, k_light) and by the persistent launches of rt_mega.h
  path RT_STREAM=0 / default  four path frames on the slot wavefront and on the dense one (k_shade_s<false>, k_light_s)
  path qlearn                 four path frames with the Q-learning sampler on (k_shade_s<true>; refused on the shiny floor)
  trace flag=f depth=d        rt_trace_batch on the camera rays of frame 0 in both modes, the scene's raytracer flag set and cleared
                              (materials built to match), depths 1, 2, 4: Trace / Sample as Tick calls them and the two general kernels"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
QBOX = ((-6, -1.5, -4), (8, 7, 10))


def shiny(assets, b, rt=True):
    """tests/test_gpu_parity.py _shiny_scene with shininess 0.25"""
    b.sky(assets.synthetic_sky(64, 32, seed=4))
    b.area_light(11, (1.0, 4.0, 1.0), 10.0, (1, 1, 1), 1.0, (0, -1, 0))
    b.area_light(12, (-1.0, 3.0, 0.5), 5.0, (1, 1, 1), 0.5, (0, -1, 0))
    gl = b.glass(1.5, (0.6, 0.6, 1.0), (0.1, 0.2, 0.05), rt=rt)
    me = b.metal(0.7, (0.85, 0.65, 0.12), rt=rt)
    df = b.diffuse(0.8, (0, 1, 0), 0.6, 0.4, 10, rt=rt)
    fl = b.diffuse(0.8, (1, 1, 1), 0.3, 0.7, 4, shininess=0.25, rt=rt)
    b.mesh_obj(1, assets.obj_path("ico"), gl, (-0.9, 0.6, 0.6), 0.5)
    b.mesh_obj(2, assets.obj_path("stellatedDode"), me, (0.9, 0.7, 0.8), 0.5)
    b.mesh_obj(3, assets.obj_path("three"), df, (0.0, 0.5, 1.8), 1.2)
    b.sphere(1, gl, (0.2, 0.35, 0.2), 0.35)
    b.plane(0, fl, (0, 1, 0), 0)
    b.build(0)
    return dict(name="shiny", tlas=False)


def dump(root):
    sys.path.insert(0, os.path.abspath(root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    assets = importlib.import_module("ray-and-pathtracer_amd.assets")
    builders = [("mixed_small", lambda b, rt: scenes.mixed_small(b, rt=rt)), ("scene3", lambda b, rt: scenes.scene3(b, rt=rt, force_diffuse=False)),
                ("pretty_tlas4", lambda b, rt: scenes.pretty_tlas(b, rt=rt, n_instances=4)), ("shiny0.25", lambda b, rt: shiny(assets, b, rt))]

    def renderer(build, rt=True, **env):
        for k in ("RT_MEGA", "RT_STREAM"):
            os.environ.pop(k, None)
        os.environ.update(env)  # read when the context is created
        r = ha.HostRenderer(W, H)
        d = build(r.scene, rt)
        r.commit()
        if "camera" in d:
            c = d["camera"]
            r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        return r

    def put(name, a):
        print("%s %s" % (hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest(), name), flush=True)

    for name, build in builders:
        for mode, frames, var, values in ((ha.RT_MODE_WHITTED, 1, "RT_MEGA", ("0", "1")), (ha.RT_MODE_PATH, 4, "RT_STREAM", ("0", None))):
            for v in values:
                r = renderer(build, **({var: v} if v is not None else {}))
                r.render(mode, 0, frames)
                put("%s %s %s" % (name, "whitted" if mode == ha.RT_MODE_WHITTED else "path", "%s=%s" % (var, v) if v is not None else "default"), r.accumulator())
                r.close()
        r = renderer(build)
        try:
            r.qlearn_enable(8, QBOX[0], QBOX[1], 0.3, 0.2, 1.0, 0)
            r.render(ha.RT_MODE_PATH, 0, 4)
            put("%s path qlearn" % name, r.accumulator())
        except RuntimeError as e:  # a scene whose path mode runs the general kernel (the shiny floor) has no sampler: the entry records the refusal
            if "error %d" % ha.RT_E_UNSUPPORTED not in str(e):
                raise
            put("%s path qlearn (RT_E_UNSUPPORTED)" % name, np.frombuffer(b"RT_E_UNSUPPORTED", np.uint8))
        r.close()
        for flag in (True, False):
            r = renderer(build, rt=flag)
            O, D = r.sample_rays(0)
            r.scene.set_raytracer(flag)
            r.set_scene_raytracer(1 if flag else 0)
            for mode in (ha.RT_MODE_WHITTED, ha.RT_MODE_PATH):
                for depth in (1, 2, 4):
                    put("%s trace %s flag=%d depth=%d" % (name, "whitted" if mode == ha.RT_MODE_WHITTED else "path", flag, depth),
                        r.trace_batch(mode, O, D, depth=depth, seed_base=4242, energy=(0.9, 0.8, 0.7)))
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the checkout compared against")
    ap.add_argument("--json", default=None)
    ap.add_argument("--dump", metavar="ROOT", help="(the child process: print ROOT's digests)")
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    sides = {}
    for side, root in (("parent", a.parent), ("this", HERE)):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", root], check=True, timeout=600, stdout=subprocess.PIPE, text=True).stdout
        sides[side] = dict((l.split(" ", 1)[1], l.split(" ", 1)[0]) for l in out.splitlines() if len(l.split(" ", 1)[0]) == 64)
    names = sorted(set(sides["parent"]) | set(sides["this"]))
    differing = [n for n in names if sides["parent"].get(n) != sides["this"].get(n)]
    res = dict(size="%dx%d" % (W, H), entries=len(names), differing=differing, bit_equal=not differing and len(names) > 0,
               digests=[dict(entry=n, parent=sides["parent"].get(n), this=sides["this"].get(n)) for n in names])
    print(json.dumps(dict(res, digests=len(names))))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    return 0 if res["bit_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
