"""What following a deformation costs: k_reproject_deform beside k_reproject_motion, the G-buffer's fifth array, and rt_set_triangles under a
live history, on config 3's scene (pretty_tlas, 8 instances of two BLASes) at 1920x1080, the frame of profiles/reproject_motion_bench.py.
  python3 profiles/reproject_deform_bench.py [--rounds N] [--json out.json] [--parent parent.json]      (GPU box, repository root)
  python3 profiles/reproject_deform_bench.py --root <checkout of the parent commit> --baseline --json parent.json
Kernel figures are the library's own HIP-event times (rt_set_profiling: k_reproject_motion, k_reproject_deform, k_primary_aovs and the
capture's copies are each one launch of rt_profile.query); rt_set_triangles is wall time around the call and an rt_synchronize (the copy on
first write sits in front of the call's profiled part).  A warm-up of every variant, then N rounds with the variants taken in turn within a
round; reported as median, minimum, maximum and every value.
  motion                 rt_reproject_motion from a history nothing has moved or deformed since (the camera moved by 0.05)
  deform_none            rt_reproject_deform on the same frame: no BLAS has a kept copy (one 4-byte load and the table lookup per pixel more)
  deform_same            both BLASes rewritten with the same bits: every instance pixel reads and compares its two records, none differs
  deform_half / _all     BLAS 0 / both BLASes shrunk by 5 %: that share of the instance pixels runs the barycentric path
  each with the default parameters (the instances are glass and metal: not eligible, so their pixels leave before the records are read) and
  with carry_view_dependent (every hit pixel is eligible)
  set_triangles_*        BLAS 0 (12,584 triangles): without a history, the first call after a capture (one more device copy of its
                         records), the second call after it
  render_aovs, history_capture, motion and set_triangles_plain are what --baseline measures on another checkout's library (the parent
  commit's); --parent embeds that file's figures.
--quality: instead of the timings, the experiment of tests/reproject_deform_shapes.py (what a carry across a deformation is worth), as
tests/test_gpu_reproject_deform.py runs it."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4), all=[round(float(x), 4) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    if not (os.path.exists(ha.RT_SO) and os.path.exists(ha.HOST_SO)):
        ha.build()
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    if a.quality:
        import reproject_deform_shapes as shapes
        import reproject_motion_shapes as ms
        q = shapes.QUALITY
        r = ha.HostRenderer(q["width"], q["height"])
        ms.quality_scene(r.scene)
        r.scene.set_raytracer(False)
        r.commit()
        r.stats_enable(True)
        with np.errstate(all="ignore"):
            out = shapes.quality(ha, r)
        out["build"] = r.build_info()
        r.close()
    else:
        out = timings(ha, scenes, a)
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


def timings(ha, scenes, a):
    import triangles_desc as td
    import triangles_ref as tr
    w, h = 1920, 1080
    PATH = ha.RT_MODE_PATH
    r = ha.HostRenderer(w, h)
    d = scenes.pretty_tlas(r.scene, 8)
    r.scene.set_raytracer(False)
    r.commit()
    c = d["camera"]
    A = np.array([c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"]], np.float32)
    B = (A + np.float32([0.05, 0, 0])).astype(np.float32)
    r.set_camera(*A)
    r.stats_enable(True)
    r.render(PATH, 0, 16)
    desc = td.Desc(ha, r.scene)
    same = [np.ascontiguousarray(t) for t in desc.tris]

    def shrunk(k):
        """BLAS k 5 % nearer to its origin; the two closing triangles of a .tri mesh (every vertex at 999) stay, with N = 0"""
        v9 = tr.v9_of(desc.tris[k])
        new = np.concatenate([tr.scale(v9[:-2], 0.95), v9[-2:]])
        return np.ascontiguousarray(tr.triangles(desc.tris[k], new, tr.sentinel_normals(new)))

    small = [shrunk(k) for k in range(len(desc.tris))]

    def query_ms(call):
        r.set_profiling(True)
        r.profile()
        call()
        ms = r.profile()["query"]["ms"]
        r.set_profiling(False)
        return ms

    def wall_ms(call):
        r.synchronize()
        t0 = time.perf_counter()
        call()
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def capture_and_aovs(cap, aov):
        r.set_camera(*A)
        r.render_aovs(0.001)
        cap.append(query_ms(r.history_capture))
        r.set_camera(*B)
        aov.append(query_ms(lambda: r.render_aovs(0.001)))

    def send(k, tris):
        assert r.set_triangles(k, tris) == 0

    sets = dict(default=None, view_dependent=dict(carry_view_dependent=1))
    out = dict(width=w, height=h, pixels=w * h, rounds=a.rounds, build=r.build_info(), blas_triangles=[len(t) for t in desc.tris])
    cap, aov, plain = [], [], []
    motion = {p: [] for p in sets}
    carried = {p: {} for p in sets}
    names = ("deform_none", "deform_same", "deform_half", "deform_all")
    times = {p: {k: [] for k in names} for p in sets}
    first, second = [], []
    for rnd in range(a.rounds + 1):  # round 0: the warm-up of every variant, not kept
        keep = rnd > 0
        # without a history: rt_set_triangles as the parent runs it
        r.stats_enable(False)
        ms = wall_ms(lambda: send(0, small[0]))
        ms2 = wall_ms(lambda: send(0, same[0]))
        if keep:
            plain += [ms, ms2]
        r.stats_enable(True)
        r.set_camera(*A)
        r.render(PATH, 0, 4)
        capture_and_aovs(cap if keep else [], aov if keep else [])
        for p, P in sets.items():
            ms = query_ms(lambda: carried[p].__setitem__("motion", r.reproject_motion(P)))
            if keep:
                motion[p].append(ms)
        if a.baseline:
            continue
        states = dict(deform_none=[], deform_same=[(0, same[0]), (1, same[1])], deform_half=[(0, small[0])], deform_all=[(1, small[1])])
        for name in names:
            for j, (k, tris) in enumerate(states[name]):
                ms = wall_ms(lambda: send(k, tris))
                if keep and name == "deform_same" and k == 0:
                    first.append(ms)      # the first rewrite of BLAS 0 after the capture: the copy on first write
            if name == "deform_same":
                ms = wall_ms(lambda: send(0, same[0]))
                if keep:
                    second.append(ms)     # the second: nothing more than without a history
            r.render_aovs(0.001)
            for p, P in sets.items():
                ms = query_ms(lambda: carried[p].__setitem__(name, r.reproject_deform(P)))
                if keep:
                    times[p][name].append(ms)
        for k in range(len(same)):
            send(k, same[k])
    out.update(history_capture_ms=summary(cap), render_aovs_ms=summary(aov), set_triangles_plain_ms=summary(plain))
    for p in sets:
        out[p] = dict(motion=dict(summary(motion[p]), carried_share=round(carried[p]["motion"] / (w * h), 4)))
    if not a.baseline:
        inst = r.aov_instances()
        blas_of = np.array([int(r.scene.instance_dump(i)["blas"]) for i in range(8)])
        on0 = (inst >= 0) & (blas_of[np.maximum(inst, 0)] == 0)
        out.update(instance_pixels_share=round(float((inst >= 0).mean()), 4), blas0_pixels_share=round(float(on0.mean()), 4),
                   set_triangles_first_after_capture_ms=summary(first), set_triangles_second_after_capture_ms=summary(second))
        for p in sets:
            for k in names:
                out[p][k] = dict(summary(times[p][k]), carried_share=round(carried[p][k] / (w * h), 4), over_motion=round(float(np.median(times[p][k])) / out[p]["motion"]["median"], 3))
    if a.parent:
        out["parent"] = json.load(open(a.parent))
    r.close()
    return out


if __name__ == "__main__":
    main()
