"""What following instance motion costs: k_reproject_motion beside k_reproject, on config 3's scene (pretty_tlas, 8 instances) at 1920x1080,
the frame of profiles/reproject_bench.py.
  python3 profiles/reproject_motion_bench.py [--rounds N] [--json out.json] [--parent parent.json]      (GPU box, repository root)
  python3 profiles/reproject_motion_bench.py --root <checkout of the parent commit> --baseline --json parent.json
Every figure is the library's own HIP-event time of the call (rt_set_profiling: k_reproject, k_reproject_motion, k_primary_aovs and the
capture's copies are each one launch of rt_profile.query), after a warm-up of every variant, N rounds with the variants taken in turn within
a round; reported as median, minimum, maximum and every value.
  reproject                     rt_reproject (k_reproject: the same instructions as the parent commit's) from a history nothing has moved since
  motion_none / _one / _all     rt_reproject_motion with no, one and all eight instances moved since the capture (a turn of 0.05 and a shift of
                                0.1), the camera moved by 0.05 as in reproject_bench.py
  each once with the default parameters (the instances are glass and metal: not eligible, so their pixels leave before the transforms are
  read) and once with carry_view_dependent (every hit pixel is eligible: the moved instances' pixels read both records and do the arithmetic)
  history_capture, render_aovs  the calls that got one more 4-byte array per pixel; --baseline measures these two alone on another checkout's
                                library (the parent commit's), --parent embeds that file's figures
--quality: instead of the timings, the experiment of tests/reproject_motion_shapes.py (what a carry across an instance move is worth: its
quality_scene at 64 x 40), as tests/test_gpu_reproject_motion.py runs it."""
import argparse
import importlib
import json
import os
import sys

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
    ha.build()
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    if a.quality:
        import reproject_motion_shapes as shapes
        q = shapes.QUALITY
        r = ha.HostRenderer(q["width"], q["height"])
        shapes.quality_scene(r.scene)
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

    def query_ms(call):
        r.set_profiling(True)
        r.profile()
        call()
        ms = r.profile()["query"]["ms"]
        r.set_profiling(False)
        return ms

    def capture_and_aovs(cap, aov):
        r.set_camera(*A)
        r.render_aovs(0.001)
        cap.append(query_ms(r.history_capture))
        r.set_camera(*B)
        aov.append(query_ms(lambda: r.render_aovs(0.001)))

    cap, aov = [], []
    capture_and_aovs([], [])  # allocation and first launches
    out = dict(width=w, height=h, pixels=w * h, rounds=a.rounds, build=r.build_info())
    if a.baseline:
        for _ in range(a.rounds):
            capture_and_aovs(cap, aov)
        out.update(history_capture_ms=summary(cap), render_aovs_ms=summary(aov))
        r.close()
        return out

    import reproject_motion_shapes as shapes
    n = 8
    dumps = [r.scene.instance_dump(i) for i in range(n)]
    blas, base = [int(x["blas"]) for x in dumps], [np.asarray(x["T"], np.float32).reshape(16) for x in dumps]
    moved = [shapes.translated(shapes.turned(T, 0.05), (0.1, 0.0, 0.0)) for T in base]
    states = dict(none=base, one=moved[:1] + base[1:], all=moved)
    sets = dict(default=None, view_dependent=dict(carry_view_dependent=1))
    times = {p: {k: [] for k in ("reproject", "motion_none", "motion_one", "motion_all")} for p in sets}
    carried = {p: {} for p in sets}
    for rnd in range(a.rounds + 1):  # round 0: the warm-up of every variant, not kept
        keep = rnd > 0
        assert r.set_instances(0, shapes.records(ha, blas, base)) == 0
        capture_and_aovs(cap if keep else [], aov if keep else [])
        for p, P in sets.items():
            ms = query_ms(lambda: carried[p].__setitem__("reproject", r.reproject(P)))
            if keep:
                times[p]["reproject"].append(ms)
        for name, Ts in states.items():
            assert r.set_instances(0, shapes.records(ha, blas, Ts)) == 0
            r.render_aovs(0.001)
            for p, P in sets.items():
                ms = query_ms(lambda: carried[p].__setitem__("motion_" + name, r.reproject_motion(P)))
                if keep:
                    times[p]["motion_" + name].append(ms)
    inst = r.aov_instances()
    out.update(instance_pixels_share=round(float((inst >= 0).mean()), 4), first_instance_pixels_share=round(float((inst == 0).mean()), 4),
               history_capture_ms=summary(cap), render_aovs_ms=summary(aov))
    for p in sets:
        out[p] = {k: dict(summary(v), carried_share=round(carried[p][k] / (w * h), 4)) for k, v in times[p].items()}
        base_ms = out[p]["reproject"]["median"]
        for k in ("motion_none", "motion_one", "motion_all"):
            out[p][k]["over_reproject"] = round(out[p][k]["median"] / base_ms, 3)
    if a.parent:
        out["parent"] = json.load(open(a.parent))
    r.close()
    return out


if __name__ == "__main__":
    main()
