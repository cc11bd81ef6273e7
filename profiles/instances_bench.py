"""rt_set_instances against the rt_upload_scene it replaces, on the two instanced BASELINE scenes at their sizes: pretty_tlas (8 instances,
config 3, 1920x1080) and bigb_instanced (16 instances, config 5, 3840x2160).
  python3 profiles/instances_bench.py [--reps N] [--json profiles/instances_bench.json]   (GPU box, repository root)
One process, one context per scene.  Every repetition turns all instances a little further about y (a different transform every time).
After --warmup untimed repetitions, wall milliseconds over --reps repetitions of
  set_instances        rt_set_instances of all instances (bounds6 NULL), as the call returns: its 4-byte read-back included, its commit
                       kernel still queued
  set_instances_sync   the same followed by rt_synchronize: everything the call queued has run
  upload               rt_upload_scene of the updated description followed by rt_synchronize -- the only way to move an instance before this
                       call.  The description is flattened by the host mirror BEFORE the clock starts (SetTransform, tlas::build and
                       Scene::Describe on the host are not charged to it)
  tick                 Renderer::Tick, one path frame, nothing moved
  tick_moved           bvhInstance::SetTransform of every instance + Scene::CommitInstances + Renderer::Tick
Each series is reported as median, min, max and the 10th / 90th percentiles; ratio = upload median / set_instances_sync median.
The result is stamped with rt_build_info / rt_tuning_info of the library that was measured."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
SCENES = [("pretty_tlas", dict(n_instances=8), 1920, 1080), ("bigb_instanced", dict(n=16), 3840, 2160)]


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    Lh = ha.host_lib()
    out = dict(reps=a.reps, warmup=a.warmup, scenes={})
    for name, kw, w, h in SCENES:
        r = ha.HostRenderer(w, h)
        d = scenes.REGISTRY[name](r.scene, **kw)
        r.commit()
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        out.setdefault("build", r.build_info())
        s = r.scene
        n = kw.get("n_instances", kw.get("n"))
        base = [s.instance_dump(i) for i in range(n)]
        step = [0]

        def moved():
            """every instance's uploaded transform turned a little further about y: (transforms, rt_instance records)"""
            step[0] += 1
            rot = np.eye(4, dtype=np.float32)
            ang = np.float32(0.01 * step[0])
            rot[0, 0], rot[0, 2], rot[2, 0], rot[2, 2] = np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)
            Ts = [(x["T"].reshape(4, 4) @ rot).astype(np.float32).reshape(16) for x in base]
            rec = np.zeros(n, dtype=ha.RT_INSTANCE_DTYPE)
            for i, T in enumerate(Ts):
                inv = np.zeros(16, dtype=np.float32)
                Lh.rth_mat4_inverse(T.ctypes.data, inv.ctypes.data)
                rec[i] = (base[i]["blas"], T, inv)
            return Ts, rec

        Lh.rth_mat4_inverse.argtypes = [ha.C.c_void_p, ha.C.c_void_p]
        series = dict(set_instances=[], set_instances_sync=[], upload=[], tick=[], tick_moved=[])
        for k in range(a.warmup + a.reps):
            keep = k >= a.warmup
            _, rec = moved()
            r.synchronize()
            t0 = time.perf_counter()
            assert r.set_instances(0, rec) == 0
            t1 = time.perf_counter()
            r.synchronize()
            t2 = time.perf_counter()
            if keep:
                series["set_instances"].append((t1 - t0) * 1e3), series["set_instances_sync"].append((t2 - t0) * 1e3)
        for k in range(a.warmup + a.reps):
            Ts, _ = moved()
            s.set_transforms(0, Ts)
            s.rebuild_tlas()
            desc = s.describe()
            r.synchronize()
            t0 = time.perf_counter()
            r.upload_desc(desc)
            r.synchronize()
            if k >= a.warmup:
                series["upload"].append((time.perf_counter() - t0) * 1e3)
        s.set_raytracer(False)  # path Ticks
        for key in ("tick", "tick_moved"):
            for k in range(a.warmup + a.reps):
                Ts, _ = moved()
                r.synchronize()
                t0 = time.perf_counter()
                if key == "tick_moved":
                    s.set_transforms(0, Ts)
                    s.commit_instances()
                r.tick()
                r.synchronize()
                if k >= a.warmup:
                    series[key].append((time.perf_counter() - t0) * 1e3)
        res = {k: summary(v) for k, v in series.items()}
        res["ratio_upload_over_set_instances_sync"] = round(res["upload"]["median"] / res["set_instances_sync"]["median"], 2)
        res["tick_cost_of_a_move_ms"] = round(res["tick_moved"]["median"] - res["tick"]["median"], 4)
        res["size"], res["instances"] = [w, h], n
        out["scenes"][name] = res
        print(name, json.dumps(res))
        r.close()
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
