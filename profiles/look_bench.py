"""rt_set_lights, rt_set_materials and rt_set_sky against the rt_upload_scene they replace, on the out-of-cache terrain (8.4 M triangles, no
TLAS), pretty_tlas (8 instances) and bigb_instanced (16 instances of BigB).
  python3 profiles/look_bench.py [--reps N] [--terrain-n N] [--only SCENE] [--json profiles/look_bench.json]   (GPU box, repository root)
One process, one context per scene.  After --warmup untimed rounds, every round times, each as wall milliseconds of the call followed by
rt_synchronize (the stream is drained before the clock starts):
  set_lights              rt_set_lights: the scene's table with another strength (the first call of a scene, which allocates, is a warm-up)
  set_materials_same      rt_set_materials of the whole table, colours changed, every type kept: the table copy alone
  set_materials_retype    rt_set_materials of the whole table with every type rotated: the copy and k_retype_prims over every record
  set_sky                 rt_set_sky with another image of the uploaded size (a 64 x 32 one where the scene has none)
  upload_scene            rt_upload_scene of the description (--upload-reps rounds only: the terrain's takes seconds); it also puts the
                          uploaded types back, so that the next round's retype changes every record again
Each series is reported as median, min, max and the 10th / 90th percentiles.  One more call of each kind runs under rt_set_profiling: its
rt_profile.query entry is the device time; for the retype the records k_retype_prims visits (64 bytes each: prims[] of all BLASes, the
brute-force records, rt_set_time's originals) over that time is its achieved rate.  The result is stamped with rt_build_info /
rt_tuning_info."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = [("terrain", None, 1920, 1080, True), ("pretty_tlas", dict(n_instances=8), 1920, 1080, False), ("bigb_instanced", dict(n=16), 3840, 2160, False)]


class RtBlas(C.Structure):  # include/rt_amd.h rt_blas
    _fields_ = [("nodes", C.c_void_p), ("nodes_used", C.c_uint32), ("prim_idx", C.c_void_p), ("n_prims", C.c_uint32), ("tris", C.c_void_p), ("n_tri", C.c_uint32),
                ("spheres", C.c_void_p), ("n_sph", C.c_uint32), ("planes", C.c_void_p), ("n_pla", C.c_uint32)]


class RtSceneDesc(C.Structure):  # include/rt_amd.h rt_scene_desc
    _fields_ = [("use_tlas", C.c_int32), ("blas", C.c_void_p), ("n_blas", C.c_uint32), ("instances", C.c_void_p), ("n_instances", C.c_uint32),
                ("tlas_nodes", C.c_void_p), ("tlas_nodes_used", C.c_uint32), ("brute_spheres", C.c_void_p), ("n_brute_spheres", C.c_uint32),
                ("brute_planes", C.c_void_p), ("n_brute_planes", C.c_uint32), ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32), ("sky_pixels", C.c_void_p), ("sky_w", C.c_int32), ("sky_h", C.c_int32), ("sky_n", C.c_int32)]


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4), n=len(v))


def records(ptr, dtype, n):
    return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype).copy() if ptr and n else np.zeros(0, dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--upload-reps", type=int, default=3)
    ap.add_argument("--terrain-n", type=int, default=2048)
    ap.add_argument("--only", default="", help="one scene by name")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    out = dict(reps=a.reps, warmup=a.warmup, upload_reps=a.upload_reps, scenes={})
    if a.json and os.path.exists(a.json):  # scenes measured by an earlier call (--only) stay
        out["scenes"] = json.load(open(a.json)).get("scenes", {})
    for name, kw, w, h, dev_build in SCENES:
        if a.only and a.only != name:
            continue
        r = ha.HostRenderer(w, h)
        if dev_build:
            r.scene.device_build(r.ctx)
        scenes.REGISTRY[name](r.scene, **(dict(n=a.terrain_n) if kw is None else kw))
        r.commit()
        r.synchronize()
        out["build"] = r.build_info()
        ptr = r.scene.describe()  # valid while the scene is not described again
        d = RtSceneDesc.from_address(ptr.value)
        blas = (RtBlas * d.n_blas).from_address(d.blas)
        mats0, lights0 = records(d.materials, ha.RT_MATERIAL_DTYPE, d.n_materials), records(d.lights, ha.RT_LIGHT_DTYPE, d.n_lights)
        sky_shape = (d.sky_h, d.sky_w, d.sky_n) if d.sky_pixels and d.sky_w > 0 and d.sky_h > 0 else (32, 64, 3)
        prim_records = sum(b.n_prims for b in blas)
        visited = prim_records + ((d.n_brute_spheres + d.n_brute_planes) if d.use_tlas else blas[0].n_prims)  # + the brute-force records, or rt_set_time's originals
        rng = np.random.default_rng(1)

        def edits(k):
            lights = lights0.copy()
            lights["strength"] *= np.float32(1.0 + 0.01 * (k + 1))
            same = mats0.copy()
            same["col"] = np.clip(same["col"] * np.float32(1.0 - 0.002 * (k + 1)), 0, 1)
            retype = same.copy()
            retype["type"] = (mats0["type"] - 1 + 1 + k % 2) % 3 + 1  # never the uploaded type
            retype["shinieness"] = 0
            return lights, same, retype, rng.integers(0, 256, sky_shape, dtype=np.uint8)

        def timed(call):
            r.synchronize()
            t0 = time.perf_counter()
            rc = call()
            r.synchronize()
            assert rc in (0, None), ha.rt_lib().rt_last_error(r.ctx)
            return (time.perf_counter() - t0) * 1e3

        keys = ("set_lights", "set_materials_same", "set_materials_retype", "set_sky")
        series = {k: [] for k in keys + ("upload_scene",)}
        for k in range(a.warmup + a.reps):
            lights, same, retype, sky = edits(k)
            ms = dict(set_lights=timed(lambda: r.set_lights(lights)), set_materials_same=timed(lambda: r.set_materials(0, same)),
                      set_materials_retype=timed(lambda: r.set_materials(0, retype)), set_sky=timed(lambda: r.set_sky(sky)))
            if k >= a.warmup:
                for key in keys:
                    series[key].append(ms[key])
            if k < a.warmup + a.upload_reps:
                up = timed(lambda: r.upload_desc(ptr))
                if k >= a.warmup:
                    series["upload_scene"].append(up)
            else:
                assert r.set_materials(0, mats0) == 0  # the uploaded types again, outside the clock
        # what the device takes: one rt_profile.query entry per call
        lights, same, retype, sky = edits(a.warmup + a.reps)
        r.set_profiling(True)
        device = {}
        for key, call in (("set_lights", lambda: r.set_lights(lights)), ("set_materials_same", lambda: r.set_materials(0, same)),
                          ("set_materials_retype", lambda: r.set_materials(0, retype)), ("set_sky", lambda: r.set_sky(sky))):
            r.profile()
            assert call() == 0
            q = r.profile()["query"]
            assert q["launches"] == 1
            device[key] = round(q["ms"], 4)
        r.set_profiling(False)
        res = {k: summary(s) for k, s in series.items()}
        res["device_ms_of_one_call"] = device
        res["size"], res["materials"], res["lights"], res["sky"] = [w, h], int(d.n_materials), int(d.n_lights), list(sky_shape)
        res["primitive_records"], res["records_retype_visits"] = int(prim_records), int(visited)
        res["retype_bytes"] = int(visited) * 64
        res["retype_GB_per_s_device"] = round(visited * 64 / (device["set_materials_retype"] * 1e-3) / 1e9, 2) if device["set_materials_retype"] > 0 else None
        res["retype_GB_per_s_wall"] = round(visited * 64 / (res["set_materials_retype"]["median"] * 1e-3) / 1e9, 2)
        for key in keys:
            res["upload_over_" + key] = round(res["upload_scene"]["median"] / res[key]["median"], 1)
        out["scenes"][name] = res
        print(name, json.dumps(res), flush=True)
        r.close()
    sc = out["scenes"]
    if "terrain" in sc and "pretty_tlas" in sc:  # an edit without a type change: does its time follow the size of the scene?
        out["same_type_edit_terrain_over_pretty_tlas"] = {
            k: dict(ratio_of_medians=round(sc["terrain"][k]["median"] / sc["pretty_tlas"][k]["median"], 3), terrain=[sc["terrain"][k][q] for q in ("p10", "median", "p90")],
                    pretty_tlas=[sc["pretty_tlas"][k][q] for q in ("p10", "median", "p90")]) for k in ("set_lights", "set_materials_same")}
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
