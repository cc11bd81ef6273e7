"""rt_set_instance_list against the two calls beside it, on pretty_tlas (8 instances, two BLASes of 12,584 triangles) and on two 16-instance
scenes that differ in the size of their BLASes alone: bigb16 (BigB.obj, 11,830 triangles, and one instance of lowBigB) and lowbigb16
(lowBigB.obj, 14 triangles, and one instance of ico), under the same transforms.
  python3 profiles/instance_list_bench.py [--reps N] [--only SCENE] [--json profiles/instance_list_bench.json]   (GPU box, repository root)
One process, one context per scene.  Three edits of the uploaded list L of n instances: grow (L and a copy of its last instance, moved), shrink
(L without its last instance) and repoint (L with instance 0 on the other BLAS).  After --warmup untimed rounds, every round times for each
edit, each as wall milliseconds of the call followed by rt_synchronize (the stream is drained before the clock starts):
  set_instance_list   rt_set_instance_list of the edited list, bounds6 NULL, on a context that holds L
  set_instances_all   rt_set_instances over ALL instances of the edited list, bounds6 NULL, on the context as the list call left it: the
                      same device work (k_instance_bounds, k_build_tlas, the read-back, k_pack_tlas) without a change of the list -- the floor
  upload_scene        rt_upload_scene of the updated description (L's with instances / n_instances replaced and tlas_nodes = rt_download_tlas
                      after the list call); --upload-reps rounds only
and puts L back outside the clock.  Each series is reported as median, min, max and the 10th / 90th percentiles; one more call of each
edit runs under rt_set_profiling (device ms of its rt_profile.query entry).  The result is stamped with rt_build_info / rt_tuning_info."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class RtSceneDesc(C.Structure):  # include/rt_amd.h rt_scene_desc
    _fields_ = [("use_tlas", C.c_int32), ("blas", C.c_void_p), ("n_blas", C.c_uint32), ("instances", C.c_void_p), ("n_instances", C.c_uint32),
                ("tlas_nodes", C.c_void_p), ("tlas_nodes_used", C.c_uint32), ("brute_spheres", C.c_void_p), ("n_brute_spheres", C.c_uint32),
                ("brute_planes", C.c_void_p), ("n_brute_planes", C.c_uint32), ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32), ("sky_pixels", C.c_void_p), ("sky_w", C.c_int32), ("sky_h", C.c_int32), ("sky_n", C.c_int32)]


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4), n=len(v))


def sixteen(b, assets, big, small):
    """15 instances of mesh 'big' and one of 'small' on a 4 x 4 grid (scenes.bigb_instanced's placements)"""
    red, gold, floor = b.diffuse(0.8, (1, 0, 0), 0.0, 1, 1), b.diffuse(0.8, (1, 0.84, 0), 0.8, 0.2, 1), b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
    m0 = b.mesh_obj(1, assets.obj_path(big), red, (0, 0.5, 0), 1)
    m1 = b.mesh_obj(2, assets.obj_path(small), gold, (0, 0.5, 0), 1)
    b.plane(0, floor, (0, 1, 0), 0)
    inst = [((m1 if i == 5 else m0), b.trs((-3.0 + 2.0 * (i % 4), 0.0, 2.0 + 2.0 * (i // 4)), 1.5, 0.0, 0.4 * i, 0.0)) for i in range(16)]
    b.build_tlas(0, inst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--only", default="", help="one scene by name")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    assets = importlib.import_module("ray-and-pathtracer_amd.assets")
    builders = [("pretty_tlas", lambda b: scenes.pretty_tlas(b, 8)), ("bigb16", lambda b: sixteen(b, assets, "BigB", "lowBigB")),
                ("lowbigb16", lambda b: sixteen(b, assets, "lowBigB", "ico"))]
    out = dict(reps=a.reps, warmup=a.warmup, upload_reps=a.upload_reps, bounds6="NULL", scenes={})
    for name, build in builders:
        if a.only and a.only != name:
            continue
        r = ha.HostRenderer(64, 64)
        build(r.scene)
        r.commit()
        r.synchronize()
        out["build"] = r.build_info()
        ptr = r.scene.describe()  # valid while the scene is not described again
        d0 = RtSceneDesc.from_address(ptr.value)
        n, n_blas = int(d0.n_instances), int(d0.n_blas)
        base = np.frombuffer(C.string_at(d0.instances, n * ha.RT_INSTANCE_DTYPE.itemsize), dtype=ha.RT_INSTANCE_DTYPE).copy()

        def inv(T):  # mat4::Inverted, as SetTransform takes it
            o = np.zeros(16, np.float32)
            ha.host_lib().rth_mat4_inverse(T.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p))
            return o

        def edited(kind, k):
            """the edited list of round k (the moved copy's place changes with k, so that no round repeats the one before)"""
            if kind == "shrink":
                return base[:-1].copy()
            lst = base.copy() if kind == "repoint" else np.concatenate([base, base[-1:]])
            if kind == "repoint":
                lst["blas"][0] = (lst["blas"][0] + 1) % n_blas
            else:
                T = lst["transform"][-1].copy()
                T[3] += np.float32(1.0 + 0.01 * k)  # row 0's translation
                lst["transform"][-1], lst["inv_transform"][-1] = T, inv(np.ascontiguousarray(T))
            return lst

        def timed(call):
            r.synchronize()
            t0 = time.perf_counter()
            rc = call()
            r.synchronize()
            assert rc in (0, None), ha.rt_lib().rt_last_error(r.ctx)
            return (time.perf_counter() - t0) * 1e3

        def updated_desc(lst):
            d = RtSceneDesc.from_buffer_copy(d0)
            nodes = np.ascontiguousarray(r.download_tlas())
            d.instances, d.n_instances, d.tlas_nodes, d.tlas_nodes_used = lst.ctypes.data, len(lst), nodes.ctypes.data, len(nodes)
            return d, nodes

        kinds = ("grow", "shrink", "repoint")
        series = {kind: dict(set_instance_list=[], set_instances_all=[], upload_scene=[]) for kind in kinds}
        for k in range(a.warmup + a.reps):
            for kind in kinds:
                lst = edited(kind, k)
                ms_list = timed(lambda: r.set_instance_list(lst))
                ms_all = timed(lambda: r.set_instances(0, lst))
                ms_up = None
                if k < a.warmup + a.upload_reps:
                    d, nodes = updated_desc(lst)
                    ms_up = timed(lambda: r.upload_desc(C.c_void_p(C.addressof(d))))
                    assert r.upload_desc(ptr) is None  # L's own scene again, outside the clock
                else:
                    assert r.set_instance_list(base) == 0  # L again, outside the clock
                if k >= a.warmup:
                    series[kind]["set_instance_list"].append(ms_list), series[kind]["set_instances_all"].append(ms_all)
                    if ms_up is not None:
                        series[kind]["upload_scene"].append(ms_up)
        r.set_profiling(True)
        device = {}
        for kind in kinds:
            lst = edited(kind, a.warmup + a.reps)
            r.profile()
            assert r.set_instance_list(lst) == 0
            q = r.profile()["query"]
            assert q["launches"] == 1
            device[kind] = round(q["ms"], 4)
            assert r.set_instance_list(base) == 0
            r.profile()
        r.set_profiling(False)
        res = dict(instances=n, blases=n_blas, device_ms_of_one_list_call=device)
        for kind in kinds:
            s = {key: summary(v) for key, v in series[kind].items()}
            s["list_over_set_instances_all"] = round(s["set_instance_list"]["median"] / s["set_instances_all"]["median"], 3)
            s["upload_over_list"] = round(s["upload_scene"]["median"] / s["set_instance_list"]["median"], 1)
            res[kind] = s
        out["scenes"][name] = res
        print(name, json.dumps(res), flush=True)
        r.close()
    sc = out["scenes"]
    if "bigb16" in sc and "lowbigb16" in sc:  # the same 16 placements over BLASes of 11,830 and of 14 triangles: does the call's time follow their size?
        out["bigb16_over_lowbigb16"] = {kind: dict(ratio_of_medians=round(sc["bigb16"][kind]["set_instance_list"]["median"] / sc["lowbigb16"][kind]["set_instance_list"]["median"], 3),
                                                   bigb16=[sc["bigb16"][kind]["set_instance_list"][q] for q in ("p10", "median", "p90")],
                                                   lowbigb16=[sc["lowbigb16"][kind]["set_instance_list"][q] for q in ("p10", "median", "p90")]) for kind in ("grow", "shrink", "repoint")}
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
