"""rt_set_triangles against the rt_upload_scene it replaces: one BigB BLAS of bigb_instanced (16 instances, 3840x2160), the one mesh of
pretty_tlas (8 instances, 1920x1080) and the out-of-cache terrain without a TLAS (2 n^2 triangles, where the wide refit levels dominate).
  python3 profiles/triangles_bench.py [--reps N] [--terrain-n N] [--json profiles/triangles_bench.json]   (GPU box, repository root)
One process, one context per scene.  Every repetition displaces every vertex of the mesh a little differently (a travelling sine wave along
y) and recomputes the normals as Triangle::update does.  After --warmup untimed repetitions, wall milliseconds over --reps repetitions of
  set_triangles   rt_set_triangles of the whole BLAS followed by rt_synchronize: everything the call queued has run
  upload          rt_upload_scene of the updated description followed by rt_synchronize -- what a caller did before this call.  The
                  description is made by the host mirror BEFORE the clock starts (the mesh rewritten, bvh::Refit, the instances' boxes,
                  the TLAS, Scene::Describe are not charged to it)
  tick            Renderer::Tick, one path frame, nothing deformed
  tick_deformed   the mesh rewritten + Scene::CommitTriangles (host Refit, rt_set_triangles, the TLAS read back) + Renderer::Tick
Each series is reported as median, min, max and the 10th / 90th percentiles; ratio = upload median / set_triangles median.
upload_first_ms is the scene's first rt_upload_scene (Scene::Commit), which now also keeps the inverse of prim_idx and every BLAS's refit
order.  The result is stamped with rt_build_info / rt_tuning_info of the library that was measured."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
f32 = np.float32


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4), n=len(v))


def normals(v9):
    """Triangle::update: N = normalize(cross(v1 - v0, v2 - v0)) in f32"""
    v = v9.reshape(-1, 3, 3)
    c = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(f32)
    with np.errstate(all="ignore"):
        return (c * (f32(1) / np.sqrt((c * c).sum(1, dtype=f32), dtype=f32))[:, None]).astype(f32)


class RtBlas(C.Structure):  # include/rt_amd.h rt_blas
    _fields_ = [("nodes", C.c_void_p), ("nodes_used", C.c_uint32), ("prim_idx", C.c_void_p), ("n_prims", C.c_uint32), ("tris", C.c_void_p), ("n_tri", C.c_uint32),
                ("spheres", C.c_void_p), ("n_sph", C.c_uint32), ("planes", C.c_void_p), ("n_pla", C.c_uint32)]


def read_tris(ha, desc, blas):
    """the rt_triangle records of BLAS 'blas' of an rt_scene_desc (its second and third fields: blas, n_blas), as a copy"""
    class Head(C.Structure):
        _fields_ = [("use_tlas", C.c_int32), ("blas", C.c_void_p), ("n_blas", C.c_uint32)]
    head = Head.from_address(desc.value)
    b = (RtBlas * head.n_blas).from_address(head.blas)[blas]
    return np.frombuffer(C.string_at(b.tris, b.n_tri * ha.RT_TRIANGLE_DTYPE.itemsize), dtype=ha.RT_TRIANGLE_DTYPE).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--terrain-n", type=int, default=2048)
    ap.add_argument("--terrain-reps", type=int, default=5, help="the terrain's re-upload takes seconds: fewer repetitions")
    ap.add_argument("--only", default="", help="one scene by name")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    # (scene, arguments, width, height, BLAS on the device, BLAS for the host mirror, build on the device)
    SCENES = [("bigb_instanced", dict(n=16), 3840, 2160, 0, 0, False), ("pretty_tlas", dict(n_instances=8), 1920, 1080, 0, 0, False),
              ("terrain", dict(n=a.terrain_n), 1920, 1080, 0, -1, True)]
    out = dict(reps=a.reps, warmup=a.warmup, scenes={})
    for name, kw, w, h, blas, host_blas, dev_build in SCENES:
        if a.only and a.only != name:
            continue
        reps = min(a.reps, a.terrain_reps) if name == "terrain" else a.reps
        warm = min(a.warmup, 1) if name == "terrain" else a.warmup
        r = ha.HostRenderer(w, h)
        if dev_build:
            r.scene.device_build(r.ctx)
        d = scenes.REGISTRY[name](r.scene, **kw)
        r.synchronize()
        t0 = time.perf_counter()
        r.commit()
        r.synchronize()
        first_upload = (time.perf_counter() - t0) * 1e3
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        out.setdefault("build", r.build_info())
        s = r.scene
        # the BLAS's triangles as uploaded: every mesh of a scene BVH, or the one mesh of an instanced BLAS
        meshes = list(range(s.n_meshes())) if host_blas < 0 else [0]
        base = np.concatenate([s.mesh_tris(m)[0][:, :9] for m in meshes]).astype(f32)
        counts = [len(s.mesh_tris(m)[0]) for m in meshes]
        tris = np.zeros(len(base), dtype=ha.RT_TRIANGLE_DTYPE)
        old = read_tris(ha, s.describe(), blas)
        tris["obj_idx"], tris["material"] = old["obj_idx"], old["material"]
        extent = float(np.abs(base).max())
        step = [0]

        def deformed():
            """every vertex pushed along x by a sine of its y: a different phase every time"""
            step[0] += 1
            v = base.reshape(-1, 3).copy()
            v[:, 0] += (f32(0.01 * extent) * np.sin(v[:, 1] * f32(3.0 / max(extent, 1e-6)) + f32(0.3 * step[0]))).astype(f32)
            v9 = v.reshape(-1, 9)
            tris["v0"], tris["v1"], tris["v2"], tris["N"] = v9[:, 0:3], v9[:, 3:6], v9[:, 6:9], normals(v9)
            return v9

        def to_mirror(v9):
            at = 0
            for m, n in zip(meshes, counts):
                s.set_mesh_vertices(m, v9[at:at + n])
                at += n

        series = dict(set_triangles=[], upload=[], tick=[], tick_deformed=[])
        for k in range(warm + reps):
            deformed()
            r.synchronize()
            t0 = time.perf_counter()
            assert r.set_triangles(blas, tris) == 0
            r.synchronize()
            if k >= warm:
                series["set_triangles"].append((time.perf_counter() - t0) * 1e3)
        for k in range(warm + reps):
            to_mirror(deformed())
            s.commit_triangles(host_blas)  # the mirror after the deformation: refitted nodes, fresh boxes, the device's TLAS
            desc = s.describe()
            r.synchronize()
            t0 = time.perf_counter()
            r.upload_desc(desc)
            r.synchronize()
            if k >= warm:
                series["upload"].append((time.perf_counter() - t0) * 1e3)
        s.set_raytracer(False)  # path Ticks
        for key in ("tick", "tick_deformed"):
            for k in range(warm + reps):
                v9 = deformed()
                r.synchronize()
                t0 = time.perf_counter()
                if key == "tick_deformed":
                    to_mirror(v9)
                    s.commit_triangles(host_blas)
                r.tick()
                r.synchronize()
                if k >= warm:
                    series[key].append((time.perf_counter() - t0) * 1e3)
        res = {k: summary(v) for k, v in series.items()}
        res["ratio_upload_over_set_triangles"] = round(res["upload"]["median"] / res["set_triangles"]["median"], 2)
        res["tick_cost_of_a_deformation_ms"] = round(res["tick_deformed"]["median"] - res["tick"]["median"], 4)
        res["upload_first_ms"] = round(first_upload, 3)
        res["size"], res["triangles"], res["host_link_bytes"] = [w, h], len(tris), int(tris.nbytes)
        out["scenes"][name] = res
        print(name, json.dumps(res), flush=True)
        r.close()
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
