"""rt_set_vertices and rt_set_vertices_device against the rt_set_triangles they stand beside, on the scenes of profiles/triangles_bench.py:
one BigB BLAS of bigb_instanced (16 instances), the one mesh of pretty_tlas (8 instances) and the out-of-cache terrain without a TLAS.
  python3 profiles/vertices_bench.py [--reps N] [--terrain-n N] [--only SCENE] [--json profiles/vertices_bench.json]   (GPU box, repository root)
  python3 profiles/vertices_bench.py --parent-root DIR ...   also: rt_set_triangles of THIS build against the build under DIR (a checkout of
                                                            the parent commit with its libraries built), in alternated rounds
One process, one context per scene.  Every repetition displaces every vertex a little differently (a travelling sine wave along y).  After
--warmup untimed repetitions, the three calls are timed in alternated rounds (triangles, vertices, device, triangles, ...), each as wall
milliseconds of the call followed by rt_synchronize:
  set_triangles        rt_set_triangles: 56-byte records with the caller's normals
  set_vertices         rt_set_vertices: the vertex array from host memory (the indices were bound once, before the clock)
  set_vertices_device  rt_set_vertices_device: the same array in a torch tensor produced (and synchronised) before the clock starts
and the host-side preparation each needs, timed apart from the call: prep_triangles (displace, expand to records, Triangle::update's
normals in NumPy), prep_vertices (displace), prep_device (the displacement as torch operations on the device, synchronised).
Each series is reported as median, min, max and the 10th / 90th percentiles, with the bytes each call sends over the host link.
The refactor's condition: with --parent-root, child processes of this script time rt_set_triangles alone, this build and the parent's
build turn by turn (--rounds each, the first of a round changing every round); the result holds both summaries over all rounds and whether this build's median lies within the
parent's own p10-p90 band.  The result is stamped with rt_build_info / rt_tuning_info of the library that was measured."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
SCENES = [("bigb_instanced", dict(n=16), 3840, 2160, 0, 0, False), ("pretty_tlas", dict(n_instances=8), 1920, 1080, 0, 0, False),
          ("terrain", None, 1920, 1080, 0, -1, True)]  # (scene, arguments, width, height, BLAS, BLAS for the host mirror, build on the device)


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


def weld(v9):
    """(xyz, idx) of a triangle soup: distinct vertex bit patterns; a regular grid in x and z (the terrain) is indexed by its coordinates"""
    v = np.ascontiguousarray(v9, dtype=f32).reshape(-1, 3)
    xs, zs = np.unique(v[:, 0]), np.unique(v[:, 2])
    if len(xs) * len(zs) < len(v) // 2:
        idx = (np.searchsorted(xs, v[:, 0]) * len(zs) + np.searchsorted(zs, v[:, 2])).astype(np.uint32)
        xyz = np.zeros((len(xs) * len(zs), 3), f32)
        xyz[idx] = v
        if np.array_equal(xyz[idx].view(np.uint32), v.view(np.uint32)):  # one height per (x, z): a height field
            return xyz, idx.reshape(-1, 3)
    keys = v.view(np.dtype((np.void, 12))).reshape(-1)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    return v[first].copy(), np.asarray(inverse).reshape(-1, 3).astype(np.uint32)


def open_scene(ha, scenes, name, kw, w, h, dev_build, terrain_n):
    r = ha.HostRenderer(w, h)
    if dev_build:
        r.scene.device_build(r.ctx)
    d = scenes.REGISTRY[name](r.scene, **(dict(n=terrain_n) if kw is None else kw))
    r.commit()
    r.synchronize()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return r


def base_triangles(ha, r, blas, host_blas):
    sys.path.insert(0, HERE)
    from triangles_bench import read_tris
    s = r.scene
    meshes = list(range(s.n_meshes())) if host_blas < 0 else [0]
    base = np.concatenate([s.mesh_tris(m)[0][:, :9] for m in meshes]).astype(f32)
    tris = np.zeros(len(base), dtype=ha.RT_TRIANGLE_DTYPE)
    old = read_tris(ha, s.describe(), blas)
    tris["obj_idx"], tris["material"] = old["obj_idx"], old["material"]
    return base, tris


def displaced(v, extent, step):
    out = v.copy()
    out[:, 0] += (f32(0.01 * extent) * np.sin(v[:, 1] * f32(3.0 / max(extent, 1e-6)) + f32(0.3 * step))).astype(f32)
    return out


def only_set_triangles(a):
    """a child of the parent comparison: the medians of rt_set_triangles alone, with the package under --root"""
    sys.path.insert(0, a.root)
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    out = dict(build=None, scenes={})
    for name, kw, w, h, blas, host_blas, dev_build in SCENES:
        if a.only and a.only != name:
            continue
        r = open_scene(ha, scenes, name, kw, w, h, dev_build, a.terrain_n)
        out["build"] = r.build_info()
        base, tris = base_triangles(ha, r, blas, host_blas)
        extent = float(np.abs(base).max())
        ms = []
        reps = min(a.reps, a.terrain_reps) if name == "terrain" else a.reps
        for k in range(a.warmup + reps):
            v9 = displaced(base.reshape(-1, 3), extent, k + 1).reshape(-1, 9)
            tris["v0"], tris["v1"], tris["v2"], tris["N"] = v9[:, 0:3], v9[:, 3:6], v9[:, 6:9], normals(v9)
            r.synchronize()
            t0 = time.perf_counter()
            assert r.set_triangles(blas, tris) == 0
            r.synchronize()
            if k >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        out["scenes"][name] = ms
        r.close()
    print("CHILD " + json.dumps(out), flush=True)


def parent_comparison(a):
    here_root = os.path.dirname(HERE)
    series = {"this": {}, "parent": {}}
    builds = {}
    for rnd in range(a.rounds):
        order = (("parent", a.parent_root), ("this", here_root))
        for who, root in (order if rnd % 2 == 0 else order[::-1]):  # neither build is always the one that follows the other
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", os.path.abspath(root), "--reps", str(a.reps), "--warmup", str(a.warmup),
                   "--terrain-n", str(a.terrain_n), "--terrain-reps", str(a.terrain_reps)] + (["--only", a.only] if a.only else [])
            text = subprocess.check_output(cmd, cwd=os.path.abspath(root), timeout=900).decode()
            res = json.loads([ln for ln in text.splitlines() if ln.startswith("CHILD ")][-1][6:])
            builds[who] = res["build"]
            for name, ms in res["scenes"].items():
                series[who].setdefault(name, []).extend(ms)
    out = dict(rounds=a.rounds, builds=builds, scenes={})
    for name in series["this"]:
        t, p = summary(series["this"][name]), summary(series["parent"][name])
        out["scenes"][name] = dict(this=t, parent=p, this_median_within_parent_p10_p90=bool(p["p10"] <= t["median"] <= p["p90"]))
        print("set_triangles, this build against the parent's:", name, json.dumps(out["scenes"][name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--terrain-n", type=int, default=2048)
    ap.add_argument("--terrain-reps", type=int, default=5, help="the terrain's host-side preparation takes seconds: fewer repetitions")
    ap.add_argument("--only", default="", help="one scene by name")
    ap.add_argument("--json", default="")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its libraries built: compare rt_set_triangles with it")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return only_set_triangles(a)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    out = dict(reps=a.reps, warmup=a.warmup, scenes={})
    if a.json and os.path.exists(a.json):  # scenes measured by an earlier call (--only) stay
        out["scenes"] = json.load(open(a.json)).get("scenes", {})
    for name, kw, w, h, blas, host_blas, dev_build in SCENES:
        if a.only and a.only != name:
            continue
        reps = min(a.reps, a.terrain_reps) if name == "terrain" else a.reps
        warm = min(a.warmup, 1) if name == "terrain" else a.warmup
        r = open_scene(ha, scenes, name, kw, w, h, dev_build, a.terrain_n)
        out["build"] = r.build_info()
        base, tris = base_triangles(ha, r, blas, host_blas)
        xyz, idx = weld(base)
        assert np.array_equal(xyz[idx.reshape(-1)].reshape(-1, 9).view(np.uint32), base.view(np.uint32))
        assert r.set_mesh_indices(blas, idx, len(xyz)) == 0
        extent = float(np.abs(base).max())
        dev = torch.device("cuda", ha.rt_lib().rt_device_of(r.ctx))
        xyz_dev = torch.from_numpy(xyz).to(dev)
        flat = idx.reshape(-1)
        series = {k: [] for k in ("set_triangles", "set_vertices", "set_vertices_device", "prep_triangles", "prep_vertices", "prep_device")}
        for k in range(warm + reps):
            ms = {}
            t0 = time.perf_counter()
            v = displaced(xyz, extent, k + 1)
            ms["prep_vertices"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            v9 = displaced(base.reshape(-1, 3), extent, k + 1).reshape(-1, 9)
            tris["v0"], tris["v1"], tris["v2"], tris["N"] = v9[:, 0:3], v9[:, 3:6], v9[:, 6:9], normals(v9)
            ms["prep_triangles"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            vd = xyz_dev.clone()
            vd[:, 0] += f32(0.01 * extent) * torch.sin(xyz_dev[:, 1] * f32(3.0 / max(extent, 1e-6)) + f32(0.3 * (k + 1)))
            torch.cuda.synchronize(dev)
            ms["prep_device"] = (time.perf_counter() - t0) * 1e3
            for key, call in (("set_triangles", lambda: r.set_triangles(blas, tris)), ("set_vertices", lambda: r.set_vertices(blas, v)),
                              ("set_vertices_device", lambda: r.set_vertices_device(blas, vd.data_ptr(), len(xyz)))):
                r.synchronize()
                t0 = time.perf_counter()
                assert call() == 0, (key, ha.rt_lib().rt_last_error(r.ctx))
                r.synchronize()
                ms[key] = (time.perf_counter() - t0) * 1e3
            if k >= warm:
                for key in series:
                    series[key].append(ms[key])
        # what the kernels take: one rt_profile.query entry per call
        r.set_profiling(True)
        kernel = {}
        for key, call in (("set_triangles", lambda: r.set_triangles(blas, tris)), ("set_vertices", lambda: r.set_vertices(blas, v)),
                          ("set_vertices_device", lambda: r.set_vertices_device(blas, vd.data_ptr(), len(xyz)))):
            r.profile()
            assert call() == 0
            kernel[key] = round(r.profile()["query"]["ms"], 4)
        r.set_profiling(False)
        res = {k: summary(s) for k, s in series.items()}
        res["device_ms_of_one_call"] = kernel
        res["triangles"], res["vertices"], res["size"] = len(tris), len(xyz), [w, h]
        res["host_link_bytes"] = dict(set_triangles=int(tris.nbytes), set_vertices=int(xyz.nbytes), set_vertices_device=0, indices_once=int(idx.nbytes))
        res["ratio_set_triangles_over_set_vertices"] = round(res["set_triangles"]["median"] / res["set_vertices"]["median"], 2)
        res["ratio_set_triangles_over_set_vertices_device"] = round(res["set_triangles"]["median"] / res["set_vertices_device"]["median"], 2)
        out["scenes"][name] = res
        print(name, json.dumps(res), flush=True)
        r.close()
    if a.parent_root:
        out["set_triangles_against_parent"] = parent_comparison(a)
    elif a.json and os.path.exists(a.json):
        prev = json.load(open(a.json))
        if "set_triangles_against_parent" in prev:
            out["set_triangles_against_parent"] = prev["set_triangles_against_parent"]
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
