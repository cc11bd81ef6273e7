#!/usr/bin/env python3
"""Generate tests/golden/oracle_vectors.npz and oracle_vectors_scenes.npz from the oracle (oracle/), at the sizes SURVEY.md section 8(c) lists.

The reference has no tests, fixtures or golden images and cannot be built in this
image without stand-ins for Windows/MSVC headers, so these vectors do NOT come from the reference:
they pin the oracle against drift (any edit that changes its arithmetic fails the CPU test tier), against
compiler dependence (tests/test_oracle_cpu.py regenerates them with a second compiler and demands the same
bits) and give the GPU tier fixed expected values that do not depend on rebuilding the oracle.
The reference-derived pins (numbers the survey observed on the patched reference itself) are asserted in
tests/test_oracle_cpu.py::test_reference_probe_observations.

Run:  python tests/golden/make_golden.py [--out FILE]      (ORACLE_LIB=<.so> selects another build of the oracle)
"""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle_api as oa  # noqa: E402

scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fixtures import RNG_SEEDS, FIXTURE_SCENES, scene_key, unit_rays, single_primitive, save_gold, gold_paths  # noqa: E402


def generate():
    out = {}
    L = oa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rng = np.random.default_rng(2024)

    # ---- RNG: first 4k outputs of 8 streams; RandomInHemisphere for 256 normals (template.cpp:684-724)
    for seed in RNG_SEEDS:
        u = np.zeros(4096, np.uint32)
        f = np.zeros(4096, np.float32)
        L.orc_rng_stream(C.c_uint(seed), 4096, P(u), P(f))
        out["rng_u_%x" % seed] = u
        out["rng_f_%x" % seed] = f
    nrm = rng.normal(size=(256, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    hemi = np.zeros((256, 3), np.float32)
    L.orc_hemisphere(C.c_uint(99), 256, P(nrm), P(hemi))
    out["hemi_normals"], out["hemi_out"] = nrm, hemi

    # ---- fresnel / refract (template/scene.h:647-672)
    I = rng.normal(size=(1024, 3)).astype(np.float32)
    I /= np.linalg.norm(I, axis=1, keepdims=True).astype(np.float32)
    N = rng.normal(size=(1024, 3)).astype(np.float32)
    N /= np.linalg.norm(N, axis=1, keepdims=True).astype(np.float32)
    kr = np.zeros(1024, np.float32)
    rf = np.zeros((1024, 3), np.float32)
    L.orc_fresnel(1024, P(I), P(N), C.c_float(1.5), P(kr))
    L.orc_refract(1024, P(I), P(N), C.c_float(1 / 1.5), P(rf))
    out["fr_I"], out["fr_N"], out["fr_kr"], out["fr_refract"] = I, N, kr, rf

    # ---- per primitive type: >= 1k rays -> (t bits, objIdx)
    # AABB slab test (bvh.cpp:819-828)
    O, D = unit_rays(rng, 2048, (0, 0, 0), 3.0)
    lo = rng.uniform(-1.5, 0.0, (2048, 3)).astype(np.float32)
    hi = (lo + rng.uniform(0.0, 1.5, (2048, 3))).astype(np.float32)
    tmax = np.where(rng.uniform(size=2048) < 0.3, rng.uniform(0.1, 4.0, 2048), 1e34).astype(np.float32)
    d = np.zeros(2048, np.float32)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    for i in range(2048):
        d[i] = L.orc_intersect_aabb(f3(O[i]), f3(D[i]), C.c_float(float(tmax[i])), f3(lo[i]), f3(hi[i]))
    out["aabb_O"], out["aabb_D"], out["aabb_tmax"], out["aabb_lo"], out["aabb_hi"], out["aabb_dist"] = O, D, tmax, lo, hi, d

    for kind in ("triangle", "sphere", "plane", "disk"):
        s = oa.OracleScene()
        single_primitive(s, kind)
        O, D = unit_rays(rng, 2048, (0, 0, 0), 3.0)
        for t_min in (1e-6, 0.001):
            r = s.find_nearest(O, D, t_min=t_min)
            out["%s_t_%g" % (kind, t_min)] = r["t"]
            out["%s_obj_%g" % (kind, t_min)] = r["obj"]
            out["%s_n_%g" % (kind, t_min)] = r["normal"]
        tm = rng.uniform(0.2, 6.0, 2048).astype(np.float32)
        out[kind + "_occ"] = s.is_occluded(O, D, tm)["occluded"]
        out[kind + "_O"], out[kind + "_D"], out[kind + "_tmax"] = O, D, tm
        s.close()

    # ---- per fixture scene: builder dumps, TLAS dumps, primary maps at 64x64, accumulators at 64x64
    for name, kw in FIXTURE_SCENES:
        s = oa.OracleScene()
        dsc = scenes.REGISTRY[name](s, **kw)
        key = scene_key(name, kw)
        b = s.bvh_dump(0 if dsc["tlas"] else -1)
        out[key + "_nodes"] = np.delete(b["nodes"], 1, axis=0)  # node 1 is never written (Q4)
        out[key + "_prim_idx"] = b["prim_idx"]
        if dsc["tlas"]:
            out[key + "_tlas"] = s.tlas_dump()
            out[key + "_inst"] = np.stack([np.concatenate([s.instance_dump(i)["T"], s.instance_dump(i)["invT"], s.instance_dump(i)["bounds"]]) for i in range(s.n_instances)])
        r = oa.OracleRenderer(s, 64, 64)
        if "camera" in dsc:
            c = dsc["camera"]
            r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        obj, t, cnt = r.primary_hits(1e-6)
        out[key + "_obj"], out[key + "_t"] = obj, t
        out[key + "_cnt"] = np.array([cnt[k] for k in oa.COUNTER_NAMES], dtype=np.uint64)
        s.set_raytracer(True)
        r.clear()
        r.render(0, 1)
        out[key + "_whitted"] = r.accumulator()
        s.set_raytracer(False)
        for frames in (1, 4, 16):
            r.clear()
            r.render(0, frames)
            out[key + "_path%d" % frames] = r.accumulator()
        r.close()
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "oracle_vectors.npz"))
    args = ap.parse_args()
    out = generate()
    save_gold(args.out, out)
    print("wrote %d arrays to %s" % (len(out), " and ".join(gold_paths(args.out))))


if __name__ == "__main__":
    main()
