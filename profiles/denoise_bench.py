"""G-buffer pass and denoiser timings on config 3's scene (pretty_tlas) at 1920x1080 and 3840x2160.
  python3 profiles/denoise_bench.py [--reps N] [--json out.json]          (GPU box, repository root)
Times, with HIP events around the calls on the context's stream (rt_get_profile for rt_render_aovs, a synchronised host clock for
rt_denoise), after warm-up, over repeated calls:
  rt_render_aovs after a camera change (the camera is nudged back and forth, so every call traces the frame)
  rt_denoise with the defaults (5 iterations) on a 1-spp accumulator
and prices one denoise iteration from the shapes: unique HBM bytes (4 float4 reads + 1 float4 write per pixel) and tap bytes through L1
(25 taps x 64 B per pixel at most: colour, position, normal, albedo), each over its peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

HBM_PEAK = 8.0e12        # B/s, MI355X HBM3E
L1_PEAK = 256 * 64 * 2.4e9  # B/s: 256 CUs x 64 B/clk (one 64-B line per CU per clock) x 2.4 GHz


def run(ha, scenes, w, h, reps):
    r = ha.HostRenderer(w, h)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    r.render(ha.RT_MODE_PATH, 0, 1)
    r.synchronize()
    cam = r.camera()
    r.set_profiling(True)
    aov_ms = []
    for k in range(reps + 2):
        off = np.float32(0.001 if k % 2 else 0.0)
        r.set_camera(cam[0] + off, cam[1], cam[2], cam[3])
        r.profile()
        r.render_aovs(0.001)
        p = r.profile()["query"]
        assert p["launches"] == 1
        if k >= 2:
            aov_ms.append(p["ms"])
    r.set_profiling(False)
    for _ in range(3):
        r.denoise(1)
    r.synchronize()
    den_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r.denoise(1)
        r.synchronize()
        den_ms.append((time.perf_counter() - t0) * 1e3)
    n = w * h
    it = ha.DENOISE_DEFAULTS["iterations"]
    hbm = n * 5 * 16
    taps = n * 25 * 64
    med = float(np.median(den_ms))
    out = dict(width=w, height=h, pixels=n, reps=reps,
               render_aovs_ms=dict(median=round(float(np.median(aov_ms)), 4), min=round(float(np.min(aov_ms)), 4), max=round(float(np.max(aov_ms)), 4)),
               denoise_ms=dict(median=round(med, 4), min=round(float(np.min(den_ms)), 4), max=round(float(np.max(den_ms)), 4), iterations=it),
               per_iteration=dict(ms=round(med / it, 4), unique_hbm_bytes=hbm, tap_bytes_l1=taps,
                                  hbm_frac_of_peak=round(hbm / (med / it * 1e-3) / HBM_PEAK, 4),
                                  l1_frac_of_peak=round(taps / (med / it * 1e-3) / L1_PEAK, 4)),
               peaks=dict(hbm_Bps=HBM_PEAK, l1_Bps=L1_PEAK), build=r.build_info())
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    ha.build()
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    res = [run(ha, scenes, w, h, a.reps) for w, h in ((1920, 1080), (3840, 2160))]
    for r in res:
        print(json.dumps(r))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
