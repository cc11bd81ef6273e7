"""What a camera move costs with rt_reproject and without, on config 3's scene (pretty_tlas) at 1920x1080.
  python3 profiles/reproject_bench.py [--rounds N] [--json out.json]          (GPU box, repository root)
With reprojection a move is rt_history_capture + rt_render_aovs (new camera) + rt_reproject; each is timed by the library's own HIP
events (rt_set_profiling: the capture's seven copies, k_primary_aovs and k_reproject are each one launch of rt_profile.query), N rounds
alternating the two cameras, the history a 16-frame render with statistics on.  Without it a move is rt_clear + min_samples (16) whole
frames: timed on the host clock between two rt_synchronize, once as 16 calls of one frame (what Renderer::Tick does) and once as one call
of 16 frames.  Reported: every round's figure, sorted, and the median; k_reproject's bytes from the shapes (36 B read of the current
G-buffer and at most 40 B of the history's per pixel, 24 B more per carried pixel, 28 B written) over the HBM peak."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E
MIN_SAMPLES = 16   # RT_ADAPTIVE_DEFAULTS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    ha.build()
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    w, h = 1920, 1080
    PATH = ha.RT_MODE_PATH
    r = ha.HostRenderer(w, h)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    c = d["camera"]
    A = np.array([c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"]], np.float32)
    B = (A + np.float32([0.05, 0, 0])).astype(np.float32)
    r.set_camera(*A)
    r.stats_enable(True)
    r.render(PATH, 0, MIN_SAMPLES)
    r.render_aovs(0.001)
    r.history_capture()  # allocation and first launches
    r.set_camera(*B)
    r.render_aovs(0.001)
    carried = r.reproject()

    def query_ms(call):
        r.set_profiling(True)
        call()
        ms = r.profile()["query"]["ms"]
        r.set_profiling(False)
        return ms

    cap, rep, aov = [], [], []
    for _ in range(a.rounds):
        r.set_camera(*A)
        r.render_aovs(0.001)
        cap.append(query_ms(r.history_capture))
        r.set_camera(*B)
        aov.append(query_ms(lambda: r.render_aovs(0.001)))
        rep.append(query_ms(r.reproject))

    def wall(call):
        r.synchronize()
        t0 = time.perf_counter()
        call()
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def ticks():
        r.clear()
        for f in range(MIN_SAMPLES):
            r.render(PATH, f, 1)

    def one_call():
        r.clear()
        r.render(PATH, 0, MIN_SAMPLES)

    per_tick = [wall(ticks) for _ in range(3)]
    batched = [wall(one_call) for _ in range(3)]
    n = w * h
    moved = n * (36 + 40 + 28) + carried * 24

    def figures(v):
        return dict(median=round(float(np.median(v)), 4), all=[round(x, 4) for x in sorted(v)])

    out = dict(width=w, height=h, pixels=n, rounds=a.rounds, carried_pixels=carried, carried_share=round(carried / n, 4),
               history_capture_ms=figures(cap), render_aovs_ms=figures(aov), reproject_ms=figures(rep),
               reproject_bytes=moved, reproject_hbm_frac_of_peak=round(moved / (float(np.median(rep)) * 1e-3) / HBM_PEAK, 4),
               capture_bytes=2 * n * 76, capture_hbm_frac_of_peak=round(2 * n * 76 / (float(np.median(cap)) * 1e-3) / HBM_PEAK, 4),
               clear_plus_16_frames_ms=dict(one_frame_per_call=figures(per_tick), one_call=figures(batched)),
               build=r.build_info())
    r.close()
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
