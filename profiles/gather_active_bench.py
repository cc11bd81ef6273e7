"""The pushes of adaptive sampling over several contexts, timed between two contexts on ONE device at 1920x1080 on config 3's scene
(pretty_tlas): same-device traffic.  Nothing here crosses a link between two GPUs; how k_push_active's scatter behaves over xGMI is not
measured by this script or by anyone yet.
  python3 profiles/gather_active_bench.py [--json out.json]          (GPU box, repository root)
Context B renders 16 whole frames with statistics on, then:
  select      rt_select_active against rt_select_active_rows of the half-frame shard (1, 2, 540), and the selected counts of the eight
              shards (k, 8, 135): the imbalance an interleaved split leaves (printed, not acted on)
  push        into context A: rt_gather_active at the selected set and at every 2nd, 8th and 64th pixel (rt_set_active_pixels);
              rt_gather_stats_rows of the half-frame shard; rt_gather_rows of that shard -- the call the parent commit has, unchanged here
              (it issues the same operations), as the yardstick
Times: the library's HIP events (rt_set_profiling on the context that queues the work: one rt_profile.query entry per selection -- its
three launches -- and per push -- its copies or kernel on the source's stream, behind the ordering wait), one call per entry, medians of
seven after a warm-up call; the host clock around the same call, both contexts drained before and after, is kept beside it ('host_ms':
mostly the host's stream operations and the synchronises).  Bytes: what the operation must move (a listed pixel: 4 B of list, 28 B read,
28 B written; a pixel of a row: 28 B or 16 B each way; a selection: 12 B per pixel read twice, 4 B per listed pixel written); frac:
bytes / event time over 8 TB/s (data sheet) and over 6.29 TB/s (the measured streaming rate of the part)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 1920, 1080
P = dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3)
ROUNDS = 7


def summary(v):
    return dict(median=round(float(np.median(v)), 5), min=round(float(np.min(v)), 5), max=round(float(np.max(v)), 5))


def setup(ha, scenes):
    r = ha.HostRenderer(W, H)
    d = scenes.pretty_tlas(r.scene, 8)
    r.scene.set_raytracer(False)
    r.commit()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    r.stats_enable(True)
    r.clear()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(HERE))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    A, B = setup(ha, scenes), setup(ha, scenes)
    B.render(ha.RT_MODE_PATH, 0, 16)

    B.set_profiling(True)  # B queues everything that is timed: the selections on its stream, the pushes as their source

    def timed(fn):
        """(event ms, host ms) of ROUNDS single calls after one warm-up call; both contexts drained before and after each"""
        ev, host = [], []
        for k in range(ROUNDS + 1):
            A.synchronize(), B.synchronize()
            B.profile(reset=True)
            t0 = time.perf_counter()
            fn()
            B.synchronize(), A.synchronize()
            t1 = time.perf_counter()
            q = B.profile(reset=True)["query"]
            assert q["launches"] == 1, q
            if k > 0:
                ev.append(q["ms"]), host.append((t1 - t0) * 1e3)
        return ev, host

    def record(times, nbytes, **more):
        ev, host = times
        sec = float(np.median(ev)) * 1e-3
        return dict(more, event_ms=summary(ev), host_ms=summary(host), bytes=int(nbytes), GBps=round(nbytes / sec / 1e9, 1),
                    frac_of_8TBps=round(nbytes / sec / 8e12, 4), frac_of_6_29TBps=round(nbytes / sec / 6.29e12, 4))

    res = dict(width=W, height=H, rounds=ROUNDS, params=P, build=B.build_info(),
               note="two contexts on one device: same-device traffic, no link between GPUs is measured")
    # ---- selection
    n_whole = B.select_active(P)
    n_half = B.select_active_rows(1, 2, H // 2, P)
    sel = dict(active=n_whole, frame_pixels=W * H, active_in_half_frame_shard=n_half,
               whole_frame=record(timed(lambda: B.select_active(P)), 24 * W * H + 4 * n_whole),
               half_frame_shard=record(timed(lambda: B.select_active_rows(1, 2, H // 2, P)), 12 * W * H + 4 * n_half))
    sel["shard_over_whole_frame"] = round(sel["half_frame_shard"]["event_ms"]["median"] / sel["whole_frame"]["event_ms"]["median"], 4)
    per_shard = [B.select_active_rows(k, 8, (H - k + 7) // 8, P) for k in range(8)]
    assert sum(per_shard) == n_whole
    sel["active_per_shard_of_8"] = per_shard
    sel["imbalance_max_over_mean"] = round(max(per_shard) / (n_whole / 8.0), 4) if n_whole else None
    res["select"] = sel
    print("selected %d of %d pixels; per shard of 8: %s (max / mean %s)" % (n_whole, W * H, per_shard, sel["imbalance_max_over_mean"]))
    # ---- pushes
    push = {}
    lists = [("selected", None)] + [("every_%d" % s, np.arange(0, W * H, s, dtype=np.uint32)) for s in (2, 8, 64)]
    for name, lst in lists:
        if lst is None:
            n = B.select_active(P)
        else:
            B.set_active(lst)
            n = len(lst)
        go = lambda: A.gather_active(B)  # noqa: E731
        push["gather_active_" + name] = record(timed(go), 60 * n, entries=n, share_of_frame=round(n / float(W * H), 5))
        got, want = A.stats()[0].reshape(-1), B.stats()[0].reshape(-1)
        on = B.active()[0]
        assert np.array_equal(got[on], want[on])
    rows = (1, 2, H // 2)
    pix = rows[2] * W
    go = lambda: A.gather_stats_rows(B, *rows)  # noqa: E731
    push["gather_stats_rows_half_frame"] = record(timed(go), 56 * pix, pixels=pix)
    go = lambda: A.gather_rows(B, *rows)  # noqa: E731
    push["gather_rows_half_frame"] = record(timed(go), 32 * pix, pixels=pix)
    res["push"] = push
    # where the sparse push stops being cheaper than the shard's whole rows, from the measured points (linear between neighbours)
    rows_ms = push["gather_stats_rows_half_frame"]["event_ms"]["median"]
    pts = sorted((v["share_of_frame"], v["event_ms"]["median"]) for k, v in push.items() if k.startswith("gather_active_every"))
    cross = None
    for (s0, t0), (s1, t1) in zip(pts, pts[1:]):
        if t0 <= rows_ms < t1:
            cross = round(s0 + (s1 - s0) * (rows_ms - t0) / (t1 - t0), 4)
    res["crossover"] = dict(against="gather_stats_rows_half_frame", rows_ms=rows_ms, points=pts, share_of_frame_at_equal_time=cross,
                            note="None: the sparse push was cheaper (or dearer) than the half-frame rows at every measured share")
    A.close(), B.close()
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
