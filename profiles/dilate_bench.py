"""Dilated adaptive selection, timed on config 3's scene (pretty_tlas) at 1920x1080 on the statistics of 16 whole frames.
  python3 profiles/dilate_bench.py --parent <checkout of the parent commit, built> [--parent-dilated] [--rounds N] [--json out.json]   (GPU box, repository root)
Every measurement runs in a child process of its own (two builds of the library cannot share a process), parent and this commit
alternated round by round in one session.  Per call, after two warm-up calls of the same shape, medians of --reps (7) calls:
  event_ms   HIP events on the context's stream (rt_set_profiling: the call's entry of rt_profile.query) -- rt_select_active and
             rt_select_active_dilated bracket their launches, rt_select_budget_dilated the whole call with its read-backs;
             rt_select_budget has no entry of its own, so it has no event time
  wall_ms    host time of the call between two rt_synchronize: launches, the read-back of the count and its synchronisation included
  rt_select_active, rt_select_budget (pass_cap 64): parent build and this build
  rt_select_active_dilated at radius 0, 1, 4, 16; rt_select_budget_dilated at radius 1, 4: this build, same statistics, same process
    (--parent-dilated: the parent commit has these calls too, and they are timed on its build as well)
The yardstick: per pixel the undilated selection reads 12 B of statistics twice (count, scatter), the dilated one once, plus bitmasks of
width * height / 8 bytes that stay in the L2; bytes / event time is printed as GB/s beside the device's HBM rate.
The result is stamped with rt_build_info of both libraries."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
P = dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3)
W, H = 1920, 1080


def summary(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4), all=[round(float(x), 4) for x in v])


def measure(r, fn, reps, events=True):
    """(wall ms, event ms or None) per call, the first two calls dropped"""
    wall, ev = [], []
    for k in range(reps + 2):
        r.profile(reset=True)
        r.synchronize()
        t0 = time.perf_counter()
        fn()
        r.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        q = r.profile(reset=True)["query"]
        if k >= 2:
            wall.append(ms)
            if events:
                assert q["launches"] == 1, q
                ev.append(q["ms"])
    return dict(wall_ms=summary(wall), event_ms=summary(ev) if events else None)


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    r = ha.HostRenderer(W, H)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    r.stats_enable(True)
    r.clear()
    r.render(ha.RT_MODE_PATH, 0, 16)
    r.set_profiling(True)
    B = dict(select=P, pass_cap=64)
    out = dict(build=r.build_info(), width=W, height=H, params=P, reps=a.reps, calls={})
    out["calls"]["select_active"] = dict(measure(r, lambda: r.select_active(P), a.reps), listed=r.select_active(P))
    out["calls"]["select_budget"] = dict(measure(r, lambda: r.select_budget(B), a.reps, events=False), listed=r.select_budget(B)[0])
    if not a.baseline:
        for radius in (0, 1, 4, 16):
            out["calls"]["select_active_dilated_r%d" % radius] = dict(measure(r, lambda: r.select_active_dilated(radius, P), a.reps), listed=r.select_active_dilated(radius, P))
        for radius in (1, 4):
            n, total, used = r.select_budget_dilated(radius, B)
            out["calls"]["select_budget_dilated_r%d" % radius] = dict(measure(r, lambda: r.select_budget_dilated(radius, B), a.reps), listed=n, pass_samples=total, cap_used=used)
        assert out["calls"]["select_active_dilated_r0"]["listed"] == out["calls"]["select_active"]["listed"]
    r.close()
    print("RESULT " + json.dumps(out))


def run_child(root, a, baseline):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--reps", str(a.reps)] + (["--baseline"] if baseline else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit("child %s failed with %d" % (" ".join(cmd), p.returncode))  # nothing more is started on the device
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--parent-dilated", action="store_true", help="the parent commit has the dilated calls: time them on its build too")
    ap.add_argument("--child", action="store_true", help="(a child's work)")
    ap.add_argument("--baseline", action="store_true", help="(child) only the calls the parent commit has")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent:
        raise SystemExit("--parent: a built checkout of the parent commit")
    runs = dict(parent=[], this=[])
    for rnd in range(a.rounds):  # alternated: parent, this, parent, this, ...
        runs["parent"].append(run_child(a.parent, a, not a.parent_dilated))
        runs["this"].append(run_child(a.root, a, False))

    def merged(rs):
        calls = {}
        for name in rs[0]["calls"]:
            c = {k: v for k, v in rs[0]["calls"][name].items() if k not in ("wall_ms", "event_ms")}
            for kind in ("wall_ms", "event_ms"):
                if rs[0]["calls"][name][kind] is not None:
                    c[kind] = summary([x for run in rs for x in run["calls"][name][kind]["all"]])
                    c[kind + "_per_round_median"] = [run["calls"][name][kind]["median"] for run in rs]
            calls[name] = c
        return dict(build=rs[0]["build"], calls=calls)

    res = dict(width=W, height=H, params=P, rounds=a.rounds, reps=a.reps, parent=merged(runs["parent"]), this=merged(runs["this"]))
    px = W * H
    bytes_read = dict(select_active=24 * px)
    for radius in (0, 1, 4, 16):
        bytes_read["select_active_dilated_r%d" % radius] = 12 * px  # (+ the bitmasks: 4 x px / 8 written, read back from the L2)
    res["statistics_gb_per_s_by_event_time"] = {k: round(b / (res["this"]["calls"][k]["event_ms"]["median"] * 1e-3) / 1e9, 1) for k, b in bytes_read.items()}
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
