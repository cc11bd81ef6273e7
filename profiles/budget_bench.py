"""Budgeted adaptive passes, timed on config 3's scene (pretty_tlas) at 1920x1080 (the selection at 3840x2160 too).
  python3 profiles/budget_bench.py --parent <checkout of the parent commit, built> [--parent-budget] [--rounds N] [--json out.json]   (GPU box, repository root)
Every measurement runs in a child process of its own (two builds of the library cannot share a process), parent and this commit
alternated round by round in one session; host times bracketed by rt_synchronize, after a warm-up call of the same shape.
  overhead   one pass over the FULL list with every budget forced to 16 (from rt_clear with min_samples = 16 = pass_cap: rt_render_budget
             alone is timed, its selection beside it) against whole16 (rt_render of 16 frames, statistics off) and full_list16
             (rt_render_active of 16 frames, every pixel listed) of the parent commit AND of this one, and whole16 with statistics on
             (--parent-budget: the parent commit has the budgeted calls too, and its selection and pass are timed as well)
  loops      from rt_clear until nothing is active under the same rt_adaptive_params:
               (a) rt_select_active + rt_render_active(frame, 1), as TickAdaptive does (min_samples whole frames first)
               (b) rt_select_budget + rt_render_budget at pass_cap 8, 64, 512
             wall time, passes, samples taken, and the overshoot samples(b) / samples(a): a budget is a prediction from the current
             variance, so (b) may take more samples -- the file states the number
  select     rt_select_budget beside rt_select_active on the statistics of 16 whole frames, 1920x1080 and 3840x2160
The result is stamped with rt_build_info / rt_tuning_info of both libraries."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LOOP = dict(min_samples=16, max_samples=256, threshold=0.05, floor=1e-3)  # (a) ends within max_samples passes
CAPS = (8, 64, 512)


def timed(r, fn):
    r.synchronize()
    t0 = time.perf_counter()
    fn()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4), all=[round(float(x), 4) for x in v])


def setup(ha, scenes, w, h):
    r = ha.HostRenderer(w, h)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return r


def part_overhead(ha, scenes, reps, has_budget):
    w, h = 1920, 1080
    PATH = ha.RT_MODE_PATH
    r = setup(ha, scenes, w, h)
    r.set_active(np.arange(w * h, dtype=np.uint32))
    forced = dict(select=dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3), pass_cap=16)
    times = {}

    def add(name, ms, k):
        if k > 1:
            times.setdefault(name, []).append(ms)

    for k in range(reps + 2):  # rounds 0 and 1 warm every shape up (allocations, the primary-hit table; the first whole16 after the first
        #                        budgeted pass is slow once more: 33-37 ms against 10)
        r.stats_enable(False)
        add("whole16", timed(r, lambda: r.render(PATH, 16, 16)), k)
        r.set_active(np.arange(w * h, dtype=np.uint32))
        add("full_list16", timed(r, lambda: r.render_active(16, 16)), k)
        r.stats_enable(True)
        add("whole16_stats", timed(r, lambda: r.render(PATH, 16, 16)), k)
        if has_budget:
            r.clear()
            got = []
            add("select_budget_full_list", timed(r, lambda: got.append(r.select_budget(forced))), k)
            assert got[0] == (w * h, 16 * w * h, 16), got
            add("budget16", timed(r, lambda: r.render_budget(0)), k)
            if k == 0:  # (checked in the warm-up round only: a download here would idle the device before the next round's whole16)
                cnt = r.stats()[0]
                assert int(cnt.min()) == 16 == int(cnt.max())
    out = dict(ms={k: summary(v) for k, v in times.items()}, build=r.build_info())
    r.close()
    return out


def part_loops(ha, scenes, rounds):
    w, h = 1920, 1080
    PATH = ha.RT_MODE_PATH
    r = setup(ha, scenes, w, h)
    r.stats_enable(True)

    def frame_by_frame():
        r.clear()
        passes = samples = frame = 0
        while True:
            if frame < LOOP["min_samples"]:
                r.render(PATH, frame, 1)
                n = w * h
            else:
                n = r.select_active(LOOP)
                if n == 0:
                    break
                r.render_active(frame, 1)
            passes, samples, frame = passes + 1, samples + n, frame + 1
        return passes, samples

    def budgeted(cap):
        def go():
            r.clear()
            passes = samples = 0
            while True:
                n, total, used = r.select_budget(dict(select=LOOP, pass_cap=cap))
                if n == 0:
                    break
                r.render_budget(0)
                passes, samples = passes + 1, samples + total
            return passes, samples
        return go

    variants = {"frame_by_frame": frame_by_frame}
    for cap in CAPS:
        variants["budget_cap_%d" % cap] = budgeted(cap)
    res = {k: dict(ms=[], passes=None, samples=None) for k in variants}
    for rnd in range(rounds + 1):  # round 0 warms up
        for name, fn in variants.items():
            got = []
            ms = timed(r, lambda: got.append(fn()))
            assert int(r.stats()[0].sum(dtype=np.int64)) == got[0][1] and r.select_active(LOOP) == 0
            if rnd > 0:
                res[name]["ms"].append(ms)
                assert res[name]["passes"] in (None, got[0][0])  # the loops are deterministic
                res[name]["passes"], res[name]["samples"] = got[0]
    base = res["frame_by_frame"]
    out = dict(params=LOOP, width=w, height=h, rounds=rounds, loops={}, build=r.build_info())
    for name, v in res.items():
        m = summary(v["ms"])
        out["loops"][name] = dict(ms=m, passes=v["passes"], samples=v["samples"], overshoot=round(v["samples"] / base["samples"], 4),
                                  time_over_frame_by_frame=round(m["median"] / float(np.median(base["ms"])), 4))
    r.close()
    return out


def part_select(ha, scenes, reps):
    out = []
    P = dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3)
    for w, h in ((1920, 1080), (3840, 2160)):
        r = setup(ha, scenes, w, h)
        r.stats_enable(True)
        r.clear()
        r.render(ha.RT_MODE_PATH, 0, 16)
        sa, sb = [], []
        for k in range(reps + 2):
            a = timed(r, lambda: r.select_active(P))
            b = timed(r, lambda: r.select_budget(dict(select=P, pass_cap=64)))
            if k >= 2:
                sa.append(a), sb.append(b)
        n, total, used = r.select_budget(dict(select=P, pass_cap=64))
        out.append(dict(width=w, height=h, reps=reps, active=n, pass_samples=total, cap_used=used, select_active_ms=summary(sa), select_budget_ms=summary(sb), build=r.build_info(),
                        budget_over_active=round(float(np.median(sb) / np.median(sa)), 4)))
        r.close()
    return out


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    if a.part == "overhead":
        res = part_overhead(ha, scenes, a.reps, not a.baseline)
    elif a.part == "loops":
        res = part_loops(ha, scenes, a.rounds)
    else:
        res = part_select(ha, scenes, a.reps)
    print("RESULT " + json.dumps(res))


def run_child(root, part, a, baseline=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--root", root, "--rounds", str(a.rounds), "--reps", str(a.reps)] + (["--baseline"] if baseline else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit("child %s failed with %d" % (" ".join(cmd), p.returncode))  # nothing more is started on the device
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (the overhead part's baseline)")
    ap.add_argument("--parent-budget", action="store_true", help="the parent commit has the budgeted calls: time them on its build too")
    ap.add_argument("--part", default=None, choices=["overhead", "loops", "select"], help="(a child's work)")
    ap.add_argument("--baseline", action="store_true", help="(child) only the calls the parent commit has")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.part:
        return child(a)
    if not a.parent:
        raise SystemExit("--parent: a built checkout of the parent commit")
    over = dict(parent=[], this=[])
    for rnd in range(a.rounds):  # alternated: parent, this, parent, this, ...
        over["parent"].append(run_child(a.parent, "overhead", a, baseline=not a.parent_budget))
        over["this"].append(run_child(a.root, "overhead", a))

    def merged(runs):
        names = runs[0]["ms"].keys()
        return dict(ms={k: summary([x for run in runs for x in run["ms"][k]["all"]]) for k in names},
                    per_round_median={k: [run["ms"][k]["median"] for run in runs] for k in names}, build=runs[0]["build"])

    overhead = dict(parent=merged(over["parent"]), this=merged(over["this"]))
    p, t = overhead["parent"]["ms"], overhead["this"]["ms"]
    overhead["ratios"] = dict(budget16_over_parent_whole16=round(t["budget16"]["median"] / p["whole16"]["median"], 4),
                              budget16_over_parent_full_list16=round(t["budget16"]["median"] / p["full_list16"]["median"], 4),
                              budget16_over_whole16_stats=round(t["budget16"]["median"] / t["whole16_stats"]["median"], 4),
                              whole16_this_over_parent=round(t["whole16"]["median"] / p["whole16"]["median"], 4),
                              full_list16_this_over_parent=round(t["full_list16"]["median"] / p["full_list16"]["median"], 4))
    res = dict(overhead=overhead, loops=run_child(a.root, "loops", a), select=run_child(a.root, "select", a))
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
