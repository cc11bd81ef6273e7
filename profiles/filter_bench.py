"""The pixel filter of path-mode camera samples, timed on config 3's scene (pretty_tlas) at 1920x1080 in 64-frame and 16-frame batches.
  python3 profiles/filter_bench.py [--parent <checkout of the parent commit, built>] [--rounds N] [--json out.json]   (GPU box, repository root)
Every measurement runs in a child process of its own (a context reads its knobs when it is created; two builds of the library cannot share
a process), the lines alternated round by round in one session.  Lines, all on this build:
  reference_table    reference mode, the defaults: round 0 of a batch reads the primary-hit table
  reference_traced   reference mode with RT_PRIMARY_TABLE=0: every camera ray is traced -- the like-for-like yardstick of BOX
  box                RT_FILTER_BOX (the table answers "no" by itself)
Per line and batch size, after one warm-up batch: wall ms of rt_clear + rt_render + rt_synchronize over --reps batches, and a checksum of
the accumulator (the same on every round, or the run fails).
With --parent the default bench line (bench.py --gpus 1 --no-cpu-baseline) is alternated --rounds times between the parent's build and
this one: ms_per_step of each run, then one --full line per build for its frame_checksum.
The result is stamped with rt_build_info of the libraries."""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 1920, 1080
LINES = dict(reference_table=(0, {}), reference_traced=(0, {"RT_PRIMARY_TABLE": "0"}), box=(2, {}))


def summary(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3), all=[round(float(x), 3) for x in v])


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    kind = LINES[a.line][0]
    r = ha.HostRenderer(W, H)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    r.set_pixel_filter(kind)
    out = dict(line=a.line, build=r.build_info(), batches={})
    for frames in (64, 16):
        ms = []
        for k in range(a.reps + 1):
            r.clear()
            r.synchronize()
            t0 = time.perf_counter()
            r.render(ha.RT_MODE_PATH, 0, frames)
            r.synchronize()
            if k >= 1:
                ms.append((time.perf_counter() - t0) * 1e3)
        out["batches"][str(frames)] = dict(ms=summary(ms), checksum=hashlib.sha256(r.accumulator().tobytes()).hexdigest()[:16])
    r.close()
    print("RESULT " + json.dumps(out))


def run_child(a, line):
    env = dict(os.environ)
    for k in ("RT_PRIMARY_TABLE", "RT_PRIMARY_TABLE_MIN", "RT_FUSE", "RT_STREAM", "RT_SLOTS"):
        env.pop(k, None)
    env.update(LINES[line][1])
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", a.root, "--reps", str(a.reps), "--line", line]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout, env=env)
    if p.returncode != 0:
        raise SystemExit("child %s failed with %d" % (" ".join(cmd), p.returncode))  # nothing more is started on the device
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def run_bench(a, root, full=False):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline"] + (["--full"] if full else [])
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout, cwd=os.path.abspath(root))
    if p.returncode != 0:
        raise SystemExit("bench.py in %s failed with %d" % (root, p.returncode))
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    return dict(ms_per_step=line["ms_per_step"], frame_checksum=line.get("frame_checksum"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="the checkout whose library is measured")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the default bench line is alternated with it")
    ap.add_argument("--bench-steps", type=int, default=5)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--child", action="store_true", help="(a child's work)")
    ap.add_argument("--line", default="box", choices=sorted(LINES))
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {line: [] for line in LINES}
    for rnd in range(a.rounds):  # alternated: table, traced, box, table, ...
        for line in LINES:
            runs[line].append(run_child(a, line))
    res = dict(width=W, height=H, rounds=a.rounds, reps=a.reps, build=runs["box"][0]["build"], lines={})
    for line, rs in runs.items():
        res["lines"][line] = {}
        for frames in ("64", "16"):
            sums = {r["batches"][frames]["checksum"] for r in rs}
            if len(sums) != 1:
                raise SystemExit("%s x %s frames: the accumulator differs between rounds: %s" % (line, frames, sorted(sums)))
            per_round = [r["batches"][frames]["ms"]["median"] for r in rs]
            res["lines"][line][frames] = dict(ms=summary([x for r in rs for x in r["batches"][frames]["ms"]["all"]]), per_round_median=per_round,
                                              spread_of_round_medians=round(max(per_round) - min(per_round), 3), checksum=sums.pop())
    for frames in ("64", "16"):
        m = {line: res["lines"][line][frames]["ms"]["median"] for line in LINES}
        res["box_minus_reference_traced_ms_%s" % frames] = round(m["box"] - m["reference_traced"], 3)
        res["box_minus_reference_table_ms_%s" % frames] = round(m["box"] - m["reference_table"], 3)
    if a.parent:
        ab = dict(parent=[], this=[])
        for rnd in range(a.rounds):
            ab["parent"].append(run_bench(a, a.parent))
            ab["this"].append(run_bench(a, a.root))
        # (frame_checksum is part of a --full line, whose HIP-event timers are not part of the plain line's time: one more run per build)
        full = dict(parent=run_bench(a, a.parent, True), this=run_bench(a, a.root, True))
        res["default_bench_line"] = {k: dict(ms_per_step=summary([x["ms_per_step"] for x in v]), frame_checksum_of_a_full_line=full[k]["frame_checksum"]) for k, v in ab.items()}
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
