"""The shutter of path-mode camera samples, timed on config 3's scene (pretty_tlas) at 1920x1080 in 64-frame and 16-frame batches.
  python3 profiles/shutter_bench.py [--parent <checkout of the parent commit, built>] [--rounds N] [--json out.json]   (GPU box, repository root)
Every measurement runs in a child process of its own, the lines alternated round by round in one session.  Lines, all on this build:
  box               RT_FILTER_BOX, no lens, no shutter: every camera ray is traced from cam_pos
  box_lens          RT_FILTER_BOX and rt_set_lens(radius 0.05, focus = rt_focus_at of the first pixel of the centre column, from the centre
                    down, that sees a surface: profiles/lens_bench.py's lens)
  box_shutter       RT_FILTER_BOX and rt_set_shutter(the camera moved by MOVE, all four points)
  box_lens_shutter  that lens and that shutter
Per line and batch size, after one warm-up batch: wall ms of rt_clear + rt_render + rt_synchronize over --reps batches, and a checksum of
the accumulator (the same on every round, or the run fails); then, outside the timed batches, one 64-frame batch with rt_set_profiling
on: the per-kind kernel times that say where the time of a slower line goes.
With --parent the default bench line (bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline) is alternated --rounds times between the
parent's build and this one, the parent first in each pair: ms_per_step of each run, then one --full line per build for its frame_checksum.
The result is stamped with rt_build_info of the library."""
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
RADIUS = 0.05
MOVE = (0.1, 0.02, 0.05)  # the camera's translation over the exposure
LINES = ("box", "box_lens", "box_shutter", "box_lens_shutter")


def summary(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(np.min(v)), 3), max=round(float(np.max(v)), 3), all=[round(float(x), 3) for x in v])


def child(a):
    sys.path.insert(0, os.path.abspath(a.root))
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    r = ha.HostRenderer(W, H)
    d = scenes.pretty_tlas(r.scene, 8)
    r.commit()
    c = d["camera"]
    r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    r.set_pixel_filter(ha.RT_FILTER_BOX)
    out = dict(line=a.line, build=r.build_info(), batches={})
    if "lens" in a.line:
        y = H // 2
        focus = float(r.focus_at(W // 2, y))
        while not focus > 0 and y + 1 < H:
            y += 1
            focus = float(r.focus_at(W // 2, y))
        if not focus > 0:
            raise SystemExit("the centre column sees the sky from pixel %d down: no focus distance" % (H // 2))
        r.set_lens(RADIUS, focus)
        out["lens"] = dict(radius=RADIUS, focus_distance=focus, focus_pixel=[W // 2, y])
    if "shutter" in a.line:
        r.set_shutter(*(np.float32(r.camera()) + np.float32(MOVE)))
        out["shutter"] = dict(move=list(MOVE))
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
    r.set_profiling(True)
    r.profile()
    r.clear()
    r.render(ha.RT_MODE_PATH, 0, 64)
    r.synchronize()
    out["kernel_ms_64"] = {k: round(v["ms"], 3) for k, v in r.profile().items()}
    r.close()
    print("RESULT " + json.dumps(out))


def run_child(a, line):
    env = dict(os.environ)
    for k in ("RT_PRIMARY_TABLE", "RT_PRIMARY_TABLE_MIN", "RT_FUSE", "RT_STREAM", "RT_SLOTS"):
        env.pop(k, None)
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
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="(a child's work)")
    ap.add_argument("--line", default="box", choices=LINES)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {line: [] for line in LINES}
    for rnd in range(a.rounds):  # alternated: box, box_lens, box_lens_near, box, ...
        for line in LINES:
            runs[line].append(run_child(a, line))
            print("round %d %s: %s ms per 64-frame batch" % (rnd, line, runs[line][-1]["batches"]["64"]["ms"]["median"]), file=sys.stderr, flush=True)
    res = dict(width=W, height=H, rounds=a.rounds, reps=a.reps, build=runs["box"][0]["build"], lens=runs["box_lens"][0]["lens"], shutter=runs["box_shutter"][0]["shutter"], lines={})
    for line, rs in runs.items():
        res["lines"][line] = dict(kernel_ms_64=[r["kernel_ms_64"] for r in rs])
        for frames in ("64", "16"):
            sums = {r["batches"][frames]["checksum"] for r in rs}
            if len(sums) != 1:
                raise SystemExit("%s x %s frames: the accumulator differs between rounds: %s" % (line, frames, sorted(sums)))
            per_round = [r["batches"][frames]["ms"]["median"] for r in rs]
            res["lines"][line][frames] = dict(ms=summary([x for r in rs for x in r["batches"][frames]["ms"]["all"]]), per_round_median=per_round,
                                              spread_of_round_medians=round(max(per_round) - min(per_round), 3), checksum=sums.pop())
    for frames in ("64", "16"):
        med = {line: res["lines"][line][frames]["ms"]["median"] for line in LINES}
        for line, base in (("box_lens", "box"), ("box_shutter", "box"), ("box_lens_shutter", "box"), ("box_lens_shutter", "box_lens")):
            res["%s_over_%s_%s" % (line, base, frames)] = dict(ms=round(med[line] - med[base], 3), ratio=round(med[line] / med[base], 4))
    if a.parent:
        ab = dict(parent=[], this=[])
        for rnd in range(a.rounds):
            ab["parent"].append(run_bench(a, a.parent))
            ab["this"].append(run_bench(a, a.root))
            print("round %d default bench line: parent %s, this %s ms per step" % (rnd, ab["parent"][-1]["ms_per_step"], ab["this"][-1]["ms_per_step"]), file=sys.stderr, flush=True)
        # (frame_checksum is part of a --full line, whose HIP-event timers are not part of the plain line's time: one more run per build)
        full = dict(parent=run_bench(a, a.parent, True), this=run_bench(a, a.root, True))
        res["default_bench_line"] = {k: dict(ms_per_step=summary([x["ms_per_step"] for x in v]), frame_checksum_of_a_full_line=full[k]["frame_checksum"]) for k, v in ab.items()}
        p = res["default_bench_line"]["parent"]["ms_per_step"]
        res["default_bench_line"]["parent_spread_max_minus_min"] = round(p["max"] - p["min"], 3)
    print(json.dumps(res))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
