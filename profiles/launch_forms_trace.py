#!/usr/bin/env python3
"""The launch forms the bench scene does not reach, for a kernel trace: rocprofv3 --kernel-trace --stats -- python3 profiles/launch_forms_trace.py [checkout]
One process, one context per setting, the environment set before each rt_create: 16 x 8 pixels of mixed_small (glass and metal: the scene of
tests/test_gpu_chain_table.py), two calls of 32 path frames each -- the first crosses the 12-samples-per-record threshold and builds every
table, the second reads them.  Settings: the defaults; RT_ROUND0_ENTRIES=1 (k_generate_t, shade without TABLE0); RT_BOUNCE_DEPTH=1 (BOUNCE
without CHAIN); RT_BOUNCE_TABLE=0 (TABLE0 alone); RT_PRIMARY_TABLE=0 (k_generate_s, the plain shade); the sampler on (QL); a fisheye camera;
RT_FUSE 0, 1 and 2.  [checkout]: the root of the tree whose library is traced (default: this one); calls per kernel name of two trees are
then compared from the two kernel_stats.csv files (profiles/launch_forms_launch_counts.txt)."""
import importlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OWN = ("RT_ROUND0_ENTRIES", "RT_BOUNCE_DEPTH", "RT_BOUNCE_TABLE", "RT_PRIMARY_TABLE", "RT_FUSE")
SETTINGS = [("defaults", {}, None), ("round0_entries=1", {"RT_ROUND0_ENTRIES": "1"}, None), ("bounce_depth=1", {"RT_BOUNCE_DEPTH": "1"}, None),
            ("bounce_table=0", {"RT_BOUNCE_TABLE": "0"}, None), ("primary_table=0", {"RT_PRIMARY_TABLE": "0"}, None), ("sampler", {}, "sampler"),
            ("fisheye", {}, "fisheye"), ("fuse=0", {"RT_FUSE": "0"}, None), ("fuse=1", {"RT_FUSE": "1"}, None), ("fuse=2", {"RT_FUSE": "2"}, None)]


def main():
    ha = importlib.import_module("ray-and-pathtracer_amd.host_api")
    scenes = importlib.import_module("ray-and-pathtracer_amd.scenes")
    for name, env, extra in SETTINGS:
        for k in OWN:
            os.environ.pop(k, None)
        os.environ.update(env)
        r = ha.HostRenderer(16, 8)
        scenes.mixed_small(r.scene)
        r.commit()
        if extra == "fisheye":
            c = r.camera()
            r.set_camera(c[0], c[1], c[2], c[3], fisheye=True)
        if extra == "sampler":
            r.qlearn_enable(8, (-4, -1, -4), (4, 5, 6), 0.3, 0.2, 1.0, 0)
        r.clear()
        for call in range(2):
            r.render(ha.RT_MODE_PATH, 32 * call, 32)
        rgb = r.accumulator()[..., :3]
        print("%-18s sum of the finite channels %.6g" % (name, float(rgb[rgb == rgb].clip(0, 1e6).sum())), flush=True)
        r.close()


if __name__ == "__main__":
    main()
