"""Scenes, depth lists, inputs and thresholds shared by the start-depth tests.  A plain helper module of the test suite, numpy only:
tests/test_depths_cpu.py shows on the oracle alone that neighbouring depths of every case differ on enough rays to tell a wrong depth
from a right one, tests/test_gpu_depths.py holds the device to the oracle at the same scenes, functions and depths.

A function is (mode, flag): Renderer::Trace (mode 0) or Renderer::Sample (mode 1), called while scene.raytracer is 'flag'.  Tick calls
Trace with the flag set and Sample with it clear; the other two combinations run k_trace_general / k_sample_general, and so does Sample
with the flag clear on a scene the wavefront cannot replay (a shiny diffuse material, materials built with raytracer == false)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from budget_shapes import shiny  # noqa: E402  (the scene tests/test_gpu_adaptive.py renders under this name)

W, H = 48, 32                 # the caller rays: the primary rays of the scene's own camera at this size
ENERGY = (0.9, 0.8, 0.7)
SEED_BASE = 4242
TRACE, SAMPLE = 0, 1          # RT_MODE_WHITTED, RT_MODE_PATH


def hall(b):
    """two facing shiny planes around one light: the mirror child of every diffuse hit meets a shiny diffuse surface again, so the
    general kernels' suspended frames nest once per level of depth"""
    b.area_light(11, (0.5, 1.5, 1.0), 10.0, (1, 1, 1), 0.3, (0, -1, 0))
    sh = b.diffuse(0.8, (1, 1, 1), 0.3, 0.7, 4, shininess=0.25, rt=False)
    b.plane(0, sh, (0, 1, 0), 0)
    b.plane(1, sh, (0, -1, 0), 3)
    b.build(0)
    return dict(name="hall", tlas=False)


class _Materials:
    """a scene builder whose materials are all built with raytracer == rt, whatever the scene function passes"""

    def __init__(self, b, rt):
        self._b, self._rt = b, rt

    def __getattr__(self, name):
        f = getattr(self._b, name)
        if name in ("diffuse", "glass", "metal"):
            return lambda *a, **k: f(*a, **dict(k, rt=self._rt))
        return f


def shiny_rt(b):
    """'shiny' as a scene constructed while the flag is set has it: what Tick's Trace renders"""
    return shiny(_Materials(b, True))


def scene_fn(scenes, name):
    """name -> (scene function, keyword arguments)"""
    return {"mixed_small": (scenes.mixed_small, {}), "pretty_tlas": (scenes.pretty_tlas, {"n_instances": 4}),
            "mixed_small_rt0": (scenes.mixed_small, {"rt": False}), "pretty_tlas_rt0": (scenes.pretty_tlas, {"n_instances": 4, "rt": False}),
            "shiny": (shiny, {}), "shiny_rt": (shiny_rt, {}), "hall": (hall, {})}[name]


# ---- part A: Sample as Tick calls it, on the round pipelines ------------------------------------------------------------------------------
PATH_SCENES = ("mixed_small", "pretty_tlas")
PATH_DEPTHS = (-1, 0, 1, 2, 3, 4, 5, 6, 7)
PATH_ENVS = [{}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}, {"RT_DECIDE": "0"}, {"RT_STREAM": "0"}, {"RT_STREAM": "0", "RT_SLOTS": "777"}]
PREFIX_DEPTHS, PREFIX_SIZES = (0, 6), (1, 65)

# ---- part B: the general kernels ------------------------------------------------------------------------------------------------------
D1_7 = (1, 2, 3, 4, 5, 6, 7)
# (scene, mode, flag, depths)
GENERAL_CASES = [
    ("mixed_small_rt0", TRACE, False, D1_7), ("mixed_small_rt0", SAMPLE, True, D1_7),
    ("pretty_tlas_rt0", TRACE, False, D1_7), ("pretty_tlas_rt0", SAMPLE, True, D1_7),
    ("shiny", TRACE, False, D1_7), ("shiny", SAMPLE, False, (-1, 0) + D1_7),
    # depth 5 of Sample nests RT_SAMPLE_FRAMES = 6 frames and depth 12 of Trace nests RT_TRACE_FRAMES = 12: the last depths that fit
    # (Trace with the flag clear weighs its indirect child with dot(scatteredDir, (1, 1, 1)), of either sign: the terms of a tree partly
    # cancel, and the device adds them top-down where the recursion adds bottom-up.  On an MI355X: 7.5e-5 relative at most up to depth 7
    # and 9.2e-5 at depth 12, up to 4096 leaves a ray -- the largest error of all these cases, within the 1e-4 bar; the same function on the other scenes 2.1e-5, every other function 1.2e-6)
    ("hall", SAMPLE, False, (0, 1, 2, 3, 4, 5)), ("hall", TRACE, False, D1_7 + (12,)),
]
SAMPLE_FRAMES, TRACE_FRAMES = 6, 12          # csrc/rt_kernels.h
HALL_SAMPLE_FITS, HALL_SAMPLE_OVERFLOWS = 5, 6
HALL_TRACE_FITS, HALL_TRACE_OVERFLOWS = 12, 13
ONE_RAY, ONE_DEPTH, ONE_SEED = 900, 5, 0x12345678  # rapt::Renderer::Trace / Sample on one ray (a floor hit: ray 700 of mixed_small sees the sky at any depth)

# ---- part C: Whitted ----------------------------------------------------------------------------------------------------------------------
WHITTED_ENVS = [{}, {"RT_MEGA": "0"}, {"RT_MEGA_LEVELS": "1"}]
# scene -> (frame width, frame height, depths); 'shiny_rt' stops at 3: deeper shiny trees against the 12 pending branches a pixel may
# hold have not been measured
WHITTED_CASES = {"mixed_small": (97, 61, (1, 2, 3, 5, 7)), "pretty_tlas": (120, 67, (1, 2, 3, 5, 7)), "shiny_rt": (97, 61, (1, 2, 3))}

# ---- what tests/test_depths_cpu.py asks of these inputs -----------------------------------------------------------------------------------
# the share of the rays, finite at both depths, whose value differs between two neighbouring tested depths
MIN_SHARE, MIN_SHARE_DEEP, DEEP_FROM = 0.005, 0.002, 6   # ... up to depth 5; when the deeper of the two is 6 or 7 (3 of 1536 rays)
MIN_SHARE_ROULETTE = 0.30                                # 4 -> 5 where 'depth < 5' gates the first hit's roulette draw
MIN_SHARE_HALL = 0.90                                    # every step on 'hall'


def roulette_case(mode, flag):
    """the functions whose first hit draws a roulette number below depth 5 only: Trace with the flag clear, Sample with it set"""
    return (mode == TRACE and not flag) or (mode == SAMPLE and flag)


def changed_share(a, b):
    """the share of rays, finite in both, whose value differs (a, b: [n][3])"""
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    return float((fin & (a.view(np.uint32) != b.view(np.uint32)).any(1)).mean())


def oracle_pair(scenes, oracle_api, name, w=W, h=H):
    """the oracle's scene and a renderer of w x h at the scene's own camera"""
    fn, kw = scene_fn(scenes, name)
    o = oracle_api.OracleScene()
    d = fn(o, **kw)
    orr = oracle_api.OracleRenderer(o, w, h)
    if "camera" in d:
        c = d["camera"]
        orr.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return o, orr


_REFS = {}


def oracle_values(scenes, oracle_api, name, mode, flag, depths):
    """depth -> the oracle's [W * H][3] values of the function on the caller rays (computed once per session, never written to)"""
    key = (name, mode, bool(flag))
    have = _REFS.setdefault(key, {})
    if any(d not in have for d in depths):
        o, orr = oracle_pair(scenes, oracle_api, name)
        o.set_raytracer(bool(flag))
        O, D = orr.primary_rays()
        for d in depths:
            if d not in have:
                have[d] = orr.trace_rays(mode, O, D, d, ENERGY, seed_base=SEED_BASE)
                have[d].setflags(write=False)
        orr.close()
        o.close()
    return {d: have[d] for d in depths}
