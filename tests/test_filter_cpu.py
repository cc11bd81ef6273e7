"""The pixel filter of path-mode camera samples on the CPU: tests/filter_ref.py's offsets against the moments of their distributions, its
pinhole ray against the oracle's primary_rays() bit for bit, and the quality experiment on the oracle that tests/test_gpu_filter.py reruns
with the device's renders (QUALITY, quality_scene, the quality fixture, quality_mse)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as fr  # noqa: E402

SKEWED = ((0.3, 1.2, -2.5), (-1.9, 2.3, -0.4), (1.6, 2.1, 0.2), (-1.7, 0.2, -0.6))
SIZES = [(48, 27), (65, 1), (257, 3), (1920, 1080)]

# the quality experiment: a frame of 48 x 27 under the default camera over a 96 x 48 two-colour checkerboard sky; one small sphere and one
# small light, both behind the camera, so that every camera ray's radiance is a texel (no random draw decides anything)
QUALITY = dict(width=48, height=27, sky=(96, 48), colours=((250, 240, 230), (10, 20, 30)), truth_grid=8, frames=(4, 16, 64), seed_base=0x12345678,
               ratio_max=0.25)


# ---- offsets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,half,var,m4", [(fr.BOX, 0.5, 1 / 12, 1 / 80), (fr.TENT, 1.0, 1 / 6, 1 / 15)], ids=["box", "tent"])
def test_offsets_have_their_distribution_s_moments(kind, half, var, m4):
    """uniform on [-1/2, 1/2]: variance 1/12, fourth moment 1/80; the tent 1 - |x| on [-1, 1]: variance 2 (1/3 - 1/4) = 1/6, fourth moment
    2 (1/5 - 1/6) = 1/15.  Standard error of the mean sqrt(var / n), of the sample variance sqrt((m4 - var^2) / n)."""
    n = 1 << 16
    s = (np.arange(n, dtype=np.uint64) + 0x12345678).astype(np.uint32)
    se_mean, se_var = np.sqrt(var / n), np.sqrt((m4 - var * var) / n)
    for d in fr.offsets(kind, s):
        assert d.dtype == np.float32 and d.min() >= -half and d.max() <= half
        d = d.astype(np.float64)
        print("kind %d: mean %.5f (se %.5f), variance %.5f (expected %.5f, se %.5f)" % (kind, d.mean(), se_mean, d.var(), var, se_var))
        assert abs(d.mean()) <= 5 * se_mean
        assert abs(d.var() - var) <= 5 * se_var


def test_offset_end_points():
    ends = np.float32([0.0, 1.0])
    assert np.array_equal(fr.offset(fr.BOX, ends), np.float32([-0.5, 0.5]))
    assert np.array_equal(fr.offset(fr.TENT, ends), np.float32([-1.0, 1.0]))
    assert np.array_equal(fr.offset(fr.POINT, ends), np.float32([0.0, 0.0]))
    assert np.array_equal(fr.offset(fr.TENT, np.float32([0.5])), np.float32([0.0]))
    # RandomFloat reaches both: state 2^32 - 1 rounds to 1.0f
    assert np.float32(np.uint32(0xFFFFFFFF)) * np.float32(2.3283064365387e-10) == np.float32(1.0)


def test_jitter_stream_is_not_the_path_stream():
    w, h = 64, 40
    for f in range(4):
        s = fr.sample_index(w, h, f, 0x12345678)
        path, jit = fr.stream_seed(s), fr.stream_seed(~s)
        assert np.all(path != jit)
        # ... and stays apart over the draws the jitter takes
        for _ in range(2):
            path, a = fr.random_float(path)
            jit, b = fr.random_float(jit)
            assert np.all(path != jit)


def test_streams_restate_the_oracle(oracle_api):
    import ctypes as C
    L = oracle_api.lib()
    for index in (0, 1, 0x12345678, 0xFFFFFFFF, 0xEDCBA987):
        u, f = np.zeros(4, np.uint32), np.zeros(4, np.float32)
        L.orc_rng_stream(C.c_uint(index), 4, u.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p))
        s = fr.stream_seed(np.uint32([index]))
        for k in range(4):
            s, x = fr.random_float(s)
            assert s[0] == u[k] and x[0] == f[k]


# ---- rays -----------------------------------------------------------------------------------------------------------------
def _tiny_scene(b):
    b.sky(np.full((4, 8, 3), 128, np.uint8))
    b.area_light(11, (0.0, 3.0, -6.0), 1.0, (1, 1, 1), 0.1, (0, -1, 0))
    m = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    b.sphere(1, m, (0.0, 1.0, -6.0), 0.1)
    b.build(0)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_point_rays_are_the_oracle_s_primary_rays(size, oracle_api):
    w, h = size
    o = oracle_api.OracleScene()
    _tiny_scene(o)
    orr = oracle_api.OracleRenderer(o, w, h)
    for cam in (None, SKEWED):
        if cam:
            orr.set_camera(*cam)
        O_ref, D_ref = orr.primary_rays()
        O, D = fr.rays(fr.POINT, orr.camera(), w, h, 3, 0xFFFFFF00)
        assert np.array_equal(O.view(np.uint32), O_ref.view(np.uint32))
        assert np.array_equal(D.view(np.uint32), D_ref.view(np.uint32))
    orr.close()
    o.close()


# ---- the quality experiment -------------------------------------------------------------------------------------------------
def quality_scene(b):
    q = QUALITY
    sw, sh = q["sky"]
    yy, xx = np.mgrid[0:sh, 0:sw]
    sky = np.where(((xx + yy) & 1)[..., None] == 0, np.uint8(q["colours"][0]), np.uint8(q["colours"][1])).astype(np.uint8)
    b.sky(sky)
    b.area_light(11, (0.0, 3.0, -6.0), 1.0, (1, 1, 1), 0.1, (0, -1, 0))
    m = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
    b.sphere(1, m, (0.0, 1.0, -6.0), 0.1)
    b.build(0)


def quality_truth(orr):
    """the mean over truth_grid^2 restated POINT sub-samples spanning [x - 0.5, x + 0.5) x [y - 0.5, y + 0.5) of the gamma-corrected radiance"""
    w, h, g = QUALITY["width"], QUALITY["height"], QUALITY["truth_grid"]
    x, y = fr.pixel_xy(w, h)
    acc = np.zeros((w * h, 3), np.float64)
    for j in range(g):
        for i in range(g):
            fx = x + np.float32(-0.5 + (i + 0.5) / g)
            fy = y + np.float32(-0.5 + (j + 0.5) / g)
            O, D = fr.primary_ray_f(orr.camera(), w, h, fx, fy)
            acc += fr.gamma(orr.trace_rays(1, O, D, depth=4, seed_base=0))
    return (acc / (g * g)).reshape(h, w, 3)


@pytest.fixture(scope="module")
def quality(oracle_api):
    """the experiment on the oracle, once per module that asks for it: dict(scene, renderer, truth); closed when the module is done"""
    o = oracle_api.OracleScene()
    quality_scene(o)
    o.set_raytracer(False)
    orr = oracle_api.OracleRenderer(o, QUALITY["width"], QUALITY["height"])
    yield dict(scene=o, renderer=orr, truth=quality_truth(orr))
    orr.close()
    o.close()


def quality_mse(mean, truth):
    """MSE over the interior finite pixels"""
    a, b = np.asarray(mean, np.float64)[1:-1, 1:-1, :3], truth[1:-1, 1:-1]
    fin = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    assert fin.sum() > 0.9 * fin.size
    return float(((a[fin] - b[fin]) ** 2).mean())


def test_box_filter_antialiases_where_the_reference_mode_cannot(quality):
    q = QUALITY
    orr, truth = quality["renderer"], quality["truth"]
    cam = orr.camera()
    mse = {}
    for n in q["frames"]:
        mse[n] = quality_mse(fr.accumulate(orr, fr.BOX, cam, 0, n, q["seed_base"]) / n, truth)
    nmax = q["frames"][-1]
    point = quality_mse(fr.accumulate(orr, fr.POINT, cam, 0, 1, q["seed_base"]), truth)  # (every frame of POINT is the same frame here)
    orr.clear()
    orr.render(0, nmax, q["seed_base"], nthreads=0)
    reference = quality_mse(orr.accumulator()[..., :3] / nmax, truth)
    print("MSE box %s, point %.5f, reference mode (%d frames) %.5f: box / point %.3f, box / reference %.3f"
          % (" ".join("%d: %.5f" % kv for kv in mse.items()), point, nmax, reference, mse[nmax] / point, mse[nmax] / reference))
    assert mse[nmax] <= q["ratio_max"] * point
    assert mse[nmax] <= q["ratio_max"] * reference
    assert mse[q["frames"][0]] > mse[q["frames"][1]] > mse[q["frames"][2]]
