"""Reprojection without a device: the numpy restatement (tests/reproject_ref.py) on crafted G-buffers, and the experiment run on the oracle's
own samples -- the evidence that the device test of the same experiment (tests/test_gpu_reproject.py) can be met."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_ref as rr  # noqa: E402

F32 = np.float32
# The quality experiment, fixed here on the CPU and used unchanged by tests/test_gpu_reproject.py: scenes.scene3 with every material
# diffuse, 96 x 54, the default camera A; all four camera vectors moved by each of 'moves'; 32 frames at A (0 .. 31) carried to B against
# the 4 fresh frames at B a renderer would go on with (32 .. 35: a stream of their own, not the history's first four again), both measured against 256 further frames at B (1000 .. 1255: independent of either).  bar: twice the ideal 4 / 32.
QUALITY = dict(scene="scene3", width=96, height=54, history_frames=32, fresh_frame0=32, fresh_frames=4, reference_frames=256, reference_frame0=1000,
               moves=((0.05, 0.0, 0.0), (0.2, 0.05, 0.1)), bar=0.25,
               # measured on the oracle (test_experiment_on_the_oracle prints them): MSE ratio, share of the frame carried
               oracle=((0.126, 0.474), (0.138, 0.463)))

PRETTY = np.array([(0.0, 2.0, -3.0), (-16 / 9, 3.0, -1.0), (16 / 9, 3.0, -1.0), (-16 / 9, 1.0, -1.0)], F32)  # scenes.pretty_tlas's camera
SKEWED = np.array([(0.3, 1.7, -2.6), (-1.9, 2.8, -0.7), (1.5, 3.1, -1.2), (-1.7, 0.9, -0.5)], F32)          # no right angle, no axis


def pixel_points(camera, w, h, t):
    """cam + normalize(P - cam) * t for the screen point P of every pixel (Camera::GetPrimaryRay's u = x / W, v = y / H), f32"""
    cam, TL, TR, BL = np.asarray(camera, F32)
    u = (np.arange(w, dtype=F32) * F32(1.0 / w)).astype(F32)[None, :, None]
    v = (np.arange(h, dtype=F32) * F32(1.0 / h)).astype(F32)[:, None, None]
    P = (TL + u * (TR - TL) + v * (BL - TL)).astype(F32)
    D = P - cam
    D = (D / np.sqrt((D * D).sum(-1, keepdims=True))).astype(F32)
    return (cam + D * np.asarray(t, F32)[..., None]).astype(F32)


@pytest.mark.parametrize("camera", [PRETTY, SKEWED], ids=["pretty_tlas", "skewed"])
@pytest.mark.parametrize("size", [(64, 40), (97, 41), (320, 180), (1920, 1080)], ids=lambda s: "%dx%d" % s)
def test_unmoved_camera_maps_every_pixel_to_itself(size, camera):
    w, h = size
    t = np.random.default_rng(w * 1000 + h).uniform(0.5, 30.0, (h, w)).astype(F32)
    rx, ry, ok = rr.project(pixel_points(camera, w, h, t), camera, w, h)
    assert rx.dtype == F32 and ry.dtype == F32
    ys, xs = np.mgrid[0:h, 0:w]
    miss = ~ok | (rx != xs) | (ry != ys)
    assert miss.sum() == 0, "%d of %d pixels do not land on themselves" % (miss.sum(), w * h)


# ---- crafted G-buffers ---------------------------------------------------------------------------------------------------------------
W, H = 8, 6
MAT_TYPE = np.array([1, 1, 2, 1], np.int32)          # 0, 1 diffuse; 2 metal; 3 a shiny diffuse
MAT_SHINY = np.array([0, 0, 0, 0.5], F32)


def crafted():
    """a wall z = 0 seen by PRETTY (cam z = -3, screen z = -1: the wall's points are cam + 1.5 (P - cam), z exactly 0), normal (0, 0, -1),
    object 3, material 0, 5 samples per pixel; the current G-buffer is the history's: every pixel is carried from itself"""
    cam, TL, TR, BL = PRETTY
    u = (np.arange(W, dtype=F32) / F32(W))[None, :, None]
    v = (np.arange(H, dtype=F32) / F32(H))[:, None, None]
    P = (TL + u * (TR - TL) + v * (BL - TL)).astype(F32)
    pos = (cam + F32(1.5) * (P - cam)).astype(F32)
    assert np.all(pos[..., 2] == 0)
    g = dict(pos=pos, normal=np.tile(np.array([0, 0, -1], F32), (H, W, 1)), t=np.full((H, W), 2.0, F32),
             obj=np.full((H, W), 3, np.int32), mat=np.zeros((H, W), np.int32))
    cur = {k: a.copy() for k, a in g.items()}
    rng = np.random.default_rng(1)
    acc = rng.random((H, W, 4)).astype(F32) * 5
    cnt = np.full((H, W), 5, np.uint32)
    sy, syy = rng.random((H, W)).astype(F32) * 5, rng.random((H, W)).astype(F32) * 5
    return cur, g, acc, cnt, sy, syy


def run(cur, hist, acc, cnt, sy, syy, **params):
    return rr.reproject(cur, hist, acc, cnt, sy, syy, PRETTY, MAT_TYPE, MAT_SHINY, **params)


def failing(out):
    return sorted(map(tuple, np.argwhere(out[5] < 0).tolist()))


def test_crafted_unmoved_frame_is_carried_whole():
    cur, hist, acc, cnt, sy, syy = crafted()
    a, c, y, yy, n, src, el = run(cur, hist, acc, cnt, sy, syy)
    assert n == W * H and el.all() and np.array_equal(src, np.arange(W * H).reshape(H, W))
    assert np.array_equal(a.view(np.uint32), acc.view(np.uint32)) and np.array_equal(c, cnt)
    assert np.array_equal(y.view(np.uint32), sy.view(np.uint32)) and np.array_equal(yy.view(np.uint32), syy.view(np.uint32))
    assert a.dtype == F32 and c.dtype == np.uint32 and y.dtype == F32 and yy.dtype == F32


def test_crafted_failures_are_exactly_the_named_pixels():
    cur, hist, acc, cnt, sy, syy = crafted()
    cam = PRETTY[0]
    named = []
    cur["pos"][0, 1] = cam - (cur["pos"][0, 1] - cam)            # behind the camera: lam < 0
    named.append((0, 1))
    cur["pos"][0, 3] = cam                                        # the camera itself: d = 0, lam is not finite
    named.append((0, 3))
    cur["pos"][1, 2] += np.array([100, 0, 0], F32)                # projects outside the frame, to the right
    named.append((1, 2))
    cur["pos"][1, 4] += np.array([0, 100, 0], F32)                # ... above it
    named.append((1, 4))
    cur["obj"][2, 0] = 4                                          # another object
    named.append((2, 0))
    cur["mat"][2, 5] = 1                                          # another material (eligible itself)
    named.append((2, 5))
    tol = F32(0.25)
    cur["normal"][3, 1] = (np.nextafter(tol, F32(1)), 0, -1)      # |n_p - n'_q| one ulp over the tolerance
    named.append((3, 1))
    cur["normal"][3, 2] = (tol, 0, -1)                            # exactly on it: carried
    lim = F32(0.01) * F32(2.0)
    cur["pos"][4, 3, 2] = np.nextafter(lim, F32(1))               # off the history pixel's plane by one ulp more than 0.01 t_p
    named.append((4, 3))
    cur["pos"][4, 4, 2] = lim                                     # exactly on the limit: carried
    cur["pos"][4, 5, 2] = -lim                                    # the other side
    cur["pos"][4, 6, 2] = -np.nextafter(lim, F32(1))
    named.append((4, 6))
    cnt[5, 7] = 0                                                 # an empty history pixel
    named.append((5, 7))
    cur["obj"][5, 0] = -1                                         # a miss
    named.append((5, 0))
    cur["mat"][0, 6], hist["mat"][0, 6] = 2, 2                    # metal on both sides
    cur["mat"][0, 7], hist["mat"][0, 7] = 3, 3                    # shiny diffuse on both sides
    cur["mat"][3, 7], hist["mat"][3, 7] = 7, 7                    # a material index outside the table
    cur["mat"][3, 6], hist["mat"][3, 6] = -1, -1
    view = [(0, 6), (0, 7), (3, 6), (3, 7)]
    out = run(cur, hist, acc, cnt, sy, syy)
    assert failing(out) == sorted(named + view)
    assert out[4] == W * H - len(named) - len(view)
    assert sorted(map(tuple, np.argwhere(~out[6]).tolist())) == sorted([(5, 0)] + view)
    # a failed pixel is zero, a carried one has the history's bits
    off = out[5] < 0
    assert not out[0][off].any() and not out[1][off].any() and not out[2][off].any() and not out[3][off].any()
    assert np.array_equal(out[0][~off].view(np.uint32), acc[~off].view(np.uint32)) and np.array_equal(out[1][~off], cnt[~off])
    # with carry_view_dependent the view-dependent materials are carried; the miss still is not
    out = run(cur, hist, acc, cnt, sy, syy, carry_view_dependent=1)
    assert failing(out) == sorted(named) and out[6].sum() == W * H - 1
    # zero tolerances: only exact agreement passes
    out = run(cur, hist, acc, cnt, sy, syy, carry_view_dependent=1, normal_tolerance=0.0, plane_tolerance=0.0)
    assert failing(out) == sorted(named + [(3, 2), (4, 4), (4, 5)])


def test_crafted_moved_camera_gathers_from_the_neighbour():
    """the history camera one pixel's width to the left of the wall's grid: every pixel's point lands one history pixel to the right"""
    cur, hist, acc, cnt, sy, syy = crafted()
    step = (PRETTY[2] - PRETTY[1]) / F32(W)                       # one pixel on the screen plane ...
    moved = (PRETTY - F32(1.5) * step).astype(F32)                # ... is 1.5 of it on the wall
    out = rr.reproject(cur, hist, acc, cnt, sy, syy, moved, MAT_TYPE, MAT_SHINY)
    src = out[5]
    assert np.all(src[:, :-1] == np.arange(W * H).reshape(H, W)[:, 1:]) and np.all(src[:, -1] == -1)
    assert np.array_equal(out[0][:, :-1].view(np.uint32), acc[:, 1:].view(np.uint32))


def test_max_history_scales_sums_and_caps_counts():
    cur, hist, acc, cnt, sy, syy = crafted()
    cnt[0, :4] = (5, 8, 9, 40)
    a, c, y, yy, n, _, _ = run(cur, hist, acc, cnt, sy, syy, max_history=8)
    assert n == W * H
    assert c[0, :4].tolist() == [5, 8, 8, 8]
    for x in (0, 1):                                              # at or below the cap: the bits stay
        assert np.array_equal(a[0, x].view(np.uint32), acc[0, x].view(np.uint32)) and y[0, x] == sy[0, x] and yy[0, x] == syy[0, x]
    for x, k in ((2, 9), (3, 40)):
        f = F32(F32(8) / F32(k))
        assert np.array_equal(a[0, x], (acc[0, x] * f).astype(F32)) and y[0, x] == F32(sy[0, x] * f) and yy[0, x] == F32(syy[0, x] * f)
        # the mean stays within rounding
        assert np.allclose(a[0, x] / 8, acc[0, x] / k, rtol=1e-6)
    # max_history = 0: no cap
    a, c = run(cur, hist, acc, cnt, sy, syy)[:2]
    assert c[0, :4].tolist() == [5, 8, 9, 40] and np.array_equal(a.view(np.uint32), acc.view(np.uint32))


# ---- the experiment ------------------------------------------------------------------------------------------------------------------
def mse_ratio(carried_mean, fresh_mean, reference, on):
    """MSE of the carried pixels' history mean against 'reference' over the MSE of the fresh render, on the carried pixels that are finite
    in all three; also the pixels compared"""
    fin = on & np.isfinite(carried_mean).all(-1) & np.isfinite(fresh_mean).all(-1) & np.isfinite(reference).all(-1)
    mse_c = ((carried_mean[fin] - reference[fin]) ** 2).mean()
    mse_f = ((fresh_mean[fin] - reference[fin]) ** 2).mean()
    return float(mse_c / mse_f), int(fin.sum())


def test_experiment_on_the_oracle(scenes, oracle_api):
    """32 frames at camera A, carried to camera B by the restatement (the oracle's G-buffers: primary rays, find_nearest at Sample's
    0.001), against 4 fresh frames at B; both against a 256-frame mean at B.  A carry from the right surface point has the variance of 32
    samples, 1 / 8 of the fresh render's; a carry from a wrong point adds a bias that does not shrink.  Asserted: ratio < 0.25."""
    q = QUALITY
    w, h = q["width"], q["height"]
    o = rr.MaterialRecorder(oracle_api.OracleScene())
    getattr(scenes, q["scene"])(o)
    o.set_raytracer(False)
    mt, ms = o.tables()
    r = oracle_api.OracleRenderer(o, w, h)
    cam_a = r.camera()
    r.render(0, q["history_frames"], nthreads=0)
    acc_a = r.accumulator()
    g_a = rr.gbuffer_of(o, r)
    cnt = np.full((h, w), q["history_frames"], np.uint32)
    zero = np.zeros((h, w), F32)
    for move, (want_ratio, want_share) in zip(q["moves"], q["oracle"]):
        cam_b = (cam_a + np.array(move, F32)).astype(F32)
        r.set_camera(*cam_b)
        g_b = rr.gbuffer_of(o, r)
        acc, c, _, _, n, src, el = rr.reproject(g_b, g_a, acc_a, cnt, zero, zero, cam_a, mt, ms)
        r.clear()
        r.render(q["fresh_frame0"], q["fresh_frames"], nthreads=0)
        fresh = r.accumulator()[..., :3].astype(np.float64) / q["fresh_frames"]
        r.clear()
        r.render(q["reference_frame0"], q["reference_frames"], nthreads=0)
        ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
        with np.errstate(all="ignore"):
            mean = acc[..., :3].astype(np.float64) / c[..., None]
        ratio, compared = mse_ratio(mean, fresh, ref, src >= 0)
        print("oracle move %s: MSE ratio carried / fresh %.3f on %d pixels, %.1f %% of the frame carried, %.1f %% of the eligible pixels rejected"
              % (move, ratio, compared, 100.0 * n / (w * h), 100.0 * (el.sum() - n) / max(1, el.sum())))
        assert n >= 0.1 * w * h, "the experiment carries too little to say anything"
        assert ratio < q["bar"], ratio
        # the oracle is deterministic: the recorded figures hold to their last printed digit and a little more
        assert abs(ratio - want_ratio) < 0.005 and abs(n / (w * h) - want_share) < 0.005, (ratio, n / (w * h))
    r.close()
    o.close()
