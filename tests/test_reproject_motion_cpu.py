"""rt_reproject_motion without a device: the numpy restatement (tests/reproject_motion_ref.py) on crafted G-buffers.  Every G-buffer is made
here by intersecting the pinhole rays of a camera with quads that carry an instance index, in front of a wall of index -1 (no instance):
the translation, rotation, wrong-instance and singular-inverse cases of the definition in include/rt_amd.h, each with a result that can be
named pixel by pixel.  tests/test_gpu_reproject_motion.py holds k_reproject_motion against the same restatement bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_ref as rr  # noqa: E402
import reproject_motion_ref as rm  # noqa: E402

F32 = np.float32
CAMERA = np.array([(0.0, 2.0, -3.0), (-16 / 9, 3.0, -1.0), (16 / 9, 3.0, -1.0), (-16 / 9, 1.0, -1.0)], F32)  # scenes.pretty_tlas's camera
MAT_TYPE, MAT_SHINY = np.array([1, 1], np.int32), np.array([0, 0], F32)  # two plain diffuse materials: every hit is eligible
W, H = 48, 27          # square pixels under CAMERA's 16 : 9 screen
WALL_Z, QUAD_Z = 2.0, 1.0
PX = (32 / 9) / W * ((QUAD_Z + 3) / 2)  # one pixel's footprint on the plane z = QUAD_Z (the screen is 2 in front of the camera, the plane 4)


def column_x(x, w=W):
    """world x where pixel column x's ray crosses z = QUAD_Z (a fractional x: between two rays)"""
    return (QUAD_Z + 3) / 2 * (-16 / 9 + x * (32 / 9) / w)


def row_y(y, h=H):
    return 2 + (QUAD_Z + 3) / 2 * (1 - 2 * y / h)


def translate(x, y, z):
    M = np.eye(4)
    M[:3, 3] = (x, y, z)
    return M


def rotate(axis, deg):
    a, M = np.radians(deg), np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)]["xyz".index(axis)]
    M[i, i], M[i, j], M[j, i], M[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return M


def quad(T, hx, hy, obj=5, mat=1):
    """an instance: the local rectangle |x| <= hx, |y| <= hy of the plane z = 0, local normal (0, 0, -1), under the 4 x 4 transform T"""
    T = np.asarray(T, np.float64)
    return dict(T=T.astype(F32), invT=np.linalg.inv(T).astype(F32), hx=hx, hy=hy, obj=obj, mat=mat)


def xf_table(quads):
    return rm.table([q["T"] for q in quads], [q["invT"] for q in quads])


def gbuffer(quads, camera=CAMERA, w=W, h=H):
    """what rt_render_aovs would store for the wall z = WALL_Z (object 1, material 0, no instance) with the quads in front of it: per pixel
    the nearest hit of Camera::GetPrimaryRay's ray (u = x / W, v = y / H); the world normal of a quad is normalize(T n) like resolve_hit's"""
    cam, TL, TR, BL = np.asarray(camera, np.float64)
    u, v = (np.arange(w) / w)[None, :, None], (np.arange(h) / h)[:, None, None]
    D = TL + u * (TR - TL) + v * (BL - TL) - cam
    D /= np.sqrt((D * D).sum(-1, keepdims=True))
    t = (WALL_Z - cam[2]) / D[..., 2]
    g = dict(t=t, normal=np.tile(np.array([0.0, 0, -1]), (h, w, 1)), obj=np.full((h, w), 1, np.int32), mat=np.zeros((h, w), np.int32), inst=np.full((h, w), -1, np.int32))
    for k, q in enumerate(quads):
        inv, T = q["invT"].astype(np.float64), q["T"].astype(np.float64)
        Ol, Dl = inv[:3, :3] @ cam + inv[:3, 3], D @ inv[:3, :3].T
        with np.errstate(all="ignore"):
            tq = -Ol[2] / Dl[..., 2]
            P = Ol + Dl * tq[..., None]
            hit = (tq > 0) & (tq < g["t"]) & (np.abs(P[..., 0]) <= q["hx"]) & (np.abs(P[..., 1]) <= q["hy"])
        n = T[:3, :3] @ np.array([0.0, 0, -1])
        g["t"] = np.where(hit, tq, g["t"])
        g["normal"][hit] = n / np.sqrt(n @ n)
        g["obj"][hit], g["mat"][hit], g["inst"][hit] = q["obj"], q["mat"], k
    g["t"], g["normal"] = g["t"].astype(F32), g["normal"].astype(F32)
    g["pos"] = (np.asarray(camera, F32)[0] + (D.astype(F32) * g["t"][..., None]).astype(F32)).astype(F32)
    return g


def history(h=H, w=W, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 4)).astype(F32) * 5, rng.integers(1, 40, (h, w)).astype(np.uint32), rng.random((h, w)).astype(F32) * 5, rng.random((h, w)).astype(F32) * 5)


def run(cur, hist, hs, cur_quads, hist_quads, camera=CAMERA, **params):
    return rm.reproject(cur, hist, *hs, camera, xf_table(cur_quads), xf_table(hist_quads), MAT_TYPE, MAT_SHINY, **params)


def bits(out):
    return [np.asarray(a).view(np.uint32) if np.asarray(a).dtype == F32 else np.asarray(a) for a in out[:4]] + [out[4]]


def non_vacuous(out):
    """the bars of the motion cases: at least 10 % of the frame carried, at least 1 % of the eligible pixels rejected"""
    src, el = out[5], out[6]
    carried, rejected = int((src >= 0).sum()), int((el & (src < 0)).sum())
    assert carried >= 0.10 * src.size, "only %d of %d pixels carried" % (carried, src.size)
    assert rejected >= 0.01 * el.sum(), "only %d of %d eligible pixels rejected" % (rejected, el.sum())


def centred(x0, x1, y0, y1, z=QUAD_Z):
    """the transform and half extents of a quad that covers pixel columns x0 .. x1 and rows y0 .. y1 at z, its edges half way between rays"""
    cx, cy = column_x((x0 + x1) / 2), row_y((y0 + y1) / 2)
    return translate(cx, cy, z), (x1 - x0 + 1) / 2 * PX, (y1 - y0 + 1) / 2 * PX


# ---- unmoved equivalence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 9), (1, 1)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("params", [{}, dict(max_history=8), dict(normal_tolerance=0.0, plane_tolerance=0.0)], ids=["defaults", "max_history", "zero_tolerances"])
def test_identical_tables_are_rt_reproject_bit_for_bit(size, params):
    w, h = size
    moved_cam = (CAMERA + F32([0.05, 0.02, 0.0])).astype(F32)
    quads = [quad(translate(-0.4, 2.1, QUAD_Z) @ rotate("y", 20), 0.8, 0.5), quad(translate(0.9, 1.8, 0.5), 0.4, 0.4, obj=6)]
    if size == (1, 1):
        quads = [quad(translate(0, 2, QUAD_Z), 5, 5)]  # the one pixel's ray (the screen's top left corner) hits the instance
    hist, cur = gbuffer(quads, CAMERA, w, h), gbuffer(quads, moved_cam, w, h)
    assert (cur["inst"] >= 0).any()
    hs = history(h, w)
    got = rm.reproject(cur, hist, *hs, CAMERA, xf_table(quads), xf_table(quads), MAT_TYPE, MAT_SHINY, **params)
    want = rr.reproject(cur, hist, *hs, CAMERA, MAT_TYPE, MAT_SHINY, **params)
    for a, b in zip(bits(got), bits(want)):
        assert np.array_equal(a, b)
    assert np.array_equal(got[5], want[5])
    if size != (1, 1):
        assert got[4] > 0 and (got[5] < 0).any()
    # a scene without a TLAS: no tables at all, every index -1
    cur["inst"][:], hist["inst"][:] = -1, -1
    got = rm.reproject(cur, hist, *hs, CAMERA, None, None, MAT_TYPE, MAT_SHINY, **params)
    for a, b in zip(bits(got), bits(want)):
        assert np.array_equal(a, b)


# ---- translation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(3, 0), (-4, 2)], ids=["right3", "left4_down2"])
def test_translation_by_whole_pixels_carries_from_the_shifted_pixel(shift):
    mx, my = shift
    T0, hx, hy = centred(14, 29, 7, 18)
    T1, _, _ = centred(14 + mx, 29 + mx, 7 + my, 18 + my)
    was, now = [quad(T0, hx, hy)], [quad(T1, hx, hy)]
    hist, cur = gbuffer(was), gbuffer(now)
    assert np.array_equal(np.argwhere(hist["inst"] == 0).min(0), (7, 14)) and np.array_equal(np.argwhere(cur["inst"] == 0).max(0), (18 + my, 29 + mx))
    hs = history()
    out = run(cur, hist, hs, now, was)
    src = out[5]
    ys, xs = np.mgrid[0:H, 0:W]
    on = cur["inst"] == 0
    # the quad: every pixel carries from exactly the pixel the translation took it from (all of them lie in the frame here)
    assert np.array_equal(src[on], ((ys - my) * W + (xs - mx))[on])
    # the wall the quad uncovered starts empty (the history saw the quad there: another object); the wall elsewhere carries from itself
    uncovered = (hist["inst"] == 0) & ~on
    assert uncovered.sum() > 0 and np.all(src[uncovered] == -1)
    rest = ~on & ~uncovered
    assert np.array_equal(src[rest], (ys * W + xs)[rest])
    # the carried values are the history's, from those pixels
    q = np.where(src >= 0, src, 0)
    assert np.array_equal(out[0][src >= 0].view(np.uint32), hs[0].reshape(-1, 4)[q][src >= 0].view(np.uint32)) and np.array_equal(out[1][src >= 0], hs[1].reshape(-1)[q][src >= 0])
    assert not out[0][src < 0].any() and not out[1][src < 0].any()
    non_vacuous(out)
    # plain rt_reproject on the same frames would keep the quad's overlap with its old place and nothing else of it
    plain = rr.reproject(cur, hist, *hs, CAMERA, MAT_TYPE, MAT_SHINY)[5]
    assert (plain[on] >= 0).sum() == (on & (hist["inst"] == 0)).sum() < on.sum()


def test_translation_out_of_the_frame_leaves_the_part_without_a_source_empty():
    T0, hx, hy = centred(2, 17, 7, 18)
    T1, _, _ = centred(-3, 12, 7, 18)          # 5 pixels to the left: columns -3 .. -1 have left the frame
    was, now = [quad(T0, hx, hy)], [quad(T1, hx, hy)]
    hist, cur = gbuffer(was), gbuffer(now)
    src = run(cur, hist, history(), now, was)[5]
    ys, xs = np.mgrid[0:H, 0:W]
    on = cur["inst"] == 0
    assert on.sum() == 13 * 12 and np.array_equal(src[on], (ys * W + xs + 5)[on])
    # and the other way: moved INTO the frame, the pixels whose source lies outside the history's frame start empty
    src = run(hist, cur, history(), was, now)[5]
    on = hist["inst"] == 0
    inside = on & (xs - 5 >= 0)
    assert np.array_equal(src[inside], (ys * W + xs - 5)[inside]) and np.all(src[on & ~inside] == -1) and (on & ~inside).sum() == 3 * 12


# ---- rotation ----------------------------------------------------------------------------------------------------------------------
def interior(cur, hist, now, was, k=0):
    """the pixels of instance k whose taken-back point (f64) lands at least one pixel inside the instance's history footprint"""
    cam, TL, TR, BL = np.asarray(CAMERA, np.float64)
    M = was[k]["T"].astype(np.float64) @ now[k]["invT"].astype(np.float64)
    x = cur["pos"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    d = x - cam
    lam = (TL[2] - cam[2]) / d[..., 2]
    P = cam + d * lam[..., None] - TL
    rx, ry = np.floor(P[..., 0] / (TR - TL)[0] * W + 0.5).astype(int), np.floor(P[..., 1] / (BL - TL)[1] * H + 0.5).astype(int)
    ok = (cur["inst"] == k) & (rx >= 1) & (rx < W - 1) & (ry >= 1) & (ry < H - 1)
    rx, ry = np.clip(rx, 1, W - 2), np.clip(ry, 1, H - 2)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok &= hist["inst"][ry + dy, rx + dx] == k
    return ok


def test_rotation_about_the_quads_normal_keeps_the_plane():
    T0, hx, hy = centred(12, 31, 6, 19)
    was, now = [quad(T0, hx, hy)], [quad(T0 @ rotate("z", 30), hx, hy)]
    hist, cur = gbuffer(was), gbuffer(now)
    out = run(cur, hist, history(), now, was)
    src = out[5]
    inner = interior(cur, hist, now, was)
    assert inner.sum() >= 100 and np.all(src[inner] >= 0)
    assert np.all(hist["inst"].reshape(-1)[src[(cur["inst"] == 0) & (src >= 0)]] == 0)
    # the corners the rotation swung over fresh wall, and the wall it left: rejected
    non_vacuous(out)
    # the normal did not change, so the wrong normal carries the same pixels: this axis cannot tell
    assert np.array_equal(run(cur, hist, history(), now, was, wrong_normal=True)[5], src)


@pytest.mark.parametrize("axis,deg", [("y", 30), ("x", -25)])
def test_rotation_about_another_axis_needs_the_normal_taken_back(axis, deg):
    T0, hx, hy = centred(12, 31, 6, 19)
    was, now = [quad(T0, hx, hy)], [quad(T0 @ rotate(axis, deg), hx, hy)]
    hist, cur = gbuffer(was), gbuffer(now)
    on = cur["inst"] == 0
    # the world normal turned by more than the default tolerance: |n_p - n'_q| = 2 sin(deg / 2) > 0.25
    assert np.all(np.sqrt(((cur["normal"][on] - F32([0, 0, -1])) ** 2).sum(-1)) > 0.25)
    out = run(cur, hist, history(), now, was)
    inner = interior(cur, hist, now, was)
    assert inner.sum() >= 100 and np.all(out[5][inner] >= 0)
    non_vacuous(out)
    wrong = run(cur, hist, history(), now, was, wrong_normal=True)[5]
    assert np.all(wrong[on] == -1)            # n_h = n_p: the default normal_tolerance rejects the whole instance
    assert np.array_equal(wrong[~on], out[5][~on])


# ---- wrong instance ----------------------------------------------------------------------------------------------------------------
def test_two_alike_instances_swapped_in_place_carry_nothing_between_them():
    Ta, hx, hy = centred(6, 17, 8, 17)
    Tb, _, _ = centred(28, 39, 8, 17)
    was, now = [quad(Ta, hx, hy), quad(Tb, hx, hy)], [quad(Tb, hx, hy), quad(Ta, hx, hy)]  # one BLAS, the same object and material ids
    hist, cur = gbuffer(was), gbuffer(now)
    for k in ("pos", "normal", "t", "obj", "mat"):   # the two frames show the same surfaces: only the instance index tells them apart
        assert np.array_equal(hist[k], cur[k])
    assert np.array_equal(cur["inst"] == 0, hist["inst"] == 1) and np.array_equal(cur["inst"] == 1, hist["inst"] == 0)
    hs = history()
    src = run(cur, hist, hs, now, was)[5]
    ys, xs = np.mgrid[0:H, 0:W]
    on = cur["inst"] >= 0
    assert np.all(src[on] >= 0) and np.array_equal(hist["inst"].reshape(-1)[src[on]], cur["inst"][on])  # each from its OWN old place ...
    assert np.array_equal(src[cur["inst"] == 0], (ys * W + xs - 22)[cur["inst"] == 0]) and np.array_equal(src[cur["inst"] == 1], (ys * W + xs + 22)[cur["inst"] == 1])
    assert np.array_equal(src[~on], (ys * W + xs)[~on])
    # ... and where only the index differs (the tables say nobody moved, the history saw the OTHER instance at the pixel) nothing is
    # carried, although object, material, normal and plane all agree: plain rt_reproject takes every one of those pixels
    src = run(cur, hist, hs, now, now)[5]
    assert np.all(src[on] == -1) and np.array_equal(src[~on], (ys * W + xs)[~on])
    assert np.all(rr.reproject(cur, hist, *hs, CAMERA, MAT_TYPE, MAT_SHINY)[5] == ys * W + xs)


# ---- singular inverse --------------------------------------------------------------------------------------------------------------
def test_all_zero_inverse_leaves_the_instance_empty_and_the_rest_untouched():
    Ta, hx, hy = centred(6, 17, 8, 17)
    Tb, _, _ = centred(28, 39, 8, 17)
    was = [quad(Ta, hx, hy), quad(Tb, hx, hy, obj=6)]
    now = [dict(was[0]), dict(was[1])]
    now[1]["invT"] = np.zeros((4, 4), F32)          # instance 1 'moved': its inverse is singular
    hist = gbuffer(was)
    cur = {k: a.copy() for k, a in hist.items()}
    hs = history()
    out = run(cur, hist, hs, now, was)
    base = run(cur, hist, hs, was, was)
    bad = cur["inst"] == 1
    assert bad.sum() == 120 and np.all(out[5][bad] == -1) and np.array_equal(out[5][~bad], base[5][~bad]) and np.all(base[5] >= 0)
    for a, b in zip(out[:4], base[:4]):
        assert np.isfinite(a).all() and not a[bad].any() and np.array_equal(a[~bad], b[~bad])
    # a NaN in the capture's transform does the same
    was2 = [dict(was[0]), dict(was[1])]
    was2[1]["T"] = np.full((4, 4), np.nan, F32)
    out = run(cur, hist, hs, was, was2)
    assert np.all(out[5][bad] == -1) and np.array_equal(out[5][~bad], base[5][~bad]) and all(np.isfinite(a).all() for a in out[:4])
