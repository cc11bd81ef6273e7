"""Reprojection on the device, through host_api: k_reproject against its numpy restatement (tests/reproject_ref.py) bit for bit, the unmoved
camera, idempotence, what the call leaves alone, rt_render_active after it, the error and invalidation cases, Renderer::Tick's
reprojecting mode against the same sequence driven by hand, and what the carried samples are worth (the experiment
tests/test_reproject_cpu.py fixes on the oracle)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import reproject_ref as rr  # noqa: E402
import support as sp  # noqa: E402
from test_reproject_cpu import QUALITY, mse_ratio  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
ADAPTIVE, MOVES, PARAMS = rr.ADAPTIVE, rr.MOVES, rr.PARAMS
# 1 x 1: the frame's one ray is the top left corner's; this camera points it at the floor beside the meshes
ONE_PIXEL_CAMERA = np.array([(0, 1, -2), (2, 0.2, 0), (3, 0.2, 0), (2, -0.8, 0)], F32)


def _renderer(host_api, scenes, monkeypatch, name, w, h, camera=None):
    return sp.renderer(host_api, monkeypatch, getattr(scenes, name), w, h, camera=camera)


def _gbuffer(r):
    """the current G-buffer as the device holds it"""
    a = r.aovs()
    return dict(pos=r.aov_positions(), normal=a["normal"], t=a["t"], obj=a["obj"], mat=a["mat"])


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("mixed_small", (64, 40)), ("mixed_small", (33, 9)), ("mixed_small", (97, 41)), ("pretty_tlas", (320, 180)), ("mixed_small", (1, 1))],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_kernel_equals_the_restatement(name, size, scenes, host_api, monkeypatch):
    """Every move x history x parameter set of one frame size on one context: accumulator, count, both sums and n_carried bit for bit against
    the restatement, which is fed the device's own downloads taken before the move and the current G-buffer.  So that no case is vacuous:
    for the two real moves the restatement carries >= 10 % of the frame and rejects >= 1 % of the eligible pixels (with the tolerances of
    the defaults; a frame of one pixel can do neither, it is held to carrying its pixel with the camera unmoved instead)."""
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, name, w, h, ONE_PIXEL_CAMERA if size == (1, 1) else None)
    A = r.camera()
    mt, ms = rr.materials(r)
    r.stats_enable(True)
    for kind in ("uniform", "adaptive", "list"):
        r.set_camera(*A)
        rr.make_history(r, host_api, kind, w, h)
        r.render_aovs(0.001)
        g_a, hist = _gbuffer(r), sp.state(r)
        cnt_a = hist[1]
        if kind == "adaptive" and w * h > 1:
            assert len(np.unique(cnt_a)) > 1, "the adaptive history has even counts"
        if kind == "list":
            assert (cnt_a == 0).any() or w * h == 1
        if kind == "uniform":
            assert np.all(cnt_a == 12)  # above max_history = 8: the capped case scales every carried pixel
        r.history_capture()
        for move_name, move in MOVES.items():
            B = rr.moved(A, move)
            r.set_camera(*B)
            r.render_aovs(0.001)
            g_b = _gbuffer(r)
            if move_name == "behind" and w * h > 1:
                lam = rr.depth_ratio(g_b["pos"], A)
                assert ((g_b["obj"] != -1) & ~(lam > 0)).any(), "nothing the new camera sees lies behind the old one"
            for pname, P in PARAMS.items():
                n = r.reproject(P)
                got = sp.state(r)
                acc, cnt, sy, syy, n_ref, src, el = rr.reproject(g_b, g_a, *hist, A, mt, ms, **P)
                what = (kind, move_name, pname)
                assert n == n_ref, what
                assert np.array_equal(got[1], cnt), what
                assert sp.same(got[0], acc) and sp.same(got[2], sy) and sp.same(got[3], syy), what
                carried, rejected = n_ref / (w * h), (el.sum() - n_ref) / max(1, el.sum())
                if move_name in ("small", "large") and pname != "exact" and w * h > 1:
                    assert carried >= 0.10 and rejected >= 0.01, (what, carried, rejected)
                if move_name == "none" and pname == "defaults":
                    # the unmoved camera: every eligible pixel keeps its own bits, everything else is zero
                    keep = el & (cnt_a > 0)
                    assert np.array_equal(src >= 0, keep), what
                    assert np.array_equal(src[keep], np.arange(w * h).reshape(h, w)[keep]), what
                    for g, b in zip(got, hist):
                        assert sp.same(g[keep], b[keep]) and not sp.bits(g[~keep]).any(), what
                    if kind == "uniform":
                        assert keep.any(), "nothing is eligible"
    r.close()


# ---- 2. idempotence, and what the call leaves alone ----------------------------------------------------------------------------
def test_reproject_twice_and_untouched_state(scenes, host_api, monkeypatch):
    w, h = 97, 41
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    A = r.camera()
    r.stats_enable(True)
    rr.make_history(r, host_api, "adaptive", w, h)
    r.render_aovs(0.001)
    r.history_capture()
    lst = np.flatnonzero(rr.list_mask(w, h, seed=9)).astype(np.uint32)
    r.set_active(lst)
    r.set_camera(*rr.moved(A, MOVES["large"]))
    r.render_aovs(0.001)
    g_b = _gbuffer(r)
    n1 = r.reproject()
    first = sp.state(r)
    n2 = r.reproject()
    assert n1 == n2 > 0 and sp.same_state(first, sp.state(r))
    # the history is the capture's, whatever has happened to the accumulator since
    r.clear()
    assert r.reproject() == n1 and sp.same_state(first, sp.state(r))
    r.render(host_api.RT_MODE_PATH, 50, 2)
    assert r.reproject(None) == n1 and sp.same_state(first, sp.state(r))
    # NULL parameters are the defaults, a NULL count is allowed
    assert r.reproject(dict(host_api.REPROJECT_DEFAULTS)) == n1 and sp.same_state(first, sp.state(r))
    assert r.rt.rt_reproject(r.ctx, None, None) == 0 and sp.same_state(first, sp.state(r))
    # the active-pixel list and the G-buffer are not touched
    got, k = r.active()
    assert k == len(lst) and np.array_equal(got, lst)
    after = _gbuffer(r)
    assert all(sp.same(g_b[key], after[key]) for key in g_b)
    # rt_clear and rt_set_camera leave the history alone: back at the old camera every eligible pixel is carried from itself
    r.clear()
    r.set_camera(*A)
    r.render_aovs(0.001)
    assert r.reproject() > n1
    r.close()


# ---- 3. rt_render_active after a reproject ---------------------------------------------------------------------------------------
def test_select_and_render_active_after_a_reproject(scenes, host_api, monkeypatch):
    w, h = 97, 41
    pair = [_renderer(host_api, scenes, monkeypatch, "mixed_small", w, h) for _ in range(2)]
    A = pair[0].camera()
    lists, states = [], []
    for r in pair:
        r.stats_enable(True)
        rr.make_history(r, host_api, "adaptive", w, h)
        r.render_aovs(0.001)
        r.history_capture()
        r.set_camera(*rr.moved(A, MOVES["small"]))
        r.render_aovs(0.001)
        r.reproject()
        cnt, sy, syy = r.stats()
        n = r.select_active(ADAPTIVE)
        lst, k = r.active()
        assert k == n and np.array_equal(lst, ar.active_list(cnt, sy, syy, **ADAPTIVE))
        assert np.isin(np.flatnonzero(cnt.reshape(-1) < ADAPTIVE["min_samples"]), lst).all()  # every pixel that starts empty is sampled
        assert (cnt == 0).any() and 0 < n < w * h
        r.render_active(20, 2)
        after = r.stats()[0]
        on = np.zeros(w * h, bool)
        on[lst] = True
        assert np.array_equal(after.reshape(-1), cnt.reshape(-1) + 2 * on)
        lists.append(lst)
        states.append(sp.state(r))
    assert np.array_equal(lists[0], lists[1]) and sp.same_state(states[0], states[1])
    for r in pair:
        r.close()


# ---- 4. errors and invalidation -----------------------------------------------------------------------------------------------
def test_errors_and_invalidation(scenes, host_api, monkeypatch):
    w, h = 64, 40
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    L, ctx = r.rt, r.ctx
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    A = r.camera()
    n = C.c_int(-7)
    xyz = np.zeros((h, w, 3), F32)
    pxyz = xyz.ctypes.data_as(C.c_void_p)

    def rep(context=ctx, **kw):
        p = host_api.reproject_params(kw)
        return L.rt_reproject(context, C.byref(p), C.byref(n))

    def why():
        return L.rt_last_error(ctx).decode()

    # parameters: refused before the context is looked at
    for bad in (dict(normal_tolerance=-0.1), dict(normal_tolerance=float("nan")), dict(plane_tolerance=-1e-9), dict(plane_tolerance=float("nan")), dict(max_history=-1)):
        assert rep(**bad) == ARG and rep(None, **bad) == ARG, bad
    assert rep(None) == ARG and L.rt_history_capture(None) == ARG
    # the position download: rt_download_aovs's errors
    assert L.rt_download_aov_positions(ctx, 0, h, pxyz) == STATE
    assert L.rt_download_aov_positions(None, 0, h, pxyz) == ARG
    # statistics off
    r.render_aovs(0.001)
    assert L.rt_history_capture(ctx) == STATE and "statistics" in why()
    assert rep() == STATE and "statistics" in why()
    for y0, y1 in ((-1, h), (0, h + 1), (3, 3), (5, 2)):
        assert L.rt_download_aov_positions(ctx, y0, y1, pxyz) == ARG
    assert L.rt_download_aov_positions(ctx, 0, h, None) == ARG
    assert sp.same(r.aov_positions(3, 9), r.aov_positions()[3:9])
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 3)
    # no history yet
    assert rep() == STATE and "history" in why()
    # a stale G-buffer (the camera changed since rt_render_aovs): no capture
    r.set_camera(*rr.moved(A, MOVES["small"]))
    assert L.rt_history_capture(ctx) == STATE and "G-buffer" in why()
    r.set_camera(*A)
    r.render_aovs(0.001)
    r.history_capture()
    # ... and no reproject
    r.set_camera(*rr.moved(A, MOVES["small"]))
    assert rep() == STATE and "G-buffer" in why()
    r.render_aovs(0.001)
    assert rep() == 0 and n.value > 0
    # a fisheye on either side
    r.set_camera(*A, fisheye=True)
    r.render_aovs(0.001)
    assert rep() == UNSUP and L.rt_history_capture(ctx) == UNSUP
    r.set_camera(*A)
    r.render_aovs(0.001)
    assert rep() == 0  # the history taken before is still valid

    def recapture():
        r.set_camera(*A)
        r.render_aovs(0.001)
        r.history_capture()
        assert rep() == 0

    # what changes the surfaces drops the history: rt_set_time, rt_upload_scene; and rt_stats_enable(0), even when switched on again
    for drop in (lambda: r.set_time(0.5), r.commit, lambda: (r.stats_enable(False), r.stats_enable(True))):
        recapture()
        drop()
        r.render_aovs(0.001)
        assert rep() == STATE and "history" in why()
    # rt_clear and rt_set_camera do not
    recapture()
    r.clear()
    r.set_camera(*rr.moved(A, MOVES["large"]))
    r.render_aovs(0.001)
    assert rep() == 0
    r.close()


# ---- 5. Renderer::Tick -----------------------------------------------------------------------------------------------------------
def _set_camera_unsynced(r, cam):
    """the camera as an application moves it: Renderer::camera changes, the contexts learn of it in the next Tick (HostRenderer.set_camera
    syncs at once)"""
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    r.L.rth_renderer_set_camera(r.h, f3(cam[0]), f3(cam[1]), f3(cam[2]), f3(cam[3]), 0, C.c_float(0.25), C.c_float(0.0))


def test_tick_reproject_equals_the_sequence_by_hand(scenes, host_api, monkeypatch):
    w, h = 96, 64
    RP = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=16, carry_view_dependent=0)
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    r.set_adaptive(True, ADAPTIVE)
    r.set_reproject(True, RP)
    off = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)  # the flag set and cleared again: today's adaptive Tick
    off.set_adaptive(True, ADAPTIVE)
    off.set_reproject(True, RP)
    off.set_reproject(False)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    plain = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    A = r.camera()
    for x in (hand, plain):
        x.set_camera(*A)
        x.stats_enable(True)
        x.clear()
    whole = {id(hand): 0, id(plain): 0}

    def step(x, t):
        if whole[id(x)] < ADAPTIVE["min_samples"]:
            x.render(PATH, t, 1)
            whole[id(x)] += 1
            return w * h
        k = x.select_active(ADAPTIVE)
        x.render_active(t, 1)
        return k

    moves = {2: MOVES["small"], 8: MOVES["large"], 9: MOVES["small"]}  # before min_samples whole frames, after them, and on the very next tick
    # the move of tick 8 reaches the context in the Tick itself (the old camera is still the context's); the other two were synced by the
    # caller before the Tick, which then puts the camera of the samples back for the capture
    unsynced = {8}
    cam = A
    carried = []
    for t in range(13):
        if t in moves:
            cam = rr.moved(cam, moves[t])
            if t in unsynced:
                _set_camera_unsynced(r, cam)
            else:
                r.set_camera(*cam)
            off.set_camera(*cam)
            hand.render_aovs(0.001)
            hand.history_capture()
            hand.set_camera(*cam)
            hand.render_aovs(0.001)
            carried.append(hand.reproject(RP))
            whole[id(hand)] = ADAPTIVE["min_samples"]
            plain.set_camera(*cam)
            plain.clear()
            whole[id(plain)] = 0
        r.tick()
        off.tick()
        n, m = step(hand, t), step(plain, t)
        assert r.active_pixels() == n and off.active_pixels() == m, t
        if t in moves:
            assert r.carried_pixels() == carried[-1] > 0, t
            assert np.all(off.stats()[0] == 1), t
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
        assert sp.same(off.tick_accumulator(), plain.accumulator()) and sp.same_state(sp.state(off), sp.state(plain)), t
        assert np.array_equal(off.tick_pixels(), plain.resolve_adaptive()), t
    assert len(carried) == 3
    # a fisheye on either side of the move: the Tick clears as ever
    r.set_camera(*cam, fisheye=True)
    r.tick()
    assert np.all(r.stats()[0] == 1)
    r.set_camera(*cam)
    r.tick()
    assert np.all(r.stats()[0] == 1)
    # a Whitted Tick in between has overwritten the accumulator under its own camera: the next path Tick with a moved camera clears
    r.tick()
    assert np.all(r.stats()[0] == 2)
    r.scene.set_raytracer(True)
    r.tick()
    r.scene.set_raytracer(False)
    r.set_camera(*rr.moved(cam, MOVES["small"]))
    r.tick()
    assert np.all(r.stats()[0] == 1) and r.active_pixels() == w * h
    # reproject without adaptive: refused, naming the limit
    r.set_adaptive(False)
    with pytest.raises(RuntimeError, match="reproject"):
        r.tick()
    r.set_reproject(False)
    r.tick()
    for x in (r, off, hand, plain):
        x.close()


# ---- 6. quality --------------------------------------------------------------------------------------------------------------------
def test_carried_samples_beat_fresh_ones(scenes, host_api, monkeypatch):
    """The experiment of tests/test_reproject_cpu.py (scene, size, moves, frame counts) on the device, against the device's own 256-frame
    mean at the new camera.  Asserted: MSE ratio carried / fresh < 0.25 for both moves (the oracle's figures are 0.126 and 0.138).
    Measured on an MI355X: see DESIGN.md, the reprojection section."""
    q = QUALITY
    w, h = q["width"], q["height"]
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, q["scene"], w, h)
    A = r.camera()
    r.stats_enable(True)
    r.clear()
    r.render(PATH, 0, q["history_frames"])
    r.render_aovs(0.001)
    r.history_capture()
    ratios = []
    for move in q["moves"]:
        r.set_camera(*rr.moved(A, move))
        r.render_aovs(0.001)
        n = r.reproject()
        acc, cnt = r.accumulator(), r.stats()[0]
        assert n == int((cnt > 0).sum()) and set(np.unique(cnt)) <= {0, q["history_frames"]}
        r.clear()
        r.render(PATH, q["fresh_frame0"], q["fresh_frames"])
        fresh = r.accumulator()[..., :3].astype(np.float64) / q["fresh_frames"]
        r.clear()
        r.render(PATH, q["reference_frame0"], q["reference_frames"])
        ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
        with np.errstate(all="ignore"):
            mean = acc[..., :3].astype(np.float64) / cnt[..., None]
        ratio, compared = mse_ratio(mean, fresh, ref, cnt > 0)
        print("device move %s: MSE ratio carried / fresh %.3f on %d pixels, %.1f %% of the frame carried" % (move, ratio, compared, 100.0 * n / (w * h)))
        assert n >= 0.1 * w * h
        ratios.append(ratio)
    r.close()
    assert all(x < q["bar"] for x in ratios), ratios
