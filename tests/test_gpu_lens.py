"""The thin lens of path-mode camera samples on the device (rt_set_lens, rt_get_lens, rt_focus_at), through host_api: the rays against
tests/lens_ref.py bit for bit, the accumulator against the oracle's Sample on the restated rays on every pipeline, the composition with
split calls, row shards, lists, budget plans and the statistics bit for bit against rt_render, 'off' left as the parent's bits, the error
cases and what rt_set_lens leaves alone, rt_focus_at and Renderer::Tick, and the plane experiment tests/test_lens_cpu.py fixes on the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as fr  # noqa: E402
import lens_ref as lr  # noqa: E402
import support as sp  # noqa: E402
import test_filter_cpu as fc  # noqa: E402
import test_gpu_filter as gf  # noqa: E402
import test_lens_cpu as lc  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x12345678
RADIUS, FOCUS = 0.05, 3.0
KIND_NAMES = ["point", "box", "tent"]
PARITY_SIZES = [(24, 16), (65, 3)]
PARITY_KINDS = ["box", "point"]
FRAME0, NFRAMES = 5, 3
W, H = 40, 21


def _renderer(host_api, scenes, monkeypatch, name, env=None, w=24, h=16, **kw):
    return gf._renderer(host_api, scenes, monkeypatch, name, env, w, h, **kw)


def _lens(host_api, radius, focus):
    return C.byref(host_api.RtLens(radius, focus))


# ---- 1. rays ----------------------------------------------------------------------------------------------------------------
# one lane; a partial wave; a wave and a lane; a block less one; a ragged last block; a skewed camera
@pytest.mark.parametrize("size", lc.GPU_RAY_SIZES, ids=lambda s: "%dx%d" % s)
def test_sample_rays_equal_the_restatement(size, host_api, monkeypatch):
    w, h = size
    sp.clean_env(monkeypatch)
    r = host_api.HostRenderer(w, h)
    if size == (24, 16):
        r.set_camera(*fc.SKEWED)
    cam = r.camera()
    seed_base = lc.ray_seed_base(w, h)
    r.set_lens(RADIUS, FOCUS)
    assert r.lens() == (float(np.float32(RADIUS)), FOCUS)
    for name in KIND_NAMES:
        r.set_pixel_filter(fr.KINDS[name])
        for frame in lc.GPU_RAY_FRAMES:
            O, D = r.sample_rays(frame, seed_base)
            O_ref, D_ref = lr.rays(fr.KINDS[name], cam, w, h, frame, seed_base, RADIUS, FOCUS)
            assert sp.same(O, O_ref), (name, frame)
            assert sp.same(D, D_ref), (name, frame)
            assert not sp.same(D, fr.rays(fr.KINDS[name], cam, w, h, frame, seed_base)[1])
    # rows [y0, y1) are those rows of the frame
    if h > 1:
        O, D = r.sample_rays(lc.GPU_RAY_FRAMES[-1], seed_base, 1, h)
        assert sp.same(D, D_ref[w:]) and sp.same(O, O_ref[w:])
    # radius 0: the filter's rays
    r.set_lens(0.0, FOCUS)
    for name in KIND_NAMES:
        r.set_pixel_filter(fr.KINDS[name])
        O, D = r.sample_rays(7, seed_base)
        O_ref, D_ref = fr.rays(fr.KINDS[name], cam, w, h, 7, seed_base)
        assert sp.same(O, O_ref) and sp.same(D, D_ref), name
    r.close()


# ---- 2. parity with the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(oracle_api, scenes):
    """reference(name, size, kind): filter_ref.accumulate of the parity frames on the restated lens rays, computed once per (scene, size,
    kind) and left unchanged; the oracle's scenes and renderers are closed when the module is done"""
    oracles, refs = {}, {}

    def reference(name, size, kind):
        key = (name, size, kind)
        if key not in refs:
            if name not in oracles:
                o = oracle_api.OracleScene()
                gf._scene_fn(scenes, name)(o)
                o.set_raytracer(False)
                oracles[name] = o
            if (name, size) not in oracles:
                oracles[(name, size)] = oracle_api.OracleRenderer(oracles[name], *size)
            orr = oracles[(name, size)]
            refs[key] = fr.accumulate(orr, kind, orr.camera(), FRAME0, NFRAMES, SEED, ray_fn=lr.ray_fn(RADIUS, FOCUS))
            refs[key].setflags(write=False)
        return refs[key]

    yield reference
    for key in sorted(oracles, key=lambda k: not isinstance(k, tuple)):  # renderers before their scenes
        oracles[key].close()


def _check_parity(host_api, references, scenes, monkeypatch, name, env):
    from conftest import rel_err
    for size in PARITY_SIZES:
        r = _renderer(host_api, scenes, monkeypatch, name, env, *size)
        r.set_lens(RADIUS, FOCUS)
        for kname in PARITY_KINDS:
            kind = fr.KINDS[kname]
            ref = references(name, size, kind)
            r.set_pixel_filter(kind)
            r.clear()
            r.render(host_api.RT_MODE_PATH, FRAME0, NFRAMES, SEED)
            got = r.accumulator()[..., :3]
            err, cls_ok = rel_err(got, ref)
            print("%s %s %dx%d %s + lens: max rel err %.3g" % (name, sp.env_id(env), size[0], size[1], kname, err.max()))
            assert cls_ok, (size, kname)
            assert err.max() <= 1e-4, (size, kname, err.max())
        r.close()


@pytest.mark.parametrize("env", gf.PIPELINES, ids=sp.env_id)
@pytest.mark.parametrize("name", ["scene3", "tlas_test2", "mixed_small"])
def test_accumulator_equals_the_oracle_on_the_restated_rays(name, env, scenes, host_api, references, monkeypatch):
    _check_parity(host_api, references, scenes, monkeypatch, name, env)


def test_accumulator_equals_the_oracle_in_the_general_kernel(scenes, host_api, references, monkeypatch):
    """a shiny diffuse floor: path mode runs k_sample_general"""
    _check_parity(host_api, references, scenes, monkeypatch, "shiny", {})


# ---- 3. schedules -------------------------------------------------------------------------------------------------------------
def test_schedules_are_bit_equal_under_box_and_lens(scenes, host_api, monkeypatch):
    first = None
    for env in gf.SCHEDULES:
        r = _renderer(host_api, scenes, monkeypatch, "tlas_test2", env, 65, 3)
        r.set_pixel_filter(host_api.RT_FILTER_BOX)
        r.set_lens(RADIUS, FOCUS)
        r.render(host_api.RT_MODE_PATH, FRAME0, NFRAMES, SEED)
        acc = r.accumulator()
        r.close()
        if first is None:
            first = acc
        assert sp.same(acc, first), env


# ---- 4. composition -----------------------------------------------------------------------------------------------------------
def test_split_calls_rows_lists_and_plans_equal_render(scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    F = 3
    a = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    b = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    for r in (a, b):
        r.set_pixel_filter(host_api.RT_FILTER_BOX)
        r.set_lens(RADIUS, FOCUS)
        r.stats_enable(True)
    # the states after F .. F + 11 frames, one frame at a time
    stack = [sp.state(a)]
    for n in range(12):
        a.render(PATH, F + n, 1, SEED)
        stack.append(sp.state(a))
    # four frames in one call, and as two calls of split frames
    for split in ((4,), (1, 3)):
        b.clear()
        f = F
        for n in split:
            b.render(PATH, f, n, SEED)
            f += n
        assert sp.same_state(sp.state(b), stack[4]), split
        assert np.all(b.stats()[0] == 4)
    # two row shards
    b.clear()
    for k in range(2):
        b.render_rows(PATH, F, 4, k, 2, (H - k + 1) // 2, SEED)
    assert sp.same_state(sp.state(b), stack[4])
    # a seeded list with the frame's corners and both edge columns: the listed pixels take frames F + 4 .. F + 6, the rest is unwritten
    lst = gf._seeded_list(W, H)
    on = np.zeros(W * H, bool)
    on[lst] = True
    on = on.reshape(H, W)
    assert on[0, 0] and on[0, -1] and on[-1, 0] and on[-1, -1] and on[:, 0].all() and on[:, -1].all() and not on.all()
    b.set_active(lst)
    b.render_active(F + 4, 3, SEED)
    for x, y7, y4 in zip(sp.state(b), stack[7], stack[4]):
        assert sp.same(x[on], y7[on]) and sp.same(x[~on], y4[~on])
    # a budgeted pass after 2 whole frames: a pixel with count n holds the state after n frames from F
    b.clear()
    b.render(PATH, F, 2, SEED)
    na, total, cap = b.select_budget(dict(select=dict(min_samples=2, max_samples=12, threshold=0.02, floor=1e-3), pass_cap=5))
    assert 0 < na < W * H and total > na  # some pixels are quiet after two frames and stay at 2, the noisy ones get up to 5 more
    b.render_budget(F, SEED)
    got = sp.state(b)
    cnt = got[1]
    assert cnt.min() >= 2 and cnt.max() <= 12 and len(np.unique(cnt)) >= 2
    assert sp.differs_from_snapshot_of_its_count(got, stack) is None
    a.close()
    b.close()


# ---- 5. off means off ---------------------------------------------------------------------------------------------------------
def test_a_lens_switched_off_leaves_the_filter_s_bits(scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    never = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    never.set_pixel_filter(host_api.RT_FILTER_BOX)
    never.render(PATH, 0, 3, SEED)
    want = never.accumulator()
    never.close()
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    r.set_lens(RADIUS, FOCUS)
    r.render(PATH, 0, 3, SEED)
    assert not sp.same(r.accumulator(), want)
    r.set_lens(0.0, FOCUS)
    r.clear()
    r.render(PATH, 0, 3, SEED)
    assert sp.same(r.accumulator(), want)
    r.set_lens(RADIUS, FOCUS)
    assert r.rt.rt_set_lens(r.ctx, None) == 0
    assert r.lens()[0] == 0.0
    r.clear()
    r.render(PATH, 0, 3, SEED)
    assert sp.same(r.accumulator(), want)
    r.close()


@pytest.mark.parametrize("env", [{"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}, {"RT_PRIMARY_TABLE": "0"}], ids=sp.env_id)
def test_reference_mode_after_a_lens_is_the_parent_s(env, scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    a = _renderer(host_api, scenes, monkeypatch, "mixed_small", env, W, H)
    b = _renderer(host_api, scenes, monkeypatch, "mixed_small", env, W, H)
    a.set_pixel_filter(host_api.RT_FILTER_BOX)
    a.set_lens(RADIUS, FOCUS)
    a.render(PATH, 0, 3, SEED)
    lensed = a.accumulator()
    a.clear()
    a.set_lens(0.0, FOCUS)
    a.set_pixel_filter(host_api.RT_FILTER_REFERENCE)
    for r in (a, b):
        r.render(PATH, 0, 3, SEED)
    assert sp.same(a.accumulator(), b.accumulator())
    assert not sp.same(lensed, b.accumulator())
    # the rays of reference mode: the truncated jitter lands on the integer pixels [x - 1, x] x [y - 1, y]
    O, D = a.sample_rays(0, SEED)
    a.set_pixel_filter(host_api.RT_FILTER_POINT)
    _, P = a.sample_rays(0, SEED)
    P, inner = P.reshape(H, W, 3), D.reshape(H, W, 3)[1:, 1:]
    cands = [P[1 - dy:H - dy, 1 - dx:W - dx] for dy in (0, 1) for dx in (0, 1)]
    assert np.all(np.any([np.all(sp.bits(inner) == sp.bits(c), axis=-1) for c in cands], axis=0))
    a.close()
    b.close()


# ---- 6. errors and state ------------------------------------------------------------------------------------------------------
def test_set_lens_arguments(host_api, monkeypatch):
    sp.clean_env(monkeypatch)
    r = host_api.HostRenderer(8, 5)
    L, ARG = r.rt, host_api.RT_E_ARG
    assert r.lens() == (0.0, 1.0)  # a context's default: off
    r.set_lens(0.25, 2.5)
    for radius, focus in ((-0.1, 3.0), (np.nan, 3.0), (np.inf, 3.0), (-np.inf, 3.0), (0.05, 0.0), (0.05, -1.0), (0.05, np.nan), (0.05, np.inf)):
        assert L.rt_set_lens(r.ctx, _lens(host_api, radius, focus)) == ARG, (radius, focus)
        assert r.lens() == (0.25, 2.5)
        with pytest.raises(RuntimeError):
            r.set_lens(radius, focus)
        assert r.lens() == (0.25, 2.5)
    assert L.rt_set_lens(None, _lens(host_api, 0.05, 3.0)) == ARG
    assert L.rt_get_lens(r.ctx, None) == ARG and L.rt_get_lens(None, _lens(host_api, 0, 0)) == ARG
    assert L.rt_set_lens(r.ctx, _lens(host_api, 0.0, -7.0)) == 0  # with the lens off the focus distance is not looked at
    assert r.lens()[0] == 0.0
    r.close()


def test_unsupported_combinations_leave_the_accumulator(scenes, host_api, monkeypatch):
    PATH, UNSUP = host_api.RT_MODE_PATH, host_api.RT_E_UNSUPPORTED
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    L = r.rt
    buf = np.zeros((W * H, 3), np.float32)
    p = buf.ctypes.data_as(C.c_void_p)

    def refused(what):
        before = sp.state(r)
        assert L.rt_render(r.ctx, PATH, 2, 1, SEED, 0, H, 4) == UNSUP, what
        assert b"lens" in L.rt_last_error(r.ctx)
        assert L.rt_render_rows(r.ctx, PATH, 2, 1, SEED, 0, 2, H // 2, 4) == UNSUP, what
        assert L.rt_render_active(r.ctx, 2, 1, SEED, 4) == UNSUP, what
        assert L.rt_render_budget(r.ctx, 0, SEED, 4) == UNSUP, what
        assert L.rt_sample_rays(r.ctx, 0, SEED, 0, H, p, p) == UNSUP, what
        assert sp.same_state(sp.state(r), before), what

    r.stats_enable(True)
    r.render(PATH, 0, 2, SEED)
    r.set_active([0, 5, W * H - 1])
    na, total, _ = r.select_budget(dict(select=dict(min_samples=4, max_samples=8, threshold=0.02, floor=1e-3), pass_cap=3))
    assert na > 0
    # the reference's jitter with a lens
    r.set_lens(RADIUS, FOCUS)
    refused("reference")
    assert b"rt_set_pixel_filter" in L.rt_last_error(r.ctx)
    # ... and the next valid calls work: the plan and the list are still there
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    r.render_budget(0, SEED)
    r.set_active([0, 5, W * H - 1])
    r.render_active(9, 1, SEED)
    r.render(PATH, 10, 1, SEED)
    r.sample_rays(0, SEED)
    # a fisheye camera with a lens (POINT: the kind a fisheye camera renders)
    cam = r.camera()
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    r.set_camera(*cam, fisheye=True, view_angle=0.3)
    r.select_budget(dict(select=dict(min_samples=4, max_samples=40, threshold=0.0, floor=1e-3), pass_cap=3))
    refused("fisheye")
    assert L.rt_render(r.ctx, host_api.RT_MODE_WHITTED, 0, 1, SEED, 0, H, 4) == 0  # Whitted mode ignores the lens
    r.set_lens(0.0, FOCUS)
    r.render(PATH, 11, 1, SEED)
    # a degenerate screen rectangle: the camera lies in the screen's plane, lam is not finite
    r.set_lens(RADIUS, FOCUS)
    r.set_camera(cam[1], cam[1], cam[2], cam[3])
    r.select_budget(dict(select=dict(min_samples=4, max_samples=40, threshold=0.0, floor=1e-3), pass_cap=3))
    refused("degenerate")
    r.close()


def test_set_lens_keeps_the_g_buffer_the_history_and_the_other_modes(scenes, host_api, monkeypatch):
    PATH, WHITTED = host_api.RT_MODE_PATH, host_api.RT_MODE_WHITTED
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    # Whitted frames and rt_trace_batch with the lens off ...
    O1, D1 = np.float32([[0, 1, -2]] * 4), np.float32([[0, 0, 1], [0.1, 0, 1], [0, -0.3, 1], [0.3, 0.2, 1]])
    r.render(WHITTED, 0, 1, SEED)
    whitted, traced = r.accumulator(), (r.trace_batch(PATH, O1, D1), r.trace_batch(WHITTED, O1, D1))
    aov_t, hits = None, r.primary_hits(0.001)
    # the accumulator, the G-buffer and a captured history outlive rt_set_lens
    r.clear()
    r.stats_enable(True)
    r.render(PATH, 0, 3, SEED)
    r.render_aovs(0.001)
    aov_t = r.aovs()["t"]
    r.history_capture()
    before = sp.state(r)
    r.set_profiling(True)
    r.profile()
    r.set_lens(RADIUS, FOCUS)
    assert sp.same_state(sp.state(r), before)
    r.render_aovs(0.001)  # current: returns without a launch
    assert r.profile()["query"]["launches"] == 0
    r.set_profiling(False)
    assert sp.same(r.aovs()["t"], aov_t)
    h2 = r.primary_hits(0.001)
    assert np.array_equal(h2[0], hits[0]) and sp.same(h2[1], hits[1])
    cam = r.camera()
    r.set_camera(*(cam + np.float32([0.05, 0, 0])))
    r.render_aovs(0.001)
    assert r.reproject() > 0
    r.set_camera(*cam)
    # ... and with it on
    r.stats_enable(False)
    r.render(WHITTED, 0, 1, SEED)
    assert sp.same(r.accumulator(), whitted)
    assert sp.same(r.trace_batch(PATH, O1, D1), traced[0]) and sp.same(r.trace_batch(WHITTED, O1, D1), traced[1])
    r.close()


# ---- 7. rt_focus_at and Tick ----------------------------------------------------------------------------------------------------
def test_focus_at_equals_the_restatement(scenes, host_api, monkeypatch):
    w, h = 24, 16
    r = _renderer(host_api, scenes, monkeypatch, "tlas_test2", None, w, h)
    cam = r.camera()
    r.render_aovs(0.001)
    a = r.aovs()
    t, obj = a["t"].reshape(-1), a["obj"].reshape(-1)
    _, D = fr.rays(fr.POINT, cam, w, h, 0, SEED)
    want = lr.focus_distance(cam, t, D)
    hit = np.flatnonzero(obj >= 0)
    assert len(hit) >= 5
    r.set_profiling(True)
    r.profile()
    for p in hit[np.linspace(0, len(hit) - 1, 5).astype(int)]:
        got = r.focus_at(int(p % w), int(p // w))
        assert got > 0 and sp.same(np.float32([got]), want[p:p + 1]), (p, got, want[p])
    assert r.profile()["query"]["launches"] == 5  # one query each
    r.set_profiling(False)
    for p in np.flatnonzero(obj < 0)[:2]:
        assert sp.same(np.float32([r.focus_at(int(p % w), int(p // w))]), np.float32([0.0]))
    assert r.lens()[0] == 0.0  # it sets nothing
    # errors
    L, d = r.rt, C.c_float(-1.0)
    for x, y in ((-1, 0), (w, 0), (0, -1), (0, h)):
        assert L.rt_focus_at(r.ctx, x, y, C.byref(d)) == host_api.RT_E_ARG
    assert L.rt_focus_at(r.ctx, 0, 0, None) == host_api.RT_E_ARG and L.rt_focus_at(None, 0, 0, C.byref(d)) == host_api.RT_E_ARG
    r.set_camera(*cam, fisheye=True, view_angle=0.3)
    assert L.rt_focus_at(r.ctx, 0, 0, C.byref(d)) == host_api.RT_E_UNSUPPORTED
    assert d.value == -1.0
    r.close()


def test_focus_at_the_sky_and_without_a_scene(host_api, monkeypatch):
    w, h = 8, 5
    r = sp.renderer(host_api, monkeypatch, fc._tiny_scene, w, h, scene_camera=False)  # everything of the scene is behind the camera
    for x, y in ((0, 0), (w // 2, h // 2), (w - 1, h - 1)):
        assert sp.same(np.float32([r.focus_at(x, y)]), np.float32([0.0]))
    r.close()
    sp.clean_env(monkeypatch)
    r = host_api.HostRenderer(w, h)
    d = C.c_float(-1.0)
    assert r.rt.rt_focus_at(r.ctx, 0, 0, C.byref(d)) == host_api.RT_E_STATE
    r.close()


def test_tick_clears_on_a_change_of_lens_only(scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    t = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H, path_ticks=True)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    for r in (t, hand):
        r.set_pixel_filter(host_api.RT_FILTER_BOX)
    for _ in range(2):
        t.tick()  # path frames 0, 1 under BOX, no lens
    t.set_lens(RADIUS, FOCUS)
    t.tick()  # frame 2 alone, under the lens
    hand.set_lens(RADIUS, FOCUS)
    hand.render(PATH, 2, 1, SEED)
    assert sp.same(t.tick_accumulator(), hand.accumulator())
    t.set_lens(RADIUS, FOCUS)  # the same lens again: no clear
    t.tick()  # ... frame 3 on top
    hand.render(PATH, 3, 1, SEED)
    assert sp.same(t.tick_accumulator(), hand.accumulator())
    t.set_lens(RADIUS, 2.0)  # another focus distance: frame 4 alone
    t.tick()
    hand.set_lens(RADIUS, 2.0)
    hand.clear()
    hand.render(PATH, 4, 1, SEED)
    assert sp.same(t.tick_accumulator(), hand.accumulator())
    t.close()
    hand.close()


# ---- 8. the plane experiment on the device -----------------------------------------------------------------------------------------
def test_a_point_on_the_focal_plane_is_sharp_and_one_behind_it_is_spread(host_api, monkeypatch):
    w, h = lc.PW, lc.PH
    hits = {}
    for depth in (FOCUS, 2 * FOCUS):
        r = sp.renderer(host_api, monkeypatch, lc.plane_scene(depth), w, h, scene_camera=False)
        cam = r.camera()
        r.set_pixel_filter(host_api.RT_FILTER_POINT)
        nearest = lambda O, D: r.find_nearest(O, D, t_min=0.001)["t"]  # noqa: E731  (rt_intersect_batch)
        if depth != FOCUS:
            hits["pinhole"] = lc.hit_points(nearest, fr.POINT, cam, w, h, 1, 0, 0, rays_fn=lambda f: r.sample_rays(f, SEED))[0]
        r.set_lens(RADIUS, FOCUS)
        hits[depth] = lc.hit_points(nearest, fr.POINT, cam, w, h, lc.FRAMES, RADIUS, FOCUS, rays_fn=lambda f: r.sample_rays(f, SEED))
        r.close()
    lc.check_spread(hits[FOCUS], hits[2 * FOCUS], hits["pinhole"])
