"""The pixel filter of path-mode camera samples on the device (rt_set_pixel_filter, rt_sample_rays), through host_api: the rays against
tests/filter_ref.py bit for bit, the accumulator against the oracle's Sample on the restated rays on every pipeline, the composition with
row shards, lists, budget plans, statistics and Renderer::Tick bit for bit against rt_render, the reference mode left untouched, the error
cases, and the quality experiment tests/test_filter_cpu.py fixes on the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_shapes as tc  # noqa: E402
import filter_ref as fr  # noqa: E402
import support as sp  # noqa: E402
import test_filter_cpu as fc  # noqa: E402
from test_filter_cpu import quality  # noqa: E402,F401  (the module-scoped fixture of the quality experiment)

pytestmark = pytest.mark.gpu

# the schedules the existing tests hold bit-equal in reference mode (tests/test_gpu_parity.py, tests/test_gpu_adaptive.py SWITCHES) ...
SCHEDULES = [{}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}, {"RT_STREAM": "0"}, {"RT_PRIMARY_TABLE": "0"},
             {"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}]
# ... and the other pipelines a path batch can take: fewer slots than samples (k_finish hands slots on), the wide occlusion walks
PIPELINES = SCHEDULES + [{"RT_SLOTS": "200"}, {"RT_STREAM": "0", "RT_SLOTS": "200"}, {"RT_WIDE": "1"}, {"RT_WIDE8": "1"}]
SEED = 0x12345678
KIND_NAMES = ["point", "box", "tent"]
PARITY_SIZES = [(24, 16), (65, 3)]
FRAME0, NFRAMES = 5, 3


def _scene_fn(scenes, name):
    if name == "shiny":
        return tc.shiny
    if name == "scene3":
        return lambda b: scenes.scene3(b, force_diffuse=False)
    if name == "quality":
        return fc.quality_scene
    return getattr(scenes, name)


def _renderer(host_api, scenes, monkeypatch, name, env=None, w=24, h=16, devices=None, path_ticks=False):
    return sp.renderer(host_api, monkeypatch, _scene_fn(scenes, name), w, h, env, devices=devices, path_ticks=path_ticks, scene_camera=False)


# ---- 1. rays ----------------------------------------------------------------------------------------------------------------
# one lane; a partial wave; a wave and a lane; a block less one; a ragged last block; a skewed camera
@pytest.mark.parametrize("size,cam", [((1, 1), None), ((63, 1), None), ((65, 1), None), ((255, 1), None), ((257, 3), None), ((24, 16), fc.SKEWED)],
                         ids=["1x1", "63x1", "65x1", "255x1", "257x3", "24x16-skewed"])
def test_sample_rays_equal_the_restatement(size, cam, host_api, monkeypatch):
    w, h = size
    sp.clean_env(monkeypatch)
    r = host_api.HostRenderer(w, h)
    if cam:
        r.set_camera(*cam)
    seed_base = 0xFFFFFFF0 if w * h > 16 else 0xFFFFFFFF  # s = seed_base + pixel + frame * W * H wraps within the frame
    for name in KIND_NAMES:
        r.set_pixel_filter(fr.KINDS[name])
        assert r.pixel_filter() == fr.KINDS[name]
        for frame in (0, 7):
            O, D = r.sample_rays(frame, seed_base)
            O_ref, D_ref = fr.rays(fr.KINDS[name], r.camera(), w, h, frame, seed_base)
            assert sp.same(O, O_ref), (name, frame)
            assert sp.same(D, D_ref), (name, frame)
    # rows [y0, y1) are those rows of the frame
    if h > 1:
        O, D = r.sample_rays(7, seed_base, 1, h)
        assert sp.same(D, D_ref[w:]) and sp.same(O, O_ref[w:])
    r.close()


def test_fisheye_point_rays_are_primary_rays(host_api, oracle_api, monkeypatch):
    w, h = 24, 16
    sp.clean_env(monkeypatch)
    o = oracle_api.OracleScene()
    fc._tiny_scene(o)
    orr = oracle_api.OracleRenderer(o, w, h)
    cam = orr.camera()
    orr.set_camera(*cam, fisheye=True, view_angle=0.3, y_angle=0.1)
    O_ref, D_ref = orr.primary_rays()
    r = host_api.HostRenderer(w, h)
    r.set_camera(*cam, fisheye=True, view_angle=0.3, y_angle=0.1)
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    O, D = r.sample_rays(2, SEED)
    assert sp.same(O, O_ref) and sp.same(D, D_ref)
    r.close()
    orr.close()
    o.close()


# ---- 2. parity with the oracle ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def references(oracle_api, scenes):
    """reference(name, size, kind): filter_ref.accumulate of the parity frames, computed once per (scene, size, kind) and left unchanged;
    the oracle's scenes and renderers are closed when the module is done"""
    oracles, refs = {}, {}

    def reference(name, size, kind):
        key = (name, size, kind)
        if key not in refs:
            if name not in oracles:
                o = oracle_api.OracleScene()
                _scene_fn(scenes, name)(o)
                o.set_raytracer(False)
                oracles[name] = o
            if (name, size) not in oracles:
                oracles[(name, size)] = oracle_api.OracleRenderer(oracles[name], *size)
            orr = oracles[(name, size)]
            refs[key] = fr.accumulate(orr, kind, orr.camera(), FRAME0, NFRAMES, SEED)
            refs[key].setflags(write=False)
        return refs[key]

    yield reference
    for key in sorted(oracles, key=lambda k: not isinstance(k, tuple)):  # renderers before their scenes
        oracles[key].close()


def _check_parity(host_api, references, scenes, monkeypatch, name, env):
    from conftest import rel_err
    for size in PARITY_SIZES:
        r = _renderer(host_api, scenes, monkeypatch, name, env, *size)
        for kname in KIND_NAMES:
            kind = fr.KINDS[kname]
            ref = references(name, size, kind)
            r.set_pixel_filter(kind)
            r.clear()
            r.render(host_api.RT_MODE_PATH, FRAME0, NFRAMES, SEED)
            got = r.accumulator()[..., :3]
            err, cls_ok = rel_err(got, ref)
            print("%s %s %dx%d %s: max rel err %.3g" % (name, sp.env_id(env), size[0], size[1], kname, err.max()))
            assert cls_ok, (size, kname)
            assert err.max() <= 1e-4, (size, kname, err.max())
        r.close()


@pytest.mark.parametrize("env", PIPELINES, ids=sp.env_id)
@pytest.mark.parametrize("name", ["scene3", "tlas_test2", "mixed_small"])
def test_accumulator_equals_the_oracle_on_the_restated_rays(name, env, scenes, host_api, references, monkeypatch):
    _check_parity(host_api, references, scenes, monkeypatch, name, env)


def test_accumulator_equals_the_oracle_in_the_general_kernel(scenes, host_api, references, monkeypatch):
    """a shiny diffuse floor: path mode runs k_sample_general"""
    _check_parity(host_api, references, scenes, monkeypatch, "shiny", {})


@pytest.mark.parametrize("name", ["tlas_test2", "mixed_small"])
def test_schedules_are_bit_equal_under_box(name, scenes, host_api, monkeypatch):
    first = None
    for env in SCHEDULES:
        r = _renderer(host_api, scenes, monkeypatch, name, env, 65, 3)
        r.set_pixel_filter(host_api.RT_FILTER_BOX)
        r.render(host_api.RT_MODE_PATH, FRAME0, NFRAMES, SEED)
        acc = r.accumulator()
        r.close()
        if first is None:
            first = acc
        assert sp.same(acc, first), env


# ---- 3. composition -----------------------------------------------------------------------------------------------------------
W, H = 40, 21


def _seeded_list(w, h, frac=0.6, seed=5):
    """about 60 % of the pixels, the four corners and a complete first and last column among them"""
    rng = np.random.default_rng(seed)
    on = (rng.random(w * h) < frac - 0.04).reshape(h, w)
    on[0, 0] = on[0, -1] = on[-1, 0] = on[-1, -1] = True
    on[:, 0] = on[:, -1] = True
    return np.flatnonzero(on.reshape(-1)).astype(np.uint32)


@pytest.mark.parametrize("kname", ["box", "tent"])
def test_rows_lists_plans_and_split_calls_equal_render(kname, scenes, host_api, monkeypatch):
    PATH, kind = host_api.RT_MODE_PATH, fr.KINDS[kname]
    F = 3
    a = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    b = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    for r in (a, b):
        r.set_pixel_filter(kind)
        r.stats_enable(True)
    # the states after F .. F + 11 frames, one frame at a time
    stack = [sp.state(a)]
    for n in range(12):
        a.render(PATH, F + n, 1, SEED)
        stack.append(sp.state(a))
    # four frames as 1 + 3 calls, and as one call
    for split in ((4,), (1, 3)):
        b.clear()
        f = F
        for n in split:
            b.render(PATH, f, n, SEED)
            f += n
        assert all(sp.same(x, y) for x, y in zip(sp.state(b), stack[4])), split
        assert np.all(b.stats()[0] == 4)
    # a 3-way row interleave
    b.clear()
    for k in range(3):
        b.render_rows(PATH, F, 4, k, 3, (H - k + 2) // 3, SEED)
    assert all(sp.same(x, y) for x, y in zip(sp.state(b), stack[4]))
    # a 60 % list with the frame's edges: the listed pixels take frames F + 4 .. F + 6, the others keep four
    lst = _seeded_list(W, H)
    assert 0.5 < len(lst) / (W * H) < 0.7
    on = np.zeros(W * H, bool)
    on[lst] = True
    on = on.reshape(H, W)
    b.set_active(lst)
    b.render_active(F + 4, 3, SEED)
    for x, y7, y4 in zip(sp.state(b), stack[7], stack[4]):
        assert sp.same(x[on], y7[on]) and sp.same(x[~on], y4[~on])
    # a budgeted pass: a pixel with count n holds the state after n frames from F
    na, total, cap = b.select_budget(dict(select=dict(min_samples=6, max_samples=12, threshold=0.02, floor=1e-3), pass_cap=5))
    assert na > 0 and total >= na
    b.render_budget(F, SEED)
    got = sp.state(b)
    cnt = got[1]
    assert cnt.max() <= 12 and len(np.unique(cnt)) >= 2
    for n in np.unique(cnt):
        m = cnt == n
        assert all(sp.same(x[m], y[m]) for x, y in zip(got, stack[int(n)])), n
    a.close()
    b.close()


@pytest.mark.parametrize("kname", ["box", "tent"])
def test_adaptive_tick_over_two_contexts_equals_one(kname, scenes, host_api, monkeypatch):
    params = dict(min_samples=2, max_samples=6, threshold=0.05, floor=1e-3)
    out = []
    for devices in (None, [0, 0]):
        r = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H, devices=devices, path_ticks=True)
        r.set_adaptive(True, params)
        r.set_pixel_filter(fr.KINDS[kname])
        for _ in range(5):
            r.tick()
        out.append((r.tick_accumulator(),) + r.stats() + (np.int32([r.active_pixels()]),))
        r.close()
    assert all(sp.same(x, y) for x, y in zip(*out))


# ---- 4. reference mode is untouched -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}, {"RT_PRIMARY_TABLE": "0"}], ids=sp.env_id)
def test_reference_mode_after_a_filter_is_the_parent_s(env, scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    a = _renderer(host_api, scenes, monkeypatch, "mixed_small", env, W, H)
    b = _renderer(host_api, scenes, monkeypatch, "mixed_small", env, W, H)
    assert a.pixel_filter() == host_api.RT_FILTER_REFERENCE
    a.set_pixel_filter(host_api.RT_FILTER_BOX)
    a.render(PATH, 0, 3, SEED)
    boxed = a.accumulator()
    a.clear()
    a.set_pixel_filter(host_api.RT_FILTER_REFERENCE)
    for r in (a, b):
        r.render(PATH, 0, 3, SEED)
    assert sp.same(a.accumulator(), b.accumulator())
    assert not sp.same(boxed, b.accumulator())
    # the rays of reference mode: the truncated jitter lands on the integer pixels [x - 1, x] x [y - 1, y]
    O, D = b.sample_rays(0, SEED)
    b.set_pixel_filter(host_api.RT_FILTER_POINT)
    _, P = b.sample_rays(0, SEED)
    P, inner = P.reshape(H, W, 3), D.reshape(H, W, 3)[1:, 1:]
    cands = [P[1 - dy:H - dy, 1 - dx:W - dx] for dy in (0, 1) for dx in (0, 1)]
    assert np.all(np.any([np.all(sp.bits(inner) == sp.bits(c), axis=-1) for c in cands], axis=0))
    assert len({tuple(np.all(sp.bits(inner) == sp.bits(c), axis=-1).reshape(-1)) for c in cands}) == 4  # ... all four of them
    a.close()
    b.close()


# ---- 5. errors and state ------------------------------------------------------------------------------------------------------------
def test_errors_and_state(scenes, host_api, monkeypatch):
    PATH, UNSUP = host_api.RT_MODE_PATH, host_api.RT_E_UNSUPPORTED
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    L = r.rt
    for bad in (-1, 4, 99):
        assert L.rt_set_pixel_filter(r.ctx, bad) == host_api.RT_E_ARG
    assert L.rt_set_pixel_filter(None, 1) == host_api.RT_E_ARG
    assert r.pixel_filter() == host_api.RT_FILTER_REFERENCE
    with pytest.raises(RuntimeError):
        r.set_pixel_filter(7)
    assert r.pixel_filter() == host_api.RT_FILTER_REFERENCE
    # setting a kind neither clears the accumulator nor makes the G-buffer stale
    r.render(PATH, 0, 2, SEED)
    r.render_aovs(0.001)
    before = r.accumulator()
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    assert sp.same(r.accumulator(), before)
    r.denoise(2)
    assert np.isfinite(r.denoised()[..., :3]).any()
    # a fisheye camera: POINT renders, BOX / TENT do not
    cam = r.camera()
    r.set_camera(*cam, fisheye=True, view_angle=0.3)
    O = np.zeros((W * H, 3), np.float32)
    for kind in (host_api.RT_FILTER_BOX, host_api.RT_FILTER_TENT):
        r.set_pixel_filter(kind)
        assert L.rt_render(r.ctx, PATH, 0, 1, SEED, 0, H, 4) == UNSUP
        assert L.rt_render_rows(r.ctx, PATH, 0, 1, SEED, 0, 2, H // 2, 4) == UNSUP
        assert L.rt_sample_rays(r.ctx, 0, SEED, 0, H, O.ctypes.data_as(C.c_void_p), O.ctypes.data_as(C.c_void_p)) == UNSUP
        r.set_active([0, 5])
        assert L.rt_render_active(r.ctx, 0, 1, SEED, 4) == UNSUP
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    r.render(PATH, 0, 1, SEED)
    assert L.rt_render(r.ctx, host_api.RT_MODE_WHITTED, 0, 1, SEED, 0, H, 4) == 0  # Whitted mode ignores the filter
    r.set_camera(*cam)
    # the Q-learning sampler with a kind set
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    r.qlearn_enable(4, (-3, -1, -3), (3, 4, 5))
    assert L.rt_render(r.ctx, PATH, 0, 1, SEED, 0, H, 4) == UNSUP
    r.set_pixel_filter(host_api.RT_FILTER_REFERENCE)
    r.render(PATH, 0, 1, SEED)
    r.qlearn_disable()
    # rt_trace_batch ignores the filter
    O1, D1 = np.float32([[0, 1, -2]] * 4), np.float32([[0, 0, 1], [0.1, 0, 1], [0, -0.3, 1], [0.3, 0.2, 1]])
    ref = r.trace_batch(PATH, O1, D1)
    r.set_pixel_filter(host_api.RT_FILTER_TENT)
    assert sp.same(r.trace_batch(PATH, O1, D1), ref)
    r.close()


def test_tick_clears_on_a_change_of_filter(scenes, host_api, monkeypatch):
    PATH = host_api.RT_MODE_PATH
    t = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H, path_ticks=True)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", None, W, H)
    for _ in range(3):
        t.tick()  # path frames 0, 1, 2 in reference mode
    assert np.isfinite(t.tick_accumulator()[..., :3]).any()
    t.set_pixel_filter(host_api.RT_FILTER_BOX)
    t.tick()  # frame 3 alone, under BOX
    hand.set_pixel_filter(host_api.RT_FILTER_BOX)
    hand.clear()
    hand.render(PATH, 3, 1, SEED)
    assert sp.same(t.tick_accumulator(), hand.accumulator())
    t.tick()  # ... and frame 4 on top
    hand.render(PATH, 4, 1, SEED)
    assert sp.same(t.tick_accumulator(), hand.accumulator())
    t.close()
    hand.close()


# ---- 6. quality ---------------------------------------------------------------------------------------------------------------------
def test_box_filter_antialiases_on_the_device(scenes, host_api, quality, monkeypatch):
    q = fc.QUALITY
    PATH = host_api.RT_MODE_PATH
    truth = quality["truth"]
    r = _renderer(host_api, scenes, monkeypatch, "quality", None, q["width"], q["height"])
    nmax = q["frames"][-1]
    r.set_pixel_filter(host_api.RT_FILTER_BOX)
    mse, done = {}, 0
    for n in q["frames"]:
        r.render(PATH, done, n - done, q["seed_base"])
        done = n
        mse[n] = fc.quality_mse(r.accumulator() / n, truth)
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    r.clear()
    r.render(PATH, 0, 1, q["seed_base"])
    point = fc.quality_mse(r.accumulator(), truth)
    r.set_pixel_filter(host_api.RT_FILTER_REFERENCE)
    r.clear()
    r.render(PATH, 0, nmax, q["seed_base"])
    reference = fc.quality_mse(r.accumulator() / nmax, truth)
    r.close()
    print("device MSE box %s, point %.5f, reference mode (%d frames) %.5f: box / point %.3f, box / reference %.3f"
          % (" ".join("%d: %.5f" % kv for kv in mse.items()), point, nmax, reference, mse[nmax] / point, mse[nmax] / reference))
    assert mse[nmax] <= q["ratio_max"] * point
    assert mse[nmax] <= q["ratio_max"] * reference
    assert mse[q["frames"][0]] > mse[q["frames"][1]] > mse[q["frames"][2]]
