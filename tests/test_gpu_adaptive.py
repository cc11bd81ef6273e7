"""Adaptive sampling on the device, through host_api: the per-pixel statistics (rt_stats_enable / k_accumulate<true>) and the selection
(rt_select_active) against their numpy restatement (tests/adaptive_ref.py) bit for bit, rt_render_active against rt_render bit for bit,
the error cases, rt_resolve_adaptive, Renderer::Tick's adaptive mode against the same loop driven by hand, and what the loop buys at an
equal number of samples (the experiment tests/test_adaptive_cpu.py fixes on the oracle)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import budget_shapes as tc  # noqa: E402
import support as sp  # noqa: E402
from test_adaptive_cpu import QUALITY  # noqa: E402

pytestmark = pytest.mark.gpu

# the equivalent-path switches the GPU tier renders path frames under (a context reads them when it is created)
SWITCHES = [{}, {"RT_PRIMARY_TABLE_MIN": "0"}, {"RT_PRIMARY_TABLE": "0"}, {"RT_STREAM": "0"}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}]
W, H = 96, 64


def _renderer(host_api, scenes, monkeypatch, name, env=None, w=W, h=H):
    return sp.renderer(host_api, monkeypatch, tc.scene_fn(scenes, name), w, h, env, path_ticks=False)


def _seeded_list(w, h, seed=5):
    """about 30 % of the pixels: pixel 0, the last pixel, one complete row, isolated single pixels (neighbours left out), a seeded rest"""
    rng = np.random.default_rng(seed)
    on = rng.random(w * h) < 0.28
    on[0] = on[w * h - 1] = True
    on[7 * w:8 * w] = True                       # a complete row
    for p in (3 * w + 10, 20 * w + 50, 40 * w + 3):  # isolated: the pixel alone in its 3 x 3 block
        y, x = divmod(p, w)
        for dy in (-1, 0, 1):
            on[(y + dy) * w + x - 1:(y + dy) * w + x + 2] = False
        on[p] = True
    return np.flatnonzero(on).astype(np.uint32)


# ---- 1. statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_statistics_are_exact_and_have_no_side_effect(name, scenes, host_api, monkeypatch):
    K = 7
    r = _renderer(host_api, scenes, monkeypatch, name)
    PATH = host_api.RT_MODE_PATH
    S = np.zeros((K, H, W, 4), np.float32)
    for f in range(K):  # statistics off: the accumulator after one frame from clear is that frame's sample
        r.clear()
        r.render(PATH, f, 1)
        S[f] = r.accumulator()
    r.clear()
    r.render(PATH, 0, K)
    acc_off = r.accumulator()
    cnt_ref, sy_ref, syy_ref = ar.moments(S)
    for split in ((K,), (3, K - 3)):
        r.stats_enable(True)
        r.clear()
        f = 0
        for n in split:
            r.render(PATH, f, n)
            f += n
        cnt, sy, syy = r.stats()
        assert np.all(cnt == K)
        assert sp.same(sy, sy_ref) and sp.same(syy, syy_ref), split
        assert sp.same(r.accumulator(), acc_off), split
        # a directly viewed light sums to +inf where the accumulator does
        lit = np.isposinf(acc_off[..., :3]).all(-1)
        assert np.all(np.isposinf(sy[lit])) and np.all(np.isposinf(syy[lit]))
        r.stats_enable(False)
    # Whitted frames do not touch the statistics; enabling zeroes them, rt_clear zeroes them
    r.stats_enable(True)
    r.render(host_api.RT_MODE_WHITTED, 0, 1)
    cnt, sy, syy = r.stats()
    assert not cnt.any() and not sy.any() and not syy.any()
    r.render(PATH, 0, 2)
    assert np.all(r.stats()[0] == 2)
    r.clear()
    cnt, sy, syy = r.stats()
    assert not cnt.any() and not sp.bits(sy).any() and not sp.bits(syy).any()
    r.close()


# ---- 2. rt_render_active ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", SWITCHES, ids=sp.env_id)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2", "shiny"])
def test_render_active_equals_render_where_listed(name, env, scenes, host_api, monkeypatch):
    r = _renderer(host_api, scenes, monkeypatch, name, env)
    PATH = host_api.RT_MODE_PATH
    lst = _seeded_list(W, H)
    assert 0.2 < len(lst) / (W * H) < 0.4
    on = np.zeros(W * H, bool)
    on[lst] = True
    on = on.reshape(H, W)
    r.stats_enable(True)

    def state():
        return (r.accumulator(),) + r.stats()

    r.clear()
    r.render(PATH, 0, 4)
    four = state()
    r.render(PATH, 4, 4)
    A = state()
    r.clear()
    r.render(PATH, 0, 4)
    assert all(sp.same(x, y) for x, y in zip(state(), four))
    r.set_active(lst)
    got, n = r.active()
    assert n == len(lst) and np.array_equal(got, lst)
    r.render_active(4, 4)
    B = state()
    for b, a, f in zip(B, A, four):
        assert sp.same(b[on], a[on]) and sp.same(b[~on], f[~on])
    assert np.all(B[1][on] == 8) and np.all(B[1][~on] == 4)
    # the list survives rt_clear; every pixel listed: the whole-frame render
    r.clear()
    assert r.active()[1] == len(lst)
    r.render(PATH, 0, 4)
    r.set_active(np.arange(W * H, dtype=np.uint32))
    r.render_active(4, 4)
    assert all(sp.same(x, y) for x, y in zip(state(), A))
    # one pixel
    p = 31 * W + 17
    r.clear()
    r.render(PATH, 0, 4)
    r.set_active([p])
    r.render_active(4, 4)
    one = np.zeros((H, W), bool)
    one[31, 17] = True
    for b, a, f in zip(state(), A, four):
        assert sp.same(b[one], a[one]) and sp.same(b[~one], f[~one])
    # an empty list: OK, nothing touched
    before = state()
    r.set_active([])
    r.render_active(8, 4)
    assert r.active()[1] == 0 and all(sp.same(x, y) for x, y in zip(state(), before))
    # with statistics off: the region-of-interest render
    r.stats_enable(False)
    r.clear()
    r.render(PATH, 0, 4)
    r.set_active(lst)
    r.render_active(4, 4)
    acc = r.accumulator()
    assert sp.same(acc[on], A[0][on]) and sp.same(acc[~on], four[0][~on])
    r.close()


# ---- 3. selection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_selection_equals_the_restatement(name, scenes, host_api, monkeypatch):
    r = _renderer(host_api, scenes, monkeypatch, name)
    r.stats_enable(True)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 16)
    # uneven counts: some pixels get 5 more frames
    extra = _seeded_list(W, H, seed=9)
    r.set_active(extra)
    r.render_active(16, 5)
    cnt, sy, syy = r.stats()
    assert set(np.unique(cnt)) == {16, 21}
    INF = float("inf")
    combos = [dict(ar.DEFAULTS), dict(min_samples=2, max_samples=1024, threshold=0.1, floor=1e-3), dict(min_samples=18, max_samples=1024, threshold=0.02, floor=1e-3),
              dict(min_samples=16, max_samples=21, threshold=0.01, floor=0.5), dict(min_samples=16, max_samples=17, threshold=0.0, floor=1e-6),
              dict(min_samples=16, max_samples=1024, threshold=0.0, floor=1e-3), dict(min_samples=16, max_samples=1024, threshold=INF, floor=1e-3),
              dict(min_samples=20, max_samples=1024, threshold=INF, floor=1e-3), dict(min_samples=2, max_samples=2, threshold=0.0, floor=1.0)]
    sizes = set()
    for P in combos:
        want = ar.active_list(cnt, sy, syy, **P)
        n = r.select_active(P)
        got, n2 = r.active()
        assert n == n2 == len(got) == len(want), (P, n, len(want))
        assert np.array_equal(got, want), P
        assert np.all(np.diff(got.astype(np.int64)) > 0)
        short, n3 = r.active(cap=min(5, n))
        assert n3 == n and np.array_equal(short, want[:min(5, n)])
        sizes.add(n)
    assert len(sizes) >= 4, sizes  # the combinations really select different sets
    # threshold 0: every finite pixel below max_samples whose samples differ at all; threshold +inf: only count < min_samples
    fin = np.isfinite(sy) & np.isfinite(syy)
    n0 = r.select_active(dict(min_samples=16, max_samples=1024, threshold=0.0, floor=1e-3))
    got = r.active()[0]
    assert n0 > 0 and fin.reshape(-1)[got].all()
    e = ar.relative_error(cnt, sy, syy, 1e-3)
    assert np.array_equal(got, np.flatnonzero((fin & (e > 0)).reshape(-1)))
    assert r.select_active(dict(min_samples=16, max_samples=1024, threshold=INF, floor=1e-3)) == 0
    assert r.select_active(dict(min_samples=20, max_samples=1024, threshold=INF, floor=1e-3)) == int((cnt < 20).sum())
    # the library's defaults when params is NULL
    assert r.select_active(None) == len(ar.active_list(cnt, sy, syy, **ar.DEFAULTS))
    r.close()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------
def test_errors(scenes, host_api, monkeypatch):
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small")
    L, ctx = r.rt, r.ctx
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    n = C.c_int(-7)
    buf = np.zeros(W * H, np.uint32)
    px = buf.ctypes.data_as(C.c_void_p)

    def sel(**kw):
        p = host_api.adaptive_params(kw)
        return L.rt_select_active(ctx, C.byref(p), C.byref(n))

    # statistics off
    assert sel() == STATE and L.rt_resolve_adaptive(ctx, 0, H, px) == STATE and L.rt_download_stats(ctx, 0, H, None, None, None) == STATE
    # no list installed
    assert L.rt_render_active(ctx, 0, 1, 1, 4) == STATE and L.rt_download_active(ctx, px, W * H, C.byref(n)) == STATE
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    for bad in (dict(min_samples=1), dict(min_samples=0), dict(min_samples=8, max_samples=7), dict(threshold=float("nan")), dict(threshold=-0.5),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan"))):
        assert sel(**bad) == ARG, bad
    assert n.value == -7 and L.rt_render_active(ctx, 0, 1, 1, 4) == STATE  # a refused selection installs nothing
    assert sel(min_samples=2, max_samples=2) == 0 and n.value == 0
    # caller lists: refused before anything is uploaded (the installed list stays)
    good = np.array([3, 9, 10, W * H - 1], np.uint32)
    r.set_active(good)
    for bad in ([5, 4, 6], [5, 5, 6], [0, 1, W * H], [W * H + 5], [7, 8, 2 ** 32 - 1]):
        a = np.array(bad, np.uint32)
        assert L.rt_set_active_pixels(ctx, a.ctypes.data_as(C.c_void_p), len(a)) == ARG, bad
        got, k = r.active()
        assert k == 4 and np.array_equal(got, good)
    assert L.rt_set_active_pixels(ctx, None, 3) == ARG and L.rt_set_active_pixels(ctx, None, -1) == ARG
    assert L.rt_render_active(ctx, 0, 0, 1, 4) == ARG
    # the Q-learning sampler
    r.qlearn_enable(4, (-3, -1, -3), (3, 4, 5))
    assert L.rt_render_active(ctx, 0, 1, 1, 4) == UNSUP
    r.qlearn_disable()
    assert L.rt_render_active(ctx, 2, 1, 0x12345678, 4) == 0
    cnt = r.stats()[0].reshape(-1)
    assert np.all(cnt[good] == 3) and cnt.sum() == 2 * W * H + 4
    r.close()


# ---- 5. resolve ------------------------------------------------------------------------------------------------------------
def test_resolve_adaptive(scenes, host_api, monkeypatch):
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small")
    r.stats_enable(True)
    lst = _seeded_list(W, H)
    r.clear()
    r.set_active(lst)
    r.render_active(0, 3)           # count 3 on the list, 0 elsewhere
    r.set_active(lst[::2])
    r.render_active(3, 4)           # 7 on every other listed pixel
    cnt = r.stats()[0]
    assert set(np.unique(cnt)) == {0, 3, 7}
    got = r.resolve_adaptive()
    assert np.array_equal(got, ar.resolve(r.accumulator(), cnt))
    assert np.all(got[cnt == 0] == 0) and got[cnt > 0].any()
    assert np.array_equal(r.resolve_adaptive(5, 9), got[5:9])
    r.close()


# ---- 6. Renderer::Tick -----------------------------------------------------------------------------------------------------
def test_tick_adaptive_equals_the_loop_by_hand(scenes, host_api, monkeypatch):
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    TICKS = 12
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small")
    r.scene.set_raytracer(False)  # Tick renders path frames
    r.set_adaptive(True, P)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small")
    c = r.camera()
    hand.set_camera(c[0], c[1], c[2], c[3])
    hand.stats_enable(True)
    hand.clear()
    active, rendered = [], 0
    for t in range(TICKS):
        r.tick()
        if t < P["min_samples"]:
            hand.render(host_api.RT_MODE_PATH, t, 1)
            n = W * H
        else:
            n = hand.select_active(P)
            hand.render_active(t, 1)
        assert r.active_pixels() == n, t
        active.append(n)
        rendered += n
        assert sp.same(r.tick_accumulator(), hand.accumulator()), t
        assert np.array_equal(r.stats()[0], hand.stats()[0]), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
    tail = active[P["min_samples"]:]
    assert all(b <= a for a, b in zip(tail, tail[1:])), active  # a static camera: pixels only ever leave the active set
    assert 0 < tail[0] < W * H
    assert int(r.stats()[0].sum(dtype=np.int64)) == rendered
    # a camera change clears the accumulator and the counts with it
    c = r.camera()
    r.set_camera(c[0] + np.float32([0.1, 0, 0]), c[1], c[2], c[3])
    r.tick()
    assert np.all(r.stats()[0] == 1) and r.active_pixels() == W * H
    # adaptive with the denoised preview: refused, naming the limit
    r.set_denoise(True)
    with pytest.raises(RuntimeError, match="denoise"):
        r.tick()
    r.set_denoise(False)
    # switched off again: Tick is the plain one (no statistics kept)
    r.set_adaptive(False)
    r.tick()
    assert r.rt.rt_download_stats(r.ctx, 0, H, None, None, None) == host_api.RT_E_STATE
    r.close()
    hand.close()


# ---- 7. quality ------------------------------------------------------------------------------------------------------------
def test_adaptive_beats_uniform_at_equal_samples(scenes, host_api, monkeypatch):
    """The experiment of tests/test_adaptive_cpu.py (scene, size, parameters, budget) on the device, against the device's own 256-frame
    mean.  Asserted: adaptive MSE / uniform MSE < 1 (the oracle's figure is 0.600).  Measured on an MI355X: 0.602 (1,840,125 of 1,843,200 samples, largest count 59)."""
    q = QUALITY
    w, h, P = q["width"], q["height"], q["params"]
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, q["scene"], w=w, h=h)
    r.clear()
    r.render(PATH, q["reference_frame0"], q["reference_frames"])
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
    r.clear()
    r.render(PATH, 0, q["budget_frames"])
    uni = r.accumulator()[..., :3].astype(np.float64) / q["budget_frames"]
    budget = q["budget_frames"] * w * h
    r.stats_enable(True)
    r.clear()
    r.render(PATH, 0, P["min_samples"])
    total, f = P["min_samples"] * w * h, P["min_samples"]
    while f < q["stack_frames"]:
        n = r.select_active(P)
        if n == 0 or total + n > budget:
            break
        r.render_active(f, 1)
        total, f = total + n, f + 1
    cnt = r.stats()[0]
    assert int(cnt.sum(dtype=np.int64)) == total <= budget and f < q["stack_frames"]
    with np.errstate(all="ignore"):
        ada = r.accumulator()[..., :3].astype(np.float64) / cnt[..., None]
    fin = np.isfinite(ref).all(-1) & np.isfinite(uni).all(-1) & np.isfinite(ada).all(-1)
    mse_a = ((ada[fin] - ref[fin]) ** 2).mean()
    mse_u = ((uni[fin] - ref[fin]) ** 2).mean()
    print("device adaptive / uniform MSE ratio %.3f (%d of %d samples, largest count %d, %d finite pixels)" % (mse_a / mse_u, total, budget, cnt.max(), fin.sum()))
    r.close()
    assert mse_a / mse_u < 1.0, mse_a / mse_u
