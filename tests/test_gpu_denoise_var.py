"""The variance-guided denoiser (rt_denoise_variance) on the device, through host_api: the kernels against their numpy restatement
(tests/denoise_var_ref.py) on uniformly and adaptively sampled frames, the empty and single-sample branches, freedom from side effects,
the error cases and the invalidation rule, Renderer::Tick's adaptive denoised preview, and what the filter buys on the adaptive frame of
the experiment tests/test_denoise_var_cpu.py fixes on the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dr  # noqa: E402
import denoise_var_ref as dv  # noqa: E402
import support as sp  # noqa: E402
from test_adaptive_cpu import QUALITY  # noqa: E402
from test_denoise_var_cpu import quality_ratio  # noqa: E402
from test_gpu_denoise import make  # noqa: E402

pytestmark = pytest.mark.gpu

RADIANCE_TOL = 1e-4
INF = float("inf")
ALL_INF = dict(sigma_luminance=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF)
PARAMS = [dict(iterations=1), dict(iterations=5), dict(ALL_INF, iterations=5),
          dict(iterations=3, sigma_luminance=1.5, sigma_normal=INF, sigma_position=0.05, sigma_albedo=1.0, epsilon=1e-2)]
ADAPT = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)


def kernel_vs_ref(orr, r, params, label=""):
    """rt_denoise_variance of the renderer's current accumulator and statistics against the restatement: colour and variance channels,
    conftest.rel_err <= 1e-4 each, non-finite classes equal.  The variance channel is held at the same bar under rel_err's 1e-3 floor (the
    variances of the mean are far below it, so the bar is absolute there: 1e-7; measured: at most 7.4e-5 under rel_err); its error
    against its own size is printed and held at a bar that the conditioning of the weights explains: y_p and y_q each carry about four
    roundings of 2^-24 (three products, two sums, and the f32 colour itself against the f64 one), their difference is multiplied by
    kl <= 1 / epsilon, so an exponent moves by up to 8 x 2^-24 x max(y, 1) / epsilon, w^2 by twice that, once per iteration: 9.5e-3 per
    iteration with epsilon 1e-4 and y <= 1 (measured: 3.3e-3 after one iteration, 2.1e-2 after five), 1e-5 without the luminance term.
    A wrong sum w^2 / (sum w)^2 normalisation is off by tens of per cent at the first iteration and cannot hide below either bar."""
    r.render_aovs(0.001)
    r.denoise_variance(params)
    got = r.denoised()
    g = r.aovs()
    O, D = orr.primary_rays()
    pos = dv.positions(O, D, g["t"].reshape(-1))
    cnt, sy, syy = r.stats()
    ref = dv.denoise(r.accumulator(), cnt, sy, syy, g, pos, params)
    err, cls_ok = rel_err(got[..., :3], ref[..., :3])
    assert cls_ok, "non-finite pixels differ from the restatement"
    verr, vcls_ok = rel_err(got[..., 3], ref[..., 3])
    vown = rel_err(got[..., 3], ref[..., 3], floor=1e-30)[0]
    P = dict(dv.DEFAULTS, **(params or {}))
    with np.errstate(all="ignore"):
        ymax = np.nanmax(np.where(np.isfinite(ref[..., :3]).all(-1), np.abs(dv.luminance(ref[..., :3])), 0.0))
    kl_max = 1.0 / P["epsilon"] if np.isfinite(P["sigma_luminance"]) else 0.0
    own_bar = 1e-5 + P["iterations"] * 2 * kl_max * 8 * 2.0 ** -24 * max(ymax, 1.0)
    print("%s %s: colour error %.3g, variance error %.3g (against its own size %.3g)" % (label, params, err.max(), verr.max(), vown.max()))
    assert err.max() <= RADIANCE_TOL, "denoised colour error %g" % err.max()
    assert vcls_ok and verr.max() <= RADIANCE_TOL, "denoised variance error %g" % verr.max()
    assert vown.max() <= own_bar, "denoised variance error against its own size %g (bar %g)" % (vown.max(), own_bar)
    c, v, empty, passed = dv.inputs(r.accumulator(), cnt, sy, syy)
    off = empty | passed
    assert np.all(got[..., 3][off] == 0) and np.all(got[..., :3][empty] == 0)
    assert np.array_equal(got[..., :3][passed], c[passed], equal_nan=True)  # passed through: c_p as it is
    return got, ref


def _adaptive_loop(r, host_api, P, frames):
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, P["min_samples"])
    for f in range(P["min_samples"], P["min_samples"] + frames):
        if r.select_active(P) == 0:
            break
        r.render_active(f, 1)


@pytest.mark.parametrize("name,w,h", [("mixed_small", 64, 40), ("scene3", 320, 180), ("pretty_tlas", 320, 180)])
@pytest.mark.parametrize("sampling", [1, 4, 16, "adaptive"])
def test_kernel_equals_the_restatement(name, w, h, sampling, scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, getattr(scenes, name), w, h)
    r.stats_enable(True)
    if sampling == "adaptive":
        _adaptive_loop(r, host_api, ADAPT, 12)
        cnt = r.stats()[0]
        assert cnt.min() >= ADAPT["min_samples"] and len(np.unique(cnt)) > 2  # uneven counts
    else:
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, sampling)
    for p in PARAMS:
        kernel_vs_ref(orr, r, p, "%s %dx%d %s" % (name, w, h, sampling))
    r.close()


@pytest.mark.parametrize("w,h", [(1, 1), (33, 9), (97, 41)])
def test_odd_sizes(w, h, scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, w, h)
    r.stats_enable(True)
    for frames in (1, 4):
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        for p in PARAMS:
            kernel_vs_ref(orr, r, p, "mixed_small %dx%d %d" % (w, h, frames))
    r.close()


def test_empty_and_single_sample_pixels(scenes, oracle_api, host_api):
    """a caller's list leaves some pixels at count 0 and renders others for exactly one frame"""
    w, h = 64, 40
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, w, h)
    r.stats_enable(True)
    rng = np.random.default_rng(8)
    kind = rng.integers(0, 3, w * h)  # 0: never sampled, 1: one frame, 2: five frames
    kind[:w] = 0                      # a whole empty row, an empty block, and isolated ones from the draw
    kind[10 * w + 20:10 * w + 30] = 0
    r.clear()
    r.set_active(np.flatnonzero(kind >= 1).astype(np.uint32))
    r.render_active(0, 1)
    r.set_active(np.flatnonzero(kind == 2).astype(np.uint32))
    r.render_active(1, 4)
    cnt = r.stats()[0]
    assert set(np.unique(cnt)) == {0, 1, 5}
    for p in PARAMS:
        got, ref = kernel_vs_ref(orr, r, p, "caller's list")
        assert np.all(got[cnt == 0] == 0)
    r.close()


def test_tiny_epsilon_and_zero_variance_stay_finite(scenes, oracle_api, host_api):
    """an accepted epsilon whose reciprocal overflows f32 (1e-40), on a frame with pixels of zero variance: kl is clamped to FLT_MAX, the
    centre tap's zero difference adds 0 and nothing turns NaN (one iteration: with such a kl a weight is 0 or 1 by the last bit of y)"""
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)
    r.stats_enable(True)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 2)
    cnt, sy, syy = r.stats()
    c, v, empty, passed = dv.inputs(r.accumulator(), cnt, sy, syy)
    assert (v[~passed] == 0).any()  # the case is there: two equal samples (a miss sees the same sky twice) give v = 0 exactly
    got, ref = kernel_vs_ref(orr, r, dict(iterations=1, epsilon=1e-40), "tiny epsilon")
    assert np.isfinite(got[~passed]).all()
    r.close()


def test_kernel_equals_the_restatement_full_size(scenes, oracle_api, host_api):
    """config 3's scene at 1920 x 1080 after an adaptive loop, the defaults"""
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.pretty_tlas, 1920, 1080)
    r.stats_enable(True)
    _adaptive_loop(r, host_api, ADAPT, 4)
    got, ref = kernel_vs_ref(orr, r, None, "pretty_tlas 1920x1080 adaptive")
    assert np.all(np.isfinite(got[..., :3]), -1).mean() > 0.5  # (the rest: directly viewed lights, passed through)
    r.close()


def test_no_side_effects(scenes, oracle_api, host_api):
    def start():
        r = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)[2]
        r.stats_enable(True)
        _adaptive_loop(r, host_api, ADAPT, 3)
        return r

    def state(r):
        return (r.accumulator(),) + tuple(r.stats()) + (r.resolve_adaptive(),)

    r = start()
    before = state(r)
    r.render_aovs(0.001)
    r.denoise_variance()
    r.resolve_denoised()
    after = state(r)
    assert all(sp.same(a, b) for a, b in zip(before, after))
    r.select_active(ADAPT)
    r.render_active(20, 2)
    r2 = start()
    r2.select_active(ADAPT)
    r2.render_active(20, 2)
    assert all(sp.same(a, b) for a, b in zip(state(r), state(r2)))
    r.close(), r2.close()


def _rc(r, host_api, params=None):
    p = host_api.denoise_var_params(params)
    return host_api.rt_lib().rt_denoise_variance(r.ctx, C.byref(p) if p is not None else None)


def test_errors_and_invalidation(scenes, oracle_api, host_api):
    ARG, STATE = host_api.RT_E_ARG, host_api.RT_E_STATE
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.pretty_animation_scene, 64, 40)
    r.render(host_api.RT_MODE_PATH, 0, 1)
    r.render_aovs(0.001)
    assert _rc(r, host_api) == STATE and "statistics" in r.rt.rt_last_error(r.ctx).decode()  # statistics off (the G-buffer is there)
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    assert _rc(r, host_api) == 0
    r2 = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)[2]
    r2.stats_enable(True)
    r2.render(host_api.RT_MODE_PATH, 0, 2)
    assert _rc(r2, host_api) == STATE and "missing" in r2.rt.rt_last_error(r2.ctx).decode()  # no G-buffer yet
    r2.close()
    for bad in (dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(sigma_luminance=0.0), dict(sigma_luminance=-INF),
                dict(sigma_luminance=float("nan")), dict(sigma_normal=-1.0), dict(sigma_normal=float("nan")), dict(sigma_position=0.0),
                dict(sigma_position=float("nan")), dict(sigma_albedo=0.0), dict(sigma_albedo=float("nan")), dict(epsilon=0.0),
                dict(epsilon=-1e-4), dict(epsilon=float("nan"))):
        assert _rc(r, host_api, bad) == ARG, bad
    assert _rc(r, host_api, dict(ALL_INF, iterations=8)) == 0
    # staleness: rt_denoise's rule
    cam = r.camera()
    r.set_camera(cam[0], cam[1], cam[2], cam[3])  # the same record: still current
    assert _rc(r, host_api) == 0
    r.set_camera(cam[0] + np.float32(0.01), cam[1], cam[2], cam[3])
    assert _rc(r, host_api) == STATE and "stale" in r.rt.rt_last_error(r.ctx).decode()
    r.render_aovs(0.001)
    assert _rc(r, host_api) == 0
    r.scene.set_time(0.7)
    assert _rc(r, host_api) == STATE
    r.render_aovs(0.001)
    assert _rc(r, host_api) == 0
    r.commit()  # rt_upload_scene
    assert _rc(r, host_api) == STATE
    r.render_aovs(0.001)
    assert _rc(r, host_api) == 0
    r.close()


def test_rt_denoise_afterwards_is_its_own(scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 4)
    r.render_aovs(0.001)
    r.denoise(4)
    plain = r.denoised()
    r.stats_enable(True)  # (zeroes the statistics only)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 4)
    for its in (1, 2, 5):  # the variance filter's result in either ping-pong buffer
        r.denoise_variance(dict(iterations=its))
        var = r.denoised()
        assert (var[..., 3] > 0).any()
        r.denoise(4)
        again = r.denoised()
        assert np.all(again[..., 3] == 0) and sp.same(again, plain)
        assert not sp.same(again[..., :3], var[..., :3])
    r.close()


# ---- Renderer::Tick ----
def _ticker(scenes, host_api, adaptive=None, denoise_variance=None):
    r = host_api.HostRenderer(64, 40)
    scenes.mixed_small(r.scene)
    r.commit()
    r.scene.set_raytracer(False)
    if adaptive is not None:
        r.set_adaptive(adaptive, ADAPT)
    if denoise_variance is not None:
        r.set_denoise_variance(denoise_variance)
    return r


def test_tick_adaptive_denoised(scenes, host_api):
    P = dict(iterations=3, sigma_luminance=2.0, epsilon=1e-3)
    r = _ticker(scenes, host_api, adaptive=True)
    r.set_denoise_variance(True, P)
    for t in range(8):
        r.tick()
        px = r.tick_pixels()
        assert sp.same(r.tick_accumulator(), r.accumulator())  # the raw accumulator
        r.denoise_variance(P)  # directly, on the same state
        assert np.array_equal(px, r.resolve_denoised()), t
        assert not np.array_equal(px, r.resolve_adaptive())
    assert len(np.unique(r.stats()[0])) > 1  # past min_samples: uneven counts
    # a camera move refreshes the G-buffer
    cam = r.camera()
    r.set_camera(cam[0] + np.float32(0.2), cam[1], cam[2], cam[3])
    r.tick()
    r.denoise_variance(P)
    assert np.array_equal(r.tick_pixels(), r.resolve_denoised())
    # the defaults when no parameters were given
    r.close()
    r = _ticker(scenes, host_api, adaptive=True, denoise_variance=True)
    for t in range(3):
        r.tick()
    r.denoise_variance(None)
    assert np.array_equal(r.tick_pixels(), r.resolve_denoised())
    # adaptive with rt_denoise's preview stays refused
    r.set_denoise(True)
    with pytest.raises(RuntimeError, match="denoise"):
        r.tick()
    r.close()


def test_tick_denoise_variance_alone_throws(scenes, host_api):
    r = _ticker(scenes, host_api, denoise_variance=True)
    with pytest.raises(RuntimeError, match="statistics"):
        r.tick()
    r.close()


def test_tick_with_both_flags_off_is_the_plain_tick(scenes, host_api):
    """denoiseVariance never set or set to false, adaptive off: Tick's accumulator and pixels are rt_render + rt_resolve driven by hand"""
    K = 5
    hand = _ticker(scenes, host_api)
    for flag in (None, False):
        r = _ticker(scenes, host_api, denoise_variance=flag)
        c = r.camera()
        hand.set_camera(c[0], c[1], c[2], c[3])
        hand.clear()
        for k in range(K):
            r.tick()
            hand.render(host_api.RT_MODE_PATH, k, 1)
            assert sp.same(r.tick_accumulator(), hand.accumulator()), k
        its = [it for it in range(1, K + 2) if np.array_equal(r.tick_pixels(), hand.resolve(it))]
        assert len(its) == 1, its  # rt_resolve of the same sums with Tick's frame count, and nothing else
        r.close()
    hand.close()


def test_tick_adaptive_with_the_flag_off_is_the_adaptive_tick(scenes, host_api):
    """adaptive on, denoiseVariance never set or set to false: Tick is the rt_select_active / rt_render_active loop driven by hand and
    shows rt_resolve_adaptive"""
    K = 8
    for flag in (None, False):
        r = _ticker(scenes, host_api, adaptive=True, denoise_variance=flag)
        hand = _ticker(scenes, host_api)
        c = r.camera()
        hand.set_camera(c[0], c[1], c[2], c[3])
        hand.stats_enable(True)
        hand.clear()
        for k in range(K):
            r.tick()
            if k < ADAPT["min_samples"]:
                hand.render(host_api.RT_MODE_PATH, k, 1)
            else:
                hand.select_active(ADAPT)
                hand.render_active(k, 1)
            assert sp.same(r.tick_accumulator(), hand.accumulator()), k
            assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), k
        r.close(), hand.close()


# ---- quality ----
def test_denoised_adaptive_frame_beats_the_raw_one(scenes, host_api):
    """The experiment of tests/test_denoise_var_cpu.py (scene, size, adaptive parameters, budget, RT_DENOISE_VAR_DEFAULTS) on the device,
    against the device's own 256-frame mean.  Asserted: denoised MSE / raw adaptive MSE < 1 (the oracle's figure is 0.352).
    Measured on an MI355X: 0.352 (1,840,125 of 1,843,200 samples, counts 16 .. 59).  Printed, not asserted (neither default set is tuned): the same
    filter against rt_denoise on a uniform 16-frame render of the scene (measured: 0.158 against 0.294 of the raw mean's MSE)."""
    q = QUALITY
    w, h, P = q["width"], q["height"], q["params"]
    PATH = host_api.RT_MODE_PATH
    r = host_api.HostRenderer(w, h)
    getattr(scenes, q["scene"])(r.scene)
    r.commit()
    r.render(PATH, q["reference_frame0"], q["reference_frames"])
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
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
    r.render_aovs(0.001)
    r.denoise_variance(None)
    den = r.denoised().astype(np.float64)
    ratio, finite = quality_ratio(den, r.accumulator(), cnt, ref)
    print("device denoised / raw adaptive MSE ratio %.3f (%d of %d samples, counts %d .. %d, %d finite pixels)" % (ratio, total, budget, cnt.min(), cnt.max(), finite))
    # uniform 16 frames: the two filters side by side
    r.clear()
    r.render(PATH, 0, 16)
    acc16, cnt16 = r.accumulator(), r.stats()[0]
    r.denoise_variance(None)
    a, _ = quality_ratio(r.denoised().astype(np.float64), acc16, cnt16, ref)
    r.denoise(16)
    b, _ = quality_ratio(r.denoised().astype(np.float64), acc16, cnt16, ref)
    print("uniform 16 frames, MSE over the raw mean's: rt_denoise_variance %.3f, rt_denoise %.3f" % (a, b))
    r.close()
    assert ratio < 1.0, ratio
