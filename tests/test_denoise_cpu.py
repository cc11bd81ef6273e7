"""G-buffer + denoiser without a GPU: the C ABI's new entry points exist and check their arguments, and the numpy restatement of the
filter (tests/denoise_ref.py) has the properties its definition promises."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dr  # noqa: E402

NEW = ["rt_render_aovs", "rt_download_aovs", "rt_denoise", "rt_download_denoised", "rt_resolve_denoised"]
INF = float("inf")


def test_denoise_symbols_exported(host_api):
    L = host_api.rt_lib()
    for sym in NEW:
        assert sym in host_api.RT_SYMBOLS
        assert hasattr(L, sym), sym
    assert hasattr(host_api.host_lib(), "rth_renderer_set_denoise")


def test_null_context_and_null_arguments(host_api):
    L = host_api.rt_lib()
    buf = np.zeros(64, np.float32)
    assert L.rt_render_aovs(None, C.c_float(0.001)) == host_api.RT_E_ARG
    assert L.rt_download_aovs(None, 0, 1, buf.ctypes.data, None) == host_api.RT_E_ARG
    assert L.rt_denoise(None, 1, None) == host_api.RT_E_ARG
    assert L.rt_download_denoised(None, 0, 1, buf.ctypes.data) == host_api.RT_E_ARG
    assert L.rt_download_denoised(None, 0, 1, None) == host_api.RT_E_ARG
    assert L.rt_resolve_denoised(None, 0, 1, buf.ctypes.data) == host_api.RT_E_ARG


@pytest.mark.parametrize("bad", [dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(sigma_color=0.0), dict(sigma_normal=-1.0),
                                 dict(sigma_position=float("nan")), dict(sigma_albedo=0.0), dict(sigma_color=-INF)])
def test_bad_params_are_argument_errors(host_api, bad):
    """The parameters are checked before the context: without a GPU (null context) the error names the parameter"""
    L = host_api.rt_lib()
    p = host_api.denoise_params(bad)
    assert L.rt_denoise(None, 1, C.byref(p)) == host_api.RT_E_ARG
    msg = L.rt_last_error(None).decode()
    assert "iterations" in msg or "sigma" in msg, msg


def test_bad_iteration_is_an_argument_error(host_api):
    L = host_api.rt_lib()
    for it in (0, -3):
        assert L.rt_denoise(None, it, None) == host_api.RT_E_ARG
        assert "iteration" in L.rt_last_error(None).decode()
    # good parameters, sigma = inf included: only the missing context is left to complain about
    p = host_api.denoise_params(dict(sigma_color=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF, iterations=8))
    assert L.rt_denoise(None, 1, C.byref(p)) == host_api.RT_E_ARG
    assert "null context" in L.rt_last_error(None).decode()


def test_defaults_agree_everywhere(host_api):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_amd.h")).read()
    line = [l for l in hdr.splitlines() if l.startswith("#define RT_DENOISE_DEFAULTS")][0]
    vals = [float(v.strip().rstrip("f")) for v in line.split("{")[1].split("}")[0].split(",")]
    keys = ["iterations", "sigma_color", "sigma_normal", "sigma_position", "sigma_albedo"]
    assert dict(zip(keys, vals)) == host_api.DENOISE_DEFAULTS == dr.DEFAULTS


# ---- the restatement ----
def _scene(h=24, w=32, seed=1):
    """a synthetic G-buffer: two planes (left and right half, different normals and albedos), a miss band on top, noisy colour"""
    rng = np.random.default_rng(seed)
    normal = np.zeros((h, w, 3)); normal[:, : w // 2] = (0, 1, 0); normal[:, w // 2:] = (1, 0, 0)
    albedo = np.zeros((h, w, 3)); albedo[:, : w // 2] = (0.8, 0.2, 0.2); albedo[:, w // 2:] = (0.2, 0.2, 0.8)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    pos = np.stack([xs * 0.05, np.zeros_like(xs), ys * 0.05 + 2], axis=-1)
    t = np.full((h, w), 3.0)
    hit = np.ones((h, w), bool)
    hit[:4] = False
    albedo[~hit] = 0; normal[~hit] = 0
    color = np.clip(0.5 + 0.3 * rng.standard_normal((h, w, 3)), 0, None)
    color[~hit] = (0.1, 0.3, 0.9)
    return color, normal, pos, albedo, t, hit


ALL_INF = dict(sigma_color=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF)


def _b3_blur(c, iterations, valid=None):
    """the plain B3 a-trous blur with the image border handled by renormalisation (skipped taps)"""
    hgt, wid = c.shape[:2]
    for i in range(iterations):
        s = 1 << i
        out = np.zeros_like(c)
        for y in range(hgt):
            for x in range(wid):
                sw, acc = 0.0, np.zeros(3)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qy, qx = y + dy * s, x + dx * s
                        if 0 <= qy < hgt and 0 <= qx < wid and (valid is None or valid[qy, qx] == valid[y, x]):
                            w = dr.H[dx + 2] * dr.H[dy + 2]
                            sw += w
                            acc += w * c[qy, qx]
                out[y, x] = acc / sw
        c = out
    return c


def test_constant_image_stays_constant():
    color, normal, pos, albedo, t, hit = _scene()
    color[:] = (0.25, 0.5, 0.75)
    out = dr.atrous(color, normal, pos, albedo, t, hit, dict(iterations=5))
    assert np.allclose(out, color, rtol=1e-12, atol=0)


def test_all_sigmas_inf_is_the_plain_b3_blur():
    color, normal, pos, albedo, t, _ = _scene(16, 20)
    hit = np.ones(t.shape, bool)
    out = dr.atrous(color, normal, pos, albedo, t, hit, dict(ALL_INF, iterations=3))
    assert np.allclose(out, _b3_blur(color, 3), rtol=1e-12, atol=1e-15)


def test_non_finite_pixel_passes_through_and_does_not_leak():
    color, normal, pos, albedo, t, hit = _scene()
    color[10, 8] = (np.inf, np.inf, np.inf)
    color[12, 20] = (np.nan, 0.5, 0.5)
    out = dr.atrous(color, normal, pos, albedo, t, hit, dict(iterations=4))
    assert np.all(np.isposinf(out[10, 8]))
    assert np.isnan(out[12, 20, 0]) and np.all(out[12, 20, 1:] == 0.5)
    fin = np.ones(t.shape, bool)
    fin[10, 8] = fin[12, 20] = False
    assert np.all(np.isfinite(out[fin]))
    # the same as filtering an image in which those two pixels do not exist at all for their neighbours
    c2 = color.copy()
    c2[10, 8] = 1e6
    c2[12, 20] = -1e6
    ref = dr.atrous(c2, normal, pos, albedo, t, hit, dict(ALL_INF, iterations=1))
    got = dr.atrous(color, normal, pos, albedo, t, hit, dict(ALL_INF, iterations=1))
    assert not np.allclose(ref[fin], got[fin])  # (the big values do leak when they are finite)
    assert np.all(np.abs(got[fin]) < 10)


def test_nothing_crosses_a_hit_miss_boundary():
    color, normal, pos, albedo, t, hit = _scene()
    out = dr.atrous(color, normal, pos, albedo, t, hit, dict(ALL_INF, iterations=5))
    # the misses are a constant sky colour and only ever see each other: they stay exactly that colour
    assert np.allclose(out[~hit], (0.1, 0.3, 0.9), rtol=1e-12)
    # the hits never see the sky: the result equals the blur of the hit region alone
    ref = _b3_blur(color, 5, valid=hit)
    assert np.allclose(out[hit], ref[hit], rtol=1e-12, atol=1e-15)


def test_edges_of_the_guides_are_kept():
    """two halves of different normal and albedo: with the geometric terms on, the halves barely mix; with them off they do"""
    color, normal, pos, albedo, t, hit = _scene()
    color[hit] = 0.0
    color[:, 16:][hit[:, 16:]] = 1.0
    on = dr.atrous(color, normal, pos, albedo, t, hit, dict(sigma_color=INF, iterations=3))
    off = dr.atrous(color, normal, pos, albedo, t, hit, dict(ALL_INF, iterations=3))
    assert on[10, 15].max() < 1e-3 and on[10, 16].min() > 1 - 1e-3
    assert off[10, 15].max() > 0.1


def test_mean_color_is_the_f32_division():
    acc = np.array([[[1.0, 2.0, 3.0, 0.0], [np.inf, 0.1, 0.2, 0.0]]], np.float32)
    c = dr.mean_color(acc, 3)
    assert np.array_equal(c[0, 0], (np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), np.float32(1.0)))
    assert np.isposinf(c[0, 1, 0])


@pytest.mark.parametrize("params", [dict(sigma_color=5e-19, iterations=5), dict(sigma_color=1e-30, iterations=8), dict(sigma_normal=1e-20),
                                    dict(sigma_position=1e-20, iterations=8), dict(sigma_albedo=1e-20), dict(tiny_t=True)])
def test_tiny_sigma_keeps_every_pixel_finite(params):
    """a k that overflows f32 is clamped to FLT_MAX (include/rt_amd.h): the centre tap's zero distance weighs 1, not 0 x inf = NaN, and
    where every neighbour differs in the tiny-sigma feature no neighbour mixes in -- the output is the input.  (Before the clamp every
    hit pixel came out NaN, and with sigma_color = 5e-19 kc_4 = 4e36 x 256 overflowed on the fifth iteration.)  tiny_t: t_p = 1e-30 and
    the default sigma_position, where kx / t_p^2 overflows per pixel."""
    params = dict(params)
    color, normal, pos, albedo, t, hit = _scene(19, 37, seed=3)
    hit[:] = True
    rng = np.random.default_rng(5)
    # every pixel distinct from every other in every feature
    color = rng.uniform(0.1, 1.0, color.shape)
    normal = rng.standard_normal(normal.shape)
    pos = rng.uniform(-1, 1, pos.shape)
    albedo = rng.uniform(0, 1, albedo.shape)
    if params.pop("tiny_t", False):
        t = np.full(t.shape, 1e-30)
    key = [k for k in params if k.startswith("sigma")]
    # the other terms off, so that only the tiny sigma (or the tiny t) stands between the pixels
    others = {k: INF for k in ("sigma_color", "sigma_normal", "sigma_position", "sigma_albedo") if k not in key and (key or k != "sigma_position")}
    out = dr.atrous(color, normal, pos, albedo, t, hit, dict(others, **params))
    assert np.all(np.isfinite(out))
    assert np.allclose(out, color, rtol=1e-12, atol=0)
    # pixels identical in that feature still mix: a constant guide with the colour test off is the plain blur
    if key and key[0] != "sigma_color":
        feat = {"sigma_normal": normal, "sigma_position": pos, "sigma_albedo": albedo}[key[0]]
        feat[:] = feat[0, 0]
        out = dr.atrous(color, normal, pos, albedo, t, hit, dict(others, **params))
        assert np.allclose(out, _b3_blur(color, params.get("iterations", 5)), rtol=1e-12, atol=1e-15)


def test_overflowing_k_is_clamped_in_f32():
    fmax = float(np.finfo(np.float32).max)
    assert dr.k_of(1e-20) == dr.k_of(1e-30) == fmax and dr.k_of(INF) == 0 and dr.k_of(1e30) == 0
    assert dr.k_of(0.5) == 4.0 and dr.kc_of(dr.k_of(0.5), 3) == 256.0
    kc0 = dr.k_of(5e-19)
    assert kc0 < fmax and dr.kc_of(kc0, 3) < fmax and dr.kc_of(kc0, 4) == fmax  # 4e36 x 256 overflows
    assert np.all(dr.kx_of(100.0, np.array([1e-30, 0.0, 2.0])) == (fmax, fmax, 25.0))
