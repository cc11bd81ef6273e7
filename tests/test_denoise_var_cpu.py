"""The variance-guided denoiser without a GPU: the C ABI's entry point exists and checks its arguments, the numpy restatement of the
filter (tests/denoise_var_ref.py) has the properties its definition promises, and on the oracle's own samples it improves an adaptively
sampled frame -- the evidence that the device test of the same experiment (tests/test_gpu_denoise_var.py) can be met."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import denoise_ref as dr  # noqa: E402
import denoise_var_ref as dv  # noqa: E402
from test_adaptive_cpu import QUALITY  # noqa: E402

F32 = np.float32
INF = float("inf")
ALL_INF = dict(sigma_luminance=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF)
SUM_H2 = float((dr.H ** 2).sum())  # 70 / 256


# ---- the C ABI, as far as it goes without a device ----
def test_symbols_exported(host_api):
    assert "rt_denoise_variance" in host_api.RT_SYMBOLS
    assert hasattr(host_api.rt_lib(), "rt_denoise_variance")
    assert hasattr(host_api.host_lib(), "rth_renderer_set_denoise_variance")


@pytest.mark.parametrize("bad", [dict(iterations=0), dict(iterations=9), dict(iterations=-1), dict(sigma_luminance=0.0), dict(sigma_normal=-1.0),
                                 dict(sigma_position=float("nan")), dict(sigma_albedo=0.0), dict(sigma_luminance=-INF), dict(epsilon=0.0),
                                 dict(epsilon=-1e-4), dict(epsilon=float("nan"))])
def test_bad_params_are_argument_errors(host_api, bad):
    """The parameters are checked before the context: without a GPU (null context) the error names the parameter"""
    L = host_api.rt_lib()
    p = host_api.denoise_var_params(bad)
    assert L.rt_denoise_variance(None, C.byref(p)) == host_api.RT_E_ARG
    msg = L.rt_last_error(None).decode()
    assert "iterations" in msg or "sigma" in msg or "epsilon" in msg, msg


def test_good_params_reach_the_context_check(host_api):
    L = host_api.rt_lib()
    for p in (None, host_api.denoise_var_params(dict(ALL_INF, iterations=8)), host_api.denoise_var_params(dict(epsilon=INF))):
        assert L.rt_denoise_variance(None, C.byref(p) if p is not None else None) == host_api.RT_E_ARG
        assert "null context" in L.rt_last_error(None).decode()


def test_defaults_agree_everywhere(host_api):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rt_amd.h")).read()
    line = [l for l in hdr.splitlines() if l.startswith("#define RT_DENOISE_VAR_DEFAULTS")][0]
    vals = [float(v.strip().rstrip("f")) for v in line.split("{")[1].split("}")[0].split(",")]
    keys = ["iterations", "sigma_luminance", "sigma_normal", "sigma_position", "sigma_albedo", "epsilon"]
    assert dict(zip(keys, vals)) == host_api.DENOISE_VAR_DEFAULTS == dv.DEFAULTS


# ---- the restatement on crafted frames ----
def _flat(h, w):
    """a G-buffer without edges: one plane seen at one distance, every feature equal in every pixel"""
    normal = np.tile(np.array([0.0, 1.0, 0.0]), (h, w, 1))
    albedo = np.tile(np.array([0.5, 0.5, 0.5]), (h, w, 1))
    return dict(normal=normal, pos=np.zeros((h, w, 3)), albedo=albedo, t=np.ones((h, w)), hit=np.ones((h, w), bool))


def _run(color, var, g, params, valid=None, trace=None):
    valid = np.ones(var.shape, bool) if valid is None else valid
    return dv.atrous(color, var, valid, g["normal"], g["pos"], g["albedo"], g["t"], g["hit"], params, trace)


def _border_sums(n, s):
    """per coordinate 0 .. n-1: the sum of h and of h^2 over the taps at step s that lie inside"""
    a, b = np.zeros(n), np.zeros(n)
    for d in range(-2, 3):
        inside = (np.arange(n) + d * s >= 0) & (np.arange(n) + d * s < n)
        a += np.where(inside, dr.H[d + 2], 0.0)
        b += np.where(inside, dr.H[d + 2] ** 2, 0.0)
    return a, b


def test_constant_image_keeps_its_colour_and_scales_its_variance():
    h, w, v0 = 72, 80, 0.37
    color = np.tile(np.array([0.3, 0.6, 0.1]), (h, w, 1))
    trace = []
    c, v = _run(color, np.full((h, w), v0), _flat(h, w), dict(iterations=3), trace=trace)
    assert np.allclose(c, color, rtol=0, atol=1e-15)
    # every weight is h[dx] h[dy] (all exponents 0): the first iteration everywhere, the border included, in closed form
    ay, by = _border_sums(h, 1)
    ax, bx = _border_sums(w, 1)
    want = v0 * np.outer(by, bx) / np.outer(ay, ax) ** 2
    assert np.allclose(trace[0][1], want, rtol=1e-13)
    # away from the border (2 (1 + 2 + 4) = 14 pixels after three iterations) sum w = 1 and sum w^2 = (70 / 256)^2 per iteration
    for i in range(3):
        m = 2 * ((1 << (i + 1)) - 1)
        assert np.allclose(trace[i][1][m:h - m, m:w - m], v0 * SUM_H2 ** (2 * (i + 1)), rtol=1e-13)
    assert np.allclose(v[14:-14, 14:-14], v0 * SUM_H2 ** 6, rtol=1e-13)


def _step(h=24, w=32):
    color = np.zeros((h, w, 3))
    color[:, : w // 2], color[:, w // 2:] = 0.2, 0.8
    return color


def test_step_edge_without_variance_is_preserved_exactly():
    color = _step()
    c, v = _run(color, np.zeros(color.shape[:2]), _flat(*color.shape[:2]), dict(iterations=5, epsilon=1e-6))
    # kl = 1 / epsilon = 1e6: a tap across the edge weighs exp(-0.6e6) = 0, the others average equal values
    assert np.allclose(c, color, rtol=0, atol=1e-15) and np.all(v == 0)


def test_step_edge_with_a_large_variance_is_smoothed():
    color = _step()
    h, w = color.shape[:2]
    c, v = _run(color, np.ones((h, w)), _flat(h, w), dict(iterations=5, epsilon=1e-6))
    # kl = 1 / 4: a tap across the edge weighs exp(-0.15): the two sides run into each other
    assert c[h // 2, w // 2 - 1, 0] > 0.3 and c[h // 2, w // 2, 0] < 0.7
    assert np.all(c[..., 0] > 0.2) and np.all(c[..., 0] < 0.8)
    assert np.all(v < 1) and np.all(v > 0)


def _moments(h, w, n, y, spread=0.0):
    """(acc, count, sum_y, sum_yy) of a grey image whose every pixel got n samples y +- spread (alternating)"""
    s = np.empty((n, h, w, 3), F32)
    s[0::2], s[1::2] = F32(y + spread), F32(y - spread)
    cnt, sy, syy = ar.moments(s)
    acc = np.zeros((h, w, 4), F32)
    for f in range(n):
        acc[..., :3] += s[f]
    return acc, cnt, sy, syy


def _aov(g):
    return dict(obj=np.where(g["hit"], 0, -1), normal=g["normal"], albedo=g["albedo"], t=g["t"])


def test_empty_pixel_stays_black_and_pulls_nothing():
    h, w = 16, 20
    acc, cnt, sy, syy = _moments(h, w, 4, 0.5, 0.25)
    cnt[7, 9] = 0
    acc[7, 9] = 1e6  # whatever the accumulator holds there
    g = _flat(h, w)
    out = dv.denoise(acc, cnt, sy, syy, _aov(g), g["pos"], dict(iterations=3))
    assert np.all(out[7, 9] == 0)
    rest = np.ones((h, w), bool)
    rest[7, 9] = False
    assert np.allclose(out[rest][:, :3], 0.5, rtol=0, atol=1e-12) and np.all(out[rest][:, 3] > 0)
    # the variance around the hole is the closed form over the taps that are left (first iteration, all weights h h)
    one = dv.denoise(acc, cnt, sy, syy, _aov(g), g["pos"], dict(iterations=1))
    v0 = float(dv.inputs(acc, cnt, sy, syy)[1][0, 0])
    hh = np.outer(dr.H, dr.H)
    assert np.isclose(one[7, 10, 3], v0 * ((hh ** 2).sum() - hh[2, 1] ** 2) / (1 - hh[2, 1]) ** 2, rtol=1e-12)
    assert np.isclose(one[7, 13, 3], v0 * (hh ** 2).sum(), rtol=1e-12)  # out of the hole's reach


@pytest.mark.parametrize("where", ["acc", "sum_y", "sum_yy"])
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_non_finite_pixel_passes_through_and_pulls_nothing(where, bad):
    h, w = 16, 20
    acc, cnt, sy, syy = _moments(h, w, 4, 0.5, 0.25)
    if where == "acc":
        acc[7, 9, 1] = bad
    elif where == "sum_y":
        sy[7, 9] = bad
    else:
        syy[7, 9] = bad
    g = _flat(h, w)
    out = dv.denoise(acc, cnt, sy, syy, _aov(g), g["pos"], dict(iterations=3))
    want = (acc[7, 9, :3] / F32(4)).astype(np.float64)  # c_p as it is
    assert np.array_equal(out[7, 9, :3], want, equal_nan=True) and out[7, 9, 3] == 0
    rest = np.ones((h, w), bool)
    rest[7, 9] = False
    assert np.isfinite(out[rest]).all() and np.allclose(out[rest][:, :3], 0.5, rtol=0, atol=1e-12)


def test_overflowing_kl_and_variance_are_clamped():
    """epsilon 1e-40 on a zero variance: kl = FLT_MAX, not inf -- the centre tap weighs exp(0) and a constant image stays what it is;
    one huge single sample (y^2 overflows f32): v is FLT_MAX, so a tap of weight 0 adds 0 and nothing turns NaN"""
    h, w = 12, 16
    g = _flat(h, w)
    color = _step(h, w)
    c, v = _run(color, np.zeros((h, w)), g, dict(iterations=3, epsilon=1e-40))
    assert np.array_equal(c, color) and np.all(v == 0)
    acc, cnt, sy, syy = _moments(h, w, 4, 0.5, 0.25)
    acc[5, 6, :3], cnt[5, 6] = 3e19, 1
    sy[5, 6], syy[5, 6] = 3e19, 3e38
    ci, vi, empty, passed = dv.inputs(acc, cnt, sy, syy)
    assert not passed.any() and vi[5, 6] == np.finfo(F32).max
    out = dv.denoise(acc, cnt, sy, syy, _aov(g), g["pos"], dict(iterations=3))
    assert np.isfinite(out).all() and np.all(out[..., 3] <= float(np.finfo(F32).max))


def test_inputs_follow_the_header_in_f32():
    rng = np.random.default_rng(5)
    n = 200
    cnt = rng.integers(0, 40, n).astype(np.uint32)
    cnt[:4] = (0, 1, 1, 2)
    acc = (rng.random((n, 4)) * cnt[:, None]).astype(F32)
    sy = (rng.random(n) * cnt).astype(F32)
    syy = (sy * sy / np.maximum(cnt, 1) * (1 + rng.random(n))).astype(F32)
    c, v, empty, passed = dv.inputs(acc, cnt, sy, syy)
    assert c.dtype == F32 and v.dtype == F32 and not passed.any() and np.array_equal(empty, cnt == 0)
    for i in range(n):
        if cnt[i] == 0:
            assert np.all(c[i] == 0) and v[i] == 0
            continue
        k = F32(cnt[i])
        ci = acc[i, :3] / k
        assert np.array_equal(c[i], ci)
        y = F32(F32(F32(0.2126) * ci[0]) + F32(F32(0.7152) * ci[1])) + F32(F32(0.0722) * ci[2])
        if cnt[i] == 1:
            assert v[i] == F32(y * y)  # one sample: its own square
        else:
            m = F32(sy[i] / k)
            s = F32(F32(syy[i] - F32(sy[i] * m)) / F32(k - F32(1)))
            s = s if s > 0 else F32(0)
            assert v[i] == F32(s / k)
    # the square root of v is the e of rt_select_active (d = floor = 1 where the mean is below it)
    two = cnt >= 2
    small = two & (sy / np.maximum(cnt, 1) <= 1)
    assert np.array_equal(np.sqrt(v[small]), ar.relative_error(cnt[small], sy[small], syy[small], 1.0))


def test_hit_and_miss_never_mix():
    h, w = 20, 24
    color = _step(h, w)
    g = _flat(h, w)
    g["hit"][:, w // 2:] = False
    c, v = _run(color, np.ones((h, w)), g, dict(ALL_INF, iterations=5))
    assert np.allclose(c, color, rtol=0, atol=1e-15)
    # ... and the variance prefilter stays on its side too: a huge variance on the miss side does not loosen the hit side's edge stop
    var = np.where(g["hit"], 0.0, 1e6)
    color[:, : w // 4] = 0.1
    c, v = _run(color, var, g, dict(iterations=4, epsilon=1e-6))
    assert np.allclose(c, color, rtol=0, atol=1e-15)


def test_equal_counts_and_no_luminance_term_is_rt_denoise_without_its_colour_term():
    rng = np.random.default_rng(9)
    h, w, n = 24, 32, 8
    normal = np.zeros((h, w, 3)); normal[:, : w // 2] = (0, 1, 0); normal[:, w // 2:] = (1, 0, 0)
    albedo = rng.random((h, w, 3)).round(1)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    pos = np.stack([xs * 0.05, np.zeros_like(xs), ys * 0.05 + 2], axis=-1)
    t = np.full((h, w), 3.0)
    hit = np.ones((h, w), bool)
    hit[:4] = False
    acc = np.zeros((h, w, 4), F32)
    acc[..., :3] = rng.random((h, w, 3)) * n
    acc[5, 5, 0], acc[2, 20, 2] = np.inf, np.nan
    cnt = np.full((h, w), n, np.uint32)
    sy = (ar.luminance(acc) * F32(1)).astype(F32)
    sy = np.where(np.isfinite(sy), sy, F32(1))  # (the passed-through pixels are the ones whose COLOUR is not finite, as rt_denoise's)
    syy = (sy * sy).astype(F32)
    aov = dict(obj=np.where(hit, 3, -1), normal=normal, albedo=albedo, t=t)
    for it in (1, 5):
        mine = dv.denoise(acc, cnt, sy, syy, aov, pos, dict(iterations=it, sigma_luminance=INF))
        theirs = dr.atrous(dr.mean_color(acc, n), normal, pos, albedo, t, hit, dict(iterations=it, sigma_color=INF))
        assert np.allclose(mine[..., :3], theirs, rtol=1e-13, atol=0, equal_nan=True)


# ---- what the filter buys on an adaptively sampled frame ----
def adaptive_state(samples, params, budget):
    """adaptive_ref.adaptive_loop, and with it the f32 accumulator and statistics a device would hold: a pixel's samples are frames
    0 .. count - 1 (a pixel that has stopped does not start again: its statistics no longer change), added in frame order"""
    _, cnt, total = ar.adaptive_loop(samples, budget, **params)
    acc = np.zeros(cnt.shape + (4,), F32)
    sy, syy = np.zeros(cnt.shape, F32), np.zeros(cnt.shape, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(int(cnt.max())):
            on = cnt > f
            acc[on, :3] += samples[f][on][..., :3]
            _, sy[on], syy[on] = ar.moments(samples[f:f + 1][:, on], None, sy[on], syy[on])
    return acc, cnt, sy, syy, total


def quality_ratio(den, acc, cnt, reference):
    """MSE of the denoised frame over MSE of the raw per-count mean, against 'reference', on the pixels finite in all three"""
    with np.errstate(all="ignore"):
        raw = acc[..., :3].astype(np.float64) / cnt[..., None]
    fin = np.isfinite(reference).all(-1) & np.isfinite(raw).all(-1) & np.isfinite(den[..., :3]).all(-1)
    mse_d = ((den[..., :3][fin] - reference[fin]) ** 2).mean()
    mse_r = ((raw[fin] - reference[fin]) ** 2).mean()
    return float(mse_d / mse_r), int(fin.sum())


def test_denoised_adaptive_frame_beats_the_raw_one_on_the_oracle(scenes, oracle_api):
    """tests/test_adaptive_cpu.py's experiment (BASELINE config 2's scene at 320 x 180, 16 whole frames, then threshold 0.02 up to 32
    frames' worth of samples, a 256-frame mean of other frames as the truth), its frame then filtered by the restatement with
    RT_DENOISE_VAR_DEFAULTS on the oracle's own G-buffer (t_min 0.001).
    Oracle result: MSE denoised / raw adaptive = 0.352 (1,840,125 samples, counts 16 .. 59, 38,990 pixels finite in all three).  Asserted: < 1."""
    from test_gpu_denoise import Recorder
    q = QUALITY
    w, h = q["width"], q["height"]
    o = oracle_api.OracleScene()
    rec = Recorder(o)
    getattr(scenes, q["scene"])(rec)
    o.set_raytracer(False)
    r = oracle_api.OracleRenderer(o, w, h)
    S = np.zeros((q["stack_frames"], h, w, 3), F32)
    for f in range(q["stack_frames"]):
        r.clear()
        r.render(f, 1, nthreads=0)
        S[f] = r.accumulator()[..., :3]
    r.clear()
    r.render(q["reference_frame0"], q["reference_frames"], nthreads=0)
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
    O, D = r.primary_rays()
    hits = o.find_nearest(O, D, None, 0.001)
    r.close()
    obj, mat = hits["obj"].reshape(h, w), hits["mat"].reshape(h, w)
    aov = dict(obj=obj, normal=hits["normal"].reshape(h, w, 3), t=hits["t"].reshape(h, w), albedo=rec.albedo(obj, mat))
    pos = dv.positions(O, D, hits["t"].reshape(-1))
    o.close()
    acc, cnt, sy, syy, total = adaptive_state(S, q["params"], q["budget_frames"] * w * h)
    assert cnt.max() < q["stack_frames"], "the loop ran out of recorded frames"
    den = dv.denoise(acc, cnt, sy, syy, aov, pos, None)
    ratio, finite = quality_ratio(den, acc, cnt, ref)
    print("oracle denoised / raw adaptive MSE ratio %.3f, %d samples, counts %d .. %d, %d finite pixels" % (ratio, total, cnt.min(), cnt.max(), finite))
    assert ratio < 1, ratio
