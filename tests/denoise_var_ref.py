"""numpy restatement of rt_denoise_variance (include/rt_amd.h): the variance-guided a-trous filter of an adaptively sampled frame (the
spatial half of SVGF, Schied et al. 2017) as this library defines it.  A plain helper module of the test suite:
tests/test_denoise_var_cpu.py holds its properties, tests/test_gpu_denoise_var.py holds the kernels against it.

The per-pixel inputs (mean colour, luminance, variance of the mean) are computed in f32 operation by operation as the header writes them;
the iterations run in float64 on those f32 values."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from denoise_ref import FLT_MAX, H, k_of, kx_of, positions  # noqa: E402,F401  (positions: re-exported for the callers)

F32 = np.float32
K3 = np.array([1 / 4, 1 / 2, 1 / 4])
DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.25, sigma_position=0.1, sigma_albedo=0.1, epsilon=1e-4)


def luminance(c):
    """(0.2126 r + 0.7152 g) + 0.0722 b in the array's own precision (f32 in: one rounding per operation)"""
    t = c.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        return (t(F32(0.2126)) * c[..., 0] + t(F32(0.7152)) * c[..., 1]) + t(F32(0.0722)) * c[..., 2]


def inputs(acc, count, sum_y, sum_yy):
    """(c, v, empty, passed): the f32 mean colour (h, w, 3), the f32 variance of the mean luminance (h, w) and the two masks of pixels
    that are not filtered and are no tap of any neighbour"""
    a = np.asarray(acc, F32)[..., :3]
    count = np.asarray(count, np.uint32)
    sy, syy = np.asarray(sum_y, F32), np.asarray(sum_yy, F32)
    empty = count == 0
    with np.errstate(all="ignore"):
        n = count.astype(F32)
        c = (a / n[..., None]).astype(F32)
        y = luminance(c).astype(F32)
        m = (sy / n).astype(F32)
        s = ((syy - (sy * m).astype(F32)).astype(F32) / (n - F32(1)).astype(F32)).astype(F32)
        s = np.where(s > F32(0), s, F32(0)).astype(F32)
        v = np.where(count >= 2, (s / n).astype(F32), (y * y).astype(F32)).astype(F32)
        v = np.minimum(v, F32(FLT_MAX))  # clamped: a tap of weight 0 then adds 0, not 0 x inf
    passed = ~empty & ~(np.isfinite(c).all(-1) & np.isfinite(sy) & np.isfinite(syy))
    c = np.where(empty[..., None], F32(0), c).astype(F32)
    v = np.where(empty | passed, F32(0), v).astype(F32)
    return c, v, empty, passed


def _windows(hgt, wid, oy, ox):
    """slices of the pixels p whose tap q = p + (ox, oy) lies inside the image, and of those taps"""
    ys, xs = slice(max(0, -oy), min(hgt, hgt - oy)), slice(max(0, -ox), min(wid, wid - ox))
    yq, xq = slice(max(0, oy), min(hgt, hgt + oy)), slice(max(0, ox), min(wid, wid + ox))
    return ys, xs, yq, xq


def prefilter(v, valid, hit):
    """g: the 3 x 3 (1/4, 1/2, 1/4)^2 mean of v at ONE pixel distance over valid taps of the pixel's own hit class, normalised by the
    weights used (0 where the pixel itself is not valid)"""
    hgt, wid = v.shape
    sw, sv = np.zeros((hgt, wid)), np.zeros((hgt, wid))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs, yq, xq = _windows(hgt, wid, dy, dx)
            if ys.start >= ys.stop or xs.start >= xs.stop:
                continue
            ok = valid[ys, xs] & valid[yq, xq] & (hit[ys, xs] == hit[yq, xq])
            k = K3[dx + 1] * K3[dy + 1]
            sw[ys, xs] += np.where(ok, k, 0.0)
            sv[ys, xs] += np.where(ok, k * np.where(ok, v[yq, xq], 0.0), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(valid, sv / sw, 0.0)


def atrous(color, var, valid, normal, pos, albedo, t, hit, params=None, trace=None):
    """The iterations on an (h, w, 3) colour image and its (h, w) variance; 'valid' marks the pixels that are filtered and may be taps.
    Returns (colour (h, w, 3), variance (h, w)) in float64; pixels that are not valid keep their colour, their variance is 0.
    trace: a list that receives (colour, variance) after every iteration."""
    p = dict(DEFAULTS, **(params or {}))
    c = np.array(color, dtype=np.float64)
    v = np.where(valid, np.asarray(var, np.float64), 0.0)
    n, x, a = (np.asarray(u, np.float64) for u in (normal, pos, albedo))
    t = np.asarray(t, np.float64)
    hit, valid = np.asarray(hit, bool), np.asarray(valid, bool)
    hgt, wid = v.shape
    kn, kx, ka = k_of(p["sigma_normal"]), k_of(p["sigma_position"]), k_of(p["sigma_albedo"])
    kxp = np.where(hit, kx_of(kx, t), 0.0) if kx else np.zeros_like(t)
    sl, eps = float(F32(p["sigma_luminance"])), float(F32(p["epsilon"]))
    for i in range(int(p["iterations"])):
        s = 1 << i
        y = luminance(c)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            kl = np.minimum(1.0 / (sl * np.sqrt(prefilter(v, valid, hit)) + eps), FLT_MAX) if np.isfinite(sl) else np.zeros((hgt, wid))
        sw, sc, sv = np.zeros((hgt, wid)), np.zeros((hgt, wid, 3)), np.zeros((hgt, wid))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ys, xs, yq, xq = _windows(hgt, wid, dy * s, dx * s)
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                ok = valid[ys, xs] & valid[yq, xq] & (hit[ys, xs] == hit[yq, xq])
                with np.errstate(invalid="ignore", over="ignore"):
                    e = np.where(kl[ys, xs] != 0, np.abs(y[ys, xs] - y[yq, xq]) * kl[ys, xs], 0.0)
                    geo = np.zeros(ok.shape)
                    if kn:
                        geo += np.sum((n[ys, xs] - n[yq, xq]) ** 2, axis=-1) * kn
                    if kx:
                        geo += np.sum((x[ys, xs] - x[yq, xq]) ** 2, axis=-1) * kxp[ys, xs]
                    if ka:
                        geo += np.sum((a[ys, xs] - a[yq, xq]) ** 2, axis=-1) * ka
                    e = e + np.where(hit[ys, xs], geo, 0.0)
                    w = np.where(ok, H[dx + 2] * H[dy + 2] * np.exp(-np.where(ok, e, 0.0)), 0.0)
                sw[ys, xs] += w
                sc[ys, xs] += w[..., None] * np.where(ok[..., None], c[yq, xq], 0.0)
                sv[ys, xs] += w * w * np.where(ok, v[yq, xq], 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(valid[..., None], sc / sw[..., None], c)
            v = np.where(valid, np.minimum(sv / (sw * sw), FLT_MAX), 0.0)
        if trace is not None:
            trace.append((c.copy(), v.copy()))
    return c, v


def denoise(acc, count, sum_y, sum_yy, aov, pos, params=None):
    """rt_denoise_variance from the float4 accumulator, the statistics, the G-buffer as HostRenderer.aovs() returns it and the positions
    (positions()); float64 (h, w, 4): the filtered colour and, in w, the filtered variance (0 for an empty or passed-through pixel)"""
    c, v, empty, passed = inputs(acc, count, sum_y, sum_yy)
    hit = aov["obj"] != -1
    shape = aov["normal"].shape
    cc, vv = atrous(c, v, ~(empty | passed), aov["normal"], np.asarray(pos).reshape(shape), aov["albedo"], aov["t"], hit, params)
    return np.concatenate([cc, vv[..., None]], axis=-1)
