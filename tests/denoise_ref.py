"""numpy float64 restatement of rt_denoise (include/rt_amd.h), the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010 as this
library defines it.  A plain helper module of the test suite: tests/test_denoise_cpu.py holds its properties, tests/test_gpu_denoise.py
holds the kernel against it."""
import numpy as np

H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
DEFAULTS = dict(iterations=5, sigma_color=0.5, sigma_normal=0.25, sigma_position=0.1, sigma_albedo=0.1)


FLT_MAX = float(np.finfo(np.float32).max)


def clamp_k(k):
    """every k, in f32, clamped to FLT_MAX: an overflowing k does not turn the zero distance of the centre tap into NaN"""
    return np.minimum(np.float32(k), np.float32(FLT_MAX))


def k_of(sigma):
    """1 / sigma^2 as the host computes it (f32, clamped); sigma = inf -> 0"""
    s = np.float32(sigma)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        return float(clamp_k(np.float32(1) / (s * s)))


def kc_of(kc0, i):
    """iteration i's colour k: kc0 * 4^i as an f32 product, clamped"""
    with np.errstate(over="ignore"):
        return float(clamp_k(np.float32(kc0) * np.float32(4.0 ** i)))


def kx_of(kx, t):
    """the per-pixel position k: kx / t_p^2 in f32, clamped"""
    t = np.asarray(t, np.float32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        return clamp_k(np.float32(kx) / (t * t)).astype(np.float64)


def mean_color(acc, it):
    """c_p = acc_p.xyz / it in f32 (k_resolve's division)"""
    return (np.asarray(acc, np.float32)[..., :3] / np.float32(it)).astype(np.float64)


def positions(O, D, t):
    """the G-buffer's position feature: O + D * t in f32, not contracted (O, D: (n, 3) primary rays, t: n)"""
    O, D, t = np.asarray(O, np.float32), np.asarray(D, np.float32), np.asarray(t, np.float32)
    return O + D * t[..., None]


def atrous(color, normal, pos, albedo, t, hit, params=None):
    """The filter on an (h, w, 3) colour image with (h, w, 3) normal / position / albedo features, (h, w) t and hit mask.
    Returns the (h, w, 3) result in float64."""
    p = dict(DEFAULTS, **(params or {}))
    c = np.array(color, dtype=np.float64)
    n, x, a = (np.asarray(v, np.float64) for v in (normal, pos, albedo))
    t = np.asarray(t, np.float64)
    hit = np.asarray(hit, bool)
    hgt, wid = c.shape[:2]
    kc0, kn, kx, ka = k_of(p["sigma_color"]), k_of(p["sigma_normal"]), k_of(p["sigma_position"]), k_of(p["sigma_albedo"])
    kxp = np.where(hit, kx_of(kx, t), 0.0) if kx else np.zeros_like(t)
    for i in range(int(p["iterations"])):
        s = 1 << i
        kc = kc_of(kc0, i)
        fin = np.all(np.isfinite(c), axis=-1)
        sw = np.zeros((hgt, wid))
        acc = np.zeros((hgt, wid, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                # q = p + (ox, oy): the source window of every p whose tap lies inside the image
                ys, xs = slice(max(0, -oy), min(hgt, hgt - oy)), slice(max(0, -ox), min(wid, wid - ox))
                yq, xq = slice(max(0, oy), min(hgt, hgt + oy)), slice(max(0, ox), min(wid, wid + ox))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                cp, cq = c[ys, xs], c[yq, xq]
                ok = fin[ys, xs] & fin[yq, xq] & (hit[ys, xs] == hit[yq, xq])
                with np.errstate(invalid="ignore", over="ignore"):
                    e = np.sum((cp - cq) ** 2, axis=-1) * kc if kc else np.zeros(ok.shape)
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
                acc[ys, xs] += w[..., None] * np.where(ok[..., None], cq, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.where(fin[..., None], acc / sw[..., None], c)
    return c


def denoise(acc, it, aov, pos, params=None):
    """rt_denoise from the float4 accumulator, the iteration count, the G-buffer as HostRenderer.aovs() returns it and the positions
    (positions()); float64 (h, w, 3)"""
    hit = aov["obj"] != -1
    return atrous(mean_color(acc, it), aov["normal"], np.asarray(pos).reshape(aov["normal"].shape), aov["albedo"], aov["t"], hit, params)
