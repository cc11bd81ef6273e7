"""The two kernels every displayed frame passes through after the trace, on crafted frames: k_resolve (rt_resolve, rt_resolve_denoised)
against tests/resolve_ref.py bit for bit, and k_denoise_atrous (rt_denoise) against tests/denoise_ref.py on shapes that cut its 32 x 8
tile, every iteration count, non-finite, negative and huge colours and extreme sigmas.  Chosen values reach the kernels through
rt_bind_accumulator: the accumulator is a torch tensor filled from numpy, which this module also holds to what binding means."""
import os
import sys
import zlib

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dr  # noqa: E402
import resolve_ref as rr  # noqa: E402
import support as sp  # noqa: E402

pytestmark = pytest.mark.gpu

RADIANCE_TOL = 1e-4
INF = float("inf")


class Bound:
    """an (h, w, 4) float32 torch tensor bound as a renderer's accumulator; kept alive until the renderer is closed"""
    def __init__(self, r):
        import torch
        self.torch, self.r = torch, r
        self.t = torch.zeros((r.hgt, r.w, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.bind_accumulator(self.t.data_ptr())

    def fill(self, arr):
        self.t.copy_(self.torch.from_numpy(np.ascontiguousarray(arr, np.float32).reshape(self.r.hgt, self.r.w, 4)))
        self.torch.cuda.synchronize()

    def read(self):
        """the tensor's contents through torch, after the renderer's stream has finished"""
        self.r.synchronize()
        self.torch.cuda.synchronize()
        return self.t.cpu().numpy()


def make(scenes, host_api, name, w, h, oracle_api=None):
    """a renderer of scene name (and its oracle twin when oracle_api is given: the primary rays the positions are restated from)"""
    fn = getattr(scenes, name)
    r = host_api.HostRenderer(w, h)
    d = fn(r.scene) or {}
    r.commit()
    orr = None
    if oracle_api is not None:
        o = oracle_api.OracleScene()
        fn(o)
        orr = oracle_api.OracleRenderer(o, w, h)
    if "camera" in d:
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        if orr is not None:
            orr.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return r, orr


# ---- what binding an accumulator means ----
def test_bind_reports_the_address(host_api):
    r = host_api.HostRenderer(33, 9)
    assert r.accumulator_device_ptr()
    b = Bound(r)
    assert r.accumulator_device_ptr() == b.t.data_ptr()
    r.close()


def _render(r, host_api, how):
    if how == "whitted":
        r.render(host_api.RT_MODE_WHITTED, 0, 1)
    elif how == "rows":  # two shards, as two ranks of a row-interleaved split would render them
        r.render_rows(host_api.RT_MODE_PATH, 0, 2, 0, 2, (r.hgt + 1) // 2)
        r.render_rows(host_api.RT_MODE_PATH, 0, 2, 1, 2, r.hgt // 2)
    else:
        r.render(host_api.RT_MODE_PATH, 0, 3)


@pytest.mark.parametrize("how,stream", [("path", "1"), ("path", "0"), ("whitted", "1"), ("rows", "1")])
def test_bound_render_equals_owned(how, stream, scenes, host_api, monkeypatch):
    sp.clean_env(monkeypatch, {"RT_STREAM": stream})
    a, _ = make(scenes, host_api, "mixed_small", 64, 40)
    b, _ = make(scenes, host_api, "mixed_small", 64, 40)
    t = Bound(b)
    _render(a, host_api, how)
    _render(b, host_api, how)
    ref = a.accumulator()
    assert np.any(ref[..., :3] != 0)
    assert sp.same(b.accumulator(), ref)
    assert sp.same(t.read(), ref)  # the rendering is in the tensor itself
    a.close(), b.close()


def test_bind_after_render_and_rebind(scenes, host_api):
    """binding after the owned buffer was used: the next render lands in the tensor, from zero; after rebinding to a second tensor the
    first is never written again; closing the renderer leaves the caller's memory alone"""
    r, _ = make(scenes, host_api, "mixed_small", 64, 40)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    owned = r.accumulator()
    t1 = Bound(r)
    assert np.all(t1.read() == 0) and np.all(r.accumulator() == 0)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    first = t1.read()
    assert sp.same(first, owned)
    t2 = Bound(r)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    assert sp.same(t2.read(), owned)
    r.render(host_api.RT_MODE_PATH, 2, 2)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 4, 1)
    assert sp.same(t1.read(), first)
    last = t2.read()
    assert not sp.same(last, first)
    r.close()
    t2.torch.cuda.synchronize()
    assert sp.same(t2.t.cpu().numpy(), last) and sp.same(t1.t.cpu().numpy(), first)


def test_clear_zeroes_bound_memory(scenes, host_api):
    r, _ = make(scenes, host_api, "mixed_small", 33, 9)
    t = Bound(r)
    t.fill(rr.pixels(rr.crafted_values(), 33 * 9))
    r.clear()
    assert np.all(sp.bits(t.read()) == 0)
    r.close()


def test_reads_never_write_bound_memory(scenes, host_api):
    """rt_download_accumulator, rt_resolve and rt_denoise read the tensor's values (NaN payloads included) and leave its bits alone"""
    w, h = 33, 9
    r, _ = make(scenes, host_api, "mixed_small", w, h)
    t = Bound(r)
    px = rr.pixels(rr.crafted_values(), w * h).reshape(h, w, 4)
    t.fill(px)
    assert sp.same(r.accumulator(), px)
    assert np.array_equal(r.resolve(3), rr.resolve(px, 3))
    r.render_aovs(0.001)
    r.denoise(3)
    r.resolve_denoised()
    r.denoise(1, dict(iterations=8, sigma_color=INF))
    assert sp.same(t.read(), px)
    r.close()


# ---- k_resolve against the restatement ----
_VALUES = []


def _values():
    if not _VALUES:
        _VALUES.append(rr.value_set())
    return _VALUES[0]


def _row_ranges(h):
    out = [(0, h), (0, 1), (h - 1, h)]
    if h > 2:
        out.append((h // 3, max(h // 3 + 1, 2 * h // 3)))
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (255, 1), (257, 3), (33, 9), (1920, 1080)])
def test_resolve_equals_the_restatement(w, h, host_api):
    """uint32 equality on full frames and row ranges (the 256-lane tail, the first-pixel offset) for every frame count, negative ones
    included; the 1080p frame holds the whole value set, the small ones a window of the crafted values per fill"""
    r = host_api.HostRenderer(w, h)
    t = Bound(r)
    vals = _values() if w * h >= len(_values()) else rr.crafted_values()
    n = w * h
    fills = 1 if n >= len(vals) else min(8, -(-len(vals) // n))
    allpx = rr.pixels(vals, max(n * fills, len(vals)) if n < len(vals) else n)
    for f in range(fills):
        px = allpx[f * n:(f + 1) * n].reshape(h, w, 4)
        t.fill(px)
        for it in rr.ITS:
            ref = rr.resolve(px, it)
            for y0, y1 in _row_ranges(h):
                got = r.resolve(it, y0, y1)
                bad = np.argwhere(got != ref[y0:y1])
                assert bad.size == 0, "it %d rows [%d, %d): %d pixels differ, first at %s" % (it, y0, y1, len(bad), bad[0])
    out = np.zeros((h, w), np.uint32)
    assert host_api.rt_lib().rt_resolve(r.ctx, 0, 0, h, host_api._p(out)) == host_api.RT_E_ARG
    assert sp.same(t.read(), px)
    r.close()


# ---- the row range [y0, y1) of every entry point that takes one ----
def test_every_row_range_is_checked_alike(scenes, host_api):
    """the seven entry points that take rows [y0, y1) share one range check: a range outside the frame, an empty or a reversed one, and a
    null output where one is required, is RT_E_ARG and writes nothing; the last row alone is served by each"""
    w, h = 33, 9
    r, _ = make(scenes, host_api, "mixed_small", w, h)
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    r.render_aovs(0.001)
    r.denoise(2)
    L = host_api.rt_lib()

    def buf(dtype, *tail):  # a row more than the frame, so that rows [0, h + 1) would fit
        a = np.zeros((h + 1, w) + tail, dtype)
        a.view(np.uint8)[...] = 0xA5
        return a

    # (name, the call on (y0, y1, outputs), the output arrays, whether a null output is an error)
    entries = [
        ("rt_download_accumulator", lambda y0, y1, o: L.rt_download_accumulator(r.ctx, y0, y1, *o), [buf(np.float32, 4)], True),
        ("rt_resolve", lambda y0, y1, o: L.rt_resolve(r.ctx, 2, y0, y1, *o), [buf(np.uint32)], True),
        ("rt_download_aovs", lambda y0, y1, o: L.rt_download_aovs(r.ctx, y0, y1, *o), [buf(host_api.RT_HIT_DTYPE), buf(np.float32, 3)], False),
        ("rt_download_denoised", lambda y0, y1, o: L.rt_download_denoised(r.ctx, y0, y1, *o), [buf(np.float32, 4)], True),
        ("rt_resolve_denoised", lambda y0, y1, o: L.rt_resolve_denoised(r.ctx, y0, y1, *o), [buf(np.uint32)], True),
        ("rt_download_stats", lambda y0, y1, o: L.rt_download_stats(r.ctx, y0, y1, *o), [buf(np.uint32), buf(np.float32), buf(np.float32)], False),
        ("rt_resolve_adaptive", lambda y0, y1, o: L.rt_resolve_adaptive(r.ctx, y0, y1, *o), [buf(np.uint32)], True),
    ]
    for name, call, outs, null_is_error in entries:
        ptrs = [host_api._p(a) for a in outs]
        for y0, y1 in [(-1, 1), (0, h + 1), (2, 2), (3, 2)]:
            assert call(y0, y1, ptrs) == host_api.RT_E_ARG, "%s rows [%d, %d)" % (name, y0, y1)
        if null_is_error:
            assert call(0, h, [None] * len(outs)) == host_api.RT_E_ARG, name + ": null output"
        r.synchronize()
        assert all(np.all(a.view(np.uint8) == 0xA5) for a in outs), name + ": a refused call wrote"
        assert call(h - 1, h, ptrs) == 0, name + ": the last row"  # RT_OK
        for a in outs:  # one row arrived, at the start of the output, and nothing after it
            row = a.view(np.uint8).reshape(h + 1, -1)
            assert np.any(row[0] != 0xA5) and np.all(row[1:] == 0xA5), name + ": the last row's output"
    assert sp.same(entries[0][2][0][0], r.accumulator(h - 1, h)[0])
    r.close()


# ---- k_denoise_atrous on crafted colours ----
DENOISE_SHAPES = [(1, 1), (1, 37), (37, 1), (31, 7), (33, 9), (65, 17), (97, 41), (130, 67)]
DENOISE_SCENES = ["mixed_small", "background_scene", "tlas_test2"]

PARAMS = [None, dict(iterations=8)]
PARAMS += [dict(**{k: INF}) for k in ("sigma_color", "sigma_normal", "sigma_position", "sigma_albedo")]
PARAMS += [dict(sigma_color=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF, iterations=8)]
PARAMS += [dict(sigma_color=s, sigma_normal=s, sigma_position=s, sigma_albedo=s) for s in (1e18, 1e30)]
TINY = [dict(sigma_color=5e-19), dict(sigma_color=1e-30)] + [{k: 1e-20} for k in ("sigma_normal", "sigma_position", "sigma_albedo")]
PARAMS += [dict(p, iterations=n) for p in TINY for n in (5, 8)]


def _smooth(h, w, rng):
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.4 * np.sin(xs / 7.0), 0.5 + 0.4 * np.cos(ys / 5.0), 0.3 + 0.002 * (xs + ys)], -1)
    return base + 0.05 * rng.standard_normal((h, w, 3))


def _plant(c, hit, rng):
    """one non-finite channel (NaN, +inf, -inf in turn) on tile edges and corners, on hit / miss boundaries, and a whole row and column"""
    h, w = c.shape[:2]
    bad = [np.nan, np.inf, -np.inf]
    k = 0
    for y in sorted({0, 7, 8, h - 1} & set(range(h))):
        for x in sorted({0, 31, 32, w - 1} & set(range(w))):
            c[y, x, k % 3] = bad[k % 3]
            k += 1
    edge = np.argwhere(np.diff(hit.astype(np.int8), axis=1) != 0)
    for y, x in edge[rng.permutation(len(edge))[:8]]:
        c[y, x + rng.integers(0, 2), k % 3] = bad[k % 3]
        k += 1
    c[h // 2, :, 1] = np.nan
    c[:, w // 2, 2] = np.inf
    if w > 2:
        c[:, 1, 0] = -np.inf
    return c


def _colours(h, w, hit, rng):
    """(name, mean colour, frame count, params) -- the colour cases"""
    smooth = _smooth(h, w, rng)
    huge = rng.uniform(1e18, 1e19, (h, w, 3)) * rng.choice([-1.0, 1.0], (h, w, 3))  # |c_p - c_q|^2 overflows f32
    return [("smooth", smooth, 1, None), ("planted", _plant(smooth.copy(), hit, rng), 3, None),
            ("planted_blur", _plant(smooth.copy(), hit, rng), 1, dict(sigma_color=INF, iterations=8)),
            ("negative", smooth - 1.5, 1, None), ("huge", huge, 1, None), ("frames", smooth, 7, dict(iterations=3))]


def _check_denoise(r, t, g, pos, mean, it, params, label, resolve_rows=False):
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    acc = np.concatenate([(np.float32(it) * mean.astype(np.float32)), rng.standard_normal(mean.shape[:2] + (1,))], -1).astype(np.float32)
    t.fill(acc)
    r.denoise(it, params)
    got = r.denoised()
    r.denoise(it, params)
    again = r.denoised()
    ref = dr.denoise(acc, it, g, pos, params)
    assert sp.same(got, again), label + ": a second run differs"
    assert np.all(sp.bits(got[..., 3]) == 0), label + ": w channel"
    err, cls_ok = rel_err(got[..., :3], ref)
    assert cls_ok, label + ": non-finite pixels differ from the restatement"
    assert err.max() <= RADIANCE_TOL, "%s: denoised error %g" % (label, err.max())
    fin = np.all(np.isfinite(dr.mean_color(acc, it)), -1)
    assert np.all(np.isfinite(got[..., :3][fin])), label + ": %d finite pixels came out non-finite" % (~np.isfinite(got[..., :3][fin])).any(-1).sum()
    assert sp.same(t.read(), acc), label + ": the accumulator was written"
    if resolve_rows:
        h = got.shape[0]
        for y0, y1 in _row_ranges(h):
            assert np.array_equal(r.resolve_denoised(y0, y1), rr.resolve(got[y0:y1], 1)), label + ": rt_resolve_denoised rows %d..%d" % (y0, y1)
            assert sp.same(r.denoised(y0, y1), got[y0:y1])


@pytest.mark.parametrize("name", DENOISE_SCENES)
@pytest.mark.parametrize("w,h", DENOISE_SHAPES)
def test_denoise_equals_the_restatement_on_crafted_frames(name, w, h, scenes, oracle_api, host_api):
    r, orr = make(scenes, host_api, name, w, h, oracle_api)
    r.render_aovs(0.001)
    g = r.aovs()
    O, D = orr.primary_rays()
    pos = dr.positions(O, D, g["t"].reshape(-1))
    hit = g["obj"] != -1
    t = Bound(r)
    rng = np.random.default_rng(w * 1000 + h)
    shape_i = DENOISE_SHAPES.index((w, h))
    for k, (cname, mean, it, params) in enumerate(_colours(h, w, hit, rng)):
        # every case at its own iteration count, walking 1..8 across cases and shapes (steps 1 to 128: beyond every image here)
        p = dict(params or {})
        p.setdefault("iterations", 1 + (shape_i + k) % 8)
        _check_denoise(r, t, g, pos, mean, it, p, "%s %dx%d %s %s" % (name, w, h, cname, p), resolve_rows=cname == "planted")
    smooth = _smooth(h, w, rng)
    for p in PARAMS:
        _check_denoise(r, t, g, pos, smooth, 1, p, "%s %dx%d params %s" % (name, w, h, p))
    r.close()


def test_tiny_t_keeps_every_pixel_finite(scenes, oracle_api, host_api):
    """a camera 2e-3 above mixed_small's floor, looking down: every t_p is about 2e-3, and with sigma_position 2e-19 (kx = 2.5e37) or
    1e-20 (kx = FLT_MAX) the per-pixel kx / t_p^2 overflows f32 -- the kernel's own clamp, not the host's"""
    w, h = 65, 17
    r, orr = make(scenes, host_api, "mixed_small", w, h, oracle_api)
    cam = dict(cam_pos=(0.3, 0.002, -2.0), top_left=(-0.7, -0.998, -1.5), top_right=(1.3, -0.998, -1.5), bottom_left=(-0.7, -0.998, -2.5))
    for x in (r, orr):
        x.set_camera(cam["cam_pos"], cam["top_left"], cam["top_right"], cam["bottom_left"])
    r.render_aovs(1e-6)
    g = r.aovs()
    hit = g["obj"] != -1
    assert hit.all() and g["t"].max() < 0.01
    O, D = orr.primary_rays()
    pos = dr.positions(O, D, g["t"].reshape(-1))
    t = Bound(r)
    rng = np.random.default_rng(11)
    for p in (dict(sigma_position=2e-19), dict(sigma_position=1e-20, iterations=8), dict(sigma_position=2e-19, sigma_color=INF, sigma_normal=INF, sigma_albedo=INF)):
        _check_denoise(r, t, g, pos, _smooth(h, w, rng), 1, p, "tiny t %s" % p)
    r.close()
