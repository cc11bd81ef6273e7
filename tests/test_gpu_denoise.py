"""The G-buffer pass (rt_render_aovs) against the oracle, the denoiser (rt_denoise) against its numpy restatement (tests/denoise_ref.py),
its invalidation rule, its freedom from side effects, Renderer::Tick's denoised preview, and what the filter buys on a 4-spp frame."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

RADIANCE_TOL = 1e-4
INF = float("inf")


class Recorder:
    """A scene builder that passes every call on and keeps the material and light parameters the test handed it"""
    def __init__(self, b):
        self.b, self.mats, self.lights = b, [], {}

    def diffuse(self, albedo, col, *a, **k):
        self.mats.append(("diffuse", np.float32(col), np.float32(albedo if hasattr(albedo, "__len__") else (albedo,) * 3)))
        return self.b.diffuse(albedo, col, *a, **k)

    def metal(self, fuzzy, col, *a, **k):
        self.mats.append(("metal", np.float32(col), None))
        return self.b.metal(fuzzy, col, *a, **k)

    def glass(self, ir, col, *a, **k):
        self.mats.append(("glass", np.float32(col), None))
        return self.b.glass(ir, col, *a, **k)

    def area_light(self, idx, pos, strength, col, *a, **k):
        self.lights[idx] = np.float32(col)
        return self.b.area_light(idx, pos, strength, col, *a, **k)

    def dir_light(self, idx, pos, strength, col, *a, **k):
        self.lights[idx] = np.float32(col)
        return self.b.dir_light(idx, pos, strength, col, *a, **k)

    def __getattr__(self, name):
        return getattr(self.b, name)

    def albedo(self, obj, mat):
        """the albedo rt_render_aovs defines, from the recorded parameters (f32 products)"""
        out = np.zeros(obj.shape + (3,), np.float32)
        for i in np.ndindex(obj.shape):
            if obj[i] == -1:
                continue
            if obj[i] in self.lights and 11 <= obj[i] < 11 + len(self.lights):
                out[i] = self.lights[obj[i]]
                continue
            kind, col, alb = self.mats[mat[i]]
            out[i] = col * alb if kind == "diffuse" else col
        return out


def make(scenes, oracle_api, host_api, scene_fn, w, h, **kw):
    o = oracle_api.OracleScene()
    d = scene_fn(o, **kw)
    r = host_api.HostRenderer(w, h)
    rec = Recorder(r.scene)
    scene_fn(rec, **kw)
    r.commit()
    orr = oracle_api.OracleRenderer(o, w, h)
    if "camera" in d:
        c = d["camera"]
        orr.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return o, orr, r, rec


def check_aovs(o, orr, r, rec, t_min):
    r.render_aovs(t_min)
    g = r.aovs()
    O, D = orr.primary_rays()
    ref = o.find_nearest(O, D, None, t_min)
    shape = g["obj"].shape
    assert np.array_equal(g["obj"], ref["obj"].reshape(shape))
    assert np.array_equal(g["t"].view(np.uint32), ref["t"].reshape(shape).view(np.uint32))
    # (as the batch-query parity tests: ids and normals of hits; a light's material is the oracle's own pointer)
    hit, rmat = g["obj"] != -1, ref["mat"].reshape(shape)
    assert np.array_equal(g["mat"][hit & (rmat >= 0)], rmat[hit & (rmat >= 0)])
    assert np.array_equal(g["normal"][hit].view(np.uint32), ref["normal"].reshape(shape + (3,))[hit].view(np.uint32))
    assert np.all(g["normal"][~hit] == 0) and np.all(g["mat"][~hit] == -1)
    alb = rec.albedo(g["obj"], g["mat"])
    assert np.array_equal(g["albedo"].view(np.uint32), alb.view(np.uint32))
    return g


@pytest.mark.parametrize("name,w,h", [("mixed_small", 64, 40), ("background_scene", 64, 40), ("tlas_test2", 64, 40), ("pretty_tlas", 960, 540)]
                         + [(n, w, h) for n in ("mixed_small", "background_scene", "tlas_test2") for w, h in ((1, 1), (33, 9), (97, 41))])
@pytest.mark.parametrize("t_min", [0.001, 1e-6])
def test_aovs_equal_the_oracle(name, w, h, t_min, scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, getattr(scenes, name), w, h)
    g = check_aovs(o, orr, r, rec, t_min)
    assert (g["obj"] != -1).any() or w * h == 1  # (a single pixel of the two non-TLAS scenes is a miss)
    r.close()


def test_aovs_fisheye(scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)
    cam = orr.camera()
    for rr in (orr, r):
        rr.set_camera(cam[0], cam[1], cam[2], cam[3], fisheye=True, view_angle=0.4, y_angle=0.3)
    for t_min in (0.001, 1e-6):
        check_aovs(o, orr, r, rec, t_min)
    r.close()


def kernel_vs_ref(orr, r, host_api, frames, params):
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    r.render_aovs(0.001)
    r.denoise(frames, params)
    got = r.denoised()
    g = r.aovs()
    O, D = orr.primary_rays()
    pos = dr.positions(O, D, g["t"].reshape(-1))
    ref = dr.denoise(r.accumulator(), frames, g, pos, params)
    assert np.all(got[..., 3] == 0)
    err, cls_ok = rel_err(got[..., :3], ref)
    assert cls_ok, "non-finite pixels differ from the restatement"
    assert err.max() <= RADIANCE_TOL, "denoised error %g" % err.max()
    return got, ref


PARAMS = [dict(iterations=1), dict(iterations=5), dict(iterations=5, sigma_color=INF, sigma_normal=INF, sigma_position=INF, sigma_albedo=INF),
          dict(iterations=3, sigma_color=0.2, sigma_normal=INF, sigma_position=0.05, sigma_albedo=1.0)]


@pytest.mark.parametrize("name,w,h", [("mixed_small", 64, 40), ("scene3", 320, 180), ("pretty_tlas", 320, 180)])
@pytest.mark.parametrize("frames", [1, 4])
def test_kernel_equals_the_restatement(name, w, h, frames, scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, getattr(scenes, name), w, h)
    for p in PARAMS:
        kernel_vs_ref(orr, r, host_api, frames, p)
    r.close()


def test_kernel_equals_the_restatement_full_size(scenes, oracle_api, host_api):
    """config 3's scene at 1920x1080, 64 spp, the defaults"""
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.pretty_tlas, 1920, 1080)
    got, ref = kernel_vs_ref(orr, r, host_api, 64, None)
    assert np.all(np.isfinite(got[..., :3]), -1).mean() > 0.5  # (the rest: directly viewed lights, passed through)
    r.close()


def test_no_side_effects(scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    acc0, px0 = r.accumulator(), r.resolve(2)
    r.render_aovs(0.001)
    r.denoise(2)
    r.resolve_denoised()
    acc1, px1 = r.accumulator(), r.resolve(2)
    assert np.array_equal(acc0.view(np.uint32), acc1.view(np.uint32)) and np.array_equal(px0, px1)
    r.render(host_api.RT_MODE_PATH, 2, 2)
    after = r.accumulator()
    r2 = make(scenes, oracle_api, host_api, scenes.mixed_small, 64, 40)[2]
    r2.render(host_api.RT_MODE_PATH, 0, 2)
    r2.render(host_api.RT_MODE_PATH, 2, 2)
    assert np.array_equal(after.view(np.uint32), r2.accumulator().view(np.uint32))
    r.close(), r2.close()


def _denoise_rc(r, host_api, it=1):
    return host_api.rt_lib().rt_denoise(r.ctx, it, None)


def test_invalidation(scenes, oracle_api, host_api):
    o, orr, r, rec = make(scenes, oracle_api, host_api, scenes.pretty_animation_scene, 64, 40)
    r.render(host_api.RT_MODE_PATH, 0, 1)
    assert _denoise_rc(r, host_api) == host_api.RT_E_STATE  # no G-buffer yet
    r.set_profiling(True)
    r.profile(reset=True)
    r.render_aovs(0.001)
    assert r.profile()["query"]["launches"] == 1
    assert _denoise_rc(r, host_api) == 0
    r.render_aovs(0.001)  # current: no launch
    assert r.profile()["query"]["launches"] == 0
    cam = r.camera()
    r.set_camera(cam[0], cam[1], cam[2], cam[3])  # the same record: still current
    assert _denoise_rc(r, host_api) == 0
    r.render_aovs(0.001)
    assert r.profile()["query"]["launches"] == 0
    r.set_camera(cam[0] + np.float32(0.01), cam[1], cam[2], cam[3])
    assert _denoise_rc(r, host_api) == host_api.RT_E_STATE
    r.render_aovs(0.001)
    assert r.profile()["query"]["launches"] == 1 and _denoise_rc(r, host_api) == 0
    r.scene.set_time(0.7)
    assert _denoise_rc(r, host_api) == host_api.RT_E_STATE
    r.profile()
    r.render_aovs(0.001)
    assert r.profile()["query"]["launches"] == 1 and _denoise_rc(r, host_api) == 0
    r.render_aovs(1e-6)  # a new t_min: a new pass
    assert r.profile()["query"]["launches"] == 1 and _denoise_rc(r, host_api) == 0
    r.commit()  # rt_upload_scene
    assert _denoise_rc(r, host_api) == host_api.RT_E_STATE
    r.profile()
    r.render_aovs(1e-6)
    assert r.profile()["query"]["launches"] == 1 and _denoise_rc(r, host_api) == 0
    r.close()


def _ticker(scenes, host_api, devices=None, denoise=None):
    r = host_api.HostRenderer(64, 40, devices=devices)
    scenes.mixed_small(r.scene)
    r.commit()
    r.scene.set_raytracer(False)
    if denoise is not None:
        r.set_denoise(denoise)
    return r


def _tick_it(r, px):
    """the frame count Tick resolved with: the one whose rt_denoise + rt_resolve_denoised of the same state gives its pixels"""
    found = [it for it in range(1, 12) if (r.denoise(it), np.array_equal(px, r.resolve_denoised()))[1]]
    assert found, "no frame count reproduces Tick's pixels"
    return found[0]


def test_tick_denoised(scenes, host_api):
    r = _ticker(scenes, host_api, denoise=True)
    for _ in range(4):
        r.tick()
    px = r.tick_pixels()
    acc = r.tick_accumulator()
    assert np.array_equal(acc.view(np.uint32), r.accumulator().view(np.uint32))  # the raw accumulator
    assert np.array_equal(px, r.resolve_denoised())
    it = _tick_it(r, px)
    assert it >= 2 and not np.array_equal(px, r.resolve(it))
    # a camera move refreshes the G-buffer
    g0 = r.aovs()
    cam = r.camera()
    r.set_camera(cam[0] + np.float32(0.2), cam[1], cam[2], cam[3])
    r.tick()
    g1 = r.aovs()
    assert not np.array_equal(g0["t"].view(np.uint32), g1["t"].view(np.uint32))
    assert np.array_equal(r.tick_pixels(), r.resolve_denoised())
    _tick_it(r, r.tick_pixels())
    r.close()


def test_tick_two_contexts_match_one(scenes, host_api):
    px = []
    for devices in (None, [0, 0]):
        r = _ticker(scenes, host_api, devices=devices, denoise=True)
        for _ in range(3):
            r.tick()
        px.append(r.tick_pixels())
        r.close()
    assert np.array_equal(px[0], px[1])


def test_tick_without_denoise_is_unchanged(scenes, host_api):
    out = []
    for denoise in (None, False):
        r = _ticker(scenes, host_api, denoise=denoise)
        for k in range(3):
            if k == 1:
                cam = r.camera()
                r.set_camera(cam[0] + np.float32(0.1), cam[1], cam[2], cam[3])
            r.tick()
        out.append((r.tick_pixels(), r.tick_accumulator()))
        r.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_quality_on_config2_scene(scenes, host_api):
    """4 spp denoised with the defaults against 256 spp: the mean squared error over finite pixels is at least 2x lower than the raw
    4-spp frame's (the ratio measured is printed)"""
    r = host_api.HostRenderer(320, 180)
    scenes.config2(r.scene)
    r.commit()
    r.render(host_api.RT_MODE_PATH, 4, 256)
    ref = dr.mean_color(r.accumulator(), 256)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 4)
    raw = dr.mean_color(r.accumulator(), 4)
    r.render_aovs(0.001)
    r.denoise(4)
    den = r.denoised()[..., :3].astype(np.float64)
    fin = np.all(np.isfinite(ref), -1) & np.all(np.isfinite(raw), -1) & np.all(np.isfinite(den), -1)
    mse_raw = np.mean((raw[fin] - ref[fin]) ** 2)
    mse_den = np.mean((den[fin] - ref[fin]) ** 2)
    print("quality config2 320x180: mse raw %.6g denoised %.6g ratio %.3f" % (mse_raw, mse_den, mse_raw / mse_den))
    assert mse_raw >= 2 * mse_den
    r.close()
