"""What the GPU tests share: the environment a context is created under, the bitwise comparisons every exactness claim of the suite rests
on, the renderer most files build, and the 'count alone decides a pixel' method of the adaptive tests.  A plain helper module of the test
suite (tests/test_support_cpu.py holds it to crafted inputs): numpy only at import time, no device and no library until a function that
takes host_api or a renderer is called."""
import numpy as np

# csrc/rt_ctx.h read_knobs, the library's only getenv site, in the order it reads them (tests/test_support_cpu.py compares with the source)
KNOBS = ("RT_SLOTS", "RT_SAMPLE_GIB", "RT_EXACT_GAMMA", "RT_WIDE", "RT_WIDE8", "RT_FUSE", "RT_STREAM", "RT_DECIDE", "RT_MEGA", "RT_MEGA_LPT",
         "RT_MEGA_LEVELS", "RT_DEFER_GAMMA", "RT_SHADE_LDS", "RT_TLAS_LDS", "RT_GAMMA_LUT", "RT_LEVEL_CAP", "RT_MIXED_MAX", "RT_PRIMARY_TABLE",
         "RT_PRIMARY_TABLE_MIN")


def clean_env(monkeypatch, env=None):
    """Every knob unset, then env's items set: the only place in tests/ that clears knobs.  A context reads its knobs once, in rt_create
    (csrc/rt_ctx.h read_knobs), so call this before the renderer exists."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def layout_knobs(env=None):
    """(RT_WIDE, RT_WIDE8, RT_TLAS_LDS) as rt_layout_build takes them, with the library's defaults for what env leaves out"""
    env = env or {}
    return (int(env.get("RT_WIDE", -1)), int(env.get("RT_WIDE8", 0)), int(env.get("RT_TLAS_LDS", 1)))


def env_id(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "default"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    """the same shape and the same bits: -0.0 is not 0.0, a NaN equals only its own pattern"""
    return np.array_equal(bits(a), bits(b))


def state(r):
    """accumulator, count, sum_y, sum_yy of a context with statistics on"""
    return (r.accumulator(),) + tuple(r.stats())


def same_state(a, b):
    return all(same(x, y) for x, y in zip(a, b))


def renderer(host_api, monkeypatch, build, w, h, env=None, devices=None, path_ticks=True, scene_camera=True, camera=None):
    """A HostRenderer of w x h created under clean_env(env), its scene filled by build(r.scene) and committed.  path_ticks clears the
    scene's raytracer flag (Tick then renders path frames); an explicit camera is set as given, otherwise scene_camera applies the
    camera of the dict build returned, where it returned one."""
    clean_env(monkeypatch, env)
    r = host_api.HostRenderer(w, h, devices=devices)
    d = build(r.scene)
    if path_ticks:
        r.scene.set_raytracer(False)
    r.commit()
    if camera is not None:
        r.set_camera(*camera)
    elif scene_camera and d and "camera" in d:
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    return r


# Frames first, first + 1, ... of a scene at a size, rendered one at a time by a context of its own under the default knobs: snapshot n is
# the state after n frames (0: after rt_clear).  Rendered once per (scene, w, h, first) and shared by the files that use them, never
# changed; the equivalent-path knobs do not change a bit of them (tests/test_gpu_parity.py, tests/test_gpu_adaptive.py).
_SNAPSHOTS = {}


def snapshots(host_api, monkeypatch, name, build, w, h, upto, first=0):
    """snapshots 0 .. upto of the scene 'name', which build fills"""
    key = (name, w, h, first)
    have = _SNAPSHOTS.get(key, [])
    if len(have) <= upto:
        r = renderer(host_api, monkeypatch, build, w, h)
        r.stats_enable(True)
        r.clear()
        have = [state(r)]
        for n in range(upto):
            r.render(host_api.RT_MODE_PATH, (first + n) & 0xFFFFFFFF, 1)
            have.append(state(r))
        r.close()
        _SNAPSHOTS[key] = have
    return have


def differs_from_snapshot_of_its_count(st, snaps, where=None):
    """None when every pixel (of the mask 'where') with count n holds snapshot n's accumulator and sums, else what differs"""
    acc, cnt, sy, syy = st
    for n in np.unique(cnt if where is None else cnt[where]):
        on = cnt == n if where is None else (cnt == n) & where
        a, c, y, yy = snaps[int(n)]
        assert np.all(c[on] == n)
        if not (same(acc[on], a[on]) and same(sy[on], y[on]) and same(syy[on], yy[on])):
            return "pixels with count %d differ from %d frames rendered one at a time" % (n, n)
    return None


def uneven(r, host_api, pixels):
    """tests/budget_shapes.py uneven_moments on the device: UNEVEN_WHOLE whole frames, then UNEVEN_MORE more on 'pixels', so every pixel's
    sample k is frame k; returns the statistics"""
    import budget_shapes as tc
    r.stats_enable(True)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, tc.UNEVEN_WHOLE)
    r.set_active(pixels)
    r.render_active(tc.UNEVEN_WHOLE, tc.UNEVEN_MORE)
    return r.stats()
