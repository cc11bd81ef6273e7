"""Round 0 of a dense path batch from the primary-hit table (csrc/rt_stream.h PrimaryTable, k_primary_table, k_generate_t).

sample_primary truncates the jittered pixel to ints before it builds the camera ray, so every camera ray of a batch is the
ray of an integer pixel of [-1, width] x [-1, height]; the table holds Scene::FindNearest of each of them and round 0 fans the
answers out to the samples.  Held here: the jitter range (on the CPU, in float32); accumulator bits with RT_PRIMARY_TABLE=1 equal
to those with =0 over scenes, cameras, schedules and the decide / gamma knobs, with the Q-learning sampler, from row shards, for
batches of one frame and of many; the oracle's frame; a table that goes stale with the camera, the scene's time and an upload and
only then; the counters of a counting launch; and the default rule for when a stale table is rebuilt.

A path batch of camera rays always starts at depth 4 (rt_render: five rounds), so 'rounds == 1' -- where round 0 is the last
round -- exists for caller-supplied rays only (rt_trace_batch, which never reads the table): test_trace_batch_keeps_its_rays
holds that at depth 0 next to a current table."""
import re

import numpy as np
import pytest

import support as sp

ON = {"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}  # MIN=0: the first batch builds the table, whatever its size
OFF = {"RT_PRIMARY_TABLE": "0"}
gpu = pytest.mark.gpu


# ---- the jitter range: CPU, numpy float32 ------------------------------------------------------------------------------
def _random_float(u):
    """RandomFloat (rt_dmath.h): RandomUInt(seed) * 2.3283064365387e-10f -- uint -> float32 (round to nearest even), times 2^-32"""
    return np.asarray(u, dtype=np.uint32).astype(np.float32) * np.float32(2.3283064365387e-10)


def _jitter(u):
    """RandomFloat(seed) * 2 - 1 in float32"""
    return _random_float(u) * np.float32(2) - np.float32(1)


def test_jitter_range():
    """the extreme draws give exactly -1.0 and +1.0, every draw lies between them, and for every x of [0, W) the truncated
    pixel (int)(x + jitter) lies in [-1, W]: the table's (W + 2) columns and, the same way, (H + 2) rows cover every sample"""
    assert np.float32(2.3283064365387e-10) == np.float32(2.0 ** -32)
    assert _jitter(0) == np.float32(-1.0) and _jitter(0xFFFFFFFF) == np.float32(1.0)
    assert _random_float(0xFFFFFFFF) == np.float32(1.0)  # 2^32 - 1 rounds to 2^32 as a float
    rng = np.random.default_rng(5)
    draws = np.concatenate([np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32),
                            rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)])
    j = _jitter(draws)
    assert j.min() == np.float32(-1.0) and j.max() == np.float32(1.0)
    # monotone in the draw, so the two ends bound everything in between
    s = np.sort(draws)
    assert (np.diff(_jitter(s)) >= 0).all()
    for W in (1, 2, 64, 1920, 3840, 7680):
        x = np.arange(W, dtype=np.int32)
        lo = (x.astype(np.float32) + np.float32(-1.0)).astype(np.int32)  # float newX = x + jitter; (int)newX truncates toward zero
        hi = (x.astype(np.float32) + np.float32(1.0)).astype(np.int32)
        assert lo.min() == -1 and hi.max() == W
        # x + jitter is monotone in jitter: every other draw lands between the two
        some = (x[:, None].astype(np.float32) + j[None, :4096]).astype(np.int32)
        assert some.min() >= -1 and some.max() <= W
        assert ((some >= lo[:, None]) & (some <= hi[:, None])).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _builds(r):
    """table builds of this renderer so far: the launches of the profile's query slot (profiling on; these tests run no other query)"""
    return r.profile(reset=False)["query"]["launches"]


FISHEYE = dict(fisheye=True, view_angle=0.4, y_angle=0.3)
CASES = [
    ("mixed_small", {}, 96, 64, None),                      # a scene BVH
    ("pretty_tlas", {"n_instances": 8}, 240, 135, None),    # the bench scene (config 3: instances under a TLAS) at 1/8 size
    ("mixed_small", {}, 64, 40, FISHEYE),
    ("background", {}, 96, 64, None),                       # sky texels: generate's gamma table
]


def _renderer(host_api, scenes, name, kw, w, h, cam):
    r = host_api.HostRenderer(w, h)
    d = scenes.REGISTRY[name](r.scene, **kw)
    r.commit()
    r.set_profiling(True)
    if d and "camera" in d:
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    if cam:
        c = r.camera()
        r.set_camera(c[0], c[1], c[2], c[3], **cam)
    return r


def _frame(host_api, scenes, monkeypatch, env, name, kw, w, h, cam, frames):
    sp.clean_env(monkeypatch, env)
    r = _renderer(host_api, scenes, name, kw, w, h, cam)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    out = r.accumulator().copy()
    builds = _builds(r)
    r.close()
    return out, builds


VARIANTS = [{}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}, {"RT_DECIDE": "0"}, {"RT_DEFER_GAMMA": "0"}, {"RT_GAMMA_LUT": "0"},
            {"RT_EXACT_GAMMA": "1"}, {"RT_FUSE": "0", "RT_DECIDE": "0", "RT_DEFER_GAMMA": "0", "RT_GAMMA_LUT": "0"}]


@gpu
@pytest.mark.parametrize("name,kw,w,h,cam", CASES)
def test_table_frames_equal_traced_frames(name, kw, w, h, cam, scenes, host_api, monkeypatch):
    """every schedule, RT_DECIDE, and the gamma knobs: the same accumulator bits with the table as without"""
    frames = 3
    for env in VARIANTS:
        ref, b0 = _frame(host_api, scenes, monkeypatch, dict(env, **OFF), name, kw, w, h, cam, frames)
        got, b1 = _frame(host_api, scenes, monkeypatch, dict(env, **ON), name, kw, w, h, cam, frames)
        assert b0 == 0 and b1 == 1, (env, b0, b1)
        assert np.isfinite(ref[..., :3]).mean() > 0.5
        assert sp.same(ref, got), env


@gpu
@pytest.mark.parametrize("frames", [1, 12])
def test_one_frame_and_many(frames, scenes, host_api, monkeypatch):
    ref, _ = _frame(host_api, scenes, monkeypatch, OFF, "mixed_small", {}, 96, 64, None, frames)
    got, b = _frame(host_api, scenes, monkeypatch, ON, "mixed_small", {}, 96, 64, None, frames)
    assert b == 1 and sp.same(ref, got)


@gpu
def test_oracle_frame(scenes, oracle_api, host_api, monkeypatch):
    """the oracle's frame within the project's tolerance, and its primary rays' Sample() untouched by a current table"""
    from test_gpu_parity import check_frames, make_pair
    sp.clean_env(monkeypatch, ON)
    o, orr, r, d = make_pair(scenes.mixed_small, oracle_api, host_api, 96, 64)
    r.set_profiling(True)
    check_frames(orr, r, "path", 3, host_api)
    assert _builds(r) == 1
    r.close()


@gpu
def test_trace_batch_keeps_its_rays(scenes, oracle_api, host_api, monkeypatch):
    """rt_trace_batch (caller-supplied rays, the only batches whose round 0 can be the last) never reads the table: the same
    Sample() values at depth 0, 1 and 4 with a current table as without one"""
    from test_gpu_parity import make_pair
    out = {}
    for key, env in (("off", OFF), ("on", ON)):
        sp.clean_env(monkeypatch, env)
        o, orr, r, d = make_pair(scenes.mixed_small, oracle_api, host_api, 64, 40)
        r.set_profiling(True)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 2)  # "on": the table is current from here
        pO, pD = orr.primary_rays()
        out[key] = [r.trace_batch(host_api.RT_MODE_PATH, pO, pD, depth, 99) for depth in (0, 1, 4)]
        assert _builds(r) == (1 if key == "on" else 0)
        r.close()
    for a, b in zip(out["off"], out["on"]):
        assert sp.same(a, b)


@gpu
def test_row_shards(scenes, host_api, monkeypatch):
    """two interleaved row shards against the whole frame: one table (always of the whole frame) serves both"""
    w, h, frames = 96, 63, 4
    ref, _ = _frame(host_api, scenes, monkeypatch, OFF, "mixed_small", {}, w, h, None, frames)
    sp.clean_env(monkeypatch, ON)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h, None)
    r.clear()
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 0, 2, (h + 1) // 2)
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 1, 2, h // 2)
    assert sp.same(ref, r.accumulator()) and _builds(r) == 1
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    assert sp.same(ref, r.accumulator()) and _builds(r) == 1
    r.close()


@gpu
def test_with_sampler(host_api, monkeypatch):
    """the Q-learning sampler's round 0 is the same round 0: frame, table and pending reward sums"""
    from lit_scene import lit_scene
    w, h, frames = 64, 40, 3
    out = {}
    for key, env in (("off", OFF), ("on", ON)):
        sp.clean_env(monkeypatch, env)
        r = host_api.HostRenderer(w, h)
        lit_scene(r.scene, "AD")
        r.commit()
        r.set_profiling(True)
        r.qlearn_enable(8, (-4, -1, -4), (4, 5, 6), 0.3, 0.2, 1.0, 0)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        sums = [x.copy() for x in r.qlearn_sums()]
        r.qlearn_apply()
        r.render(host_api.RT_MODE_PATH, frames, frames)
        out[key] = (r.accumulator().copy(), r.qlearn_table().copy(), sums, [x.copy() for x in r.qlearn_sums()])
        assert _builds(r) == (1 if key == "on" else 0)
        r.close()
    a, b = out["off"], out["on"]
    assert sp.same(a[0], b[0]) and sp.same(a[1], b[1])
    for k in (2, 3):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])
    assert a[2][1].sum() > 0  # rewards were paid


@gpu
def test_staleness(scenes, host_api, monkeypatch):
    """camera, re-upload and rt_set_time each make the table stale; the same camera sent again does not.  After each, the
    frame of ONE renderer equals a fresh renderer's (rendered without the table)."""
    w, h, frames = 80, 48, 3
    cam2 = None

    def fresh(steps):
        sp.clean_env(monkeypatch, OFF)
        f = _renderer(host_api, scenes, "mixed_small", {}, w, h, None)
        for s in steps:
            s(f)
        f.clear()
        f.render(host_api.RT_MODE_PATH, 0, frames)
        out = f.accumulator().copy()
        f.close()
        return out

    def move(x):
        c = x.camera()
        d = np.array([0.3, 0.1, -0.2], np.float32)
        x.set_camera(c[0] + d, c[1] + d, c[2] + d, c[3] + d)

    def again(x):
        c = x.camera()
        x.set_camera(c[0], c[1], c[2], c[3])

    def reupload(x):
        x.commit()

    def animate(x):
        x.scene.set_time(1.3)

    sp.clean_env(monkeypatch, ON)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h, None)
    again(r)  # (the record as set_camera's defaults write it)
    steps, frames_seen = [], []
    for step, builds in ((None, 1), (again, 1), (move, 2), (again, 2), (reupload, 3), (animate, 4), (again, 4)):
        if step:
            step(r)
            steps.append(step)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        got = r.accumulator().copy()
        assert _builds(r) == builds, (len(steps), _builds(r), builds)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)  # ... and once more from the table as it stands
        assert sp.same(got, r.accumulator()) and _builds(r) == builds
        frames_seen.append(got)
        sp.clean_env(monkeypatch, OFF)
        ref = fresh(list(steps))
        sp.clean_env(monkeypatch, ON)
        assert sp.same(ref, got), len(steps)
    assert not sp.same(frames_seen[0], frames_seen[2]) and not sp.same(frames_seen[4], frames_seen[5])  # the camera and the geometry really moved
    r.close()


@gpu
@pytest.mark.parametrize("name,kw,w,h", [("mixed_small", {}, 96, 64), ("pretty_tlas", {"n_instances": 4}, 160, 90)])
def test_counting(name, kw, w, h, scenes, host_api, monkeypatch):
    """the queries of a counting launch are the same with the table and without; its walk is shorter.  A table built inside the
    counting launch adds its own walk, a table that was current adds none (include/rt_amd.h)."""
    frames = 8
    cnt = {}
    for key, env in (("off", OFF), ("on", ON), ("on_current", ON)):
        sp.clean_env(monkeypatch, env)
        r = _renderer(host_api, scenes, name, kw, w, h, None)
        if key == "on_current":
            r.render(host_api.RT_MODE_PATH, 0, 1)
        r.clear()
        r.set_counting(host_api.RT_COUNT_EXECUTED); r.counters()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        near, occl = r.counters_split()
        r.set_counting(False)
        counted = r.accumulator().copy()
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        assert sp.same(counted, r.accumulator())  # counting launches render the same frame
        cnt[key] = (near, occl, counted)
        r.close()
    for key in ("on", "on_current"):
        for k in ("rays_nearest", "light_tests", "brute_tests"):
            assert cnt[key][0][k] == cnt["off"][0][k], (key, k, cnt[key][0][k], cnt["off"][0][k])
        assert cnt[key][1]["rays_occluded"] == cnt["off"][1]["rays_occluded"], key
        assert cnt[key][0]["inner_visits"] < cnt["off"][0]["inner_visits"], key
        assert sp.same(cnt[key][2], cnt["off"][2])
    assert cnt["on_current"][0]["inner_visits"] <= cnt["on"][0]["inner_visits"]
    assert cnt["off"][0]["rays_nearest"] >= frames * w * h


@gpu
def test_default_rebuild_rule(scenes, host_api, monkeypatch):
    """the default (RT_PRIMARY_TABLE_MIN samples per table record since the table went stale): one-frame batches of a camera that moves
    every call never build; a camera that rests gets its table after a few frames; the frames are the traced ones either way"""
    w, h = 64, 40
    out = {}
    for key, env in (("off", OFF), ("default", {})):
        sp.clean_env(monkeypatch, env)
        r = _renderer(host_api, scenes, "mixed_small", {}, w, h, None)
        need = int(re.search(r"primary_table_min=(\d+)", r.build_info()).group(1))
        assert need >= 2
        got = []
        for f in range(4):  # a moving camera
            c = r.camera()
            d = np.array([0.05, 0.0, 0.02], np.float32)
            r.set_camera(c[0] + d, c[1] + d, c[2] + d, c[3] + d)
            r.clear()
            r.render(host_api.RT_MODE_PATH, f, 1)
            got.append(r.accumulator().copy())
        assert _builds(r) == 0
        r.clear()
        for f in range(2 * need + 2):  # ... at rest
            r.render(host_api.RT_MODE_PATH, f, 1)
        got.append(r.accumulator().copy())
        assert _builds(r) == (1 if key == "default" else 0)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 2 * need + 2)  # one batch worth the build at once
        got.append(r.accumulator().copy())
        out[key] = got
        r.close()
    for a, b in zip(out["off"], out["default"]):
        assert sp.same(a, b)
