"""Round 0 of a dense path batch shaded straight from the primary-hit table, without round-0 entries (csrc/rt_stream.h k_generate_c,
k_shade_s<QL, BOUNCE, TABLE0>, k_light_s<TABLE0>; csrc/rt_api_render.inc run_rounds_stream).

k_generate_t copied a sample's table record into an entry (O, D, hit normal and t, hit ids) that shade(0) and light(0) read back one
launch later.  Nothing in that entry is new: O is the camera position, D the pinhole ray of the integer pixel sample_primary_pixel gives,
the rest the record's.  RT_ROUND0_ENTRIES selects the form: unset or 0 the direct one, 1 the entries, 2 the direct one with the four entry
arrays filled with 0xFF bytes behind generate, so that whoever still read one would shade NaNs and ids of -1.  Held here, as accumulator
bits and without a tolerance: the three values against each other and against a frame with every camera ray traced, over scenes,
schedules and both shade instantiations; sizes whose groups of 64 samples straddle rows and frames; row shards; pixel-list batches; the
batches that keep their entries (a fisheye camera, the Q-learning sampler); the counters of a counting launch; a table that went stale.

Every test runs with RT_PRIMARY_TABLE=1 and RT_PRIMARY_TABLE_MIN=0 (the first batch builds the table).  RT_ROUND0_ENTRIES is not one
of support.KNOBS (that list is the library's num() knobs): _env clears it here, as tests/test_gpu_bounce_table.py does for its knob."""
import numpy as np
import pytest

import support as sp

pytestmark = pytest.mark.gpu
f32 = np.float32
TABLE = {"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}
TRACED = {"RT_PRIMARY_TABLE": "0"}
VALUES = (0, 1, 2)
FISHEYE = dict(fisheye=True, view_angle=0.4, y_angle=0.3)


def _env(monkeypatch, value, more=None, base=TABLE):
    monkeypatch.delenv("RT_ROUND0_ENTRIES", raising=False)
    monkeypatch.delenv("RT_BOUNCE_TABLE", raising=False)
    env = dict(base, **(more or {}))
    bounce = env.pop("RT_BOUNCE_TABLE", None)
    sp.clean_env(monkeypatch, env)
    if bounce is not None:
        monkeypatch.setenv("RT_BOUNCE_TABLE", bounce)
    if value is not None:
        monkeypatch.setenv("RT_ROUND0_ENTRIES", str(value))


def _renderer(host_api, scenes, name, kw, w, h, fisheye=None):
    r = host_api.HostRenderer(w, h)
    d = scenes.REGISTRY[name](r.scene, **kw)
    r.commit()
    if d and "camera" in d:
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    if fisheye:
        c = r.camera()
        r.set_camera(c[0], c[1], c[2], c[3], **fisheye)
    return r


def _frame(host_api, scenes, monkeypatch, value, more, name, kw, w, h, frames, fisheye=None, base=TABLE):
    _env(monkeypatch, value, more, base)
    r = _renderer(host_api, scenes, name, kw, w, h, fisheye)
    assert ("round0_entries=%d" % (value or 0)) in r.build_info()
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    out = r.accumulator().copy()
    r.close()
    return out


# ---- 1. direct = entries = traced ---------------------------------------------------------------------------------------------------
CASES = [
    ("mixed_small", {}, 96, 64, None),                            # a scene BVH, glass and metal: k_shade_s<false, true, true>
    ("pretty_tlas", {"n_instances": 8}, 240, 135, None),          # the bench scene at 1/8 size
    ("background", {}, 96, 64, None),                             # sky texels: generate finishes them from B alone
    ("scene3", {"force_diffuse": True, "split": 3}, 96, 54, None),  # no glass, no metal, no bounce table: k_shade_s<false, false, true>
    ("mixed_small", {}, 96, 64, {"RT_BOUNCE_TABLE": "0"}),        # ... and the same instantiation on a scene that has both
]


@pytest.mark.parametrize("fuse", ["0", "1", "2"])
@pytest.mark.parametrize("name,kw,w,h,more", CASES, ids=["mixed_small", "pretty_tlas", "background", "diffuse", "mixed_small-no_bounce_table"])
def test_direct_equals_entries_equals_traced(name, kw, w, h, more, fuse, scenes, host_api, monkeypatch):
    frames = 3
    env = dict(more or {}, RT_FUSE=fuse)
    traced = _frame(host_api, scenes, monkeypatch, None, env, name, kw, w, h, frames, base=TRACED)
    assert np.isfinite(traced[..., :3]).mean() > 0.5
    for value in VALUES:
        got = _frame(host_api, scenes, monkeypatch, value, env, name, kw, w, h, frames)
        assert sp.same(traced, got), value


# ---- 2. ragged sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,frames", [(61, 37, 3), (3, 2, 1), (64, 1, 2)], ids=["61x37x3", "3x2x1", "64x1x2"])
def test_ragged_sizes(w, h, frames, scenes, host_api, monkeypatch):
    """61 x 37 x 3 = 6,771 samples: groups of 64 straddle rows and frames and the last one is partial; 3 x 2 x 1 is one partial group
    beside a 5 x 4 table; at 64 x 1 every lane sits in a border row of the table"""
    traced = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, base=TRACED)
    for value in VALUES:
        got = _frame(host_api, scenes, monkeypatch, value, None, "mixed_small", {}, w, h, frames)
        assert sp.same(traced, got), value


# ---- 3. row shards ------------------------------------------------------------------------------------------------------------------
def test_row_shards(scenes, host_api, monkeypatch):
    """two interleaved row shards of a 96 x 63 frame: the table is of the whole frame, a shard's samples index it by their own pixels"""
    w, h, frames = 96, 63, 4
    traced = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, base=TRACED)
    for value in VALUES:
        _env(monkeypatch, value)
        r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
        r.clear()
        r.render_rows(host_api.RT_MODE_PATH, 0, frames, 0, 2, (h + 1) // 2)
        r.render_rows(host_api.RT_MODE_PATH, 0, frames, 1, 2, h // 2)
        assert sp.same(traced, r.accumulator()), value
        r.close()


# ---- 4. pixel-list batches ----------------------------------------------------------------------------------------------------------
def test_pixel_list_batches(scenes, host_api, monkeypatch):
    """an active-pixel pass and a budgeted pass (RenderParams::plan: a sample's pixel and frame come from a record) at the smallest
    shape of tests/budget_shapes.py: accumulator and statistics after each under value 0 equal those under value 1"""
    import adaptive_shapes as sh
    import budget_shapes as tc
    w, h = 257, 3
    seen = {}
    for value in (0, 1):
        _env(monkeypatch, value)
        r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
        stats = sp.uneven(r, host_api, sh.seeded_list(w, h, seed=tc.UNEVEN_SEED))  # whole frames, then rt_render_active on a list
        assert set(np.unique(stats[0])) == {tc.UNEVEN_WHOLE, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE}
        after_active = sp.state(r)
        n, total, cap = r.select_budget(dict(select=tc.SELECT, pass_cap=7, max_pass_samples=0))
        assert 0 < n and n < total  # some pixel takes more than one sample: the pool is not a frame of the list
        r.render_budget(tc.UNEVEN_WHOLE + tc.UNEVEN_MORE)
        seen[value] = (after_active, sp.state(r), (n, total, cap))
        r.close()
    assert seen[0][2] == seen[1][2]
    assert sp.same_state(seen[0][0], seen[1][0]) and sp.same_state(seen[0][1], seen[1][1])
    assert not sp.same_state(seen[0][0], seen[0][1])  # the budgeted pass added samples


# ---- 5. the batches that keep their entries -----------------------------------------------------------------------------------------
def test_fisheye_keeps_its_entries(scenes, host_api, monkeypatch):
    """a fisheye camera's ray is not the pinhole expression: such a batch is not dispatched direct, and value 2 fills nothing"""
    w, h, frames = 64, 40, 3
    traced = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, fisheye=FISHEYE, base=TRACED)
    for value in VALUES:
        got = _frame(host_api, scenes, monkeypatch, value, None, "mixed_small", {}, w, h, frames, fisheye=FISHEYE)
        assert sp.same(traced, got), value


def test_sampler_keeps_its_entries(host_api, monkeypatch):
    """the Q-learning sampler on: frame, Q table and pending reward sums are the same bits under the three values"""
    from lit_scene import lit_scene
    w, h, frames = 64, 40, 3
    out = {}
    for value in VALUES:
        _env(monkeypatch, value)
        r = host_api.HostRenderer(w, h)
        lit_scene(r.scene, "AD")
        r.commit()
        r.qlearn_enable(8, (-4, -1, -4), (4, 5, 6), 0.3, 0.2, 1.0, 0)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        sums = [x.copy() for x in r.qlearn_sums()]
        r.qlearn_apply()
        r.render(host_api.RT_MODE_PATH, frames, frames)
        out[value] = (r.accumulator().copy(), r.qlearn_table().copy(), sums, [x.copy() for x in r.qlearn_sums()])
        r.close()
    a = out[1]
    assert a[2][1].sum() > 0  # rewards were paid
    for value in (0, 2):
        b = out[value]
        assert sp.same(a[0], b[0]) and sp.same(a[1], b[1]), value
        for k in (2, 3):
            assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]), (value, k)


# ---- 6. counting --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,w,h", [("mixed_small", {}, 96, 64), ("pretty_tlas", {"n_instances": 4}, 160, 90)], ids=["mixed_small", "pretty_tlas"])
def test_counting(name, kw, w, h, scenes, host_api, monkeypatch):
    """RT_COUNT_EXECUTED: the queries and the walk of a counting launch are the same under values 0 and 1 (k_generate_c tallies every
    sample as k_generate_t does), and the counted frame is the uncounted one"""
    frames = 3
    cnt = {}
    for value in (0, 1):
        _env(monkeypatch, value)
        r = _renderer(host_api, scenes, name, kw, w, h)
        r.render(host_api.RT_MODE_PATH, 0, 1)  # the tables are current from here: the counting launch builds nothing
        r.clear()
        r.set_counting(host_api.RT_COUNT_EXECUTED); r.counters()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        near, occl = r.counters_split()
        r.set_counting(False)
        counted = r.accumulator().copy()
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        assert sp.same(counted, r.accumulator()), value
        cnt[value] = (near, occl, counted)
        r.close()
    for k in ("rays_nearest", "light_tests", "brute_tests", "inner_visits"):
        assert cnt[0][0][k] == cnt[1][0][k], (k, cnt[0][0][k], cnt[1][0][k])
    assert cnt[0][0]["rays_nearest"] > 0
    assert cnt[0][1]["rays_occluded"] == cnt[1][1]["rays_occluded"] > 0
    assert sp.same(cnt[0][2], cnt[1][2])


# ---- 7. staleness -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 2])
def test_staleness(value, scenes, host_api, monkeypatch):
    """a camera move, then a re-upload, on one renderer: each makes the table stale, and the direct frame after its rebuild equals a
    fresh renderer's traced frame (k_shade_s and k_light_s take the camera of the launch, the table is the new camera's)"""
    w, h, frames = 80, 45, 3

    def move(x):
        c = x.camera()
        d = f32([0.3, 0.1, -0.2])
        x.set_camera(c[0] + d, c[1] + d, c[2] + d, c[3] + d)

    def reupload(x):
        x.commit()

    def fresh(steps):
        _env(monkeypatch, None, base=TRACED)
        f = _renderer(host_api, scenes, "mixed_small", {}, w, h)
        for s in steps:
            s(f)
        f.clear()
        f.render(host_api.RT_MODE_PATH, 0, frames)
        out = f.accumulator().copy()
        f.close()
        return out

    _env(monkeypatch, value)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
    steps, seen = [], []
    for step in (None, move, reupload):
        if step:
            step(r)
            steps.append(step)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        got = r.accumulator().copy()
        seen.append(got)
        ref = fresh(list(steps))
        _env(monkeypatch, value)
        assert sp.same(ref, got), len(steps)
    assert not sp.same(seen[0], seen[1])  # the camera really moved
    r.close()
