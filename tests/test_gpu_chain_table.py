"""All-specular bounce chains from per-level hit tables (csrc/rt_stream.h ChainLevel, k_chain_link, k_chain_table, k_shade_s CHAIN).

While every hit of a path so far was glass or metal no draw has entered a ray's origin or direction, so the round-k ray of such a path is
one of at most 2^k rays per primary record.  RT_BOUNCE_DEPTH = d keeps the hits of those rays for rounds 1 .. d (depth 1: the bounce table
of tests/test_gpu_bounce_table.py alone) in compact levels linked parent -> first child, and shade reads them instead of tracing.  Held
here, always as accumulator bits (support.same) of depth d against depth 1 of the same build, and once per scene against RT_BOUNCE_TABLE=0
and RT_PRIMARY_TABLE=0 (everything traced): scenes, cameras, schedules and RT_DECIDE; a camera inside glass under every mask; levels too
small for their records; that every level is really read (the executed walk of a counting launch falls from depth to depth, its queries
stay); caller rays at every start depth; row shards; staleness under every call that edits the scene; the sampler; the oracle; the
build threshold.

A path batch of camera rays always runs five rounds (rt_render: Sample starts at depth 4), so the last-round class nibble is read from
level 4 at depth 4 and from traced hits below; rt_trace_batch, the only call with other round counts, takes caller rays, which no table
holds: it is held to read none at any start depth.

RT_BOUNCE_DEPTH, RT_BOUNCE_DEPTH_MIN, RT_BOUNCE_CAP and RT_BOUNCE_TABLE are not among support.KNOBS (the library's num() knobs): _env
clears them here."""
import numpy as np
import pytest

import support as sp

pytestmark = pytest.mark.gpu
f32 = np.float32
TABLE = {"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}  # MIN=0: the first batch builds every level, whatever its size
TRACED = {"RT_PRIMARY_TABLE": "0"}
OWN = ("RT_BOUNCE_TABLE", "RT_BOUNCE_DEPTH", "RT_BOUNCE_DEPTH_MIN", "RT_BOUNCE_CAP")
DEPTHS = (2, 3, 4)


def _env(monkeypatch, depth, more=None, base=TABLE, mask=None, cap=None):
    for k in OWN:
        monkeypatch.delenv(k, raising=False)
    sp.clean_env(monkeypatch, dict(base, **(more or {})))
    monkeypatch.setenv("RT_BOUNCE_DEPTH", str(depth))
    if mask is not None:
        monkeypatch.setenv("RT_BOUNCE_TABLE", str(mask))
    if cap is not None:
        monkeypatch.setenv("RT_BOUNCE_CAP", str(cap))


def _builds(r):
    """entries of the profile's query slot so far"""
    return r.profile(reset=False)["query"]["launches"]


def _looking(p, half_w, half_h, dist=1.0):
    p = np.asarray(p, f32)
    return (p, p + f32([-half_w, half_h, dist]), p + f32([half_w, half_h, dist]), p + f32([-half_w, -half_h, dist]))


INSIDE_GLASS = _looking(f32([0.2 + 0.3, 0.35, 0.2]), 1.6, 1.0)  # tests/test_gpu_bounce_table.py test_inside_glass: every pixel is specular


def _renderer(host_api, scenes, name, kw, w, h, cam=None, fisheye=None):
    r = host_api.HostRenderer(w, h)
    d = scenes.REGISTRY[name](r.scene, **kw)
    r.commit()
    r.set_profiling(True)
    if cam is not None:
        r.set_camera(*cam)
    elif d and "camera" in d:
        c = d["camera"]
        r.set_camera(c["cam_pos"], c["top_left"], c["top_right"], c["bottom_left"])
    if fisheye:
        c = r.camera()
        r.set_camera(c[0], c[1], c[2], c[3], **fisheye)
    return r


def _frame(host_api, scenes, monkeypatch, depth, more, name, kw, w, h, frames, cam=None, fisheye=None, base=TABLE, mask=None, cap=None):
    _env(monkeypatch, depth, more, base, mask, cap)
    r = _renderer(host_api, scenes, name, kw, w, h, cam, fisheye)
    assert ("bounce_depth=%d" % depth) in r.build_info()
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    out = r.accumulator().copy()
    builds = _builds(r)
    r.close()
    return out, builds


FISHEYE = dict(fisheye=True, view_angle=0.4, y_angle=0.3)
CASES = [
    ("pretty_tlas", {"n_instances": 8}, 160, 90, None),  # instanced glass + metal, the glass and metal spheres by brute force
    ("mixed_small", {}, 96, 63, None),                   # a scene BVH, glass WITH absorption; groups of 64 entries straddle rows
    ("mixed_small", {}, 64, 40, FISHEYE),
    ("background", {}, 96, 64, None),                    # chains that leave into the sky
]
VARIANTS = [{}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}, {"RT_DECIDE": "0"}]


@pytest.mark.parametrize("env", VARIANTS, ids=sp.env_id)
@pytest.mark.parametrize("name,kw,w,h,fisheye", CASES, ids=["pretty_tlas", "mixed_small", "mixed_small-fisheye", "background"])
def test_frames_equal_depth_one(name, kw, w, h, fisheye, env, scenes, host_api, monkeypatch):
    """every schedule and RT_DECIDE=0: the accumulator bits of depths 2, 3, 4 equal depth 1's, and once per scene those of a frame without
    the bounce table and of a frame with every ray traced"""
    frames = 3
    ref, b1 = _frame(host_api, scenes, monkeypatch, 1, env, name, kw, w, h, frames, fisheye=fisheye)
    assert b1 == 1 and np.isfinite(ref[..., :3]).mean() > 0.5
    for depth in DEPTHS:
        got, b = _frame(host_api, scenes, monkeypatch, depth, env, name, kw, w, h, frames, fisheye=fisheye)
        assert b == 1, (depth, b)  # every level is part of the one entry of the query slot
        assert sp.same(ref, got), (depth, env)
    if not env:
        nob, _ = _frame(host_api, scenes, monkeypatch, 4, env, name, kw, w, h, frames, fisheye=fisheye, mask=0)
        traced, b2 = _frame(host_api, scenes, monkeypatch, 4, env, name, kw, w, h, frames, fisheye=fisheye, base=TRACED)
        assert b2 == 0 and sp.same(nob, ref) and sp.same(traced, ref)


@pytest.mark.parametrize("mask", [1, 2, 4, 7])
def test_fan_out_and_total_reflection(mask, scenes, host_api, monkeypatch):
    """the camera inside mixed_small's glass sphere: every pixel is specular, every level fans out by two, straight ahead the reflection
    is total (no refraction record).  Under each mask the frame of every depth is depth 1's"""
    w, h, frames = 64, 40, 3
    ref, _ = _frame(host_api, scenes, monkeypatch, 1, None, "mixed_small", {}, w, h, frames, INSIDE_GLASS, mask=mask)
    for depth in DEPTHS:
        got, _ = _frame(host_api, scenes, monkeypatch, depth, None, "mixed_small", {}, w, h, frames, INSIDE_GLASS, mask=mask)
        assert sp.same(ref, got), (mask, depth)
    if mask == 7:
        traced, _ = _frame(host_api, scenes, monkeypatch, 4, None, "mixed_small", {}, w, h, frames, INSIDE_GLASS, base=TRACED)
        assert sp.same(ref, traced)


def _counted(host_api, scenes, monkeypatch, depth, name, kw, w, h, frames, cam=None, cap=None):
    """a counting launch of 'frames' frames next to current tables: (nearest counters, occluded counters, frame, uncounted frame, builds)"""
    _env(monkeypatch, depth, cap=cap)
    r = _renderer(host_api, scenes, name, kw, w, h, cam)
    r.render(host_api.RT_MODE_PATH, 0, 1)  # the tables are current from here: the counting launch builds nothing
    r.clear()
    r.set_counting(host_api.RT_COUNT_EXECUTED); r.counters()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    near, occl = r.counters_split()
    r.set_counting(False)
    counted = r.accumulator().copy()
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    plain = r.accumulator().copy()
    builds = _builds(r)
    r.close()
    return near, occl, counted, plain, builds


QUERIES = ("rays_nearest", "light_tests", "brute_tests")


@pytest.mark.parametrize("name,kw,w,h,cam", [("mixed_small", {}, 64, 40, INSIDE_GLASS), ("pretty_tlas", {"n_instances": 8}, 160, 90, None)],
                         ids=["inside_glass", "pretty_tlas"])
def test_capacity_overflow(name, kw, w, h, cam, scenes, host_api, monkeypatch):
    """levels of a handful of records and of none: children that do not fit are traced, the bits stay, and the executed walk lies between
    depth 1's and the uncapped run's"""
    frames = 3
    one = _counted(host_api, scenes, monkeypatch, 1, name, kw, w, h, frames, cam)
    full = _counted(host_api, scenes, monkeypatch, 4, name, kw, w, h, frames, cam)
    assert sp.same(one[2], full[2]) and full[0]["inner_visits"] < one[0]["inner_visits"]
    for cap in (0, 1, 7, 64):  # (1: a glass pair never fits; 7: the last slot can stay a hole)
        got = _counted(host_api, scenes, monkeypatch, 4, name, kw, w, h, frames, cam, cap=cap)
        print("cap %d: inner_visits %d (depth 1: %d, uncapped: %d)" % (cap, got[0]["inner_visits"], one[0]["inner_visits"], full[0]["inner_visits"]))
        assert sp.same(one[2], got[2]) and sp.same(got[2], got[3]) and got[4] == 1, cap
        assert full[0]["inner_visits"] <= got[0]["inner_visits"] <= one[0]["inner_visits"], cap
        for k in QUERIES:
            assert got[0][k] == one[0][k], (cap, k)
        assert got[1]["rays_occluded"] == one[1]["rays_occluded"], cap
    zero = _counted(host_api, scenes, monkeypatch, 4, name, kw, w, h, frames, cam, cap=0)
    assert zero[0]["inner_visits"] == one[0]["inner_visits"]  # no record: depth 1's walk


def _chain_pixels(host_api, r, levels):
    """The witness, from the scene alone: per level k = 1 .. levels, the pixels whose camera ray and its first k - 1 MIRROR reflections all
    hit glass or metal (the reflection is a ray both materials can scatter; refractions are left out, so this counts a subset of the
    chain rays of round k).  Hits from rt_intersect_batch, material types from the context's material table: no table under test."""
    w, h = r.w, r.hgt
    pos, tl, tr_, bl = [x.astype(np.float64) for x in r.camera()]
    u = (np.arange(w) + 0.5) / w
    v = (np.arange(h) + 0.5) / h
    P = tl[None, None] + u[None, :, None] * (tr_ - tl)[None, None] + v[:, None, None] * (bl - tl)[None, None]
    D = (P - pos).reshape(-1, 3)
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    O = np.broadcast_to(pos, D.shape).copy()
    types = r.scene_array("mats").view(host_api.RT_MATERIAL_DTYPE)["type"]
    alive = np.ones(len(D), bool)
    counts = []
    for _ in range(levels):
        hit = r.find_nearest(O.astype(f32), D.astype(f32), t_min=1e-3)
        mat = hit["mat"]
        ok = (hit["obj"] >= 0) & (mat >= 0) & (mat < len(types))
        spec = np.zeros(len(D), bool)
        spec[ok] = np.isin(types[mat[ok]], (2, 3))
        alive &= spec
        counts.append(int(alive.sum()))
        N = hit["normal"].astype(np.float64)
        I = O + hit["t"].astype(np.float64)[:, None] * D
        I[~alive] = 0
        Dn = D - 2 * (D * N).sum(1, keepdims=True) * N
        Dn[~alive] = (0, 0, 1)
        O, D = I, Dn
    return counts


def test_every_level_is_read(scenes, host_api, monkeypatch):
    """the witness that the equalities above do not pass on tables nobody reads: with current tables the executed walk of a counting launch
    strictly falls from depth 1 to 2 to 3 to 4 while the queries stay what they were, and the counted frame is the uncounted one"""
    name, kw, w, h, frames = "pretty_tlas", {"n_instances": 8}, 160, 90, 8
    _env(monkeypatch, 1)
    r = _renderer(host_api, scenes, name, kw, w, h)
    chain = _chain_pixels(host_api, r, 4)
    r.close()
    print("pixels on an all-specular mirror chain after 1 .. 4 hits: %s of %d" % (chain, w * h))
    assert all(c > 0 for c in chain), chain  # the precondition: rounds 2-4 have chain rays at this camera
    cnt = {d: _counted(host_api, scenes, monkeypatch, d, name, kw, w, h, frames) for d in (1, 2, 3, 4)}
    print("inner_visits by depth: %s" % {d: cnt[d][0]["inner_visits"] for d in cnt})
    for d in (1, 2, 3, 4):
        assert sp.same(cnt[d][2], cnt[d][3]) and cnt[d][4] == 1, d
    for d in DEPTHS:
        for k in QUERIES:
            assert cnt[d][0][k] == cnt[1][0][k], (d, k, cnt[d][0][k], cnt[1][0][k])
        assert cnt[d][1]["rays_occluded"] == cnt[1][1]["rays_occluded"], d
        assert sp.same(cnt[d][2], cnt[1][2]), d
        assert cnt[d][0]["inner_visits"] < cnt[d - 1][0]["inner_visits"], d


def test_short_batches_read_no_table(scenes, oracle_api, host_api, monkeypatch):
    """rt_trace_batch, the call that offers other round counts than five: caller rays at start depths 0 .. 7 (one to eight rounds: batches
    that end before, at and after the table depth) give the same Sample() values next to current tables of depth 4 as next to depth 1's"""
    from test_gpu_parity import make_pair
    depths = (0, 1, 2, 3, 4, 5, 7)
    out = {}
    for d in (1, 4):
        _env(monkeypatch, d)
        o, orr, r, _ = make_pair(scenes.mixed_small, oracle_api, host_api, 64, 40)
        r.set_profiling(True)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 2)  # every level is current from here
        pO, pD = orr.primary_rays()
        out[d] = [r.trace_batch(host_api.RT_MODE_PATH, pO, pD, depth, 99) for depth in depths]
        assert _builds(r) == 1
        r.close()
    for depth, a, b in zip(depths, out[1], out[4]):
        assert sp.same(a, b), depth


@pytest.mark.parametrize("frames", [1, 12])
def test_one_frame_and_twelve(frames, scenes, host_api, monkeypatch):
    ref, _ = _frame(host_api, scenes, monkeypatch, 1, None, "mixed_small", {}, 96, 63, frames)
    for depth in DEPTHS:
        got, b = _frame(host_api, scenes, monkeypatch, depth, None, "mixed_small", {}, 96, 63, frames)
        assert b == 1 and sp.same(ref, got), depth


def test_row_shards(scenes, host_api, monkeypatch):
    """two interleaved row shards against the whole frame, with one build: the levels are always of the whole frame"""
    w, h, frames = 96, 63, 4
    ref, _ = _frame(host_api, scenes, monkeypatch, 1, None, "mixed_small", {}, w, h, frames)
    _env(monkeypatch, 4)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
    r.clear()
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 0, 2, (h + 1) // 2)
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 1, 2, h // 2)
    assert sp.same(ref, r.accumulator()) and _builds(r) == 1
    r.close()


@pytest.mark.parametrize("name,kw,which", [("mixed_small", {}, "move reupload animate diffuse undiffuse lights"),
                                           ("pretty_tlas", {"n_instances": 4}, "move instance deform diffuse undiffuse lights vertices list")],
                         ids=["scene_bvh", "tlas"])
def test_staleness(name, kw, which, scenes, host_api, monkeypatch):
    """a camera move, a re-upload, rt_set_time, rt_set_instances, rt_set_triangles, rt_set_materials (glass made diffuse, and back),
    rt_set_lights, rt_set_vertices and rt_set_instance_list each make every level stale: the frame of the long-lived renderer at depth 4
    equals a fresh renderer's traced frame, and each rebuild is exactly one more entry of the query slot"""
    import instances_ref as ir
    import triangles_desc as td
    import triangles_ref as tr
    w, h, frames = 80, 45, 3
    M = host_api.RT_MATERIAL_DTYPE
    glass_was = {}

    def move(x):
        c = x.camera()
        d = f32([0.3, 0.1, -0.2])
        x.set_camera(c[0] + d, c[1] + d, c[2] + d, c[3] + d)

    def reupload(x):
        x.commit()

    def animate(x):
        x.scene.set_time(1.3)

    def instance(x):
        d = td.Desc(host_api, x.scene)
        rec = ir.records(host_api, [int(d.inst["blas"][1])], [x.scene.trs((f32(0.3), f32(0.4), f32(4.5)), f32(0.8), 0.0, f32(1.0), 0.0)])
        assert x.set_instances(1, rec) == 0

    def deform(x):
        d = td.Desc(host_api, x.scene)
        v9 = tr.v9_of(d.tris[0])
        sentinel = bool(np.all(v9[-2:] == f32(999)))
        new = v9.copy()
        n = len(v9) - 2 if sentinel else len(v9)
        new[:n] = tr.scale(v9[:n], 1.2)
        assert x.set_triangles(0, tr.triangles(d.tris[0], new, tr.sentinel_normals(new) if sentinel else None)) == 0

    def diffuse(x):
        """every glass material becomes a copy of a diffuse one: the chains through it end"""
        m = x.scene_array("mats").view(M).copy()
        g, dif = np.flatnonzero(m["type"] == 3), np.flatnonzero(m["type"] == 1)
        assert len(g) and len(dif)
        glass_was[id(x)] = m.copy()
        m[g] = m[dif[0]]
        assert x.set_materials(0, m) == 0

    def undiffuse(x):
        """... and back (on a renderer that never went there: the table as it is, an edit all the same)"""
        m = glass_was.pop(id(x), None)
        assert x.set_materials(0, x.scene_array("mats").view(M).copy() if m is None else m) == 0

    def lights(x):
        l = x.scene_array("lights").view(host_api.RT_LIGHT_DTYPE).copy()
        assert len(l) and l["strength"][0] > 0
        l["strength"] *= f32(0.5)
        l["pos"][0] += f32([0.4, 0.0, -0.3])
        assert x.set_lights(l) == 0

    def vertices(x):
        d = td.Desc(host_api, x.scene)
        xyz = tr.v9_of(d.tris[0]).reshape(-1, 3).copy()
        idx = np.arange(len(xyz), dtype=np.uint32).reshape(-1, 3)
        keep = (xyz == f32(999)).all(1)
        new = np.where(keep[:, None], xyz, (xyz * f32(0.9)).astype(f32))
        assert x.set_mesh_indices(0, idx, len(xyz)) == 0 and x.set_vertices(0, new) == 0

    def ilist(x):
        d = td.Desc(host_api, x.scene)
        rec = np.zeros(len(d.inst) - 1, host_api.RT_INSTANCE_DTYPE)
        for k in ("blas", "transform", "inv_transform"):
            rec[k] = d.inst[k][1:]
        assert x.set_instance_list(rec) == 0

    def fresh(steps):
        _env(monkeypatch, 1, base=TRACED)
        f = _renderer(host_api, scenes, name, kw, w, h)
        for s in steps:
            s(f)
        f.clear()
        f.render(host_api.RT_MODE_PATH, 0, frames)
        out = f.accumulator().copy()
        f.close()
        return out

    _env(monkeypatch, 4)
    r = _renderer(host_api, scenes, name, kw, w, h)
    steps, seen = [], {}
    todo = dict(move=move, reupload=reupload, animate=animate, instance=instance, deform=deform, diffuse=diffuse, undiffuse=undiffuse,
                lights=lights, vertices=vertices, list=ilist)
    for key in [None] + which.split():
        if key:
            todo[key](r)
            steps.append(todo[key])
        before = _builds(r)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        got = r.accumulator().copy()
        assert _builds(r) == before + 1, (key, before, _builds(r))
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)  # ... and once more from the levels as they stand
        assert sp.same(got, r.accumulator()) and _builds(r) == before + 1, key
        seen[key] = got
        ref = fresh(list(steps))
        _env(monkeypatch, 4)
        assert sp.same(ref, got), key
    order = [None] + which.split()
    prev = lambda key: seen[order[order.index(key) - 1]]
    for key in ("move", "diffuse", "lights") + (("vertices", "list") if "list" in seen else ()):
        assert not sp.same(prev(key), seen[key]), key  # the edits really changed the frame
    assert sp.same(prev("diffuse"), seen["undiffuse"])  # ... and the glass came back
    r.close()


def test_with_sampler(host_api, monkeypatch):
    """the Q-learning sampler on: accumulator, Q table and pending reward sums are the same bits at depth 1 and depth 4 (W.w is the
    sampler's key word: the deeper levels are off there, and not built)"""
    from lit_scene import lit_scene
    w, h, frames = 64, 40, 3
    out = {}
    for depth in (1, 4):
        _env(monkeypatch, depth)
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
        out[depth] = (r.accumulator().copy(), r.qlearn_table().copy(), sums, [x.copy() for x in r.qlearn_sums()])
        assert _builds(r) == 1
        r.close()
    a, b = out[1], out[4]
    assert sp.same(a[0], b[0]) and sp.same(a[1], b[1])
    for k in (2, 3):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])
    assert a[2][1].sum() > 0  # rewards were paid


def test_oracle_frame(scenes, oracle_api, host_api, monkeypatch):
    """the oracle's frame of mixed_small 96 x 64 within the project's tolerance at depth 4"""
    from test_gpu_parity import check_frames, make_pair
    _env(monkeypatch, 4)
    o, orr, r, d = make_pair(scenes.mixed_small, oracle_api, host_api, 96, 64)
    r.set_profiling(True)
    check_frames(orr, r, "path", 3, host_api)
    assert _builds(r) == 1
    r.close()


def test_threshold(scenes, host_api, monkeypatch):
    """RT_PRIMARY_TABLE_MIN at its default: a one-frame batch after a camera move builds nothing, a long batch builds levels 0-1 and the
    deeper ones in one entry, and the frames are depth 1's"""
    w, h = 96, 63
    out = {}
    for depth in (1, 4):
        _env(monkeypatch, depth, base={"RT_PRIMARY_TABLE": "1"})
        r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 40)  # past both thresholds at once
        assert _builds(r) == 1
        acc = [r.accumulator().copy()]
        for k in range(3):  # a camera that moves before every one-frame batch
            c = r.camera()
            d = f32([0.05, 0.0, 0.02])
            r.set_camera(c[0] + d, c[1] + d, c[2] + d, c[3] + d)
            r.clear()
            r.render(host_api.RT_MODE_PATH, k, 1)
            assert _builds(r) == 1, k
            acc.append(r.accumulator().copy())
        out[depth] = acc
        r.close()
    for a, b in zip(out[1], out[4]):
        assert sp.same(a, b)


def test_levels_built_behind_the_first_two(scenes, host_api, monkeypatch):
    """batches that cross the primary table's threshold first and the deeper levels' later: levels 0-1 are built by the first crossing,
    levels 2-4 by the second as an entry of their own, and the frames are depth 1's throughout"""
    w, h = 96, 63
    out = {}
    for depth in (1, 4):
        _env(monkeypatch, depth, base={"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "2"})
        monkeypatch.setenv("RT_BOUNCE_DEPTH_MIN", "3")
        r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
        r.clear()
        builds, acc = [], []
        for k in range(4):  # 3 frames each, 0.95 samples per record and frame: levels 0-1 at 2 samples per record, the deeper ones at 6
            r.render(host_api.RT_MODE_PATH, 3 * k, 3)
            builds.append(_builds(r))
            acc.append(r.accumulator().copy())
        assert builds == ([1, 1, 1, 1] if depth == 1 else [1, 1, 2, 2]), builds
        out[depth] = acc
        r.close()
    for a, b in zip(out[1], out[4]):
        assert sp.same(a, b)
