"""The first bounce off a glass or metal primary hit from the bounce table (csrc/rt_stream.h BounceTable, k_bounce_table, k_shade_s<QL, BOUNCE>).

A camera ray is a function of an integer pixel of [-1, width] x [-1, height] (tests/test_gpu_primary_table.py), and so are its hit, the
hit's normal and t.  The ray Sample scatters at a METAL hit takes no draw, and at a GLASS hit a draw only chooses between two rays, so
Scene::FindNearest of the round-1 ray of such a sample is one of 2 (width + 2)(height + 2) answers, which the table holds and shade(0)
reads instead of tracing.  Held here, always against the same build with RT_BOUNCE_TABLE=0 and once per scene against RT_PRIMARY_TABLE=0
(everything traced): accumulator bits over scenes, cameras, schedules and RT_DECIDE; records of the table's border; a camera inside
glass; one frame and many; row shards; that each branch of the table is really read (the executed walk of a counting launch gets
shorter under every bit of the mask, its queries stay what they were); staleness; the Q-learning sampler; the oracle's frame.

RT_BOUNCE_TABLE is not one of support.KNOBS (that list is the library's num() knobs): _env clears it here."""
import numpy as np
import pytest

import support as sp

pytestmark = pytest.mark.gpu
f32 = np.float32
TABLE = {"RT_PRIMARY_TABLE": "1", "RT_PRIMARY_TABLE_MIN": "0"}  # MIN=0: the first batch builds the tables, whatever its size
TRACED = {"RT_PRIMARY_TABLE": "0"}


def _env(monkeypatch, mask, more=None, base=TABLE):
    monkeypatch.delenv("RT_BOUNCE_TABLE", raising=False)
    sp.clean_env(monkeypatch, dict(base, **(more or {})))
    if mask is not None:
        monkeypatch.setenv("RT_BOUNCE_TABLE", str(mask))


def _builds(r):
    """entries of the profile's query slot so far: one per build of the two tables (profiling on; these tests run no other query)"""
    return r.profile(reset=False)["query"]["launches"]


def _looking(p, half_w, half_h, dist=1.0):
    """a camera at p looking along +z at a screen of the given half sizes at the given distance"""
    p = np.asarray(p, f32)
    return (p, p + f32([-half_w, half_h, dist]), p + f32([half_w, half_h, dist]), p + f32([-half_w, -half_h, dist]))


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


def _frame(host_api, scenes, monkeypatch, mask, more, name, kw, w, h, frames, cam=None, fisheye=None, base=TABLE):
    _env(monkeypatch, mask, more, base)
    r = _renderer(host_api, scenes, name, kw, w, h, cam, fisheye)
    assert ("bounce_table=%d" % (7 if mask is None else mask)) in r.build_info()
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, frames)
    out = r.accumulator().copy()
    builds = _builds(r)
    r.close()
    return out, builds


FISHEYE = dict(fisheye=True, view_angle=0.4, y_angle=0.3)
CASES = [
    ("pretty_tlas", {"n_instances": 8}, 240, 135, None),  # instanced glass + metal, the glass and metal spheres by brute force
    ("mixed_small", {}, 96, 63, None),                    # a scene BVH, glass WITH absorption; groups of 64 entries straddle rows
    ("mixed_small", {}, 64, 40, FISHEYE),
    ("background", {}, 96, 64, None),                     # glass over a sky: refracted rays leave the scene and take class 0
]
VARIANTS = [{}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"}, {"RT_DECIDE": "0"}]


@pytest.mark.parametrize("name,kw,w,h,fisheye", CASES)
def test_frames_equal_traced_frames(name, kw, w, h, fisheye, scenes, host_api, monkeypatch):
    """every schedule and RT_DECIDE=0: the accumulator bits of mask 7 (the default) equal mask 0's, and once per scene those of a frame
    with every ray traced"""
    frames = 3
    for env in VARIANTS:
        ref, b0 = _frame(host_api, scenes, monkeypatch, 0, env, name, kw, w, h, frames, fisheye=fisheye)
        got, b1 = _frame(host_api, scenes, monkeypatch, None, env, name, kw, w, h, frames, fisheye=fisheye)
        assert b0 == 1 and b1 == 1, (env, b0, b1)  # the two tables are one entry of the query slot
        assert np.isfinite(ref[..., :3]).mean() > 0.5
        assert sp.same(ref, got), env
        if not env:
            traced, b2 = _frame(host_api, scenes, monkeypatch, None, env, name, kw, w, h, frames, fisheye=fisheye, base=TRACED)
            assert b2 == 0 and sp.same(traced, got)


# the spheres of mixed_small (scenes.py): metal at (-0.5, 0.25, -0.3) r 0.25, glass at (0.2, 0.35, 0.2) r 0.35
@pytest.mark.parametrize("centre,back", [((-0.5, 0.25, -0.3), 0.6), ((0.2, 0.35, 0.2), 0.8)], ids=["metal", "glass"])
def test_border_records(centre, back, scenes, host_api, monkeypatch):
    """a camera so close to a metal / glass sphere that the whole frame lies on it: the records of px = -1, W and py = -1, H are specular
    and get read"""
    w, h, frames = 70, 41, 3
    cam = _looking(np.asarray(centre, f32) - f32([0, 0, back]), 0.12, 0.07)
    _env(monkeypatch, 0)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h, cam)
    obj, t = r.primary_hits(1e-6)
    r.close()
    assert len(np.unique(obj)) == 1 and obj.flat[0] >= 0 and np.isfinite(t).all()  # one object fills the frame
    ref, _ = _frame(host_api, scenes, monkeypatch, 0, None, "mixed_small", {}, w, h, frames, cam)
    got, _ = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, cam)
    traced, _ = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, cam, base=TRACED)
    assert sp.same(ref, got) and sp.same(traced, got)


def test_inside_glass(scenes, host_api, monkeypatch):
    """a camera inside the glass sphere, 0.3 of its radius 0.35 off the centre: every primary hit comes from inside (outside == false).
    Straight ahead the surface is met at asin(0.3 / 0.35) = 59 degrees, past the critical angle of ir 1.5 (41.8): total internal
    reflection, no refraction record, the reflection always taken; towards +x the incidence is near normal and the ray refracts."""
    w, h, frames = 64, 40, 3
    cam = _looking(f32([0.2 + 0.3, 0.35, 0.2]), 1.6, 1.0)
    ref, _ = _frame(host_api, scenes, monkeypatch, 0, None, "mixed_small", {}, w, h, frames, cam)
    got, _ = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, cam)
    traced, _ = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, w, h, frames, cam, base=TRACED)
    assert sp.same(ref, got) and sp.same(traced, got)
    for mask in (2, 4):
        one, _ = _frame(host_api, scenes, monkeypatch, mask, None, "mixed_small", {}, w, h, frames, cam)
        assert sp.same(ref, one), mask


@pytest.mark.parametrize("frames", [1, 12])
def test_one_frame_and_many(frames, scenes, host_api, monkeypatch):
    ref, _ = _frame(host_api, scenes, monkeypatch, 0, None, "mixed_small", {}, 96, 63, frames)
    got, b = _frame(host_api, scenes, monkeypatch, None, None, "mixed_small", {}, 96, 63, frames)
    assert b == 1 and sp.same(ref, got)


def test_row_shards(scenes, host_api, monkeypatch):
    """two interleaved row shards against the whole frame: the tables are always of the whole frame"""
    w, h, frames = 96, 63, 4
    ref, _ = _frame(host_api, scenes, monkeypatch, 0, None, "mixed_small", {}, w, h, frames)
    _env(monkeypatch, None)
    r = _renderer(host_api, scenes, "mixed_small", {}, w, h)
    r.clear()
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 0, 2, (h + 1) // 2)
    r.render_rows(host_api.RT_MODE_PATH, 0, frames, 1, 2, h // 2)
    assert sp.same(ref, r.accumulator()) and _builds(r) == 1
    r.close()


def test_each_branch_is_read(scenes, host_api, monkeypatch):
    """the witness that the equalities above do not pass on a table nobody reads: with a current table, the executed walk of a counting
    launch is shorter under each bit of the mask than under mask 0 and shortest under mask 7, while the queries are the same"""
    w, h, frames = 160, 90, 8
    cnt = {}
    for mask in (0, 1, 2, 4, 7):
        _env(monkeypatch, mask)
        r = _renderer(host_api, scenes, "pretty_tlas", {"n_instances": 8}, w, h)
        r.render(host_api.RT_MODE_PATH, 0, 1)  # the tables are current from here: the counting launch builds nothing
        r.clear()
        r.set_counting(host_api.RT_COUNT_EXECUTED); r.counters()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        near, occl = r.counters_split()
        r.set_counting(False)
        counted = r.accumulator().copy()
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        assert sp.same(counted, r.accumulator()), mask  # the counted frame is the uncounted one
        assert _builds(r) == 1
        cnt[mask] = (near, occl, counted)
        r.close()
    for mask in (1, 2, 4, 7):
        for k in ("rays_nearest", "light_tests", "brute_tests"):
            assert cnt[mask][0][k] == cnt[0][0][k], (mask, k, cnt[mask][0][k], cnt[0][0][k])
        assert cnt[mask][1]["rays_occluded"] == cnt[0][1]["rays_occluded"], mask
        assert sp.same(cnt[mask][2], cnt[0][2]), mask
    for mask in (1, 2, 4):
        assert cnt[mask][0]["inner_visits"] < cnt[0][0]["inner_visits"], mask
        assert cnt[7][0]["inner_visits"] < cnt[mask][0]["inner_visits"], mask


@pytest.mark.parametrize("name,kw,which", [("mixed_small", {}, "move reupload animate"), ("pretty_tlas", {"n_instances": 4}, "move instance deform")],
                         ids=["scene_bvh", "tlas"])
def test_staleness(name, kw, which, scenes, host_api, monkeypatch):
    """a camera move, a re-upload, rt_set_time (the reference animates only without the TLAS), rt_set_instances and rt_set_triangles each
    make the tables stale: the frame of the long-lived renderer equals a fresh renderer's traced frame, and each rebuild is exactly one
    more entry of the query slot"""
    import instances_ref as ir
    import triangles_desc as td
    import triangles_ref as tr
    w, h, frames = 80, 45, 3

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

    def fresh(steps):
        _env(monkeypatch, None, base=TRACED)
        f = _renderer(host_api, scenes, name, kw, w, h)
        for s in steps:
            s(f)
        f.clear()
        f.render(host_api.RT_MODE_PATH, 0, frames)
        out = f.accumulator().copy()
        f.close()
        return out

    _env(monkeypatch, None)
    r = _renderer(host_api, scenes, name, kw, w, h)
    steps, seen = [], []
    todo = dict(move=move, reupload=reupload, animate=animate, instance=instance, deform=deform)
    for step in [None] + [todo[k] for k in which.split()]:
        if step:
            step(r)
            steps.append(step)
        before = _builds(r)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)
        got = r.accumulator().copy()
        assert _builds(r) == before + 1, (len(steps), before, _builds(r))
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, frames)  # ... and once more from the tables as they stand
        assert sp.same(got, r.accumulator()) and _builds(r) == before + 1
        seen.append(got)
        ref = fresh(list(steps))
        _env(monkeypatch, None)
        assert sp.same(ref, got), len(steps)
    assert not sp.same(seen[0], seen[1]) and not sp.same(seen[2], seen[3])  # the camera and the geometry really moved
    if "instance" in which:
        assert not sp.same(seen[1], seen[2])
    r.close()


def test_diffuse_scene_builds_no_bounce_table(scenes, host_api, monkeypatch):
    """a scene without glass or metal has no bounce table (rt_api_render.inc primary_table_for launches and allocates nothing for it):
    one entry of the query slot as before, the same frame"""
    kw = {"force_diffuse": True, "split": 3}
    ref, b0 = _frame(host_api, scenes, monkeypatch, 0, None, "scene3", kw, 96, 54, 3)
    got, b1 = _frame(host_api, scenes, monkeypatch, None, None, "scene3", kw, 96, 54, 3)
    traced, b2 = _frame(host_api, scenes, monkeypatch, None, None, "scene3", kw, 96, 54, 3, base=TRACED)
    assert (b0, b1, b2) == (1, 1, 0) and sp.same(ref, got) and sp.same(traced, got)


def test_with_sampler(host_api, monkeypatch):
    """the Q-learning sampler on: accumulator, Q table and pending reward sums are the same bits under either mask"""
    from lit_scene import lit_scene
    w, h, frames = 64, 40, 3
    out = {}
    for mask in (0, 7):
        _env(monkeypatch, mask)
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
        out[mask] = (r.accumulator().copy(), r.qlearn_table().copy(), sums, [x.copy() for x in r.qlearn_sums()])
        assert _builds(r) == 1
        r.close()
    a, b = out[0], out[7]
    assert sp.same(a[0], b[0]) and sp.same(a[1], b[1])
    for k in (2, 3):
        assert np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])
    assert a[2][1].sum() > 0  # rewards were paid


def test_oracle_frame(scenes, oracle_api, host_api, monkeypatch):
    """the oracle's frame within the project's tolerance with both tables on"""
    from test_gpu_parity import check_frames, make_pair
    _env(monkeypatch, None)
    o, orr, r, d = make_pair(scenes.mixed_small, oracle_api, host_api, 96, 64)
    r.set_profiling(True)
    check_frames(orr, r, "path", 3, host_api)
    assert _builds(r) == 1
    r.close()
