"""rt_set_lights, rt_set_materials and rt_set_sky on the device (include/rt_amd.h, csrc/rt_materials.h), through the C ABI: after an edit the
context holds, byte for byte, what a fresh rt_upload_scene of the updated description would -- the arrays themselves (rt_scene_array and
rt_blas_array against rt_layout_build), every frame, traced batch and executed-walk counter against a freshly uploaded context, the
radiance against the oracle on the edited scene built from scratch -- and the calls invalidate what they must, refuse bad input on the host
and leave the scene as it was when they refuse.  Comparisons between contexts and with rt_layout_build are bitwise; the oracle is held at
the suite's radiance tolerance.  The cases are tests/look_cases.py's, shown not to be vacuous by tests/test_look_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import instances_ref as ir
import look_cases as lc
import support as sp
import triangles_desc as td
import triangles_ref as tr
from conftest import random_rays, rel_err
from test_gpu_parity import RADIANCE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
ENVS = [{}, {"RT_TLAS_LDS": "0", "RT_WIDE": "1"}]
ENV_IDS = ["default", "wide_no_lds"]
SCENE_ARRAYS = ("pairs", "reach", "brute", "inst", "lights", "mats")


def _env(monkeypatch, env=None):
    sp.clean_env(monkeypatch, env)
    return sp.layout_knobs(env)


def _scalars(s):
    """RT_LAYOUT_SCALARS without wideOK and wide8OK (words 9 and 10 keep their upload-time values)"""
    return np.delete(np.asarray(s), [9, 10])


def _renderer(host_api, build, **kw):
    r = host_api.HostRenderer(lc.W, lc.H)
    build(r.scene, **kw)
    r.commit()
    return r


def _snapshot(r, n_blas, ctx=None):
    out = {a: r.scene_array(a, ctx) for a in SCENE_ARRAYS + ("scalars",)}
    for k in range(n_blas):
        out["pairs%d" % k], out["prims%d" % k] = r.blas_array(k, "pairs", ctx), r.blas_array(k, "prims", ctx)
    return out


def _check_layout(host_api, r, d, knobs, what, ctx=None):
    """the context's arrays equal rt_layout_build's of the updated description d"""
    L = host_api.layout(d.desc(), *knobs)
    for k, (p0, p1, s0, s1) in enumerate(d.ranges()):
        assert sp.same(r.blas_array(k, "prims", ctx), L["prims"][16 * s0:16 * s1]), "%s: the primitive records of blas %d" % (what, k)
        assert sp.same(r.blas_array(k, "pairs", ctx), L["pairs"][16 * p0:16 * p1]), "%s: the pair records of blas %d" % (what, k)
    for a in SCENE_ARRAYS:
        assert sp.same(r.scene_array(a, ctx), L[a]), "%s: %s differs from rt_layout_build of the updated description" % (what, a)
    assert np.array_equal(_scalars(r.scene_array("scalars", ctx)), _scalars(L["scalars"])), "%s: scalars" % what
    return L


def _send_materials(host_api, r, e, ctx=None):
    rec = lc.scene_tables(host_api, mats=e["after"])[0]
    return r.set_materials(e["first"], rec[e["first"]:e["first"] + e["count"]], ctx), rec


# ---- 1. the arrays ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tlas", [False, True], ids=["bvh", "tlas"])
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_arrays_equal_a_fresh_layout(tlas, env, host_api, monkeypatch):
    knobs = _env(monkeypatch, env)
    r = _renderer(host_api, lc.look_scene, tlas=tlas)
    d = td.Desc(host_api, r.scene)
    _check_layout(host_api, r, d, knobs, "as uploaded")
    geometry = {a: r.scene_array(a) for a in ("pairs", "reach", "inst")}
    for name, e in lc.MATERIAL_EDITS.items():
        before = lc.scene_tables(host_api, mats=e["before"])[0]
        assert r.set_materials(0, before) == 0, name  # the state the edit starts from: an edit of the whole table itself
        _check_layout(host_api, r, lc.patch(d, mats=before), knobs, name + ": before")
        was = _snapshot(r, len(d.blas))
        rc, after = _send_materials(host_api, r, e)
        assert rc == 0, name
        L = _check_layout(host_api, r, lc.patch(d, mats=after), knobs, name)
        now = _snapshot(r, len(d.blas))
        changed = {a for a in now if not sp.same(now[a], was[a])}
        assert "mats" in changed and ("scalars" in changed) == (e["unsupported"][0] != e["unsupported"][1]), (name, changed)
        assert bool(changed & {"brute"} | {a for a in changed if a.startswith("prims")}) == e["type"], (name, changed)
        assert int(L["scalars"][11]) == e["unsupported"][1]
    for n in lc.LIGHT_TABLES + (0, 1, 32, 0):
        rec = lc.scene_tables(host_api, lights=lc.lights(n))[1]
        assert r.set_lights(rec) == 0 and len(r.scene_array("lights")) == 14 * max(n, 1), n
        _check_layout(host_api, r, lc.patch(d, lights=rec), knobs, "%d lights" % n)
    for name, sky in lc.SKY_EDITS.items():
        px = None if sky is None else lc.sky_image(*sky)
        assert r.set_sky(px) == 0, name
        _check_layout(host_api, r, lc.patch(d, sky=px), knobs, "sky " + name)
    for a, v in geometry.items():
        assert sp.same(r.scene_array(a), v), a + " is untouched"
    r.close()


@pytest.mark.parametrize("n", lc.STRIP_SIZES)
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_record_counts_around_the_block(n, env, host_api, monkeypatch):
    """1 (a leaf root), 255, 256 and 257 records: the last lane of a block, a full block, one record into the next"""
    knobs = _env(monkeypatch, env)
    r = _renderer(host_api, lambda s: lc.strip_scene(s, n))
    d = td.Desc(host_api, r.scene)
    mats = lc.tables(d.ptr)[0]
    for step in range(3):  # diffuse -> metal -> glass -> diffuse
        mats = lc.retyped(mats)
        assert r.set_materials(0, mats) == 0
        L = _check_layout(host_api, r, lc.patch(d, mats=mats), knobs, "%d records, step %d" % (n, step))
        assert len(L["prims"]) == 16 * n
    # rt_set_time deforms from the originals: they carry the new type too
    fresh = host_api.HostRenderer(lc.W, lc.H)
    fresh.upload_desc(d.desc())
    for x in (r, fresh):
        x.set_time(0.7)
    for a in ("pairs", "prims"):
        assert sp.same(r.blas_array(0, a), fresh.blas_array(0, a)), a
    fresh.close(), r.close()


@pytest.mark.parametrize("name", td.LAYOUT_CASES + ("tlas_test2", "background"))
@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_the_suite_scenes_retyped(name, env, scenes, host_api, monkeypatch):
    """every material of a scene the tests did not make takes the next type, twice: all BLASes, under a TLAS or not"""
    knobs = _env(monkeypatch, env)
    r = host_api.HostRenderer(lc.W, lc.H)
    if name in td.LAYOUT_CASES:
        td.build_case(r.scene, name, scenes)
    else:
        scenes.REGISTRY[name](r.scene)
    r.commit()
    d = td.Desc(host_api, r.scene)
    mats = lc.tables(d.ptr)[0]
    base = _snapshot(r, len(d.blas))
    for step in range(2):
        mats = lc.retyped(mats)
        assert r.set_materials(0, mats) == 0
        _check_layout(host_api, r, lc.patch(d, mats=mats), knobs, "%s, step %d" % (name, step))
    now = _snapshot(r, len(d.blas))
    assert any(not sp.same(now[a], base[a]) for a in now if a.startswith("prims"))
    r.close()


def test_material_indices_outside_the_table(host_api, monkeypatch):
    """a primitive whose material index is -1 or n_materials keeps type bits 0 through every edit"""
    knobs = _env(monkeypatch)
    r = _renderer(host_api, lc.look_scene)
    d = td.Desc(host_api, r.scene)
    d.tris[0]["material"][0], d.tris[0]["material"][1] = -1, 4
    r.upload_desc(d.desc())
    _check_layout(host_api, r, d, knobs, "as uploaded")
    mats = lc.retyped(lc.tables(d.ptr)[0])
    assert r.set_materials(0, mats) == 0
    L = _check_layout(host_api, r, lc.patch(d, mats=mats), knobs, "retyped")
    kind, w = lc.kind_words(L["prims"])
    assert (kind & lc.TYPE_MASK == 0).sum() == 2
    r.close()


# ---- 2. stale answers: the results are a fresh upload's, and the oracle's -----------------------------------------------------------------------
RAYS = random_rays(256, 11, center=(0.0, 0.8, 1.0), spread=2.0)


def _results(r, host_api):
    """what a context answers: path frames (4 and 16 more spp: the second batch is past RT_PRIMARY_TABLE_MIN, a stale table would show
    there), a Whitted frame, traced batches, the sky, and the executed-walk counters of a path frame"""
    P, Wh = host_api.RT_MODE_PATH, host_api.RT_MODE_WHITTED
    out = {}
    r.clear()
    r.render(P, 0, 4)
    out["path4"] = r.accumulator()
    r.render(P, 4, 16)
    out["path20"] = r.accumulator()
    r.clear()
    r.render(Wh, 0, 1)
    out["whitted"] = r.accumulator()
    out["trace_path"], out["trace_whitted"] = r.trace_batch(P, *RAYS), r.trace_batch(Wh, *RAYS)
    out["sky"] = r.sky_color(RAYS[1])
    r.set_counting(host_api.RT_COUNT_EXECUTED)
    r.counters()
    r.clear()
    r.render(P, 0, 1)
    out["counted"], out["counters"] = r.accumulator(), r.counters()
    r.set_counting(False)
    r.clear()
    return out


def _same_results(a, b, what):
    for k in a:
        if k == "counters":
            assert a[k] == b[k], "%s: the executed walk differs from a fresh upload's" % what
        else:
            assert sp.same(a[k], b[k]), "%s: %s differs from a fresh upload's" % (what, k)


def _oracle_results(oracle_api, **kw):
    o = oracle_api.OracleScene()
    lc.look_scene(o, **kw)
    orr = oracle_api.OracleRenderer(o, lc.W, lc.H)
    out = {}
    o.set_raytracer(False)
    orr.clear()
    orr.render(0, 4, nthreads=0)
    out["path4"] = orr.accumulator()
    out["trace_path"] = orr.trace_rays(1, *RAYS)
    o.set_raytracer(True)
    orr.clear()
    orr.render(0, 1, nthreads=0)
    out["whitted"] = orr.accumulator()
    out["trace_whitted"] = orr.trace_rays(0, *RAYS)
    out["sky"] = o.sky_color(RAYS[1])
    orr.close(), o.close()
    return out


def _hold_to_oracle(got, ref, what):
    for k, want in ref.items():
        g, w = (got[k][..., :3], want[..., :3]) if want.ndim == 3 else (got[k], want)
        err, cls_ok = rel_err(g, w)
        print("%s %s: max relative error %.3g" % (what, k, err.max()))
        assert cls_ok, "%s %s: non-finite values differ by class" % (what, k)
        assert err.max() <= RADIANCE_TOL, "%s %s: max relative radiance error %g" % (what, k, err.max())


def _warm(r, host_api):
    """path frames past RT_PRIMARY_TABLE_MIN: the primary-hit and bounce tables are current, of the scene before the edit"""
    r.render(host_api.RT_MODE_PATH, 0, 16)
    r.render_aovs(0.001)


PIPELINES = [({}, False), ({}, True), ({"RT_STREAM": "0"}, True), ({"RT_MEGA": "0"}, False), ({"RT_MEGA_LEVELS": "1", "RT_WIDE": "1"}, False)]
PIPELINE_IDS = ["dense_bvh", "dense_tlas", "slot_tlas", "slot_whitted_bvh", "levels_wide_bvh"]


@pytest.mark.parametrize("name", list(lc.MATERIAL_EDITS))
@pytest.mark.parametrize("env,tlas", PIPELINES[:3], ids=PIPELINE_IDS[:3])
def test_material_edits_answer_like_a_fresh_upload(name, env, tlas, host_api, oracle_api, monkeypatch):
    _env(monkeypatch, env)
    e = lc.MATERIAL_EDITS[name]
    a = _renderer(host_api, lc.look_scene, tlas=tlas, mats=e["before"])
    _warm(a, host_api)
    assert _send_materials(host_api, a, e)[0] == 0
    b = _renderer(host_api, lc.look_scene, tlas=tlas, mats=e["after"])
    got = _results(a, host_api)
    _same_results(got, _results(b, host_api), name)
    _hold_to_oracle(got, _oracle_results(oracle_api, tlas=tlas, mats=e["after"]), name)
    a.close(), b.close()


def test_the_general_kernel_and_back(host_api, oracle_api, monkeypatch):
    """shinieness 0 -> 0.5 sends path mode to the general kernel, 0.5 -> 0 brings the wavefront back: one context, both ways"""
    _env(monkeypatch)
    on, off = lc.MATERIAL_EDITS["shiny_on"], lc.MATERIAL_EDITS["shiny_off"]
    a = _renderer(host_api, lc.look_scene, mats=on["before"])
    _warm(a, host_api)
    for e, what in ((on, "shiny"), (off, "plain again"), (on, "shiny again")):
        assert _send_materials(host_api, a, e)[0] == 0 and int(a.scene_array("scalars")[11]) == e["unsupported"][1]
        b = _renderer(host_api, lc.look_scene, mats=e["after"])
        got = _results(a, host_api)
        _same_results(got, _results(b, host_api), what)
        _hold_to_oracle(got, _oracle_results(oracle_api, mats=e["after"]), what)
        b.close()
    a.close()


@pytest.mark.parametrize("env,tlas", PIPELINES[:3], ids=PIPELINE_IDS[:3])
def test_sky_edits_answer_like_a_fresh_upload(env, tlas, host_api, oracle_api, monkeypatch):
    _env(monkeypatch, env)
    a = _renderer(host_api, lc.look_scene, tlas=tlas)
    _warm(a, host_api)
    for name in ("larger", "same_size", "none", "smaller", "larger"):  # grows, fits, off, fits again, fits the largest
        sky = lc.SKY_EDITS[name]
        assert a.set_sky(None if sky is None else lc.sky_image(*sky)) == 0
        b = _renderer(host_api, lc.look_scene, tlas=tlas, sky=sky)
        got = _results(a, host_api)
        _same_results(got, _results(b, host_api), "sky " + name)
        assert (got["sky"] != 0).any() == (sky is not None)
        _hold_to_oracle(got, _oracle_results(oracle_api, tlas=tlas, sky=sky), "sky " + name)
        b.close()
    a.close()


# ---- 3. the light count ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,tlas", PIPELINES, ids=PIPELINE_IDS)
def test_the_light_count_changes_between_renders(env, tlas, host_api, oracle_api, monkeypatch):
    """0 -> 1 -> 32 -> 0 in one context: the per-light planes of every pipeline's state follow the count"""
    _env(monkeypatch, env)
    a = _renderer(host_api, lc.look_scene, tlas=tlas, lights=lc.lights(0))
    _warm(a, host_api)
    fresh = {}
    for n in (0, 1, 32, 0, 31):
        if n not in fresh:
            b = _renderer(host_api, lc.look_scene, tlas=tlas, lights=lc.lights(n))
            fresh[n] = _results(b, host_api)
            b.close()
        assert a.set_lights(lc.scene_tables(host_api, lights=lc.lights(n))[1]) == 0
        got = _results(a, host_api)
        _same_results(got, fresh[n], "%d lights" % n)
        assert (got["counters"]["light_tests"] > 0) == (n > 0)
        if not env:
            _hold_to_oracle(got, _oracle_results(oracle_api, tlas=tlas, lights=lc.lights(n)), "%d lights" % n)
    a.close()


# ---- 4. composition with the other in-place edits ---------------------------------------------------------------------------------------------------
def test_set_time_after_a_type_change(host_api, monkeypatch):
    _env(monkeypatch)
    e = lc.MATERIAL_EDITS["diffuse_to_metal"]
    a = _renderer(host_api, lc.look_scene, mats=e["before"])
    assert _send_materials(host_api, a, e)[0] == 0
    b = _renderer(host_api, lc.look_scene, mats=e["after"])
    still = a.blas_array(0, "prims")
    for x in (a, b):
        x.set_time(0.7)
    for arr in ("pairs", "prims"):
        assert sp.same(a.blas_array(0, arr), b.blas_array(0, arr)), "rt_set_time after the edit: " + arr
    assert not sp.same(a.blas_array(0, "prims"), still), "the animation moved the triangles"
    _same_results(_results(a, host_api), _results(b, host_api), "animated")
    a.close(), b.close()


def test_set_triangles_after_a_type_change(host_api, monkeypatch):
    """k_set_triangles reads the type from the device's table: the edited one"""
    knobs = _env(monkeypatch)
    e = lc.MATERIAL_EDITS["metal_to_glass"]
    for tlas in (False, True):
        a = _renderer(host_api, lc.look_scene, tlas=tlas, mats=e["before"])
        d = td.Desc(host_api, a.scene)
        rc, after = _send_materials(host_api, a, e)
        assert rc == 0
        lc.patch(d, mats=after)
        assert a.set_triangles(0, d.deform(0, tr.twist(tr.v9_of(d.tris[0])))) == 0
        _check_layout(host_api, a, d, knobs, "deformed after the edit")
        b = host_api.HostRenderer(lc.W, lc.H)
        b.upload_desc(d.desc())
        for k in range(len(d.blas)):
            assert sp.same(a.blas_array(k, "prims"), b.blas_array(k, "prims")) and sp.same(a.blas_array(k, "pairs"), b.blas_array(k, "pairs"))
        a.close(), b.close()


def test_set_instances_after_set_lights(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    a = _renderer(host_api, lc.look_scene, tlas=True)
    d = td.Desc(host_api, a.scene)
    rec = lc.scene_tables(host_api, lights=lc.lights(5))[1]
    assert a.set_lights(rec) == 0
    lc.patch(d, lights=rec)
    move = ir.records(host_api, [int(d.inst["blas"][1])], [a.scene.trs((0.4, 0.3, 1.0), 1.2, 0.0, 0.9, 0.0)])
    assert a.set_instances(1, move) == 0
    d.move(1, move)
    _check_layout(host_api, a, d, knobs, "moved after the lights")
    b = host_api.HostRenderer(lc.W, lc.H)
    b.upload_desc(d.desc())
    _same_results(_results(a, host_api), _results(b, host_api), "moved after the lights")
    a.close(), b.close()


# ---- 5. invalidation ------------------------------------------------------------------------------------------------------------------------------
def _edits(host_api):
    """one successful call of each kind (the material edit changes a type)"""
    e = lc.MATERIAL_EDITS["diffuse_to_metal"]
    return [("lights", lambda r: r.set_lights(lc.scene_tables(host_api, lights=lc.lights(3))[1])),
            ("materials", lambda r: _send_materials(host_api, r, e)[0]),
            ("sky", lambda r: r.set_sky(lc.sky_image(*lc.SKY_EDITS["larger"]))),
            ("no sky", lambda r: r.set_sky(None))]


def test_an_edit_invalidates_the_g_buffer_and_every_history(host_api, monkeypatch):
    _env(monkeypatch)
    L = host_api.rt_lib()
    STATE = host_api.RT_E_STATE
    a = _renderer(host_api, lc.look_scene, tlas=True)
    a.stats_enable(True)
    a.render(host_api.RT_MODE_PATH, 0, 16)
    for what, edit in _edits(host_api):
        a.render_aovs(0.001)
        a.denoise(2)
        a.history_capture()
        assert a.reproject() >= 0 and a.reproject_motion() >= 0 and a.reproject_deform() >= 0, what
        a.history_capture()
        a.set_active([3, 5, 70])
        stats, acc = a.stats(), a.accumulator()
        assert edit(a) == 0, what
        assert L.rt_denoise(a.ctx, 2, None) == STATE, what
        for call in (L.rt_reproject, L.rt_reproject_motion, L.rt_reproject_deform):
            assert call(a.ctx, None, None) == STATE, what
        assert sp.same(a.accumulator(), acc) and all(sp.same(x, y) for x, y in zip(a.stats(), stats)), "accumulator and statistics are not touched"
        lst, n_act = a.active()
        assert n_act == 3 and lst.tolist() == [3, 5, 70], "an installed list survives"
        a.render_aovs(0.001)
        a.denoise(2)  # current again
        for call in (L.rt_reproject, L.rt_reproject_motion, L.rt_reproject_deform):
            assert call(a.ctx, None, None) == STATE, "the history stays invalid until a new capture"
        a.history_capture()
        assert a.reproject_deform() >= 0
    a.close()


def test_profiling_counts_one_query_per_call(host_api, monkeypatch):
    _env(monkeypatch)
    a = _renderer(host_api, lc.look_scene)
    a.set_profiling(True)
    for what, edit in _edits(host_api) + [("colour", lambda r: _send_materials(host_api, r, lc.MATERIAL_EDITS["colour"])[0])]:
        a.profile()
        assert edit(a) == 0
        prof = a.profile()
        assert prof["query"]["launches"] == 1 and all(prof[x]["launches"] == 0 for x in ("generate", "extend", "shade", "connect")), what
    a.close()


# ---- 6. refusals are atomic ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(host_api, monkeypatch):
    _env(monkeypatch)
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    L = host_api.rt_lib()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    r = _renderer(host_api, lc.look_scene, tlas=True)
    assert _send_materials(host_api, r, lc.MATERIAL_EDITS["diffuse_to_metal"])[0] == 0  # (an edited scene, so that "as before" is not "as uploaded")
    mats, lights, sky = lc.scene_tables(host_api, mats=lc.MATERIAL_EDITS["diffuse_to_metal"]["after"])
    before = _snapshot(r, 2)
    r.stats_enable(True)
    frames = _results(r, host_api)
    r.render(host_api.RT_MODE_PATH, 0, 2)
    r.render_aovs(0.001)
    r.history_capture()
    many = lc.scene_tables(host_api, lights=lc.lights(32))[1]
    many = np.concatenate([many, many[:1]])

    def typed(t):
        x = mats.copy()
        x["type"][2] = t
        return x

    cases = [("33 lights", lambda: L.rt_set_lights(r.ctx, p(many), 33), UNSUP),
             ("null lights", lambda: L.rt_set_lights(r.ctx, None, 1), ARG),
             ("lights, null context", lambda: L.rt_set_lights(None, p(many), 1), ARG),
             ("a range beyond the table", lambda: L.rt_set_materials(r.ctx, 3, 2, p(mats)), ARG),
             ("first beyond the table", lambda: L.rt_set_materials(r.ctx, 4, 1, p(mats)), ARG),
             ("a range that wraps", lambda: L.rt_set_materials(r.ctx, 0xFFFFFFFF, 2, p(mats)), ARG),
             ("no materials", lambda: L.rt_set_materials(r.ctx, 0, 0, p(mats)), ARG),
             ("null materials", lambda: L.rt_set_materials(r.ctx, 0, 4, None), ARG),
             ("materials, null context", lambda: L.rt_set_materials(None, 0, 4, p(mats)), ARG),
             ("type 0", lambda: L.rt_set_materials(r.ctx, 0, 4, p(typed(0))), ARG),
             ("type 4", lambda: L.rt_set_materials(r.ctx, 0, 4, p(typed(4))), ARG),
             ("a sky without width", lambda: L.rt_set_sky(r.ctx, p(sky), 0, 4, 3), ARG),
             ("a sky without height", lambda: L.rt_set_sky(r.ctx, p(sky), 4, 0, 3), ARG),
             ("a sky of two channels", lambda: L.rt_set_sky(r.ctx, p(sky), 4, 4, 2), ARG),
             ("sky, null context", lambda: L.rt_set_sky(None, p(sky), 4, 4, 3), ARG)]
    for what, call, want in cases:
        assert call() == want, what
    assert L.rt_set_lights(r.ctx, p(many), 33) == UNSUP and b"33 lights (limit 32)" in L.rt_last_error(r.ctx)
    after = _snapshot(r, 2)
    for a in before:
        assert sp.same(after[a], before[a]), a
    assert L.rt_denoise(r.ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    assert r.reproject_deform() >= 0, "... and so is the history"
    _same_results(_results(r, host_api), frames, "after the refusals")
    # the Q-learning sampler on: an edit after which path mode would need the general kernel is refused
    r.qlearn_enable(4, (-3.0, 0.0, -1.0), (3.0, 4.0, 5.0))
    r.render_aovs(0.001)
    r.history_capture()
    shiny = lc.scene_tables(host_api, mats=lc.MATERIAL_EDITS["shiny_on"]["after"])[0]
    assert r.set_materials(1, shiny[1:2]) == UNSUP and b"general kernel" in L.rt_last_error(r.ctx)
    after = _snapshot(r, 2)
    for a in before:
        assert sp.same(after[a], before[a]), a
    assert L.rt_denoise(r.ctx, 1, None) == 0 and r.reproject_deform() >= 0
    r.qlearn_disable()
    _same_results(_results(r, host_api), frames, "after the sampler's refusal")
    r.close()
    # no scene: RT_E_STATE
    g = host_api.HostRenderer(lc.W, lc.H)
    assert L.rt_set_lights(g.ctx, None, 0) == STATE and L.rt_set_materials(g.ctx, 0, 4, p(mats)) == STATE and L.rt_set_sky(g.ctx, None, 0, 0, 0) == STATE
    nbytes = C.c_size_t(0)
    assert L.rt_scene_array(g.ctx, 8, None, 0, C.byref(nbytes)) == STATE
    g.close()


def test_the_sampler_stays_on_across_an_edit_it_can_follow(host_api, monkeypatch):
    """with the Q-learning sampler on, an edit that keeps the wavefront is taken, and the table is not touched"""
    _env(monkeypatch)
    r = _renderer(host_api, lc.look_scene)
    r.qlearn_enable(4, (-3.0, 0.0, -1.0), (3.0, 4.0, 5.0))
    r.render(host_api.RT_MODE_PATH, 0, 2)
    r.qlearn_apply()
    table = r.qlearn_table()
    assert _send_materials(host_api, r, lc.MATERIAL_EDITS["diffuse_to_metal"])[0] == 0
    assert sp.same(r.qlearn_table(), table) and not np.all(table == table.flat[0])
    r.clear()
    r.render(host_api.RT_MODE_PATH, 2, 2)
    assert np.isfinite(r.accumulator()[..., :3]).any()
    r.close()


# ---- 7. two contexts, through the host mirror ---------------------------------------------------------------------------------------------------
def test_commits_reach_every_context(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    e = lc.MATERIAL_EDITS["range"]
    frames = []
    for devs in (None, [0, 0]):
        r = host_api.HostRenderer(32, 17, devices=devs)
        s = r.scene
        lc.look_scene(s, tlas=True, mats=e["before"])
        r.commit()  # Scene::Commit to context 0, CommitAlso to the second one
        for i in range(e["first"], e["first"] + e["count"]):
            getattr(s, "replace_" + e["after"][i][0])(i, **e["after"][i][1])
        s.clear_lights()
        for l in lc.lights(7):
            lc.add_light(s, l)
        s.sky(lc.sky_image(*lc.SKY_EDITS["larger"]))
        r.commit_materials(), r.commit_lights(), r.commit_sky()
        d = td.Desc(host_api, s)  # the mirror's own description after the edits
        want = lc.scene_tables(host_api, tlas=True, mats=e["after"], lights=lc.lights(7), sky=lc.SKY_EDITS["larger"])
        assert all(np.array_equal(x, y) for x, y in zip(lc.tables(d.ptr), want)), "the mirror describes the edited scene"
        snaps = []
        for k in range(2 if devs else 1):
            ctx = r.ctx_at(k)
            _check_layout(host_api, r, d, knobs, "context %d" % k, ctx)
            snaps.append(_snapshot(r, len(d.blas), ctx))
        assert all(sp.same(snaps[0][a], snaps[-1][a]) for a in snaps[0]), "the two contexts end bit-equal"
        r.tick()  # a Whitted Tick; with two contexts the rows are interleaved over them.  It clears: the commits asked for it
        frames.append(r.tick_accumulator().copy())
        r.close()
    assert sp.same(frames[0], frames[1]) and (frames[0][..., :3] > 0).any()
