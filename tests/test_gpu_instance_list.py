"""rt_set_instance_list on the device (include/rt_amd.h), through the C ABI and the host mirror: after the whole instance list of a loaded
TLAS scene was replaced -- another length, other BLASes -- the context holds, byte for byte, what a fresh rt_upload_scene of the updated
description would: the arrays themselves (rt_scene_array against rt_layout_build, rt_download_tlas against rt_build_tlas and tlas::build),
every query, frame and executed-walk counter against a freshly uploaded context, the hits against the oracle on a scene built from the
list.  The call composes with rt_set_instances, rt_set_triangles and rt_set_vertices, invalidates what an upload invalidates for
everything that names an instance, refuses bad input on the host and leaves the scene as it was when the build fails.  Every comparison is
bitwise.  The lists, ray sets and the updated description are tests/instance_list_ref.py's (tests/test_instance_list_cpu.py shows they
are not vacuous)."""
import ctypes as C

import numpy as np
import pytest

import instance_list_ref as il
import instances_ref as ir
import support as sp
import triangles_desc as td
import triangles_ref as tr
import vertices_ref as vr

pytestmark = pytest.mark.gpu
f32 = np.float32
ARRAYS = ("pairs", "reach", "inst", "scalars")


def _env(monkeypatch, env=None):
    sp.clean_env(monkeypatch, env)
    return sp.layout_knobs(env)


def _uploaded(host_api, w=16, h=8):
    """ir.triangles_scene under its three instances (BLASes 0, 1, 0), committed, and its description"""
    r = host_api.HostRenderer(w, h)
    ir.triangles_scene(r.scene, ir.grid_transforms(r.scene, len(il.UPLOADED)))
    r.commit()
    return r, td.Desc(host_api, r.scene)


def _behaviour(host_api, w=32, h=24):
    """il.list_scene under the behaviour test's three placements"""
    r = host_api.HostRenderer(w, h)
    il.list_scene(r.scene, il.BEHAVIOUR_LISTS[3], il.behaviour_transforms(r.scene, 3))
    r.commit()
    return r, td.Desc(host_api, r.scene)


def _scalars(s):
    """RT_LAYOUT_SCALARS without wideOK and wide8OK (words 9 and 10 keep their upload-time values across a deformation)"""
    return np.delete(np.asarray(s), [9, 10])


def _check_layout(host_api, r, d, knobs, what, ctx=None, deformed=False):
    """the context's arrays equal rt_layout_build's of the updated description; its TLAS is rt_build_tlas's and tlas::build's of the boxes"""
    if ctx is None:
        nodes = r.download_tlas()
        assert len(nodes) == 2 * d.n, what
        assert np.array_equal(nodes, r.build_tlas(d.bounds)), "%s: rt_download_tlas differs from rt_build_tlas on the same boxes" % what
        assert np.array_equal(nodes, d.tlas), "%s: rt_download_tlas differs from tlas::build on the same boxes" % what
    L = host_api.layout(d.desc(), *knobs)
    for a in ARRAYS[:3]:
        assert sp.same(r.scene_array(a, ctx), L[a]), "%s: %s differs from rt_layout_build of the updated description" % (what, a)
    got, want = r.scene_array("scalars", ctx), L["scalars"]
    assert np.array_equal(_scalars(got), _scalars(want)) and (deformed or np.array_equal(got, want)), "%s: scalars" % what
    for k, (p0, p1, s0, s1) in enumerate(d.ranges()):
        assert sp.same(r.blas_array(k, "pairs", ctx), L["pairs"][16 * p0:16 * p1]), "%s: the pair records of blas %d" % (what, k)
        assert sp.same(r.blas_array(k, "prims", ctx), L["prims"][16 * s0:16 * s1]), "%s: the primitive records of blas %d" % (what, k)
    return L


def _send(host_api, r, d, blas, Ts, bounds=None):
    """rt_set_instance_list of the list (blas, Ts) under bounds6 = bounds; the description follows when the call succeeds"""
    rec = ir.records(host_api, blas, Ts)
    rc = r.set_instance_list(rec, bounds)
    if rc == 0:
        il.set_list(d, rec, bounds)
    return rc


# ---- 1. layout equality along a walk of lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"RT_TLAS_LDS": "0", "RT_WIDE": "1", "RT_WIDE8": "1"}], ids=["default", "wide_no_lds"])
def test_layout_equals_a_fresh_layout_along_a_walk(env, host_api, monkeypatch):
    """uploaded 3 -> 5 (two entries re-pointed) -> 1 (no pair record, root INST | 0) -> 2 -> 17 -> 38 (the LDS copy off) -> 37 (on again) ->
    256 (one BLAS without an instance) -> 3, NULL and given boxes in turn"""
    knobs = _env(monkeypatch, env)
    r, d = _uploaded(host_api)
    L0 = host_api.layout(d.ptr, *knobs)
    for a in ARRAYS:  # before the first call: what upload left -- the room it reserves does not show
        assert sp.same(r.scene_array(a), L0[a]), a
    assert np.array_equal(r.download_tlas(), r.scene.tlas_dump())
    for k, st in enumerate(il.WALK):
        rec, b6 = il.walk_step(host_api, d, r.scene, k)
        assert r.set_instance_list(rec, b6) == 0, (k, r.rt.rt_last_error(r.ctx))
        n = st["n"]
        L = _check_layout(host_api, r, d, knobs, "step %d: %d instances, %s" % (k, n, "given" if st["given"] else "NULL"))
        assert L["nInst"] == n and L["tlasPairs"] == (n if n > 1 else 0) and L["tlasLds"] == (1 if knobs[2] and n < il.N_SPLIT else 0)
        if n == 1:
            assert L["root"] == 0x40000000 and L["tlasBase"] == 0 and len(r.scene_array("pairs")) == len(L0["pairs"]) - 16 * L0["tlasPairs"]
    r.close()


# ---- 2. the same results as a fresh upload, and as the oracle ---------------------------------------------------------------------------------
def _answers(host_api, r, O, D, tmax):
    r.set_counting(host_api.RT_COUNT_EXECUTED)
    r.counters()
    hit, occ = r.find_nearest(O, D), r.is_occluded(O, D, tmax)
    cq = r.counters()
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, 2)
    path = r.accumulator()
    cp = r.counters()
    r.set_counting(False)
    r.clear()
    r.render(host_api.RT_MODE_WHITTED, 0, 1)
    return hit, occ, cq, path, cp, r.accumulator()


@pytest.mark.parametrize("env", [{}, {"RT_WIDE": "1"}], ids=["default", "wide"])
def test_results_equal_a_fresh_upload_and_the_oracle(env, host_api, oracle_api, monkeypatch):
    _env(monkeypatch, env)
    a, d = _behaviour(host_api)
    a.render(host_api.RT_MODE_PATH, 0, 16)  # a dense batch above RT_PRIMARY_TABLE_MIN's 12 frames: the primary-hit table exists, of the old list
    for n, given in ((5, False), (2, True)):
        blas, Ts = il.BEHAVIOUR_LISTS[n], il.behaviour_transforms(a.scene, n)
        b6 = il.given_bounds(d, blas, Ts) if given else None
        assert _send(host_api, a, d, blas, Ts, b6) == 0
        b = host_api.HostRenderer(a.w, a.hgt)
        b.upload_desc(d.desc())
        for x in ARRAYS:
            assert sp.same(a.scene_array(x), b.scene_array(x)), (n, x)
        O, D = il.behaviour_rays(Ts, il.BEHAVIOUR_NEW[n], 50 + n)
        tmax = np.random.default_rng(4).uniform(0.1, 12.0, len(O)).astype(f32)
        (hit, occ, cq, path, cp, wh), (hit2, occ2, cq2, path2, cp2, wh2) = _answers(host_api, a, O, D, tmax), _answers(host_api, b, O, D, tmax)
        assert all(sp.same(hit[k], hit2[k]) for k in hit) and np.array_equal(occ, occ2), n
        assert cq == cq2 and cq["instance_visits"] > 0 and cq["tlas_inner"] > 0, "the executed walk (reach culling included) is the fresh upload's"
        assert sp.same(path, path2) and cp == cp2 and sp.same(wh, wh2), n
        assert np.isfinite(wh[..., :3]).any() and (path[..., :3] > 0).any() and 0 < occ.sum() < len(occ)
        o = oracle_api.OracleScene()
        il.list_scene(o, blas, il.behaviour_transforms(o, n))
        ref, on = il.hits_on(o, O, D, il.BEHAVIOUR_NEW[n])
        assert 4 * int(on.sum()) >= len(O), "the rays meet the instances that are new in the step"
        assert np.array_equal(hit["obj"], ref["obj"]) and sp.same(hit["t"], ref["t"]), n
        got = ref["obj"] != -1
        assert sp.same(hit["normal"][got], ref["normal"][got])
        o.close(), b.close()
    a.close()


# ---- 3. composition ------------------------------------------------------------------------------------------------------------------------------
def test_composes_with_the_other_edit_calls(host_api, monkeypatch):
    """list -> rt_set_instances -> rt_set_triangles -> rt_set_vertices (indices bound before the list call) -> list: each works against the
    list the call before left, and every step ends on the fresh layout of the updated description"""
    knobs = _env(monkeypatch)
    ARG = host_api.RT_E_ARG
    r, d = _uploaded(host_api)
    s = r.scene
    xyz, idx = vr.weld(tr.v9_of(d.tris[1]))
    assert r.set_mesh_indices(1, idx, len(xyz)) == 0  # bound under the uploaded list; a binding is per BLAS
    blas = [1, 0, 0, 1, 0]
    assert _send(host_api, r, d, blas, il.walk_transforms(s, 0)) == 0
    _check_layout(host_api, r, d, knobs, "list of 5")
    # rt_set_instances against the NEW list: instance 4 exists, slot 0 is an instance of BLAS 1 now
    move = lambda i, b: ir.records(host_api, [b], [s.trs((f32(0.4 * i - 1.0), 0.3, f32(2.5 + 0.2 * i)), 1.5, 0.0, f32(0.7 + i), 0.0)])
    snap = {a: r.scene_array(a) for a in ARRAYS}
    assert r.set_instances(0, move(0, 0)) == ARG, "slot 0 was re-pointed: a record carrying its old BLAS is refused"
    assert r.set_instances(5, move(5, 0)) == ARG and r.set_instances(3, ir.records(host_api, [1, 0, 0], il.walk_transforms(s, 0)[:3])) == ARG, "a range past the new n"
    assert all(sp.same(r.scene_array(a), snap[a]) for a in ARRAYS)
    for i in (0, 4):
        rec = move(i, blas[i])
        assert r.set_instances(i, rec) == 0, i
        d.move(i, rec)
        _check_layout(host_api, r, d, knobs, "instance %d moved" % i)
    # rt_set_triangles of the BLAS that gained an instance: both of its instances get fresh boxes
    assert [int(b) for b in d.inst["blas"]].count(1) == 2
    v9 = tr.twist(tr.v9_of(d.tris[1]))
    assert r.set_triangles(1, d.deform(1, v9)) == 0
    _check_layout(host_api, r, d, knobs, "deformed after the list", deformed=True)
    # rt_set_vertices through the indices bound before the list call
    new = vr.DEFORMS["scale"](xyz)
    vr.deform(d, 1, new, idx)
    assert r.set_vertices(1, new) == 0, r.rt.rt_last_error(r.ctx)
    _check_layout(host_api, r, d, knobs, "vertices after the list", deformed=True)
    # a second list: NULL boxes are fresh instances of the DEFORMED BLAS; then given ones
    assert _send(host_api, r, d, [1, 1], il.walk_transforms(s, 2)) == 0
    _check_layout(host_api, r, d, knobs, "second list", deformed=True)
    Ts = il.walk_transforms(s, 7)
    assert _send(host_api, r, d, [0, 1, 1], Ts, il.given_bounds(d, [0, 1, 1], Ts)) == 0
    _check_layout(host_api, r, d, knobs, "third list, boxes given", deformed=True)
    r.close()


# ---- 4. invalidation ---------------------------------------------------------------------------------------------------------------------------
def test_a_list_edit_invalidates_what_names_an_instance(host_api, monkeypatch):
    _env(monkeypatch)
    L = host_api.rt_lib()
    STATE = host_api.RT_E_STATE
    a, d = _behaviour(host_api)
    a.set_pixel_filter(host_api.RT_FILTER_BOX)
    a.set_lens(0.05, 3.0)
    a.stats_enable(True)
    a.render(host_api.RT_MODE_PATH, 0, 16)
    a.render_aovs(0.001)
    a.denoise(2)
    a.history_capture()
    assert a.reproject() >= 0 and a.reproject_motion() >= 0 and a.reproject_deform() >= 0
    a.history_capture()
    a.set_active([3, 5, 700])
    stats, acc = a.stats(), a.accumulator()
    assert _send(host_api, a, d, il.BEHAVIOUR_LISTS[5], il.behaviour_transforms(a.scene, 5)) == 0
    assert L.rt_denoise(a.ctx, 2, None) == STATE, "the G-buffer's instance indices renumber"
    for call in (L.rt_reproject, L.rt_reproject_motion, L.rt_reproject_deform):
        assert call(a.ctx, None, None) == STATE, "a captured history ends at every level"
    assert sp.same(a.accumulator(), acc) and all(sp.same(x, y) for x, y in zip(a.stats(), stats)), "accumulator and statistics are not touched"
    lst, n_act = a.active()
    assert n_act == 3 and lst.tolist() == [3, 5, 700], "an installed list survives"
    assert a.pixel_filter() == host_api.RT_FILTER_BOX and a.lens() == (float(f32(0.05)), 3.0), "lens and filter survive"
    a.render_aovs(0.001)
    a.denoise(2)  # current again
    for call in (L.rt_reproject, L.rt_reproject_motion, L.rt_reproject_deform):
        assert call(a.ctx, None, None) == STATE, "the history stays invalid until a new capture"
    a.history_capture()
    assert a.reproject_motion() >= 0
    # a dense path batch after the edit equals a freshly uploaded context's: a stale primary-hit or bounce table would show here
    b = host_api.HostRenderer(a.w, a.hgt)
    b.upload_desc(d.desc())
    b.set_pixel_filter(host_api.RT_FILTER_BOX)
    b.set_lens(0.05, 3.0)
    for r in (a, b):
        r.stats_enable(False)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 16)
    assert sp.same(a.accumulator(), b.accumulator())
    assert not sp.same(a.accumulator(), acc), "the edit is visible"
    a.close(), b.close()


def test_profiling_counts_one_query(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    r, d = _uploaded(host_api)
    r.set_profiling(True)
    r.profile()
    assert _send(host_api, r, d, il.WALK[3]["blas"], il.walk_transforms(r.scene, 3)) == 0
    prof = r.profile()
    assert prof["query"]["launches"] == 1 and prof["query"]["ms"] > 0 and all(prof[k]["launches"] == 0 for k in ("generate", "extend", "shade", "connect"))
    r.set_profiling(False)
    _check_layout(host_api, r, d, knobs, "profiled")
    r.close()


# ---- 5. refusals and the atomic failure ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(scenes, host_api, monkeypatch):
    _env(monkeypatch)
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    L = host_api.rt_lib()
    r, d = _behaviour(host_api)
    assert _send(host_api, r, d, il.BEHAVIOUR_LISTS[5], il.behaviour_transforms(r.scene, 5)) == 0  # (an edited scene, so that "as before" is not "as uploaded")
    before = {a: r.scene_array(a) for a in ARRAYS}
    tl = r.download_tlas()
    r.render_aovs(0.001)
    r.stats_enable(True)
    r.history_capture()
    rec = ir.records(host_api, [0, 1, 1], il.behaviour_transforms(r.scene, 3))
    b6 = il.given_bounds(d, [0, 1, 1], rec["transform"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def spoiled(field, k, j, v):
        x = rec.copy()
        x[field][k, j] = v
        return x

    too_many = np.tile(rec, 86)[:257].copy()
    nanb, bigb = b6.copy(), b6.copy()
    nanb[2, 4], bigb[0, 0] = np.nan, -2e30
    cases = [("null instances", lambda: L.rt_set_instance_list(r.ctx, 3, None, None)),
             ("null context", lambda: L.rt_set_instance_list(None, 3, p(rec), None)),
             ("n 0", lambda: L.rt_set_instance_list(r.ctx, 0, p(rec), None)),
             ("n 257", lambda: L.rt_set_instance_list(r.ctx, 257, p(too_many), None)),
             ("n wraps", lambda: L.rt_set_instance_list(r.ctx, 0xFFFFFFFF, p(rec), None)),
             ("blas 2 of 2", lambda: L.rt_set_instance_list(r.ctx, 3, p(spoiled("blas", 1, ..., 2)), None)),
             ("blas -1", lambda: L.rt_set_instance_list(r.ctx, 3, p(spoiled("blas", 2, ..., -1)), p(b6))),
             ("nan matrix", lambda: L.rt_set_instance_list(r.ctx, 3, p(spoiled("transform", 1, 5, np.nan)), p(b6))),
             ("inf inverse", lambda: L.rt_set_instance_list(r.ctx, 3, p(spoiled("inv_transform", 2, 0, np.inf)), None)),
             ("nan bound", lambda: L.rt_set_instance_list(r.ctx, 3, p(rec), p(nanb))),
             ("bound beyond 1e30", lambda: L.rt_set_instance_list(r.ctx, 3, p(rec), p(bigb))),
             ("box beyond 1e30", lambda: L.rt_set_instance_list(r.ctx, 3, p(spoiled("transform", 0, 3, 3e38)), None))]
    for what, call in cases:
        assert call() == ARG, what
    # the degenerate build: finite boxes within 1e30 whose every union area reaches FindBestMatch's 1e30 (tlas.cpp:52): the call returns
    # RT_E_UNSUPPORTED after its read-back and commits nothing -- not even the count
    wide = np.tile(np.array([-1e16, -1e16, -1e16, 1e16, 1e16, 1e16], dtype=f32), (3, 1))
    assert L.rt_set_instance_list(r.ctx, 3, p(rec), p(wide)) == UNSUP
    assert b"no finite union area" in L.rt_last_error(r.ctx)
    for a in ARRAYS:
        assert sp.same(r.scene_array(a), before[a]), a
    assert np.array_equal(r.download_tlas(), tl) and len(tl) == 10
    assert L.rt_denoise(r.ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    assert r.reproject_motion() >= 0, "... and a captured history is still valid"
    assert r.set_instances(4, ir.records(host_api, [0], il.behaviour_transforms(r.scene, 3)[:1])) == 0, "the list is still the one of 5"
    r.close()
    # no scene: RT_E_STATE; no TLAS: RT_E_UNSUPPORTED, the scene untouched
    g = host_api.HostRenderer(16, 8)
    assert L.rt_set_instance_list(g.ctx, 3, p(rec), None) == STATE
    scenes.mixed_small(g.scene)
    g.commit()
    before = {a: g.scene_array(a) for a in ARRAYS}
    assert L.rt_set_instance_list(g.ctx, 3, p(rec), None) == UNSUP
    for a in ARRAYS:
        assert sp.same(g.scene_array(a), before[a]), a
    with pytest.raises(RuntimeError, match="no TLAS"):
        g.scene.commit_instance_list()
    g.close()


# ---- 6. two contexts and the host mirror -----------------------------------------------------------------------------------------------------
def test_commit_instance_list_reaches_every_context(host_api, monkeypatch):
    """CommitAlso + Scene::CommitInstanceList leave both contexts on the fresh layout of the mirror's own description, and tl is the tree
    the device walks"""
    knobs = _env(monkeypatch)
    frames = []
    st = il.WALK[3]  # 17 instances, the meshes alternate: the BLASes keep their order of first use, so Describe() numbers them as committed
    for devs in (None, [0, 0]):
        r = host_api.HostRenderer(32, 17, devices=devs)
        s = r.scene
        ir.triangles_scene(s, ir.grid_transforms(s, len(il.UPLOADED)))
        r.commit()  # Scene::Commit to context 0, CommitAlso to the second one
        Ts = il.walk_transforms(s, 3)
        s.set_instance_list([(st["blas"][i], Ts[i]) for i in range(st["n"])])
        s.commit_instance_list()
        d = td.Desc(host_api, s)  # the mirror's own description after the edit
        assert d.n == st["n"] and np.array_equal(r.download_tlas(), s.tlas_dump()), "CommitInstanceList leaves the device's tree in tl"
        want = ir.records(host_api, st["blas"], Ts)
        assert sp.same(d.inst["transform"], want["transform"]) and sp.same(d.inst["inv_transform"], want["inv_transform"]) and list(d.inst["blas"]) == st["blas"]
        snaps = []
        for k in range(2 if devs else 1):
            ctx = r.ctx_at(k)
            _check_layout(host_api, r, d, knobs, "context %d" % k, ctx if k else None)
            snaps.append({a: r.scene_array(a, ctx) for a in ARRAYS})
        assert all(sp.same(snaps[0][a], snaps[-1][a]) for a in ARRAYS), "the two contexts end bit-equal"
        r.tick()  # a Whitted Tick; with two contexts the rows are interleaved over them
        frames.append(r.tick_accumulator().copy())
        r.close()
    assert sp.same(frames[0], frames[1]) and (frames[0][..., :3] > 0).any()


def test_renderer_commit_instance_list_clears(host_api, monkeypatch):
    """Renderer::CommitInstanceList: the next path Tick clears, and its frame is the one a fresh renderer of the new list shows after a
    clear at the same frame number"""
    _env(monkeypatch)
    n = 5
    a = host_api.HostRenderer(32, 24)
    il.list_scene(a.scene, il.BEHAVIOUR_LISTS[3], il.behaviour_transforms(a.scene, 3))
    b = host_api.HostRenderer(32, 24)
    il.list_scene(b.scene, [0, 1, 0, 1, 0], il.behaviour_transforms(b.scene, n))
    for r in (a, b):
        r.scene.set_raytracer(False)
        r.commit()
        r.tick(), r.tick()
    assert a.iteration() == b.iteration() > 1
    old = a.tick_accumulator()
    a.scene.set_instance_list([(k, T) for k, T in zip([0, 1, 0, 1, 0], il.behaviour_transforms(a.scene, n))])
    a.commit_instance_list()
    b.set_camera(*b.camera())  # the same camera, marked changed: b's next Tick clears too
    a.tick(), b.tick()
    assert a.iteration() == b.iteration() == 1, "the Tick cleared"
    assert sp.same(a.tick_accumulator(), b.tick_accumulator()) and not sp.same(a.tick_accumulator(), old)
    for x in ARRAYS:
        assert sp.same(a.scene_array(x), b.scene_array(x)), x
    a.close(), b.close()
