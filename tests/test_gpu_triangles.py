"""rt_set_triangles on the device (include/rt_amd.h, csrc/rt_triangles.h), through the C ABI: after a deformation the context holds, byte
for byte, what a fresh rt_upload_scene of the updated description would -- the arrays themselves (rt_blas_array and rt_scene_array against
rt_layout_build), every query, frame and executed-walk counter against a freshly uploaded context, the hits against the oracle on a scene
built from the deformed triangles -- and the call invalidates what rt_set_time invalidates, refuses bad input on the host and leaves the
scene as it was when it fails.  Every comparison is bitwise.  The updated description is tests/triangles_desc.py's, from the NumPy
restatements of tests/triangles_ref.py."""
import ctypes as C

import numpy as np
import pytest

import instances_ref as ir
import support as sp
import triangles_desc as td
import triangles_ref as tr

pytestmark = pytest.mark.gpu
f32 = np.float32
HOWS = ("twist", "scale", "collapse")


def _env(monkeypatch, env=None):
    sp.clean_env(monkeypatch, env)
    return sp.layout_knobs(env)


def _scalars(s):
    """RT_LAYOUT_SCALARS without wideOK and wide8OK (words 9 and 10 keep their upload-time values)"""
    return np.delete(np.asarray(s), [9, 10])


def _snapshot(r, n_blas):
    out = {a: r.scene_array(a) for a in ("pairs", "reach", "inst", "scalars")}
    for k in range(n_blas):
        out["pairs%d" % k], out["prims%d" % k] = r.blas_array(k, "pairs"), r.blas_array(k, "prims")
    return out


def _check_layout(host_api, r, d, knobs, what, ctx=None):
    """the context's arrays equal rt_layout_build's of the updated description"""
    L = host_api.layout(d.desc(), *knobs)
    for k, (p0, p1, s0, s1) in enumerate(d.ranges()):
        assert sp.same(r.blas_array(k, "pairs", ctx), L["pairs"][16 * p0:16 * p1]), "%s: the pair records of blas %d" % (what, k)
        assert sp.same(r.blas_array(k, "prims", ctx), L["prims"][16 * s0:16 * s1]), "%s: the primitive records of blas %d" % (what, k)
    for a in ("pairs", "reach", "inst"):
        assert sp.same(r.scene_array(a, ctx), L[a]), "%s: %s differs from rt_layout_build of the updated description" % (what, a)
    assert np.array_equal(_scalars(r.scene_array("scalars", ctx)), _scalars(L["scalars"])), "%s: scalars" % what
    if d.use_tlas and ctx is None:
        assert np.array_equal(r.download_tlas(), d.tlas), "%s: rt_download_tlas differs from tlas::build over the boxes" % what
    return L


def _renderer(host_api, scenes, name, w=16, h=8):
    r = host_api.HostRenderer(w, h)
    case = td.build_case(r.scene, name, scenes)
    r.commit()
    return r, case


# ---- 1. layout equality; 2. two deformations in a row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", td.LAYOUT_CASES)
@pytest.mark.parametrize("env", [{}, {"RT_TLAS_LDS": "0", "RT_WIDE": "1"}], ids=["default", "wide_no_lds"])
def test_layout_equals_a_fresh_layout(name, env, scenes, host_api, monkeypatch):
    knobs = _env(monkeypatch, env)
    r, case = _renderer(host_api, scenes, name)
    d = td.Desc(host_api, r.scene)
    k = case["k"]
    _check_layout(host_api, r, d, knobs, "as uploaded")
    other = [(j, r.blas_array(j, "pairs"), r.blas_array(j, "prims")) for j in range(len(d.blas)) if j != k]
    base = tr.v9_of(d.tris[k])
    for how in HOWS:  # each from the uploaded vertices: every later one also shows that nothing of the one before is left
        v9, N = tr.DEFORMS[how](base[:-2] if case["sentinel"] else base), None
        if case["sentinel"]:  # the two closing triangles stay where they are, with N = 0
            v9 = np.concatenate([v9, base[-2:]])
            N = tr.sentinel_normals(v9)
        assert r.set_triangles(k, d.deform(k, v9, N)) == 0, how
        L = _check_layout(host_api, r, d, knobs, how)
        for j, pairs, prims in other:
            assert sp.same(r.blas_array(j, "pairs"), pairs) and sp.same(r.blas_array(j, "prims"), prims), "blas %d is untouched" % j
    if not d.use_tlas:
        # spheres and planes in leaves keep their records; a later rt_set_time deforms from the new vertices
        kind = sp.bits(L["prims"]).reshape(-1, 16)[:, 15] & 3
        got = sp.bits(r.blas_array(0, "prims")).reshape(-1, 16)
        assert np.array_equal(got[kind != 0], sp.bits(host_api.layout(r.scene.describe(), *knobs)["prims"]).reshape(-1, 16)[kind != 0])
        fresh = host_api.HostRenderer(16, 8)
        fresh.upload_desc(d.desc())
        for x in (r, fresh):
            x.set_time(0.7)
        for a in ("pairs", "prims"):
            assert sp.same(r.blas_array(0, a), fresh.blas_array(0, a)), "rt_set_time after the call: " + a
        assert not sp.same(r.blas_array(0, "prims"), L["prims"])
        fresh.close()
    r.close()


def test_composes_with_set_instances(scenes, host_api, monkeypatch):
    """boxes sent with bounds6 before the deformation are replaced by fresh ones for the deformed BLAS's instances only; a move after it
    takes the refitted BLAS's box"""
    knobs = _env(monkeypatch)
    r, case = _renderer(host_api, scenes, "rand_s0")
    d = td.Desc(host_api, r.scene)
    s = r.scene
    Ts = [s.trs((f32(-1.0 + 0.8 * i), f32(0.2 * i), f32(3.0 + 0.3 * i)), f32(1.0 + 0.2 * i), 0.0, f32(0.4 * i + 0.2), 0.0) for i in range(d.n)]
    rec = ir.records(host_api, [int(b) for b in d.inst["blas"]], Ts)
    given = np.stack([np.concatenate([d.bounds[i, :3] - f32(0.5 + i), d.bounds[i, 3:] + f32(1.5 + i)]) for i in range(d.n)]).astype(f32)
    assert r.set_instances(0, rec, given) == 0
    d.move(0, rec, given)
    _check_layout(host_api, r, d, knobs, "moved, boxes given")
    v9 = tr.twist(tr.v9_of(d.tris[1]))
    assert r.set_triangles(1, d.deform(1, v9)) == 0
    assert sp.same(d.bounds[0], given[0]) and sp.same(d.bounds[2], given[2]) and not sp.same(d.bounds[1], given[1])
    _check_layout(host_api, r, d, knobs, "deformed after the move")
    rec1 = ir.records(host_api, [1], [s.trs((0.3, 0.4, 2.5), 1.5, 0.0, 1.0, 0.0)])
    assert r.set_instances(1, rec1) == 0
    d.move(1, rec1)
    _check_layout(host_api, r, d, knobs, "moved after the deformation")
    assert r.set_triangles(1, d.deform(1, tr.scale(v9, 3.0))) == 0
    _check_layout(host_api, r, d, knobs, "deformed again")
    r.close()


# ---- 3. the same results as a fresh upload, and as the oracle ---------------------------------------------------------------------------
def _behaviour_pair(host_api, how, w=16, h=8):
    a = host_api.HostRenderer(w, h)
    Ts = tr.spread_transforms(a.scene, tr.BEHAVIOUR_INSTANCES)
    tr.mesh_scene(a.scene, [tr.SMALL, tr.grid_mesh()], Ts)
    a.commit()
    a.render(host_api.RT_MODE_PATH, 0, 16)  # a dense batch above RT_PRIMARY_TABLE_MIN's 12 frames: the primary-hit table exists, of the old shape
    a.clear()
    d = td.Desc(host_api, a.scene)
    new = tr.BEHAVIOUR_DEFORMS[how](tr.grid_mesh())
    assert a.set_triangles(1, d.deform(1, new)) == 0
    b = host_api.HostRenderer(w, h)
    b.upload_desc(d.desc())
    return a, b, d, Ts, new


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("env", [{}, {"RT_WIDE": "1"}, {"RT_WIDE8": "1"}], ids=["default", "wide", "wide8"])
def test_results_equal_a_fresh_upload(how, env, host_api, monkeypatch):
    _env(monkeypatch, env)
    a, b, d, Ts, new = _behaviour_pair(host_api, how)
    O, D = tr.aimed_rays(tr.BEHAVIOUR_RAYS, 41, Ts[1::2], new)
    tmax = (np.random.default_rng(4).uniform(0.1, 12.0, len(O)) * (100.0 if how == "scale" else 1.0)).astype(f32)  # some short of the mesh, some beyond
    out = []
    for r in (a, b):
        r.set_counting(host_api.RT_COUNT_EXECUTED)
        r.counters()
        hit, occ = r.find_nearest(O, D), r.is_occluded(O, D, tmax)
        cq = r.counters()
        r.set_counting(False)
        scoped = [r.scope_nearest(2, 1, O, D), r.scope_nearest(3, 1, O, D), r.scope_nearest(3, 3, O, D)]  # RT_SCOPE_BLAS, RT_SCOPE_INSTANCE
        socc = [r.scope_occluded(2, 1, O, D, tmax), r.scope_occluded(3, 3, O, D, tmax)]
        r.render(host_api.RT_MODE_PATH, 0, 4)
        path4 = r.accumulator()
        r.render(host_api.RT_MODE_PATH, 4, 12)  # ... and on past RT_PRIMARY_TABLE_MIN: a table of the old shape would show here
        path16 = r.accumulator()
        r.clear()
        r.render(host_api.RT_MODE_WHITTED, 0, 1)
        out.append((hit, occ, cq, scoped, socc, path4, path16, r.accumulator()))
    (hit, occ, cq, scoped, socc, p4, p16, wh), (hit2, occ2, cq2, scoped2, socc2, p4b, p16b, wh2) = out
    assert all(sp.same(hit[k], hit2[k]) for k in hit) and np.array_equal(occ, occ2)
    assert (hit["obj"] >= 2000).sum() >= len(O) // 4 and 0 < occ.sum() < len(occ), "the rays meet the deformed mesh"
    assert cq == cq2 and cq["instance_visits"] > 0 and cq["tlas_inner"] > 0, "the executed walk is the fresh upload's"
    for x, y in zip(scoped, scoped2):
        assert all(sp.same(x[k], y[k]) for k in x)
    assert (scoped[1]["obj"] >= 2000).any()
    assert all(np.array_equal(x, y) for x, y in zip(socc, socc2))
    assert sp.same(p4, p4b) and sp.same(p16, p16b) and sp.same(wh, wh2)
    assert np.isfinite(wh[..., :3]).any() and (p16[..., :3] > 0).any()
    a.close(), b.close()


@pytest.mark.parametrize("how", HOWS)
def test_deformed_scene_equals_a_fresh_oracle_scene(how, host_api, oracle_api, monkeypatch):
    _env(monkeypatch)
    a, b, d, Ts, new = _behaviour_pair(host_api, how)
    b.close()
    o = oracle_api.OracleScene()
    tr.mesh_scene(o, [tr.SMALL, new], tr.spread_transforms(o, tr.BEHAVIOUR_INSTANCES))  # its own build over the deformed triangles: another tree
    O, D = tr.aimed_rays(tr.BEHAVIOUR_RAYS, 41, Ts[1::2], new)
    ref, got = o.find_nearest(O, D), a.find_nearest(O, D)
    assert np.array_equal(got["obj"], ref["obj"]) and sp.same(got["t"], ref["t"])
    hit = ref["obj"] != -1
    assert (ref["obj"] >= 2000).sum() >= len(O) // 4 and sp.same(got["normal"][hit], ref["normal"][hit])
    assert np.array_equal(a.is_occluded(O, D), o.is_occluded(O, D)["occluded"])
    a.close()


# ---- 4. invalidation ------------------------------------------------------------------------------------------------------------------------
def test_a_deformation_invalidates_what_set_time_invalidates(host_api, monkeypatch):
    _env(monkeypatch)
    a = host_api.HostRenderer(16, 8)
    tr.mesh_scene(a.scene, [tr.SMALL, tr.grid_mesh()], tr.spread_transforms(a.scene, tr.BEHAVIOUR_INSTANCES))
    a.commit()
    d = td.Desc(host_api, a.scene)
    a.stats_enable(True)
    a.render(host_api.RT_MODE_PATH, 0, 16)
    a.render_aovs(0.001)
    a.denoise(2)
    a.history_capture()
    a.set_active([3, 5, 70])
    stats, acc = a.stats(), a.accumulator()
    L = host_api.rt_lib()
    bad = d.tris[1].copy()
    bad["v0"][0, 0] = np.nan
    assert a.set_triangles(1, bad) == host_api.RT_E_ARG
    assert L.rt_denoise(a.ctx, 2, None) == 0 and a.reproject() >= 0 and a.reproject_motion() >= 0, "a refused call invalidates nothing"
    a.history_capture()
    stats, acc = a.stats(), a.accumulator()
    assert a.set_triangles(1, d.deform(1, tr.twist(tr.grid_mesh()))) == 0
    assert L.rt_denoise(a.ctx, 2, None) == host_api.RT_E_STATE
    assert L.rt_reproject(a.ctx, None, None) == host_api.RT_E_STATE and L.rt_reproject_motion(a.ctx, None, None) == host_api.RT_E_STATE
    assert sp.same(a.accumulator(), acc) and all(sp.same(x, y) for x, y in zip(a.stats(), stats)), "accumulator and statistics are not touched"
    lst, n_act = a.active()
    assert n_act == 3 and lst.tolist() == [3, 5, 70], "an installed list survives"
    a.render_aovs(0.001)
    a.denoise(2)  # current again
    assert L.rt_reproject_motion(a.ctx, None, None) == host_api.RT_E_STATE, "the history stays invalid until a new capture"
    a.history_capture()
    assert a.reproject_motion() >= 0
    a.close()


def test_profiling_counts_one_query(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    for tlas in (True, False):
        r = host_api.HostRenderer(16, 8)
        if tlas:
            tr.mesh_scene(r.scene, [tr.SMALL, tr.grid_mesh()], tr.spread_transforms(r.scene, 3))
        else:
            r.scene.mesh_raw(1, r.scene.diffuse(0.8, (1, 1, 1)), tr.grid_mesh())
            r.scene.build(0)
        r.commit()
        d = td.Desc(host_api, r.scene)
        k = 1 if tlas else 0
        r.set_profiling(True)
        r.profile()
        assert r.set_triangles(k, d.deform(k, tr.twist(tr.grid_mesh()))) == 0
        prof = r.profile()
        assert prof["query"]["launches"] == 1 and prof["query"]["ms"] > 0 and all(prof[x]["launches"] == 0 for x in ("generate", "extend", "shade", "connect"))
        r.set_profiling(False)
        _check_layout(host_api, r, d, knobs, "profiled")
        r.close()


# ---- 5. refusals and the atomic failure ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(host_api, monkeypatch):
    _env(monkeypatch)
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    L = host_api.rt_lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = host_api.HostRenderer(16, 8)
    Ts = tr.spread_transforms(r.scene, tr.BEHAVIOUR_INSTANCES)
    tr.mesh_scene(r.scene, [tr.SMALL, tr.grid_mesh()], Ts)  # instances 1 and 3 are the mesh
    r.commit()
    d = td.Desc(host_api, r.scene)
    assert r.set_triangles(1, d.deform(1, tr.twist(tr.grid_mesh()))) == 0  # (a deformed scene, so that "as before" is not "as uploaded")
    before = _snapshot(r, 2)
    tl = r.download_tlas()
    O, D = tr.aimed_rays(512, 5, Ts[1::2], tr.twist(tr.grid_mesh()))
    hits = r.find_nearest(O, D)
    r.render_aovs(0.001)
    t = d.tris[1].copy()
    n = len(t)

    def spoiled(field, i, j, v):
        x = t.copy()
        x[field][i, j] = v
        return x

    cases = [("null triangles", lambda: L.rt_set_triangles(r.ctx, 1, None, n)),
             ("null context", lambda: L.rt_set_triangles(None, 1, p(t), n)),
             ("blas outside", lambda: L.rt_set_triangles(r.ctx, 2, p(t), n)),
             ("one triangle short", lambda: L.rt_set_triangles(r.ctx, 1, p(t), n - 1)),
             ("another blas's count", lambda: L.rt_set_triangles(r.ctx, 0, p(t), n)),
             ("nan vertex", lambda: L.rt_set_triangles(r.ctx, 1, p(spoiled("v1", 7, 2, np.nan)), n)),
             ("inf vertex", lambda: L.rt_set_triangles(r.ctx, 1, p(spoiled("v2", n - 1, 0, -np.inf)), n)),
             ("vertex beyond 1e29", lambda: L.rt_set_triangles(r.ctx, 1, p(spoiled("v0", 0, 1, 2e29)), n))]
    for what, call in cases:
        assert call() == ARG, what
    # the atomic failure: finite vertices under the 1e29 bound whose boxes make every union area reach FindBestMatch's 1e30 (tlas.cpp:52).
    # The mesh is 0.7 x 0.2 x 0.7: a factor of 1e16 gives two instances' union an area of about 7.7e31 (1e15 would leave 7.7e29 and a
    # TLAS that builds).  The records and the tree have been rewritten by the time the build fails; the call puts them back.
    huge = tr.triangles(t, tr.scale(tr.grid_mesh(), 1e16))
    assert L.rt_set_triangles(r.ctx, 1, p(huge), n) == UNSUP
    assert b"no finite union area" in L.rt_last_error(r.ctx)
    after = _snapshot(r, 2)
    for a in before:
        assert sp.same(after[a], before[a]), a
    assert np.array_equal(r.download_tlas(), tl)
    again = r.find_nearest(O, D)
    assert all(sp.same(hits[k], again[k]) for k in hits)
    assert L.rt_denoise(r.ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    # a transform that could take the new box beyond 1e30: instance 1 scaled by 1e9 (its box given, so the move itself is accepted) and
    # vertices of 3.5e20
    rec = ir.records(host_api, [1], [r.scene.trs((0, 0, 3), 1e9, 0.0, 0.0, 0.0)])
    assert r.set_instances(1, rec, d.bounds[1:2]) == 0
    d.move(1, rec, d.bounds[1:2])
    before = _snapshot(r, 2)
    assert L.rt_set_triangles(r.ctx, 1, p(tr.triangles(t, tr.scale(tr.grid_mesh(), 1e21))), n) == ARG
    after = _snapshot(r, 2)
    for a in before:
        assert sp.same(after[a], before[a]), a
    # rt_blas_array's own refusals
    nbytes = C.c_size_t(0)
    assert L.rt_blas_array(r.ctx, 1, 2, None, 0, C.byref(nbytes)) == UNSUP  # RT_LAYOUT_WIDE
    assert L.rt_blas_array(r.ctx, 2, 0, None, 0, C.byref(nbytes)) == ARG
    assert L.rt_blas_array(r.ctx, 1, 1, p(np.zeros(4, f32)), 16, C.byref(nbytes)) == ARG and nbytes.value == before["prims1"].nbytes
    assert L.rt_blas_array(r.ctx, 1, 0, None, 0, None) == ARG
    assert L.rt_scene_array(r.ctx, 1, None, 0, C.byref(nbytes)) == UNSUP, "rt_scene_array stays as it is"
    r.close()
    # no scene: RT_E_STATE
    g = host_api.HostRenderer(16, 8)
    assert L.rt_set_triangles(g.ctx, 0, p(t), n) == STATE and L.rt_blas_array(g.ctx, 0, 0, None, 0, C.byref(nbytes)) == STATE
    g.close()


def test_one_instance_takes_the_huge_mesh(host_api, monkeypatch):
    """the triangles the atomic failure was made with, under ONE instance: there is no pair to merge, the call succeeds"""
    knobs = _env(monkeypatch)
    r = host_api.HostRenderer(16, 8)
    tr.mesh_scene(r.scene, [tr.grid_mesh()], tr.spread_transforms(r.scene, 1))
    r.commit()
    d = td.Desc(host_api, r.scene)
    assert r.set_triangles(0, d.deform(0, tr.scale(tr.grid_mesh(), 1e16))) == 0
    _check_layout(host_api, r, d, knobs, "one instance, 1e16")
    r.close()


def test_an_instance_without_a_box_is_refused(host_api, monkeypatch):
    """an uploaded TLAS that has no leaf for instance 2: deforming another BLAS than its own is refused until rt_set_instances gives it a box"""
    knobs = _env(monkeypatch)
    r = host_api.HostRenderer(16, 8)
    tr.mesh_scene(r.scene, [tr.SMALL, tr.grid_mesh()], tr.spread_transforms(r.scene, 3))  # instances 0 and 2: SMALL, 1: the mesh
    r.commit()
    d = td.Desc(host_api, r.scene)
    two = np.zeros(3, dtype=ir.TLAS_NODE)
    for i in range(2):
        two[1 + i]["aabb_min"], two[1 + i]["aabb_max"], two[1 + i]["blas"] = d.bounds[i, :3], d.bounds[i, 3:], i
    two[0]["left_right"] = 1 | (2 << 16)
    two[0]["aabb_min"], two[0]["aabb_max"] = np.minimum(d.bounds[0, :3], d.bounds[1, :3]), np.maximum(d.bounds[0, 3:], d.bounds[1, 3:])
    d.tlas = two.view(np.uint32).reshape(-1, 8)
    r.upload_desc(d.desc())
    before = _snapshot(r, 2)
    assert r.set_triangles(1, tr.triangles(d.tris[1], tr.twist(tr.grid_mesh()))) == host_api.RT_E_ARG
    assert b"no box yet" in host_api.rt_lib().rt_last_error(r.ctx)
    after = _snapshot(r, 2)
    for a in before:
        assert sp.same(after[a], before[a]), a
    rec = ir.records(host_api, [0], [d.inst["transform"][2]])
    assert r.set_instances(2, rec) == 0
    d.move(2, rec)
    assert r.set_triangles(1, d.deform(1, tr.twist(tr.grid_mesh()))) == 0
    _check_layout(host_api, r, d, knobs, "after the box was given")
    r.close()


# ---- 6. two contexts on one device, through the host mirror ------------------------------------------------------------------------------
def test_commit_triangles_reaches_every_context(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    frames = []
    new = tr.twist(tr.grid_mesh())
    for devs in (None, [0, 0]):
        r = host_api.HostRenderer(32, 17, devices=devs)
        s = r.scene
        tr.mesh_scene(s, [tr.SMALL, tr.grid_mesh()], tr.spread_transforms(s, tr.BEHAVIOUR_INSTANCES))
        r.commit()  # Scene::Commit to context 0, CommitAlso to the second one
        s.set_mesh_vertices(1, new)
        s.commit_triangles(1)
        assert np.array_equal(r.download_tlas(), s.tlas_dump()), "CommitTriangles leaves the device's tree in tl"
        d = td.Desc(host_api, s)  # the mirror's own description after the deformation: refitted nodes, fresh boxes, the downloaded TLAS
        assert sp.same(tr.v9_of(d.tris[1]), new)
        for k in range(2 if devs else 1):
            ctx = r.ctx_at(k)
            assert ctx.value and (k == 0) == (ctx.value == r.ctx.value)
            _check_layout(host_api, r, d, knobs, "context %d" % k, ctx)
        s.rebuild_tlas()  # tlas::build on the host over the mirror's bounds: the instances of the mesh hold a fresh instance's box
        assert np.array_equal(r.download_tlas(), s.tlas_dump())
        r.tick()  # a Whitted Tick; with two contexts the rows are interleaved over them
        frames.append(r.tick_accumulator().copy())
        r.close()
    assert sp.same(frames[0], frames[1]) and (frames[0][..., :3] > 0).any()
