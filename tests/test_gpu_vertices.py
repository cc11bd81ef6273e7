"""rt_set_mesh_indices, rt_set_vertices and rt_set_vertices_device on the device (include/rt_amd.h, csrc/rt_vertices.h), through the C ABI:
after a deformation sent as a vertex array the context holds, byte for byte, what rt_set_triangles leaves of the assembled triangles and
what a fresh rt_upload_scene of the updated description would hold; the device's reduction drops no lane, wave or block; the host-memory
and the device-memory form agree; refusals leave the scene as it was; the call composes with its neighbours; the hits equal the oracle's;
and the host mirror's CommitVertices equals its CommitTriangles.

Every comparison is bitwise but one: a degenerate triangle's normal is a NaN whose sign and payload are the device's (x86 and gfx950 make
different default NaNs), in N.x, N.y, N.z and d of that one record.  A test that uses the rule (vertices_ref.same_prims) first asserts how
many triangles of its input have a NaN normal: exactly the ones the input was built with -- the two sentinels of a .tri mesh, one
deliberately degenerate triangle; the one larger number is the mixed scene of triangles_desc.LAYOUT_CASES, whose stellatedDode asset
ships eight faces with two corners at one position."""
import ctypes as C

import numpy as np
import pytest

import instances_ref as ir
import support as sp
import triangles_desc as td
import triangles_ref as tr
import vertices_ref as vr

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
HOWS = ("twist", "scale", "collapse")
ENVS = [{}, {"RT_TLAS_LDS": "0", "RT_WIDE": "1"}]
BUILT_IN_NANS = {"sentinel": 2, "mixed_small": 8}  # LAYOUT_CASES with degenerate triangles: see the module's docstring


def _env(monkeypatch, env=None):
    sp.clean_env(monkeypatch, env)
    return sp.layout_knobs(env)


def _scalars(s):
    """RT_LAYOUT_SCALARS without wideOK and wide8OK (words 9 and 10 keep their upload-time values)"""
    return np.delete(np.asarray(s), [9, 10])


def _snapshot(r, n_blas, ctx=None):
    out = {a: r.scene_array(a, ctx) for a in ("pairs", "reach", "inst", "scalars")}
    for k in range(n_blas):
        out["pairs%d" % k], out["prims%d" % k] = r.blas_array(k, "pairs", ctx), r.blas_array(k, "prims", ctx)
    return out


def _same_snapshot(a, b, d=None, k=None, nan=()):
    """two snapshots, bit for bit; with nan, the primitive records of BLAS k under the NaN rule"""
    for name in a:
        if len(nan) and name == "prims%d" % k:
            if not vr.same_prims(a[name], b[name], d.prim_idx[k], nan):
                return name
        elif not sp.same(a[name], b[name]):
            return name
    return None


def _check_layout(host_api, r, d, knobs, what, k=None, nan=(), ctx=None):
    """the context's arrays equal rt_layout_build's of the updated description (the records of BLAS k's triangles nan under the NaN rule)"""
    L = host_api.layout(d.desc(), *knobs)
    for j, (p0, p1, s0, s1) in enumerate(d.ranges()):
        assert sp.same(r.blas_array(j, "pairs", ctx), L["pairs"][16 * p0:16 * p1]), "%s: the pair records of blas %d" % (what, j)
        got, want = r.blas_array(j, "prims", ctx), L["prims"][16 * s0:16 * s1]
        if j == k and len(nan):
            assert vr.same_prims(got, want, d.prim_idx[j], nan), "%s: the primitive records of blas %d (NaN rule)" % (what, j)
        else:
            assert sp.same(got, want), "%s: the primitive records of blas %d" % (what, j)
    for a in ("pairs", "reach", "inst"):
        assert sp.same(r.scene_array(a, ctx), L[a]), "%s: %s differs from rt_layout_build of the updated description" % (what, a)
    assert np.array_equal(_scalars(r.scene_array("scalars", ctx)), _scalars(L["scalars"])), "%s: scalars" % what
    if d.use_tlas and ctx is None:
        assert np.array_equal(r.download_tlas(), d.tlas), "%s: rt_download_tlas differs from tlas::build over the boxes" % what
    return L


def _shared_scene(b, xyz, idx, n_inst=3):
    """SMALL and the indexed mesh under n_inst instances (the odd ones are the mesh): BLAS 1 is the mesh"""
    return tr.mesh_scene(b, [tr.SMALL, vr.assemble(xyz, idx)], tr.spread_transforms(b, n_inst))


def _renderer(host_api, build, w=16, h=8):
    r = host_api.HostRenderer(w, h)
    out = build(r.scene)
    r.commit()
    return r, out


def _case(host_api, scenes, name):
    """(renderer, its description, BLAS, xyz, idx, the vertices that stay, the NaN count the input is built with)"""
    if name in vr.SHARED:
        xyz, idx = vr.SHARED[name]()
        r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx))
        return r, td.Desc(host_api, r.scene), 1, xyz, idx, None, 0
    r, case = _renderer(host_api, lambda b: td.build_case(b, name, scenes))
    d = td.Desc(host_api, r.scene)
    xyz, idx = vr.weld(tr.v9_of(d.tris[case["k"]]))
    keep = (xyz == f32(999.0)).all(1) if case["sentinel"] else None
    return r, d, case["k"], xyz, idx, keep, BUILT_IN_NANS.get(name, 0)


# ---- 1. equal to rt_set_triangles and to a fresh layout --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", td.LAYOUT_CASES + ("ico", "lowBigB", "grid16"))
@pytest.mark.parametrize("env", ENVS, ids=["default", "wide_no_lds"])
def test_equals_set_triangles_and_a_fresh_layout(name, env, scenes, host_api, monkeypatch):
    knobs = _env(monkeypatch, env)
    r, d, k, xyz, idx, keep, n_nan = _case(host_api, scenes, name)
    twin, d2, *_ = _case(host_api, scenes, name)
    nb = len(d.blas)
    if name in vr.SHARED:
        assert len(xyz) < len(idx), "the mesh shares its vertices"
    assert r.set_mesh_indices(k, idx, len(xyz)) == 0
    _check_layout(host_api, r, d, knobs, "bound: nothing of the scene is touched")
    other = [(j, r.blas_array(j, "pairs"), r.blas_array(j, "prims")) for j in range(nb) if j != k]
    for how in HOWS:  # each from the uploaded vertices: every later one also shows that nothing of the one before is left
        new = vr.deformed(xyz, how, keep)
        nan = vr.nan_triangles(vr.assemble(new, idx))
        assert len(nan) == n_nan and np.array_equal(nan, vr.coincident_faces(xyz, idx)), "the NaN normals are the ones the input was built with"
        recs = vr.deform(d, k, new, idx)
        assert r.set_vertices(k, new) == 0, how
        _check_layout(host_api, r, d, knobs, how, k, nan)
        assert twin.set_triangles(k, recs) == 0
        assert _same_snapshot(_snapshot(r, nb), _snapshot(twin, nb), d, k, nan) is None, "%s: rt_set_triangles with the assembled records" % how
        if d.use_tlas:
            assert np.array_equal(r.download_tlas(), twin.download_tlas())
        for j, pairs, prims in other:
            assert sp.same(r.blas_array(j, "pairs"), pairs) and sp.same(r.blas_array(j, "prims"), prims), "blas %d is untouched" % j
    if not d.use_tlas:  # a later rt_set_time deforms from the new vertices, as after rt_set_triangles
        for x in (r, twin):
            x.set_time(0.7)
        assert _same_snapshot(_snapshot(r, nb), _snapshot(twin, nb), d, k, nan) is None, "rt_set_time after the call"
    r.close(), twin.close()


# ---- 2. the reduction's boundaries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", vr.BOUNDARY_SIZES)
def test_reduction_boundaries(n, host_api, monkeypatch):
    """each of the six extremes of the box on the first triangle, the last, and either side of every 64 and 256 boundary in turn: a lane,
    wave or block the reduction dropped would move reach, inst or the TLAS away from rt_set_triangles' of the same triangles"""
    knobs = _env(monkeypatch)
    base, idx = vr.boundary_mesh(n)
    r, _ = _renderer(host_api, lambda b: _shared_scene(b, base, idx, 4))  # instances 1 and 3 are the mesh
    twin, _ = _renderer(host_api, lambda b: _shared_scene(b, base, idx, 4))
    d = td.Desc(host_api, r.scene)
    old = d.tris[1]
    assert r.set_mesh_indices(1, idx, len(base)) == 0
    assert r.set_vertices(1, base) == 0
    plain = r.scene_array("reach")  # without the extremes
    for t in vr.boundary_targets(n):
        for e in range(6):
            xyz, _ = vr.boundary_vertices(n, e, t)
            assert r.set_vertices(1, xyz) == 0
            assert twin.set_triangles(1, tr.triangles(old, vr.assemble(xyz, idx))) == 0
            a, b = _snapshot(r, 2), _snapshot(twin, 2)
            assert _same_snapshot(a, b) is None, "extreme %d on triangle %d of %d: %s" % (e, t, n, _same_snapshot(a, b))
            assert np.array_equal(r.download_tlas(), twin.download_tlas()), (e, t)
            assert not sp.same(a["reach"], plain), "the extremes move reach"
    vr.deform(d, 1, xyz, idx)
    _check_layout(host_api, r, d, knobs, "the last variant")
    r.close(), twin.close()


# ---- 3. the host and the device form ---------------------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree(host_api, monkeypatch):
    import torch
    knobs = _env(monkeypatch)
    xyz, idx = vr.grid(16, 16)
    a, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx))
    b, _ = _renderer(host_api, lambda s: _shared_scene(s, xyz, idx))
    d = td.Desc(host_api, a.scene)
    for r in (a, b):
        assert r.set_mesh_indices(1, idx, len(xyz)) == 0
    dev = torch.device("cuda", host_api.rt_lib().rt_device_of(b.ctx))
    for how in HOWS:
        new = vr.deformed(xyz, how)
        t = torch.from_numpy(new).to(dev).contiguous()
        torch.cuda.synchronize(dev)  # the caller orders the producer before the call
        assert a.set_vertices(1, new) == 0
        assert b.set_vertices_device(1, t.data_ptr(), len(new)) == 0, host_api.rt_lib().rt_last_error(b.ctx)
        t.zero_()  # the array is the caller's again
        vr.deform(d, 1, new, idx)
        assert _same_snapshot(_snapshot(a, 2), _snapshot(b, 2)) is None, how
        _check_layout(host_api, b, d, knobs, "the device form, " + how)
    # a host pointer given to the device form: refused on the host, nothing launched, nothing changed
    before, tl = _snapshot(b, 2), b.download_tlas()
    b.render_aovs(0.001)
    L = host_api.rt_lib()
    assert b.set_vertices_device(1, xyz.ctypes.data, len(xyz)) == host_api.RT_E_ARG
    assert b"device memory" in L.rt_last_error(b.ctx)
    pinned = torch.from_numpy(xyz.copy()).pin_memory()
    assert b.set_vertices_device(1, pinned.data_ptr(), len(xyz)) == host_api.RT_E_ARG, "page-locked host memory is host memory"
    t = torch.from_numpy(xyz).to(dev).contiguous()
    torch.cuda.synchronize(dev)
    assert b.set_vertices_device(1, t.data_ptr() + 2, len(xyz)) == host_api.RT_E_ARG and b"aligned" in L.rt_last_error(b.ctx)
    assert b.set_vertices_device(1, 0, len(xyz)) == host_api.RT_E_ARG
    assert _same_snapshot(before, _snapshot(b, 2)) is None and np.array_equal(b.download_tlas(), tl)
    assert L.rt_denoise(b.ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    a.close(), b.close()


# ---- 4. refusals and atomicity ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    L = host_api.rt_lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    xyz, idx = vr.with_spare_vertex(*vr.grid(16, 16))
    nv, nt = len(xyz), len(idx)
    r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx, tr.BEHAVIOUR_INSTANCES))  # instances 1 and 3 are the mesh
    d = td.Desc(host_api, r.scene)
    assert r.set_vertices(1, xyz) == STATE and b"no indices" in L.rt_last_error(r.ctx), "nothing is bound yet"
    # binding: checked on the host, the first bad triangle named
    bad = idx.copy()
    bad[7, 1] = nv
    bad[300, 0] = nv + 5
    for what, call in [("an index out of range", lambda: r.set_mesh_indices(1, bad, nv)), ("one triangle short", lambda: r.set_mesh_indices(1, idx[:-1], nv)),
                       ("another blas's count", lambda: r.set_mesh_indices(0, idx, nv)), ("no vertices", lambda: L.rt_set_mesh_indices(r.ctx, 1, p(idx), nt, 0)),
                       ("blas outside", lambda: r.set_mesh_indices(2, idx, nv)), ("too few vertices", lambda: r.set_mesh_indices(1, idx, nv - 2))]:
        assert call() == ARG, what
        if what == "an index out of range":
            assert b"triangle 7 " in L.rt_last_error(r.ctx)
    assert L.rt_set_mesh_indices(None, 1, p(idx), nt, nv) == ARG
    assert r.set_vertices(1, xyz) == STATE, "a refused binding binds nothing"
    assert r.set_mesh_indices(1, idx, nv) == 0
    assert r.set_vertices(1, vr.deformed(xyz, "twist")) == 0  # (a deformed scene, so that "as before" is not "as uploaded")
    vr.deform(d, 1, vr.deformed(xyz, "twist"), idx)
    before, tl = _snapshot(r, 2), r.download_tlas()
    r.render_aovs(0.001)

    def unchanged(what):
        assert _same_snapshot(before, _snapshot(r, 2)) is None and np.array_equal(r.download_tlas(), tl), what
        assert L.rt_denoise(r.ctx, 1, None) == 0, what + ": a refused call invalidates nothing, the G-buffer is still current"

    for what, call in [("a wrong vertex count", lambda: r.set_vertices(1, xyz[:-1])), ("null vertices", lambda: L.rt_set_vertices(r.ctx, 1, None, nv)),
                       ("null context", lambda: L.rt_set_vertices(None, 1, p(xyz), nv)), ("blas outside", lambda: L.rt_set_vertices(r.ctx, 2, p(xyz), nv))]:
        assert call() == ARG, what
    assert r.set_vertices(0, xyz) == STATE, "blas 0 has no binding"
    unchanged("argument refusals")
    spoiled = vr.refusal_inputs(xyz, idx)
    for name, (v, vtx, used) in spoiled.items():
        if used:
            assert r.set_vertices(1, v) == ARG, name
            msg = L.rt_last_error(r.ctx).decode()
            assert "non-finite vertex coordinate or one beyond 1e29" in msg
            tri = int(msg.split("triangle ")[1].split()[0])
            assert vtx in idx[tri], "the message names a triangle that has the vertex"
            unchanged(name)
    # the atomic failure of test_gpu_triangles.py: boxes whose every union area reaches FindBestMatch's 1e30
    assert r.set_vertices(1, (xyz * f32(1e16)).astype(f32)) == UNSUP
    assert b"rt_set_vertices" in L.rt_last_error(r.ctx) and b"no finite union area" in L.rt_last_error(r.ctx)
    unchanged("the TLAS build failed")
    # a transform that could take the new box beyond 1e30
    rec = ir.records(host_api, [1], [r.scene.trs((0, 0, 3), 1e9, 0.0, 0.0, 0.0)])
    assert r.set_instances(1, rec, d.bounds[1:2]) == 0, "the binding survives rt_set_instances"
    d.move(1, rec, d.bounds[1:2])
    before, tl = _snapshot(r, 2), r.download_tlas()
    r.render_aovs(0.001)
    assert r.set_vertices(1, (xyz * f32(1e21)).astype(f32)) == ARG and b"beyond 1e30" in L.rt_last_error(r.ctx)
    unchanged("a transform takes the box beyond 1e30")
    rec = ir.records(host_api, [1], [d.inst["transform"][3]])
    assert r.set_instances(1, rec) == 0
    d.move(1, rec)
    # the same values in a vertex no triangle names: accepted, and the result is the clean array's
    for name, (v, vtx, used) in spoiled.items():
        if not used:
            assert r.set_vertices(1, v) == 0, name
            vr.deform(d, 1, v, idx)
            _check_layout(host_api, r, d, knobs, name)
    # the binding survives rt_set_triangles, an unbinding ends it, so does rt_upload_scene
    assert r.set_triangles(1, d.deform(1, tr.scale(vr.assemble(xyz, idx), 2.0))) == 0
    assert r.set_vertices(1, xyz) == 0
    vr.deform(d, 1, xyz, idx)
    _check_layout(host_api, r, d, knobs, "after rt_set_triangles")
    assert r.set_mesh_indices(1, None, 0) == 0 and r.set_vertices(1, xyz) == STATE
    assert r.set_mesh_indices(1, idx, nv) == 0 and r.set_vertices(1, xyz) == 0
    r.upload_desc(d.desc())
    assert r.set_vertices(1, xyz) == STATE, "the binding ends with rt_upload_scene"
    r.close()
    g = host_api.HostRenderer(16, 8)  # no scene
    assert L.rt_set_mesh_indices(g.ctx, 0, p(idx), nt, nv) == STATE and L.rt_set_vertices(g.ctx, 0, p(xyz), nv) == STATE
    assert L.rt_set_vertices_device(g.ctx, 0, p(xyz), nv) == STATE
    g.close()


def test_one_degenerate_triangle_gets_a_nan_normal(host_api, monkeypatch):
    """a triangle with two corners at one point: its record holds NaNs in N and d, its box still counts for the tree, and the object box
    (so reach) skips it"""
    knobs = _env(monkeypatch)
    xyz, idx = vr.boundary_mesh(65)
    r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx))
    d = td.Desc(host_api, r.scene)
    assert r.set_mesh_indices(1, idx, len(xyz)) == 0
    new = xyz.copy()
    new[idx[64, 1]] = new[idx[64, 2]] = f32(5.0)  # its own two vertices at one point, far outside the others' box
    nan = vr.nan_triangles(vr.assemble(new, idx))
    assert nan.tolist() == [64], "one deliberately degenerate triangle"
    vr.deform(d, 1, new, idx)
    assert r.set_vertices(1, new) == 0
    _check_layout(host_api, r, d, knobs, "one degenerate triangle", 1, nan)
    got = sp.bits(r.blas_array(1, "prims")).reshape(-1, 16)
    slot = int(np.flatnonzero(d.prim_idx[1] == 64)[0])
    assert np.isnan(got[slot, [3, 7, 11, 12]].view(f32)).all()
    r.close()


# ---- 5. composition ----------------------------------------------------------------------------------------------------------------------------
def test_composes_with_set_instances_and_set_triangles(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    xyz, idx = vr.SHARED["ico"]()
    r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx))
    d = td.Desc(host_api, r.scene)
    s = r.scene
    assert r.set_mesh_indices(1, idx, len(xyz)) == 0
    Ts = [s.trs((f32(-1.0 + 0.8 * i), f32(0.2 * i), f32(3.0 + 0.3 * i)), f32(1.0 + 0.2 * i), 0.0, f32(0.4 * i + 0.2), 0.0) for i in range(d.n)]
    rec = ir.records(host_api, [int(b) for b in d.inst["blas"]], Ts)
    given = np.stack([np.concatenate([d.bounds[i, :3] - f32(0.5 + i), d.bounds[i, 3:] + f32(1.5 + i)]) for i in range(d.n)]).astype(f32)
    assert r.set_instances(0, rec, given) == 0
    d.move(0, rec, given)
    new = vr.deformed(xyz, "twist")
    assert r.set_vertices(1, new) == 0
    vr.deform(d, 1, new, idx)
    assert sp.same(d.bounds[0], given[0]) and sp.same(d.bounds[2], given[2]) and not sp.same(d.bounds[1], given[1])
    _check_layout(host_api, r, d, knobs, "deformed after the move")
    rec1 = ir.records(host_api, [1], [s.trs((0.3, 0.4, 2.5), 1.5, 0.0, 1.0, 0.0)])
    assert r.set_instances(1, rec1) == 0
    d.move(1, rec1)
    _check_layout(host_api, r, d, knobs, "moved after the deformation")
    # rt_set_triangles changes obj_idx and material; rt_set_vertices keeps what the records hold now
    was = d.tris[1].copy()
    d.tris[1]["obj_idx"] = was["obj_idx"] + 7
    other = 0 if int(was["material"][0]) != 0 else 1
    d.tris[1]["material"] = other
    assert r.set_triangles(1, d.deform(1, vr.assemble(new, idx))) == 0
    _check_layout(host_api, r, d, knobs, "ids and material changed")
    new2 = vr.deformed(xyz, "scale")
    assert r.set_vertices(1, new2) == 0
    recs = vr.deform(d, 1, new2, idx)
    assert (recs["material"] == other).all() and np.array_equal(recs["obj_idx"], was["obj_idx"] + 7)
    _check_layout(host_api, r, d, knobs, "deformed again: ids and material kept")
    r.close()


def test_reproject_deform_follows_set_vertices(host_api, monkeypatch):
    """the kept records, the invalidation and the carry are rt_set_triangles': accumulator, statistics and n_carried after
    rt_reproject_deform are the same bits in both contexts"""
    _env(monkeypatch)
    xyz, idx = vr.grid(16, 16)
    new = vr.deformed(xyz, "twist")
    out = []
    for vertices in (True, False):
        r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx, tr.BEHAVIOUR_INSTANCES), 33, 9)
        d = td.Desc(host_api, r.scene)
        if vertices:
            assert r.set_mesh_indices(1, idx, len(xyz)) == 0
        r.stats_enable(True)
        r.render(host_api.RT_MODE_PATH, 0, 2)
        r.render_aovs(0.001)
        r.history_capture()
        L = host_api.rt_lib()
        recs = vr.deform(d, 1, new, idx)
        assert (r.set_vertices(1, new) if vertices else r.set_triangles(1, recs)) == 0
        assert L.rt_denoise(r.ctx, 1, None) == host_api.RT_E_STATE, "the G-buffer went stale"
        assert L.rt_reproject(r.ctx, None, None) == host_api.RT_E_STATE and L.rt_reproject_motion(r.ctx, None, None) == host_api.RT_E_STATE
        r.render_aovs(0.001)
        n = r.reproject_deform()
        out.append((n, sp.state(r)))
        r.close()
    assert out[0][0] == out[1][0] > 0 and sp.same_state(out[0][1], out[1][1])


def test_profiling_counts_one_query(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    xyz, idx = vr.grid(16, 16)
    for tlas in (True, False):
        r = host_api.HostRenderer(16, 8)
        if tlas:
            _shared_scene(r.scene, xyz, idx)
        else:
            r.scene.mesh_raw(1, r.scene.diffuse(0.8, (1, 1, 1)), vr.assemble(xyz, idx))
            r.scene.build(0)
        r.commit()
        d = td.Desc(host_api, r.scene)
        k = 1 if tlas else 0
        assert r.set_mesh_indices(k, idx, len(xyz)) == 0
        r.set_profiling(True)
        r.profile()
        bad = xyz.copy()
        bad[5, 0] = np.inf
        assert r.set_vertices(k, bad) == host_api.RT_E_ARG  # a refused call leaves no entry
        new = vr.deformed(xyz, "twist")
        assert r.set_vertices(k, new) == 0
        prof = r.profile()
        assert prof["query"]["launches"] == 1 and prof["query"]["ms"] > 0 and all(prof[x]["launches"] == 0 for x in ("generate", "extend", "shade", "connect"))
        r.set_profiling(False)
        vr.deform(d, k, new, idx)
        _check_layout(host_api, r, d, knobs, "profiled")
        r.close()


def test_a_second_context_behaves_the_same(host_api, monkeypatch):
    knobs = _env(monkeypatch)
    xyz, idx = vr.SHARED["lowBigB"]()
    r = host_api.HostRenderer(32, 17, devices=[0, 0])
    _shared_scene(r.scene, xyz, idx)
    r.commit()
    d = td.Desc(host_api, r.scene)
    second = r.ctx_at(1)
    assert second.value and second.value != r.ctx.value
    assert r.set_mesh_indices(1, idx, len(xyz), second) == 0
    assert r.set_vertices(1, xyz) == host_api.RT_E_STATE, "a binding belongs to its context"
    before = _snapshot(r, 2)
    new = vr.deformed(xyz, "twist")
    assert r.set_vertices(1, new, second) == 0
    assert _same_snapshot(before, _snapshot(r, 2)) is None, "context 0 is untouched"
    vr.deform(d, 1, new, idx)
    _check_layout(host_api, r, d, knobs, "context 1", ctx=second)
    r.close()


# ---- 6. the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_hits_equal_a_fresh_oracle_scene(host_api, oracle_api, monkeypatch):
    _env(monkeypatch)
    xyz, idx = vr.grid(12, 12)
    r, _ = _renderer(host_api, lambda b: _shared_scene(b, xyz, idx, tr.BEHAVIOUR_INSTANCES))
    Ts = tr.spread_transforms(r.scene, tr.BEHAVIOUR_INSTANCES)
    assert r.set_mesh_indices(1, idx, len(xyz)) == 0
    new = vr.deformed(xyz, "twist")
    assert r.set_vertices(1, new) == 0
    v9 = vr.assemble(new, idx)
    o = oracle_api.OracleScene()
    tr.mesh_scene(o, [tr.SMALL, v9], tr.spread_transforms(o, tr.BEHAVIOUR_INSTANCES))  # its own build over the assembled triangles: another tree
    O, D = tr.aimed_rays(tr.BEHAVIOUR_RAYS, 41, Ts[1::2], v9)
    ref, got = o.find_nearest(O, D), r.find_nearest(O, D)
    assert np.array_equal(got["obj"], ref["obj"]) and sp.same(got["t"], ref["t"])
    hit = ref["obj"] != -1
    assert (ref["obj"] >= 2000).sum() >= len(O) // 4 and sp.same(got["normal"][hit], ref["normal"][hit])
    assert np.array_equal(r.is_occluded(O, D), o.is_occluded(O, D)["occluded"])
    r.close()


# ---- 7. the host mirror ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one", "two"])
def test_commit_vertices_equals_commit_triangles(devices, host_api, monkeypatch):
    """Renderer::CommitVertices of an .obj mesh (shared vertices, 1-based faces) against Renderer::CommitTriangles of the same mesh state"""
    _env(monkeypatch)
    assets = __import__("conftest").pkg("assets")

    def build(b):
        b.area_light(11, (0, 6.0, 0), 16.0, (1, 1, 1), 2.0, (0, -1, 0))
        mat = b.diffuse(0.8, (1, 0.2, 0.2), 0.0, 1, 1)
        ids = [b.mesh_raw(1, mat, tr.SMALL), b.mesh_obj(2, assets.obj_path("ico"), mat, (0.0, 0.4, 0.0), 0.4)]
        b.build_tlas(0, [(ids[i % 2], T) for i, T in enumerate(tr.spread_transforms(b, 4))])

    out = []
    for vertices in (True, False):
        r = host_api.HostRenderer(32, 17, devices=devices)
        build(r.scene)
        r.commit()
        s = r.scene
        xyz, faces = s.mesh_indexed(1)
        assert (len(xyz), len(faces)) == vr.SHARED_COUNTS["ico"]
        with pytest.raises(RuntimeError):
            r.commit_vertices(5)
        for how in ("twist", "scale"):  # the second commit finds the faces bound
            new = vr.deformed(xyz, how)
            if vertices:
                s.set_mesh_vertex_array(1, new)
                r.commit_vertices(1)
            else:
                s.set_mesh_vertices(1, vr.assemble(new, faces - 1))
                r.commit_triangles(1)
            assert np.array_equal(r.download_tlas(), s.tlas_dump()), "the device's tree is left in tl"
        assert sp.same(s.mesh_tris(1)[0][:, :9], vr.assemble(new, faces - 1)), "Mesh::update: the triangles follow the vertices"
        out.append([_snapshot(r, 2, r.ctx_at(k) if devices else None) for k in range(2 if devices else 1)] + [s.tlas_dump(), s.bvh_dump(1)["nodes"]])
        r.close()
    for a, b in zip(out[0][:-2], out[1][:-2]):
        assert _same_snapshot(a, b) is None
    assert np.array_equal(out[0][-2], out[1][-2]) and np.array_equal(out[0][-1], out[1][-1])
