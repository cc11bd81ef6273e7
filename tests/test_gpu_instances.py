"""rt_set_instances on the device (include/rt_amd.h, csrc/rt_instances.h), through the C ABI: after a move the context holds, byte for byte,
what a fresh rt_upload_scene of the updated description would -- the arrays themselves (rt_scene_array against rt_layout_build), every
query, frame and executed-walk counter against a freshly uploaded context, the hits against the oracle on a freshly built scene -- and the
call invalidates what rt_set_time invalidates, refuses bad input on the host and leaves the scene as it was when it fails."""
import ctypes as C

import numpy as np
import pytest

import instances_ref as ir
import support as sp
from conftest import random_rays
from test_layout_cpu import RtSceneDesc

pytestmark = pytest.mark.gpu
f32 = np.float32
ARRAYS = ("pairs", "reach", "inst", "scalars")
N_SPLIT = ir.smallest_n_without_lds()  # 38: the first n whose TLAS copy leaves fewer than RT_STACK_ROWS_MIN rows


def _env(monkeypatch, env=None):
    sp.clean_env(monkeypatch, env)
    return sp.layout_knobs(env)


def _build(scenes, scene, name, n=0):
    if name == "tlas_test2":
        return scenes.tlas_test2(scene)
    if name == "pretty_tlas":
        return scenes.pretty_tlas(scene, 8)
    return ir.triangles_scene(scene, ir.grid_transforms(scene, n))


def _renderer(host_api, scenes, name, n=0, w=16, h=8):
    r = host_api.HostRenderer(w, h)
    _build(scenes, r.scene, name, n)
    r.commit()
    return r


class Mirror:
    """what the test knows of the scene a context holds: the description it was uploaded from, the instance records and every instance's box"""

    def __init__(self, host_api, scene):
        self.ha, self.scene = host_api, scene
        self.ptr = scene.describe()
        d = RtSceneDesc.from_address(self.ptr.value)
        self.n = d.n_instances
        dumps = [scene.instance_dump(i) for i in range(self.n)]
        self.rec = np.zeros(self.n, dtype=host_api.RT_INSTANCE_DTYPE)
        for i, x in enumerate(dumps):
            self.rec[i] = (x["blas"], x["T"], x["invT"])
        self.bounds = np.stack([x["bounds"] for x in dumps]).astype(f32)  # == the leaf boxes of the uploaded TLAS
        self.local = {}
        for i, x in enumerate(dumps):
            nodes = scene.bvh_dump(x["blas"])["nodes"]
            self.local[i] = np.concatenate([nodes[0, 0:3], nodes[0, 4:7]]).view(f32)

    def move(self, first, Ts, given=None):
        """the records of a move of instances first.. to Ts and the boxes they get: 'given' (what is sent as bounds6), or a fresh instance's"""
        rec = ir.records(self.ha, [int(self.rec["blas"][first + k]) for k in range(len(Ts))], Ts)
        self.rec[first:first + len(Ts)] = rec
        for k, T in enumerate(Ts):
            self.bounds[first + k] = given[k] if given is not None else ir.fresh_bounds(self.local[first + k], T)
        return rec

    def desc(self, nodes):
        """the updated description: the uploaded one with the instance records and tlas_nodes replaced"""
        d = RtSceneDesc.from_buffer_copy(RtSceneDesc.from_address(self.ptr.value))
        self._keep = (self.rec.copy(), np.ascontiguousarray(nodes))
        d.instances, d.tlas_nodes, d.tlas_nodes_used = self._keep[0].ctypes.data, self._keep[1].ctypes.data, len(nodes)
        self._d = d
        return C.c_void_p(C.addressof(d))


def _check_layout(host_api, r, m, knobs, what):
    """the context's arrays equal rt_layout_build's of the updated description; its TLAS is rt_build_tlas's and tlas::build's of the boxes"""
    nodes = r.download_tlas()
    assert len(nodes) == 2 * m.n, what
    assert np.array_equal(nodes, r.build_tlas(m.bounds)), "%s: rt_download_tlas differs from rt_build_tlas on the same boxes" % what
    assert np.array_equal(nodes, ir.tlas_build(m.bounds)), "%s: rt_download_tlas differs from tlas::build on the same boxes" % what
    L = host_api.layout(m.desc(nodes), *knobs)
    for a in ARRAYS:
        assert sp.same(r.scene_array(a), L[a]), "%s: %s differs from rt_layout_build of the updated description" % (what, a)
    return L


def _union(a, b):
    return np.concatenate([np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])]).astype(f32)


# ---- 1. layout equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("triangles", 1), ("triangles", 2), ("tlas_test2", 3), ("pretty_tlas", 8), ("triangles", 17),
                                    ("triangles", N_SPLIT - 1), ("triangles", N_SPLIT)], ids=lambda v: str(v))
@pytest.mark.parametrize("env", [{}, {"RT_TLAS_LDS": "0", "RT_WIDE": "1", "RT_WIDE8": "1"}], ids=["default", "wide_no_lds"])
def test_layout_equals_a_fresh_layout(name, n, env, scenes, host_api, monkeypatch):
    knobs = _env(monkeypatch, env)
    r = _renderer(host_api, scenes, name, n)
    m = Mirror(host_api, r.scene)
    n = m.n
    L0 = host_api.layout(m.ptr, *knobs)
    for a in ARRAYS:  # before any move: what upload left
        assert sp.same(r.scene_array(a), L0[a]), a
    assert np.array_equal(r.download_tlas(), r.scene.tlas_dump())
    s = r.scene
    new = lambda i, k: s.trs((f32(-2.0 + 0.37 * i + 0.1 * k), f32(0.1 * k), f32(3.0 + 0.11 * i)), f32(1.0 + 0.25 * k), 0.0, f32(0.3 * i + k), f32(0.05 * k))
    one = n // 2
    # (a) one instance, the device computes its box
    assert r.set_instances(one, m.move(one, [new(one, 1)])) == 0
    L = _check_layout(host_api, r, m, knobs, "one, NULL")
    assert L["tlasLds"] == (1 if knobs[2] and n < N_SPLIT else 0) and L["tlasPairs"] == (n if n > 1 else 0)
    # (b) all instances, boxes given: each the union of the last box and the fresh one, as a caller's bvhInstance accumulates them
    Ts = [new(i, 2) for i in range(n)]
    given = np.stack([_union(m.bounds[i], ir.fresh_bounds(m.local[i], Ts[i])) for i in range(n)])
    assert r.set_instances(0, m.move(0, Ts, given), given) == 0
    _check_layout(host_api, r, m, knobs, "all, given")
    # (c) all, NULL; (d) the last one, given
    assert r.set_instances(0, m.move(0, [new(i, 3) for i in range(n)])) == 0
    _check_layout(host_api, r, m, knobs, "all, NULL")
    g = _union(m.bounds[n - 1], np.array([-1, -1, -1, 1, 1, 1], dtype=f32))[None]
    assert r.set_instances(n - 1, m.move(n - 1, [new(n - 1, 4)], g), g) == 0
    _check_layout(host_api, r, m, knobs, "last, given")
    r.close()


def test_hand_made_tlas_is_replaced(scenes, host_api, monkeypatch):
    """An uploaded TLAS that is not tlas::build's: a left-deep chain over tlas_test2's three instances, two pair records instead of three.
    The first update replaces it (three records) and the split of the LDS follows."""
    knobs = _env(monkeypatch)
    r = _renderer(host_api, scenes, "tlas_test2")
    m = Mirror(host_api, r.scene)
    chain = np.zeros(5, dtype=ir.TLAS_NODE)
    for i in range(3):
        chain[1 + i]["aabb_min"], chain[1 + i]["aabb_max"], chain[1 + i]["blas"] = m.bounds[i, :3], m.bounds[i, 3:], i
    for at, (a, b) in ((4, (2, 3)), (0, (1, 4))):
        chain[at]["left_right"] = a | (b << 16)
        chain[at]["aabb_min"], chain[at]["aabb_max"] = np.minimum(chain[a]["aabb_min"], chain[b]["aabb_min"]), np.maximum(chain[a]["aabb_max"], chain[b]["aabb_max"])
    chained = m.desc(chain.view(np.uint32).reshape(-1, 8))
    L0 = host_api.layout(chained, *knobs)
    assert L0["tlasPairs"] == 2
    r.upload_desc(chained)
    for a in ARRAYS:
        assert sp.same(r.scene_array(a), L0[a]), a
    assert np.array_equal(r.download_tlas(), chain.view(np.uint32).reshape(-1, 8))
    O, D = random_rays(1024, 9)
    before = r.find_nearest(O, D)
    # an update that moves nothing: the same records, the same boxes -- the tree is tlas::build's now, the hits are the same
    assert r.set_instances(0, m.rec.copy(), m.bounds) == 0
    L = _check_layout(host_api, r, m, knobs, "chain -> tlas::build")
    assert L["tlasPairs"] == 3 and len(r.scene_array("pairs")) == len(L0["pairs"]) + 16
    after = r.find_nearest(O, D)
    assert all(sp.same(before[k], after[k]) for k in before)
    r.close()


# ---- 2. the same results as a fresh upload ---------------------------------------------------------------------------------------------
def _moved_pair(host_api, scenes, name, n, w=64, h=48):
    """context A: uploaded, then moved twice; context B: a fresh rt_upload_scene of the updated description"""
    a = _renderer(host_api, scenes, name, n, w, h)
    m = Mirror(host_api, a.scene)
    s = a.scene
    if name == "tlas_test2":
        Ts = ir.mesh_transforms(s, 0.6)
    else:
        Ts = ir.grid_transforms(s, m.n, turn=0.8, scale=1.3, shift=(0.2, 0.1, -0.3))
    assert a.set_instances(0, m.move(0, Ts)) == 0
    g = _union(m.bounds[1], m.bounds[0])[None]
    assert a.set_instances(1, m.move(1, [Ts[0]], g), g) == 0  # instance 1 onto instance 0's place, under a box that holds both
    b = host_api.HostRenderer(w, h)
    b.upload_desc(m.desc(a.download_tlas()))
    return a, b, m


@pytest.mark.parametrize("name,n", [("tlas_test2", 3), ("triangles", 17)], ids=lambda v: str(v))
@pytest.mark.parametrize("env", [{}, {"RT_TLAS_LDS": "0"}, {"RT_WIDE": "1"}, {"RT_WIDE8": "1"}], ids=["default", "no_lds", "wide", "wide8"])
def test_results_equal_a_fresh_upload(name, n, env, scenes, host_api, monkeypatch):
    _env(monkeypatch, env)
    a, b, m = _moved_pair(host_api, scenes, name, n)
    for x in ARRAYS:
        assert sp.same(a.scene_array(x), b.scene_array(x)), x
    O, D = ir.aimed_rays(4096, 21, m.rec["transform"])
    tmax = np.random.default_rng(4).uniform(0.1, 12.0, len(O)).astype(f32)
    out = []
    for r in (a, b):
        r.set_counting(host_api.RT_COUNT_EXECUTED)
        r.counters()
        hit = r.find_nearest(O, D)
        occ = r.is_occluded(O, D, tmax)
        cq = r.counters()
        r.render(host_api.RT_MODE_PATH, 0, 2)
        path = r.accumulator()
        cp = r.counters()
        r.set_counting(False)
        r.clear()
        r.render(host_api.RT_MODE_WHITTED, 0, 1)
        out.append((hit, occ, cq, path, cp, r.accumulator()))
    (hit, occ, cq, path, cp, wh), (hit2, occ2, cq2, path2, cp2, wh2) = out
    assert all(sp.same(hit[k], hit2[k]) for k in hit) and np.array_equal(occ, occ2)
    # (coverage of the test's own rays, whatever the library answers: at least 1 in 20 ends on instanced geometry, mesh objIdx >= 1000)
    assert (hit["obj"] >= 1000).sum() >= len(O) // 20 and len(O) // 20 <= occ.sum() < len(occ), "the rays meet the instances"
    assert cq == cq2 and cq["instance_visits"] > 0 and cq["tlas_inner"] > 0, "the executed walk (reach culling included) is the fresh upload's"
    assert sp.same(path, path2) and cp == cp2 and sp.same(wh, wh2)
    assert np.isfinite(wh[..., :3]).any() and (path[..., :3] > 0).any()
    a.close(), b.close()


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mesh", "triangles"])
def test_moved_scene_equals_a_fresh_oracle_scene(kind, scenes, host_api, oracle_api, monkeypatch):
    _env(monkeypatch)
    r = host_api.HostRenderer(32, 16)
    s = r.scene
    if kind == "mesh":
        ir.mesh_scene(s, ir.mesh_transforms(s, 0.0))
        Ts = ir.mesh_transforms(s, 0.7)
        make = lambda o: ir.mesh_scene(o, ir.mesh_transforms(o, 0.7))
    else:
        ir.triangles_scene(s, ir.grid_transforms(s, 17))
        Ts = ir.grid_transforms(s, 17, turn=1.1, scale=1.4, shift=(0.3, 0.0, 0.2))
        make = lambda o: ir.triangles_scene(o, ir.grid_transforms(o, 17, turn=1.1, scale=1.4, shift=(0.3, 0.0, 0.2)))
    r.commit()
    m = Mirror(host_api, s)
    assert r.set_instances(0, m.move(0, Ts)) == 0  # every instance, fresh boxes: the scene a fresh build with Ts makes
    o = oracle_api.OracleScene()
    make(o)
    assert np.array_equal(r.download_tlas(), o.tlas_dump())
    O, D = ir.aimed_rays(2048, 33, Ts)
    ref = o.find_nearest(O, D)
    r.set_counting(host_api.RT_COUNT_REFERENCE)
    r.counters()
    got = r.find_nearest(O, D)
    cnt = r.counters()
    r.set_counting(False)
    assert np.array_equal(got["obj"], ref["obj"]) and sp.same(got["t"], ref["t"])
    hit = ref["obj"] != -1
    assert (ref["obj"] >= 1000).sum() >= len(O) // 20 and sp.same(got["normal"][hit], ref["normal"][hit])
    for k in ("inner_visits", "prim_tests", "tlas_inner", "instance_visits", "rays_nearest", "brute_tests", "light_tests"):
        assert cnt[k] == ref["counters"][k], k
    refo = o.is_occluded(O, D)
    r.set_counting(host_api.RT_COUNT_REFERENCE)
    r.counters()
    goto = r.is_occluded(O, D)
    cnt = r.counters()
    r.set_counting(False)
    assert np.array_equal(goto, refo["occluded"])
    for k in ("inner_visits", "prim_tests", "tlas_inner", "instance_visits", "rays_occluded"):
        assert cnt[k] == refo["counters"][k], k
    assert np.array_equal(r.is_occluded(O, D), refo["occluded"])  # the timed kernels
    r.close()


# ---- 4. repeated moves ---------------------------------------------------------------------------------------------------------------
def test_ten_moves_without_boxes_do_not_accumulate(scenes, host_api, monkeypatch):
    _env(monkeypatch)
    a, b = _renderer(host_api, scenes, "tlas_test2"), _renderer(host_api, scenes, "tlas_test2")
    m = Mirror(host_api, a.scene)
    turn = lambda k: [a.scene.trs((0.5, 0, 3), 4, 0.0, f32(np.deg2rad(36.0 * k)), 0.0)]
    for k in range(1, 11):
        assert a.set_instances(0, m.move(0, turn(k))) == 0
    assert b.set_instances(0, ir.records(host_api, [int(m.rec["blas"][0])], turn(10))) == 0
    for x in ARRAYS:
        assert sp.same(a.scene_array(x), b.scene_array(x)), x
    assert np.array_equal(a.download_tlas(), b.download_tlas())
    _check_layout(host_api, a, m, (-1, 0, 1), "ten moves")
    a.close(), b.close()


def test_commit_instances_accumulates_like_the_host_mirror(scenes, host_api, monkeypatch):
    knobs = _env(monkeypatch)
    r = _renderer(host_api, scenes, "tlas_test2")
    s = r.scene
    fresh = Mirror(host_api, s)
    for k in range(1, 11):
        s.set_transforms(0, [s.trs((0.5, 0, 3), 4, 0.0, f32(np.deg2rad(36.0 * k)), 0.0)])
        s.commit_instances()
    m = Mirror(host_api, s)  # the host mirror's own records and (grown) bounds
    want = ir.fresh_bounds(fresh.local[0], s.trs((0.5, 0, 3), 4, 0.0, f32(np.deg2rad(360.0)), 0.0))
    assert np.all(m.bounds[0, :3] <= want[:3]) and np.all(m.bounds[0, 3:] >= want[3:]) and not np.array_equal(m.bounds[0], want), "the box has grown"
    dev = r.download_tlas()
    assert np.array_equal(dev, s.tlas_dump()), "CommitInstances leaves the device's tree in tl"
    assert sp.same(dev[1:4, 0:3], m.bounds[:, :3]) and sp.same(dev[1:4, 4:7], m.bounds[:, 3:]), "the leaves are instance_dump's bounds"
    s.rebuild_tlas()  # tlas::build on the host over the same bounds
    assert np.array_equal(dev, s.tlas_dump())
    L = host_api.layout(s.describe(), *knobs)
    for x in ARRAYS:
        assert sp.same(r.scene_array(x), L[x]), x
    r.close()


# ---- 5. invalidation --------------------------------------------------------------------------------------------------------------------
def test_a_move_invalidates_what_set_time_invalidates(scenes, host_api, monkeypatch):
    _env(monkeypatch)
    w, h = 48, 32
    a = _renderer(host_api, scenes, "tlas_test2", 0, w, h)
    m = Mirror(host_api, a.scene)
    a.stats_enable(True)
    a.render(host_api.RT_MODE_PATH, 0, 16)  # a dense batch before the move, above RT_PRIMARY_TABLE_MIN's 12 frames: the primary-hit table exists
    a.render_aovs(0.001)
    a.denoise(2)
    a.history_capture()
    a.set_active([3, 5, 700])
    stats = a.stats()
    acc = a.accumulator()
    Ts = ir.mesh_transforms(a.scene, 0.9)
    assert a.set_instances(0, m.move(0, Ts)) == 0
    L = host_api.rt_lib()
    assert L.rt_denoise(a.ctx, 2, None) == host_api.RT_E_STATE
    assert L.rt_reproject(a.ctx, None, None) == host_api.RT_E_STATE
    assert sp.same(a.accumulator(), acc) and all(sp.same(x, y) for x, y in zip(a.stats(), stats)), "accumulator and statistics are not touched"
    lst, n_act = a.active()
    assert n_act == 3 and lst.tolist() == [3, 5, 700], "an installed list survives"
    a.render_aovs(0.001)
    a.denoise(2)  # current again
    assert L.rt_reproject(a.ctx, None, None) == host_api.RT_E_STATE, "the history stays invalid until a new capture"
    a.history_capture()
    assert a.reproject() >= 0
    # a dense path batch after the move equals a freshly uploaded context's: a stale primary-hit table would show here
    b = host_api.HostRenderer(w, h)
    b.upload_desc(m.desc(a.download_tlas()))
    for r in (a, b):
        r.stats_enable(False)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, 16)
    assert sp.same(a.accumulator(), b.accumulator())
    assert not sp.same(a.accumulator(), acc), "the move is visible"
    a.close(), b.close()


# ---- 6. errors and atomicity -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(scenes, host_api, monkeypatch):
    _env(monkeypatch)
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    L = host_api.rt_lib()
    r = _renderer(host_api, scenes, "tlas_test2")
    m = Mirror(host_api, r.scene)
    assert r.set_instances(1, m.move(1, [r.scene.trs((2, 0.5, 3), 3, 0.0, 1.0, 0.0)])) == 0  # (a moved scene, so that "as before" is not "as uploaded")
    before = {a: r.scene_array(a) for a in ARRAYS}
    tl = r.download_tlas()
    O, D = random_rays(512, 5, center=(0.0, 0.8, 3.0))
    hits = r.find_nearest(O, D)
    r.render_aovs(0.001)
    rec, b6 = m.rec.copy(), m.bounds.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def spoiled(field, k, j, v):
        x = rec.copy()
        x[field][k, j] = v
        return x

    bad_blas = rec.copy()
    bad_blas["blas"][1] = 1
    nanb, bigb = b6.copy(), b6.copy()
    nanb[2, 4], bigb[0, 0] = np.nan, -2e30
    huge = spoiled("transform", 0, 3, 3e38)  # finite, but it takes the BLAS's box beyond 1e30: refused where the device would compute the box
    cases = [("null instances", lambda: L.rt_set_instances(r.ctx, 0, 3, None, None)),
             ("null context", lambda: L.rt_set_instances(None, 0, 3, p(rec), None)),
             ("count 0", lambda: L.rt_set_instances(r.ctx, 0, 0, p(rec), None)),
             ("first outside", lambda: L.rt_set_instances(r.ctx, 3, 1, p(rec), None)),
             ("range outside", lambda: L.rt_set_instances(r.ctx, 1, 3, p(rec), None)),
             ("range wraps", lambda: L.rt_set_instances(r.ctx, 2, 0xFFFFFFFF, p(rec), None)),
             ("blas mismatch", lambda: L.rt_set_instances(r.ctx, 0, 3, p(bad_blas), None)),
             ("nan matrix", lambda: L.rt_set_instances(r.ctx, 0, 3, p(spoiled("transform", 1, 5, np.nan)), p(b6))),
             ("inf inverse", lambda: L.rt_set_instances(r.ctx, 0, 3, p(spoiled("inv_transform", 2, 0, np.inf)), None)),
             ("nan bound", lambda: L.rt_set_instances(r.ctx, 0, 3, p(rec), p(nanb))),
             ("bound beyond 1e30", lambda: L.rt_set_instances(r.ctx, 0, 3, p(rec), p(bigb))),
             ("box beyond 1e30", lambda: L.rt_set_instances(r.ctx, 0, 3, p(huge), None))]
    for what, call in cases:
        assert call() == ARG, what
    # the degenerate build: finite boxes within 1e30 whose every union area reaches FindBestMatch's 1e30 (tlas.cpp:52): k_build_tlas finds no
    # pair to merge and reports it (rt_build.h), the call returns RT_E_UNSUPPORTED after its read-back and commits nothing
    wide = np.tile(np.array([-1e16, -1e16, -1e16, 1e16, 1e16, 1e16], dtype=f32), (3, 1))
    assert L.rt_set_instances(r.ctx, 0, 3, p(rec), p(wide)) == UNSUP
    assert b"no finite union area" in L.rt_last_error(r.ctx)
    for a in ARRAYS:
        assert sp.same(r.scene_array(a), before[a]), a
    assert np.array_equal(r.download_tlas(), tl)
    after = r.find_nearest(O, D)
    assert all(sp.same(hits[k], after[k]) for k in hits)
    assert L.rt_denoise(r.ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    # rt_scene_array's own refusals
    nbytes = C.c_size_t(0)
    assert L.rt_scene_array(r.ctx, 1, None, 0, C.byref(nbytes)) == UNSUP  # RT_LAYOUT_PRIMS
    assert L.rt_scene_array(r.ctx, 0, p(np.zeros(4, f32)), 16, C.byref(nbytes)) == ARG and nbytes.value == before["pairs"].nbytes
    assert L.rt_scene_array(r.ctx, 0, None, 0, None) == ARG
    # rt_set_time stays unsupported under a TLAS
    assert L.rt_set_time(r.ctx, C.c_float(0.5)) == UNSUP
    r.close()
    # no TLAS: RT_E_UNSUPPORTED, the scene untouched; no scene: RT_E_STATE
    g = host_api.HostRenderer(16, 8)
    used = C.c_uint32(0)
    assert L.rt_set_instances(g.ctx, 0, 1, p(rec), None) == STATE and L.rt_download_tlas(g.ctx, p(np.zeros((7, 8), np.uint32)), C.byref(used)) == STATE
    assert L.rt_scene_array(g.ctx, 0, None, 0, C.byref(nbytes)) == STATE
    scenes.mixed_small(g.scene)
    g.commit()
    before = {a: g.scene_array(a) for a in ARRAYS}
    assert len(before["reach"]) == 0 and len(before["inst"]) == 0 and sp.same(before["pairs"], host_api.layout(g.scene.describe())["pairs"])
    assert L.rt_set_instances(g.ctx, 0, 1, p(rec), None) == UNSUP
    assert L.rt_download_tlas(g.ctx, p(np.zeros((7, 8), np.uint32)), C.byref(used)) == UNSUP
    for a in ARRAYS:
        assert sp.same(g.scene_array(a), before[a]), a
    with pytest.raises(RuntimeError, match="no TLAS"):
        g.scene.commit_instances()
    g.close()


def test_profiling_counts_one_query(scenes, host_api, monkeypatch):
    _env(monkeypatch)
    r = _renderer(host_api, scenes, "triangles", 17)
    m = Mirror(host_api, r.scene)
    r.set_profiling(True)
    r.profile()
    assert r.set_instances(0, m.move(0, ir.grid_transforms(r.scene, 17, turn=0.5))) == 0
    prof = r.profile()
    assert prof["query"]["launches"] == 1 and prof["query"]["ms"] > 0 and all(prof[k]["launches"] == 0 for k in ("generate", "extend", "shade", "connect"))
    r.set_profiling(False)
    _check_layout(host_api, r, m, (-1, 0, 1), "profiled")
    r.close()


# ---- 7. several contexts ---------------------------------------------------------------------------------------------------------------
def test_commit_instances_reaches_every_context(scenes, host_api, monkeypatch):
    knobs = _env(monkeypatch)
    frames = []
    for devs in (None, [0, 0]):
        r = host_api.HostRenderer(32, 17, devices=devs)
        scenes.tlas_test2(r.scene)
        r.commit()  # Scene::Commit to context 0, CommitAlso to the second one
        s = r.scene
        s.set_transforms(1, [s.trs((1.5, 0.3, 3.5), 3, 0.0, 0.8, 0.0), s.trs((-2.0, 0, 2.5), 4, 0.0, 2.0, 0.0)])
        s.commit_instances()
        L = host_api.layout(s.describe(), *knobs)
        for k in range(2 if devs else 1):
            ctx = r.ctx_at(k)
            assert ctx.value and (k == 0) == (ctx.value == r.ctx.value)
            for a in ARRAYS:
                assert sp.same(r.scene_array(a, ctx), L[a]), (k, a)
        r.tick()  # a Whitted Tick; with two contexts the rows are interleaved over them
        frames.append(r.tick_accumulator().copy())
        r.close()
    assert sp.same(frames[0], frames[1]) and (frames[0][..., :3] > 0).any()


# ---- the example's --spin ---------------------------------------------------------------------------------------------------------------
def test_example_spin(tmp_path, scenes, host_api, monkeypatch):
    """examples/render_scene.cpp --spin DEG: instance 0 turned about y with SetTransform + Scene::CommitInstances before the last Tick.  The
    Whitted image is the one a renderer shows whose scene was moved the same way; the path run ends on the moved scene too."""
    import os
    import subprocess
    from conftest import ROOT, pkg
    _env(monkeypatch)
    sf = pkg("scene_file")
    exe = str(tmp_path / "render_scene")
    host, csrc = os.path.join(ROOT, "ray-and-pathtracer_amd", "host"), os.path.join(ROOT, "ray-and-pathtracer_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "render_scene.cpp"), "-I" + host, "-L" + host, "-lrapt_host",
                           "-L" + csrc, "-lrt_amd", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc, "-o", exe])
    scene_path = str(tmp_path / "tlas.rapt")
    scenes.tlas_test2(sf.SceneWriter(scene_path))

    def run(mode, frames, *more):
        out = str(tmp_path / "out.ppm")
        subprocess.check_call([exe, scene_path, out, "48", "32", mode, str(frames)] + list(more))
        raw = open(out, "rb").read()
        return np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(32, 48, 3).astype(np.uint32)

    still, spun = run("whitted", 1), run("whitted", 1, "--spin", "40")
    r = host_api.HostRenderer(48, 32)
    r.scene.load_file(scene_path)
    r.commit()
    s = r.scene
    ang = f32(f32(f32(40.0) * f32(3.14159265358979)) / f32(180.0))
    s.set_transforms(0, [ir.mat_mul(s.instance_dump(0)["T"], s.trs((0, 0, 0), 1, 0.0, ang, 0.0))])
    s.commit_instances()
    r.tick()
    px = r.tick_pixels()
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1)
    assert np.array_equal(spun, want) and not np.array_equal(spun, still)
    r.close()
    assert not np.array_equal(run("path", 3, "--spin", "40"), run("path", 3))
