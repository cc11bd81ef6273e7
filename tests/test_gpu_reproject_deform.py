"""rt_reproject_deform on the device, through host_api: the primitive index of the G-buffer, k_reproject_deform against its numpy restatement
(tests/reproject_deform_ref.py) bit for bit, its equality with rt_reproject_motion and rt_reproject where nothing is deformed, idempotence and
what the call leaves alone, the third level of a history's validity, rt_set_triangles unchanged by a live history,
Renderer::CommitTriangles against the same sequence driven by hand, and what the carried samples are worth across a deformation."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_ref as rr  # noqa: E402
import reproject_motion_ref as rm  # noqa: E402
import reproject_deform_ref as rd  # noqa: E402
import reproject_motion_shapes as ms  # noqa: E402
import reproject_deform_shapes as shapes  # noqa: E402
import support as sp  # noqa: E402
import triangles_desc as td  # noqa: E402
import triangles_ref as tr  # noqa: E402
from test_gpu_denoise import Recorder  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x12345678
ADAPTIVE, MOVES, PARAMS = rr.ADAPTIVE, rr.MOVES, rr.PARAMS
NO_TLAS = shapes.NO_TLAS


def _renderer(host_api, monkeypatch, n, w, h, camera="scene's", scene=None, devices=None):
    camera = (shapes.camera(n) if scene is None else shapes.CAMERA) if isinstance(camera, str) else camera
    return sp.renderer(host_api, monkeypatch, scene or (lambda b: shapes.build_scene(b, n)), w, h, scene_camera=False, camera=camera, devices=devices)


def _base(r, n):
    dumps = [r.scene.instance_dump(i) for i in range(n)]
    return [int(d["blas"]) for d in dumps], [np.asarray(d["T"], F32).reshape(16) for d in dumps]


def _v9(d, n):
    return tr.v9_of(d.tris[shapes.target(n)["blas"]])


# ---- 1. the primitive index of the G-buffer ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 9), (64, 40)], ids=lambda s: "%dx%d" % s)
def test_prim_aov(size, scenes, host_api, oracle_api, monkeypatch):
    """pretty_tlas with 3 instances (spheres and a plane tested by brute force, two lights in view) and mixed_small (no TLAS: spheres and the
    floor in the scene BVH's leaves).  prim is -1 exactly where the hit is a miss, a light or a brute-force primitive; elsewhere the record
    at that slot of the context's RT_LAYOUT_PRIMS array carries the pixel's object and material and the pixel's point lies on its surface
    (in the instance's space under a TLAS); the other G-buffer arrays hold what they held before the array was added (the oracle's bits,
    by the checks of tests/test_gpu_reproject_motion.py test_instance_aov, which this test repeats through that file's helper)."""
    from test_gpu_reproject_motion import _gbuffer as gbuffer_before
    from test_gpu_denoise import check_aovs
    w, h = size
    for tlas, build, brute in ((True, lambda s: scenes.pretty_tlas(s, n_instances=3), {1, 6, 7, 8, 9}), (False, scenes.mixed_small, set())):
        recs = []
        r = _renderer(host_api, monkeypatch, 3, w, h, scene=lambda s: (recs.append(Recorder(s)), build(recs[-1]))[1])
        buf = np.zeros((h, w), np.int32).ctypes.data_as(C.c_void_p)
        assert r.rt.rt_download_aov_prims(r.ctx, 0, h, buf) == host_api.RT_E_STATE  # no G-buffer yet
        r.render_aovs(0.001)
        g = shapes.gbuffer(r)
        d = td.Desc(host_api, r.scene)
        P = shapes.prims(r, len(d.blas))
        prim, obj, inst = g["prim"], g["obj"], g["inst"]
        assert prim.dtype == np.int32 and prim.min() >= -1 and prim.max() < len(P)
        none = (obj == -1) | ((obj >= 11) & (obj <= 12)) | np.isin(obj, sorted(brute))
        assert np.array_equal(prim == -1, none) and (prim >= 0).any() and (none.any() or not tlas)
        if tlas:
            assert np.array_equal(prim >= 0, inst >= 0) and (obj[none] >= 11).any() and np.isin(obj[none], sorted(brute)).any()
        on = prim >= 0
        rec = P[prim[on]]
        assert np.array_equal(rec[:, 13].view(np.int32), obj[on]) and np.array_equal(rec[:, 14].view(np.int32), g["mat"][on])
        # the point on the record's surface, in f64: a triangle's and a plane's N . x + d = 0, a sphere's |x - c|^2 = r2
        x = g["pos"][on].astype(np.float64)
        if tlas:
            xf = ms.tables(r)
            M = xf["invT"][inst[on]].astype(np.float64).reshape(-1, 3, 4)
            x = np.einsum("nij,nj->ni", M[:, :, :3], x) + M[:, :, 3]
        kind = rec[:, 15].view(np.int32) & 3
        R = rec.astype(np.float64)
        tri, sph, pla = kind == 0, kind == 1, kind == 2
        size_of = np.maximum(1.0, np.abs(x).max(-1))
        assert tri.any() and np.all(np.abs((R[tri][:, [3, 7, 11]] * x[tri]).sum(-1) + R[tri, 12]) <= 1e-4 * size_of[tri])
        assert np.all(np.abs(((x[sph] - R[sph, :3]) ** 2).sum(-1) - R[sph, 3]) <= 1e-4 * np.maximum(1.0, R[sph, 3]))
        assert np.all(np.abs((R[pla, :3] * x[pla]).sum(-1) + R[pla, 3]) <= 1e-4 * size_of[pla])
        assert tlas or sph.any() or pla.any()  # (the scene BVH's leaves hold spheres and the floor as well)
        # rows, and the row download's refusals (rt_download_aov_instances')
        assert np.array_equal(r.aov_prims(2, 7), prim[2:7])
        for y0, y1 in ((-1, h), (0, h + 1), (3, 3)):
            assert r.rt.rt_download_aov_prims(r.ctx, y0, y1, buf) == host_api.RT_E_ARG
        assert r.rt.rt_download_aov_prims(r.ctx, 0, h, None) == host_api.RT_E_ARG and r.rt.rt_download_aov_prims(None, 0, h, buf) == host_api.RT_E_ARG
        # the older arrays: the oracle's bits
        o = oracle_api.OracleScene()
        build(o)
        orr = oracle_api.OracleRenderer(o, w, h)
        orr.set_camera(*shapes.CAMERA)
        got = check_aovs(o, orr, r, recs[-1], 0.001)
        want = rr.gbuffer_of(o, orr)
        hitp = want["obj"] != -1
        assert hitp.any() and (got["albedo"][hitp] != 0).any() and sp.same(r.aov_positions()[hitp], want["pos"][hitp])
        orr.close(), o.close()
        after = gbuffer_before(r)
        assert all(sp.same(g[k], v) for k, v in after.items()) and sp.same(r.aov_prims(), prim)
        r.close()


# ---- 2. the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", shapes.COUNTS + (NO_TLAS,), ids=lambda n: "%d_instances" % n if n else "no_tlas")
@pytest.mark.parametrize("size", [(33, 9), (97, 41), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement(size, n, host_api, monkeypatch):
    """Every deformation x camera x history x parameter set of one frame size and scene on one context: accumulator, count, both sums and
    n_carried bit for bit against the restatement, which is fed the device's own downloads (the G-buffers, instance records and primitive
    records of both moments).  So that no case is vacuous: under the default parameters every real deformation carries at least one pixel
    that went through the barycentric path (one is what it takes to run it), and at 97 x 41 the restatement carries >= 10 % of the frame
    and rejects >= 1 % of the eligible pixels.  The bars are conditions; they are not applied where they cannot hold by construction:
    there_and_back deforms nothing in the end, the zero tolerances ('exact') reject nearly every resampled pixel, a frame of one pixel
    has no percentages (tests/test_reproject_deform_cpu.py shows on G-buffers made on the CPU that the amplitudes meet them).  In the
    half-deformed case the pixels of untouched triangles have rt_reproject_motion's source."""
    w, h = size
    A = shapes.camera(n) if size != (1, 1) or n == NO_TLAS else ms.one_pixel_camera(n)
    r = _renderer(host_api, monkeypatch, n, w, h, A)
    mt, mats = rr.materials(r)
    blas, base = _base(r, n)
    d = td.Desc(host_api, r.scene)
    nb = len(d.blas)
    r.stats_enable(True)
    for kind in ("uniform", "adaptive"):
        shapes.restore(host_api, r, d, n, blas, base)
        r.set_camera(*A)
        rr.make_history(r, host_api, kind, w, h)
        r.render_aovs(0.001)
        g_a, hist, xf_a, prims_a = shapes.gbuffer(r), sp.state(r), ms.tables(r), shapes.prims(r, nb)
        r.history_capture()
        for dname, steps in shapes.deformations(_v9(d, n), n, base).items():
            shapes.restore(host_api, r, d, n, blas, base)
            shapes.send(host_api, r, d, n, steps, blas)
            xf_b, prims_b = ms.tables(r), shapes.prims(r, nb)
            real = dname != "there_and_back"
            assert rd.deformed_slots(prims_b, prims_a).any() == real, dname
            for cname in ("none", "small"):
                r.set_camera(*rr.moved(A, MOVES[cname]))
                r.render_aovs(0.001)
                g_b = shapes.gbuffer(r)
                for pname, P in PARAMS.items():
                    got_n = r.reproject_deform(P)
                    got = sp.state(r)
                    acc, cnt, sy, syy, n_ref, src, el, through = rd.reproject(g_b, g_a, *hist, A, xf_b, xf_a, prims_b, prims_a, mt, mats, **P)
                    what = (kind, dname, cname, pname)
                    print(what, "carried %d of %d, eligible %d, through bu bv %d" % (n_ref, w * h, el.sum(), ((src >= 0) & through).sum()))
                    assert got_n == n_ref, what
                    assert np.array_equal(got[1], cnt), what
                    assert sp.same(got[0], acc) and sp.same(got[2], sy) and sp.same(got[3], syy), what
                    if size == (97, 41) and pname != "exact" and real:
                        carried, rejected = n_ref / (w * h), (el.sum() - n_ref) / max(1, el.sum())
                        assert carried >= 0.10 and rejected >= 0.01, (what, carried, rejected)
                    if pname == "defaults" and w * h > 1 and real:
                        assert ((src >= 0) & through).sum() >= 1, (what, "no pixel of a deformed triangle is carried")
                    if dname == "half":
                        plain = rm.source(g_b, g_a, hist[1], A, xf_b, xf_a, mt, mats, **P)[0]
                        assert ((~through).any() or w * h == 1) and np.array_equal(src[~through], plain[~through]), what
                    if not real:
                        assert not through.any(), what
    r.close()


# ---- 3. nothing deformed: rt_reproject_motion's result, and rt_reproject's -----------------------------------------------------------
@pytest.mark.parametrize("n", [3, NO_TLAS], ids=["tlas", "no_tlas"])
def test_undeformed_equals_the_siblings(n, host_api, monkeypatch):
    w, h = 97, 41
    trio = [_renderer(host_api, monkeypatch, n, w, h) for _ in range(3)]
    for r in trio:
        r.stats_enable(True)
        rr.make_history(r, host_api, "adaptive", w, h)
        r.render_aovs(0.001)
        r.history_capture()
        r.set_camera(*rr.moved(shapes.camera(n), MOVES["small"]))
        r.render_aovs(0.001)
    assert (trio[0].aov_instances() >= 0).any() == (n != NO_TLAS) and (trio[0].aov_prims() >= 0).any()
    for pname, P in PARAMS.items():
        a, b, c = trio[0].reproject(P), trio[1].reproject_motion(P), trio[2].reproject_deform(P)
        assert a == b == c > 0 and sp.same_state(sp.state(trio[0]), sp.state(trio[2])) and sp.same_state(sp.state(trio[1]), sp.state(trio[2])), pname
    # an instance move (under a TLAS) and a deformation taken back to the same bits: rt_reproject_motion's result, which needs a context the
    # deformation never reached (for that call it ends the history)
    motion, deform = trio[1], trio[2]
    d = td.Desc(host_api, deform.scene)
    blas, base = _base(deform, n)
    steps = shapes.deformations(_v9(d, n), n, base)["there_and_back"]
    shapes.send(host_api, deform, d, n, steps, blas)
    if n != NO_TLAS:
        for r in (motion, deform):
            shapes.send(host_api, r, d, n, [("move", 0, [ms.translated(base[0], (0.4, 0.0, 0.1))])], blas)
    for r in (motion, deform):
        r.render_aovs(0.001)
    for pname, P in PARAMS.items():
        b, c = motion.reproject_motion(P), deform.reproject_deform(P)
        assert b == c > 0 and sp.same_state(sp.state(motion), sp.state(deform)), pname
    for r in trio:
        r.close()


# ---- 4. idempotence, and what the call leaves alone --------------------------------------------------------------------------------
def test_twice_and_untouched_state(host_api, monkeypatch):
    w, h, n = 97, 41, 3
    r = _renderer(host_api, monkeypatch, n, w, h)
    blas, base = _base(r, n)
    d = td.Desc(host_api, r.scene)
    r.stats_enable(True)
    rr.make_history(r, host_api, "adaptive", w, h)
    r.render_aovs(0.001)
    r.history_capture()
    shapes.send(host_api, r, d, n, shapes.deformations(_v9(d, n), n, base)["with_move"], blas)
    r.set_camera(*rr.moved(shapes.CAMERA, MOVES["small"]))
    r.render_aovs(0.001)
    g_b = shapes.gbuffer(r)
    lst = np.flatnonzero(np.random.default_rng(9).random(w * h) < 0.6).astype(np.uint32)
    r.set_active(lst)
    n1 = r.reproject_deform()
    first = sp.state(r)
    assert r.reproject_deform() == n1 > 0 and sp.same_state(first, sp.state(r))
    # the history is the capture's, whatever has happened to the accumulator since; NULL parameters are the defaults, a NULL count is allowed
    r.clear()
    assert r.reproject_deform(dict(host_api.REPROJECT_DEFAULTS)) == n1 and sp.same_state(first, sp.state(r))
    r.render(host_api.RT_MODE_PATH, 50, 2)
    assert r.rt.rt_reproject_deform(r.ctx, None, None) == 0 and sp.same_state(first, sp.state(r))
    # the active-pixel list and the G-buffer, the primitive indices included, are not touched
    got, k = r.active()
    assert k == len(lst) and np.array_equal(got, lst)
    after = shapes.gbuffer(r)
    assert all(sp.same(g_b[key], after[key]) for key in g_b)
    # a budget plan is dropped: every pixel's count was rewritten
    assert r.select_budget(dict(select=ADAPTIVE, pass_cap=4))[0] > 0
    r.reproject_deform()
    assert r.rt.rt_render_budget(r.ctx, 0, SEED, 4) == host_api.RT_E_STATE
    # with profiling on, the kernel is one launch of rt_profile.query
    r.set_profiling(True)
    r.profile()
    r.reproject_deform()
    assert r.profile()["query"]["launches"] == 1
    r.close()


# ---- 5. the third level of validity, and the errors ------------------------------------------------------------------------------------
def test_states_and_errors(host_api, monkeypatch):
    w, h, n = 64, 40, 3
    r = _renderer(host_api, monkeypatch, n, w, h)
    L, ctx = r.rt, r.ctx
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    blas, base = _base(r, n)
    d = td.Desc(host_api, r.scene)
    deforms = shapes.deformations(_v9(d, n), n, base)
    cnt = C.c_int(-7)

    def rep(fn, context=ctx, **kw):
        p = host_api.reproject_params(kw)
        return fn(context, C.byref(p), C.byref(cnt))

    def why():
        return L.rt_last_error(ctx).decode()

    # parameters: refused before the context is looked at
    for bad in (dict(normal_tolerance=-0.1), dict(normal_tolerance=float("nan")), dict(plane_tolerance=-1e-9), dict(plane_tolerance=float("nan")), dict(max_history=-1)):
        assert rep(L.rt_reproject_deform, **bad) == ARG and rep(L.rt_reproject_deform, None, **bad) == ARG, bad
    assert rep(L.rt_reproject_deform, None) == ARG
    # statistics off; no history yet; a stale G-buffer
    r.render_aovs(0.001)
    assert rep(L.rt_reproject_deform) == STATE and "statistics" in why()
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 3)
    assert rep(L.rt_reproject_deform) == STATE and "history" in why()

    def recapture():
        shapes.restore(host_api, r, d, n, blas, base)
        r.set_camera(*shapes.CAMERA)
        r.render_aovs(0.001)
        r.history_capture()
        assert rep(L.rt_reproject) == 0 and rep(L.rt_reproject_motion) == 0 and rep(L.rt_reproject_deform) == 0

    recapture()
    # a deformation: the G-buffer is stale for all three; with a new one the siblings have no valid history, rt_reproject_deform carries
    shapes.send(host_api, r, d, n, deforms["all"], blas)
    assert rep(L.rt_reproject_deform) == STATE and "G-buffer" in why()
    r.render_aovs(0.001)
    assert rep(L.rt_reproject) == STATE and "history" in why()
    assert rep(L.rt_reproject_motion) == STATE and "history" in why()
    assert rep(L.rt_reproject_deform) == 0 and cnt.value > 0
    # ... across any number of deformations and moves, in any order, and a camera move as well
    shapes.send(host_api, r, d, n, deforms["with_move"] + deforms["two_calls"] + deforms["with_move"][1:], blas)
    r.set_camera(*rr.moved(shapes.CAMERA, MOVES["small"]))
    r.render_aovs(0.001)
    assert rep(L.rt_reproject) == STATE and rep(L.rt_reproject_motion) == STATE and rep(L.rt_reproject_deform) == 0 and cnt.value > 0
    # a new capture after a deformation makes the deformed records the reference: an immediate carry is rt_reproject_motion's, bit for bit
    r.history_capture()
    assert rep(L.rt_reproject_motion) == 0
    want = cnt.value, sp.state(r)
    assert rep(L.rt_reproject_deform) == 0 and cnt.value == want[0] > 0 and sp.same_state(sp.state(r), want[1])
    # failed rt_set_triangles calls leave the history valid (for all three, when nothing else happened) and the carry the undeformed one:
    # the RT_E_ARG cases, refused before anything is queued ...
    recapture()
    undeformed = cnt.value, sp.state(r)  # (the last of recapture's three carries is rt_reproject_deform's)
    t = np.ascontiguousarray(d.tris[0])
    p = t.ctypes.data_as(C.c_void_p)
    nan = t.copy()
    nan["v1"][3, 2] = np.nan
    for what, call in (("null triangles", lambda: L.rt_set_triangles(ctx, 0, None, len(t))), ("blas outside", lambda: L.rt_set_triangles(ctx, len(d.blas), p, len(t))),
                       ("one triangle short", lambda: L.rt_set_triangles(ctx, 0, p, len(t) - 1)), ("nan vertex", lambda: L.rt_set_triangles(ctx, 0, nan.ctypes.data_as(C.c_void_p), len(t)))):
        assert call() == ARG, what
        assert rep(L.rt_reproject) == 0 and rep(L.rt_reproject_motion) == 0, what
        assert rep(L.rt_reproject_deform) == 0 and cnt.value == undeformed[0] and sp.same_state(sp.state(r), undeformed[1]), what
    # ... and the atomic TLAS failure of tests/test_gpu_triangles.py: the records have been rewritten (after the copy on first write) by the
    # time the build fails, and are put back: the kept copy equals them
    huge = tr.triangles(d.tris[0], tr.scale(_v9(d, n), 1e16))
    assert L.rt_set_triangles(ctx, 0, huge.ctypes.data_as(C.c_void_p), len(huge)) == UNSUP and "no finite union area" in why()
    assert L.rt_denoise(ctx, 1, None) == 0, "a refused call invalidates nothing: the G-buffer is still current"
    assert rep(L.rt_reproject) == 0 and rep(L.rt_reproject_motion) == 0
    assert rep(L.rt_reproject_deform) == 0 and cnt.value == undeformed[0] and sp.same_state(sp.state(r), undeformed[1])
    # a fisheye camera
    r.set_camera(*shapes.CAMERA, fisheye=True)
    r.render_aovs(0.001)
    assert rep(L.rt_reproject_deform) == UNSUP
    # an upload, and the statistics switched off, end the history at every level
    for drop in (r.commit, lambda: (r.stats_enable(False), r.stats_enable(True))):
        recapture()
        shapes.send(host_api, r, d, n, deforms["all"], blas)
        drop()
        r.render_aovs(0.001)
        assert rep(L.rt_reproject_deform) == STATE and "history" in why()
        assert rep(L.rt_reproject) == STATE and rep(L.rt_reproject_motion) == STATE
    r.close()
    # rt_set_time: no error either (a scene without a TLAS), while the siblings refuse
    r = _renderer(host_api, monkeypatch, NO_TLAS, w, h)
    ctx = r.ctx
    d = td.Desc(host_api, r.scene)
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 3)
    r.render_aovs(0.001)
    r.history_capture()
    for t_ in (0.4, shapes.TIME):
        r.set_time(t_)
        shapes.send(host_api, r, d, NO_TLAS, shapes.deformations(_v9(d, NO_TLAS), NO_TLAS)["two_calls"])
    r.set_time(0.9)
    r.render_aovs(0.001)
    assert rep(L.rt_reproject, ctx) == STATE and rep(L.rt_reproject_motion, ctx) == STATE and rep(L.rt_reproject_deform, ctx) == 0 and cnt.value > 0
    r.close()


# ---- 6. rt_set_triangles is unchanged by a live history ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, NO_TLAS], ids=["tlas", "no_tlas"])
def test_set_triangles_is_unchanged_by_a_live_history(n, host_api, monkeypatch):
    """two contexts of one scene, one with a captured history: after the same calls (two rt_set_triangles; without a TLAS an rt_set_time too)
    rt_blas_array PAIRS and PRIMS of every BLAS and every rt_scene_array are the same bytes"""
    w, h = 33, 9
    live, plain = (_renderer(host_api, monkeypatch, n, w, h) for _ in range(2))
    live.stats_enable(True)
    live.render(host_api.RT_MODE_PATH, 0, 2)
    live.render_aovs(0.001)
    live.history_capture()
    d = td.Desc(host_api, live.scene)
    blas, base = _base(live, n)
    deforms = shapes.deformations(_v9(d, n), n, base)
    steps = deforms["two_calls"] + (deforms["time"] + deforms["all"] if n == NO_TLAS else deforms["with_move"])
    for upto in range(1, len(steps) + 1):
        for r in (live, plain):
            shapes.send(host_api, r, d, n, steps[upto - 1:upto], blas)
        for k in range(len(d.blas)):
            for a in ("pairs", "prims"):
                assert sp.same(live.blas_array(k, a), plain.blas_array(k, a)), (upto, k, a)
        for a in ("pairs", "reach", "inst", "scalars"):
            assert sp.same(live.scene_array(a), plain.scene_array(a)), (upto, a)
    live.render_aovs(0.001)
    assert live.reproject_deform() > 0  # (and the history was live throughout)
    live.close(), plain.close()


# ---- 7. Renderer::CommitTriangles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one_context", "two_contexts"])
def test_renderer_commit_triangles_equals_the_sequence_by_hand(devices, host_api, monkeypatch):
    w, h, n = 64, 40, 3
    RP = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=16, carry_view_dependent=0)
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, monkeypatch, n, w, h, devices=devices)
    off, hand, plain = (_renderer(host_api, monkeypatch, n, w, h) for _ in range(3))
    r.set_adaptive(True, ADAPTIVE), r.set_reproject(True, RP)
    off.set_adaptive(True, ADAPTIVE)  # reproject off: CommitTriangles is Scene::CommitTriangles and a clear
    _, base = _base(r, n)
    d = td.Desc(host_api, r.scene)
    v9 = _v9(d, n)
    for x in (hand, plain):
        x.stats_enable(True)
        x.clear()
    whole = {id(hand): 0, id(plain): 0}

    def step(x, t):
        if whole[id(x)] < ADAPTIVE["min_samples"]:
            x.render(PATH, t, 1)
            whole[id(x)] += 1
            return w * h
        k = x.select_active(ADAPTIVE)
        x.render_active(t, 1)
        return k

    # a deformation alone; an instance move and a deformation with a camera move in the same Tick; one before min_samples whole frames
    changes = {6: (shapes.small(v9), None, None), 8: (shapes.small(v9, 0.9), (0, [ms.translated(base[0], (0.3, 0.0, 0.1))]), MOVES["small"]), 9: (v9, None, None)}
    cam = shapes.CAMERA
    for t in range(12):
        if t in changes:
            verts, move, cmove = changes[t]
            for x in (r, off, hand, plain):
                x.scene.set_mesh_vertices(0, verts)
                if move:
                    x.scene.set_transforms(move[0], [T.reshape(4, 4) for T in move[1]])
            if move:
                r.commit_instances(), off.commit_instances()
            r.commit_triangles(0), off.commit_triangles(0)
            hand.render_aovs(0.001)
            hand.history_capture()
            for x in (hand, plain):
                if move:
                    x.scene.commit_instances()
                x.scene.commit_triangles(0)
            plain.clear()
            whole[id(plain)] = 0
            if cmove is not None:
                cam = rr.moved(cam, cmove)
                for x in (r, off, hand, plain):
                    x.set_camera(*cam)
            hand.render_aovs(0.001)
            carried = hand.reproject_deform(RP)
            whole[id(hand)] = ADAPTIVE["min_samples"]
        r.tick()
        off.tick()
        k, m = step(hand, t), step(plain, t)
        assert r.active_pixels() == k and off.active_pixels() == m, t
        if t in changes:
            assert r.carried_pixels() == carried > 0, t
            assert np.all(off.stats()[0] == 1), t
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
        assert sp.same(off.tick_accumulator(), plain.accumulator()) and sp.same_state(sp.state(off), sp.state(plain)), t
    # a Commit() between CommitTriangles and the Tick: the upload ended the captured history, so the Tick clears (and does not throw)
    r.scene.set_mesh_vertices(0, shapes.small(v9))
    r.commit_triangles(0)
    r.commit()
    r.tick()
    assert np.all(r.stats()[0] == 1) and r.active_pixels() == w * h
    for x in (r, off, hand, plain):
        x.close()


# ---- 8. what the carry is worth --------------------------------------------------------------------------------------------------------
def test_carried_samples_beat_fresh_ones_across_a_deformation(host_api, monkeypatch):
    """One measurement (tests/reproject_deform_shapes.py quality): 32 samples per pixel, the 'three' mesh shrunk by a tenth through
    rt_set_triangles, the samples carried and 4 added, against clear + 4, on the carried pixels of the mesh and of the floor away from its
    shadow.  Asserted: pixels of the deformed mesh are carried, the safe pixels are at least a tenth of the frame, and the carried frame's
    MSE there is the lower one (an unbiased carry would give about 4 / 36).  The measured ratio and the shadow zone's figures are
    reported, not asserted.  Measured on an MI355X: ratio 0.279 on 1084 pixels (230 of the mesh), 0.447 on the 30 carried floor pixels
    of the shadow zone (profiles/reproject_deform_quality.json)."""
    q = shapes.QUALITY
    r = _renderer(host_api, monkeypatch, 1, q["width"], q["height"], camera=None, scene=ms.quality_scene)
    r.stats_enable(True)
    with np.errstate(all="ignore"):
        out = shapes.quality(host_api, r)
    r.close()
    print("carry across a deformation:", json.dumps(out))
    assert out["deformed_mesh_pixels_carried"] > 0 and out["safe_pixels"] >= 0.1 * q["width"] * q["height"]
    assert out["mse_carried"] < out["mse_fresh"], out
