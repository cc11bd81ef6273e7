"""rt_reproject_motion on the device, through host_api: the instance index of the G-buffer, k_reproject_motion against its numpy restatement
(tests/reproject_motion_ref.py) bit for bit, its equality with rt_reproject where nothing moved, idempotence and what the call leaves alone,
the two levels of a history's validity, Renderer::CommitInstances against the same sequence driven by hand, the example's --carry, and what the carried samples
are worth across an instance move."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import instances_ref as ir  # noqa: E402
import reproject_ref as rr  # noqa: E402
import reproject_motion_ref as rm  # noqa: E402
import reproject_motion_shapes as shapes  # noqa: E402
import support as sp  # noqa: E402
from test_gpu_denoise import Recorder, check_aovs  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = 0x12345678
ADAPTIVE, MOVES, PARAMS = rr.ADAPTIVE, rr.MOVES, rr.PARAMS


def _renderer(host_api, monkeypatch, n, w, h, camera=shapes.CAMERA, scene=None):
    return sp.renderer(host_api, monkeypatch, scene or (lambda b: shapes.build(b, n)), w, h, scene_camera=False, camera=camera)


def _gbuffer(r):
    """the current G-buffer as the device holds it, the instance indices included"""
    a = r.aovs()
    return dict(pos=r.aov_positions(), normal=a["normal"], t=a["t"], obj=a["obj"], mat=a["mat"], inst=r.aov_instances())


def _base(host_api, r, n):
    dumps = [r.scene.instance_dump(i) for i in range(n)]
    return [int(d["blas"]) for d in dumps], [np.asarray(d["T"], F32).reshape(16) for d in dumps]


def _apply(host_api, r, blas, base, calls):
    """every instance back at its base transform (the uploaded bits), then the motion's rt_set_instances calls"""
    assert r.set_instances(0, shapes.records(host_api, blas, base)) == 0
    for first, Ts in calls:
        Ts = base[first:first + 1] if Ts is None else Ts
        assert r.set_instances(first, shapes.records(host_api, blas[first:first + len(Ts)], Ts)) == 0


# ---- 1. the instance index of the G-buffer -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 9), (64, 40)], ids=lambda s: "%dx%d" % s)
def test_instance_aov(size, scenes, host_api, oracle_api, monkeypatch):
    """pretty_tlas with 3 instances (scope 3 below is RT_SCOPE_INSTANCE): spheres and a plane tested by brute force and two lights in view.  Every pixel with an index k >= 0
    has, on its own ray, the G-buffer's t from instance k alone (rt_intersect_scope) bit for bit; every pixel with -1 is a miss, a light or
    a brute-force primitive; the three older arrays still hold the oracle's bits; a scene without a TLAS has -1 everywhere."""
    w, h = size
    recs = []

    def recorded(fn, **kw):
        """the scene built through a Recorder (tests/test_gpu_denoise.py), which keeps the material and light colours the albedo is made of"""
        return lambda s: (recs.append(Recorder(s)), fn(recs[-1], **kw))[1]

    r = _renderer(host_api, monkeypatch, 3, w, h, scene=recorded(scenes.pretty_tlas, n_instances=3))
    assert r.rt.rt_download_aov_instances(r.ctx, 0, h, np.zeros((h, w), np.int32).ctypes.data_as(C.c_void_p)) == host_api.RT_E_STATE  # no G-buffer yet
    r.render_aovs(0.001)
    g = _gbuffer(r)
    inst = g["inst"]
    assert inst.dtype == np.int32 and inst.min() >= -1 and inst.max() <= 2 and len(np.unique(inst[inst >= 0])) >= 2
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    O, D = r.sample_rays(0)
    flat = inst.reshape(-1)
    for k in np.unique(flat[flat >= 0]):
        sel = flat == k
        hit = r.scope_nearest(3, int(k), O[sel], D[sel])
        assert sp.same(hit["t"], g["t"].reshape(-1)[sel]), k
        assert np.array_equal(hit["obj"], g["obj"].reshape(-1)[sel]), k
    # the meshes are objects 2 and 3 (their triangles count on from 2000 and 3000); spheres 6 .. 9, the plane 1, lights 11, 12, a miss -1
    mesh = g["obj"] >= 1000
    assert np.array_equal(inst >= 0, mesh)
    rest = g["obj"][inst == -1]
    assert set(np.unique(rest)) <= {-1, 1, 6, 7, 8, 9, 11, 12} and (rest >= 11).any() and np.isin(rest, (1, 6, 7, 8, 9)).any()
    # rows, and the row download's refusals
    assert np.array_equal(r.aov_instances(2, 7), inst[2:7])
    buf = np.zeros((h, w), np.int32).ctypes.data_as(C.c_void_p)
    for y0, y1 in ((-1, h), (0, h + 1), (3, 3)):
        assert r.rt.rt_download_aov_instances(r.ctx, y0, y1, buf) == host_api.RT_E_ARG
    assert r.rt.rt_download_aov_instances(r.ctx, 0, h, None) == host_api.RT_E_ARG and r.rt.rt_download_aov_instances(None, 0, h, buf) == host_api.RT_E_ARG
    def same_as_before(r, build):
        """nrm, pos and alb, every word, are what they were: nrm (normal, t), pos.w (the object) and alb (the albedo, w: the material) against
        the oracle and the recorded colours by tests/test_gpu_denoise.py's own check, pos.xyz against O + D * t of the oracle's hit"""
        o = oracle_api.OracleScene()
        build(o)
        orr = oracle_api.OracleRenderer(o, w, h)
        orr.set_camera(*shapes.CAMERA)
        got = check_aovs(o, orr, r, recs[-1], 0.001)
        want = rr.gbuffer_of(o, orr)
        hitp = want["obj"] != -1
        assert hitp.any() and (got["albedo"][hitp] != 0).any() and sp.same(r.aov_positions()[hitp], want["pos"][hitp])
        orr.close(), o.close()

    same_as_before(r, lambda o: scenes.pretty_tlas(o, 3))
    assert all(sp.same(g[k], v) for k, v in _gbuffer(r).items())  # (and the checks left the G-buffer as it was)
    r.close()
    # a scene without a TLAS
    r = _renderer(host_api, monkeypatch, 0, w, h, scene=recorded(scenes.mixed_small), camera=shapes.CAMERA)
    r.render_aovs(0.001)
    assert np.all(r.aov_instances() == -1) and (r.aovs()["obj"] != -1).any()
    same_as_before(r, scenes.mixed_small)
    r.close()


# ---- 2. the kernel against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", shapes.COUNTS, ids=lambda n: "%d_instances" % n)
@pytest.mark.parametrize("size", [(33, 9), (97, 41), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_kernel_equals_the_restatement(size, n, host_api, monkeypatch):
    """Every motion x camera x history x parameter set of one frame size and instance count on one context: accumulator, count, both sums
    and n_carried bit for bit against the restatement, which is fed the device's own downloads (the G-buffers and instance records of
    both moments).  So that no case is vacuous: in every real motion (translated, rotated, all, two_calls), under either camera, the
    restatement carries >= 10 % of the frame and rejects >= 1 % of the eligible pixels, and under the default parameters it carries at
    least one pixel of an instance that MOVED -- a pixel that went through the transforms, which is the new code; one is the bar because
    one is what it takes to run that path, and the 70-instance frames at 33 x 9 show a moved triangle on a handful of pixels only.  The
    bars are not applied where they cannot hold by construction: there_and_back moves nothing in the end (with the camera unmoved it is
    held to carrying every eligible pixel from itself instead; with the 'small' camera it is rt_reproject's case, whose bars
    tests/test_gpu_reproject.py keeps), the zero tolerances ('exact') reject nearly every resampled pixel, and a frame of one pixel
    has no percentages."""
    w, h = size
    A = shapes.one_pixel_camera(n) if size == (1, 1) else shapes.CAMERA
    r = _renderer(host_api, monkeypatch, n, w, h, A)
    mt, ms = rr.materials(r)
    blas, base = _base(host_api, r, n)
    r.stats_enable(True)
    for kind in ("uniform", "adaptive"):
        _apply(host_api, r, blas, base, [])
        r.set_camera(*A)
        rr.make_history(r, host_api, kind, w, h)
        r.render_aovs(0.001)
        g_a, hist, xf_a = _gbuffer(r), sp.state(r), shapes.tables(r)
        if size == (1, 1):
            assert g_a["inst"][0, 0] == 0, "the one pixel does not see instance 0"
        r.history_capture()
        for mname, calls in shapes.motions(n, base).items():
            _apply(host_api, r, blas, base, calls)
            xf_b = shapes.tables(r)
            mv = rm.moved(xf_b, xf_a)
            assert mv.any() == (mname != "there_and_back") and (mname != "all" or mv.all()), mname
            for cname in ("none", "small"):
                r.set_camera(*rr.moved(A, MOVES[cname]))
                r.render_aovs(0.001)
                g_b = _gbuffer(r)
                for pname, P in PARAMS.items():
                    got_n = r.reproject_motion(P)
                    got = sp.state(r)
                    acc, cnt, sy, syy, n_ref, src, el = rm.reproject(g_b, g_a, *hist, A, xf_b, xf_a, mt, ms, **P)
                    what = (kind, mname, cname, pname)
                    print(what, "carried %d of %d, eligible %d" % (n_ref, w * h, el.sum()))
                    assert got_n == n_ref, what
                    assert np.array_equal(got[1], cnt), what
                    assert sp.same(got[0], acc) and sp.same(got[2], sy) and sp.same(got[3], syy), what
                    if w * h > 1 and pname != "exact" and mname != "there_and_back":
                        carried, rejected = n_ref / (w * h), (el.sum() - n_ref) / max(1, el.sum())
                        assert carried >= 0.10 and rejected >= 0.01, (what, carried, rejected)
                    if pname == "defaults" and w * h > 1 and mname != "there_and_back":
                        k = g_b["inst"]
                        through = int(((src >= 0) & (k >= 0) & mv[np.maximum(k, 0)]).sum())
                        print(what, "pixels of moved instances carried: %d" % through)
                        assert through >= 1, (what, "no pixel of a moved instance is carried")
                    if mname == "there_and_back" and cname == "none" and pname == "defaults":
                        # moved back to the same bits: unmoved, so every eligible pixel with samples is carried from itself
                        keep = el & (hist[1] > 0)
                        assert np.array_equal(src >= 0, keep) and np.array_equal(src[keep], np.arange(w * h).reshape(h, w)[keep]), what
    r.close()


# ---- 3. nothing moved: rt_reproject's result ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tlas", [True, False], ids=["tlas", "no_tlas"])
def test_unmoved_equals_rt_reproject(tlas, scenes, host_api, monkeypatch):
    w, h = 97, 41
    pair = [_renderer(host_api, monkeypatch, 3, w, h, scene=None if tlas else scenes.mixed_small) for _ in range(2)]
    for r in pair:
        r.stats_enable(True)
        rr.make_history(r, host_api, "adaptive", w, h)
        r.render_aovs(0.001)
        r.history_capture()
        r.set_camera(*rr.moved(shapes.CAMERA, MOVES["small"]))
        r.render_aovs(0.001)
    assert (pair[0].aov_instances() >= 0).any() == tlas
    for pname, P in PARAMS.items():
        a, b = pair[0].reproject(P), pair[1].reproject_motion(P)
        assert a == b > 0 and sp.same_state(sp.state(pair[0]), sp.state(pair[1])), pname
    for r in pair:
        r.close()


# ---- 4. idempotence, and what the call leaves alone --------------------------------------------------------------------------------
def test_twice_and_untouched_state(host_api, monkeypatch):
    w, h, n = 97, 41, 3
    r = _renderer(host_api, monkeypatch, n, w, h)
    blas, base = _base(host_api, r, n)
    r.stats_enable(True)
    rr.make_history(r, host_api, "adaptive", w, h)
    r.render_aovs(0.001)
    r.history_capture()
    _apply(host_api, r, blas, base, shapes.motions(n, base)["all"])
    r.set_camera(*rr.moved(shapes.CAMERA, MOVES["small"]))
    r.render_aovs(0.001)
    g_b = _gbuffer(r)
    lst = np.flatnonzero(np.random.default_rng(9).random(w * h) < 0.6).astype(np.uint32)
    r.set_active(lst)
    n1 = r.reproject_motion()
    first = sp.state(r)
    assert r.reproject_motion() == n1 > 0 and sp.same_state(first, sp.state(r))
    # the history is the capture's, whatever has happened to the accumulator since; NULL parameters are the defaults, a NULL count is allowed
    r.clear()
    assert r.reproject_motion(dict(host_api.REPROJECT_DEFAULTS)) == n1 and sp.same_state(first, sp.state(r))
    r.render(host_api.RT_MODE_PATH, 50, 2)
    assert r.rt.rt_reproject_motion(r.ctx, None, None) == 0 and sp.same_state(first, sp.state(r))
    # the active-pixel list and the G-buffer are not touched
    got, k = r.active()
    assert k == len(lst) and np.array_equal(got, lst)
    after = _gbuffer(r)
    assert all(sp.same(g_b[key], after[key]) for key in g_b)
    # a budget plan is dropped: every pixel's count was rewritten
    assert r.select_budget(dict(select=ADAPTIVE, pass_cap=4))[0] > 0
    r.reproject_motion()
    assert r.rt.rt_render_budget(r.ctx, 0, SEED, 4) == host_api.RT_E_STATE
    # with profiling on, the kernel is one launch of rt_profile.query
    r.set_profiling(True)
    r.profile()
    r.reproject_motion()
    assert r.profile()["query"]["launches"] == 1
    r.close()


# ---- 5. the two levels of validity, and the errors -------------------------------------------------------------------------------------
def test_states_and_errors(host_api, monkeypatch):
    w, h, n = 64, 40, 3
    r = _renderer(host_api, monkeypatch, n, w, h)
    L, ctx = r.rt, r.ctx
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    blas, base = _base(host_api, r, n)
    cnt = C.c_int(-7)

    def rep(fn, context=ctx, **kw):
        p = host_api.reproject_params(kw)
        return fn(context, C.byref(p), C.byref(cnt))

    def why():
        return L.rt_last_error(ctx).decode()

    # parameters: refused before the context is looked at
    for bad in (dict(normal_tolerance=-0.1), dict(normal_tolerance=float("nan")), dict(plane_tolerance=-1e-9), dict(plane_tolerance=float("nan")), dict(max_history=-1)):
        assert rep(L.rt_reproject_motion, **bad) == ARG and rep(L.rt_reproject_motion, None, **bad) == ARG, bad
    assert rep(L.rt_reproject_motion, None) == ARG
    # statistics off; no history yet; a stale G-buffer
    r.render_aovs(0.001)
    assert rep(L.rt_reproject_motion) == STATE and "statistics" in why()
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 3)
    assert rep(L.rt_reproject_motion) == STATE and "history" in why()

    def recapture():
        _apply(host_api, r, blas, base, [])
        r.set_camera(*shapes.CAMERA)
        r.render_aovs(0.001)
        r.history_capture()
        assert rep(L.rt_reproject) == 0 and rep(L.rt_reproject_motion) == 0

    recapture()
    # an instance move: the G-buffer is stale for both; with a new one rt_reproject has no valid history, rt_reproject_motion carries
    move = shapes.motions(n, base)["translated"]
    _apply(host_api, r, blas, base, move)
    assert rep(L.rt_reproject_motion) == STATE and "G-buffer" in why()
    r.render_aovs(0.001)
    assert rep(L.rt_reproject) == STATE and "history" in why()
    assert rep(L.rt_reproject_motion) == 0 and cnt.value > 0
    # ... across any number of moves, and a camera move as well
    _apply(host_api, r, blas, base, shapes.motions(n, base)["two_calls"])
    r.set_camera(*rr.moved(shapes.CAMERA, MOVES["small"]))
    r.render_aovs(0.001)
    assert rep(L.rt_reproject) == STATE and rep(L.rt_reproject_motion) == 0 and cnt.value > 0
    # a failed rt_set_instances (a blas mismatch) leaves both calls as they were: here rt_reproject valid, there not
    bad = shapes.records(host_api, [blas[0] + 1], [base[0]])
    assert r.set_instances(0, bad) == ARG
    assert rep(L.rt_reproject) == STATE and rep(L.rt_reproject_motion) == 0
    recapture()
    assert r.set_instances(0, bad) == ARG
    assert rep(L.rt_reproject) == 0 and rep(L.rt_reproject_motion) == 0
    # a fisheye camera
    r.set_camera(*shapes.CAMERA, fisheye=True)
    r.render_aovs(0.001)
    assert rep(L.rt_reproject_motion) == UNSUP
    # what changes the shapes, and the statistics switched off, end the history for both calls
    for drop in (r.commit, lambda: (r.stats_enable(False), r.stats_enable(True))):
        recapture()
        _apply(host_api, r, blas, base, move)
        drop()
        r.render_aovs(0.001)
        assert rep(L.rt_reproject) == STATE and "history" in why()
        assert rep(L.rt_reproject_motion) == STATE and "history" in why()
    r.close()


# ---- 6. Renderer::CommitInstances ------------------------------------------------------------------------------------------------------
def test_renderer_commit_instances_equals_the_sequence_by_hand(host_api, monkeypatch):
    w, h, n = 64, 40, 3
    RP = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=16, carry_view_dependent=0)
    PATH = host_api.RT_MODE_PATH
    r, off, hand, plain = (_renderer(host_api, monkeypatch, n, w, h) for _ in range(4))
    r.set_adaptive(True, ADAPTIVE), r.set_reproject(True, RP)
    off.set_adaptive(True, ADAPTIVE)  # reproject off: CommitInstances is Scene::CommitInstances and a clear
    _, base = _base(host_api, r, n)
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

    # an instance move alone; one with a camera move in the same Tick; one before min_samples whole frames have been taken
    moves = {6: (shapes.motions(n, base)["translated"][0], None), 8: (shapes.motions(n, base)["all"][0], MOVES["small"]), 9: (shapes.motions(n, base)["rotated"][0], None)}
    cam = shapes.CAMERA
    for t in range(12):
        if t in moves:
            (first, Ts), cmove = moves[t]
            for x in (r, off, hand, plain):
                x.scene.set_transforms(first, [T.reshape(4, 4) for T in Ts])
            r.commit_instances()
            off.commit_instances()
            hand.render_aovs(0.001)
            hand.history_capture()
            hand.scene.commit_instances()
            plain.scene.commit_instances()
            plain.clear()
            whole[id(plain)] = 0
            if cmove is not None:
                cam = rr.moved(cam, cmove)
                for x in (r, off, hand, plain):
                    x.set_camera(*cam)
            hand.render_aovs(0.001)
            carried = hand.reproject_motion(RP)
            whole[id(hand)] = ADAPTIVE["min_samples"]
        r.tick()
        off.tick()
        k, m = step(hand, t), step(plain, t)
        assert r.active_pixels() == k and off.active_pixels() == m, t
        if t in moves:
            assert r.carried_pixels() == carried > 0, t
            assert np.all(off.stats()[0] == 1), t
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
        assert sp.same(off.tick_accumulator(), plain.accumulator()) and sp.same_state(sp.state(off), sp.state(plain)), t
    # a Commit() between CommitInstances and the Tick: the upload ended the captured history, so the Tick clears (and does not throw)
    r.scene.set_transforms(0, [base[0].reshape(4, 4)])
    r.commit_instances()
    r.commit()
    r.tick()
    assert np.all(r.stats()[0] == 1) and r.active_pixels() == w * h
    for x in (r, off, hand, plain):
        x.close()


# ---- 7. what the carry is worth --------------------------------------------------------------------------------------------------------
def test_carried_samples_beat_fresh_ones_across_an_instance_move(host_api, monkeypatch):
    """One measurement (tests/reproject_motion_shapes.py quality): 32 samples per pixel, the object moved, the samples carried and 4 added,
    against clear + 4, on the carried pixels of the moved object and of the floor away from its shadow.  Asserted: the carried frame's MSE
    there is the lower one.  Measured on an MI355X: ratio 0.243 on 1078 pixels, 0.69 on the 30 carried floor pixels of the shadow zone
    (profiles/reproject_motion_quality.json); under the moved
    shadow the carried samples are biased, which is reported, not asserted."""
    q = shapes.QUALITY
    r = _renderer(host_api, monkeypatch, 1, q["width"], q["height"], camera=None, scene=shapes.quality_scene)
    r.stats_enable(True)
    with np.errstate(all="ignore"):
        out = shapes.quality(host_api, r)
    r.close()
    print("carry across an instance move:", out)
    assert out["moved_object_pixels_carried"] > 0 and out["safe_pixels"] >= 0.1 * q["width"] * q["height"]
    assert out["mse_carried"] < out["mse_fresh"], out


# ---- 8. the example -----------------------------------------------------------------------------------------------------------------
def test_example_spin_carry(tmp_path, scenes, host_api, monkeypatch):
    """examples/render_scene.cpp --spin DEG --carry in path mode: adaptive Ticks with Renderer::reproject set, the move sent through
    Renderer::CommitInstances before the last Tick, which carries.  The image is the one a renderer shows that was driven the same way, and
    not the one of the clearing --spin."""
    import subprocess
    from conftest import ROOT, pkg
    sp.clean_env(monkeypatch)
    sf = pkg("scene_file")
    exe = str(tmp_path / "render_scene")
    host, csrc = os.path.join(ROOT, "ray-and-pathtracer_amd", "host"), os.path.join(ROOT, "ray-and-pathtracer_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "render_scene.cpp"), "-I" + host, "-L" + host, "-lrapt_host",
                           "-L" + csrc, "-lrt_amd", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc, "-o", exe])
    scene_path = str(tmp_path / "tlas.rapt")
    scenes.tlas_test2(sf.SceneWriter(scene_path))
    w, h, frames = 48, 32, 6

    def run(*more):
        out = str(tmp_path / "out.ppm")
        subprocess.check_call([exe, scene_path, out, str(w), str(h), "path", str(frames)] + list(more))
        raw = open(out, "rb").read()
        return np.frombuffer(raw[raw.index(b"255\n") + 4:], dtype=np.uint8).reshape(h, w, 3).astype(np.uint32)

    carried = run("--spin", "20", "--carry")
    r = host_api.HostRenderer(w, h)
    r.scene.load_file(scene_path)
    r.scene.set_raytracer(False)
    r.set_adaptive(True)
    r.set_reproject(True)
    r.commit()
    for _ in range(frames - 1):
        r.tick()
    s = r.scene
    ang = F32(F32(F32(20.0) * F32(3.14159265358979)) / F32(180.0))
    s.set_transforms(0, [ir.mat_mul(s.instance_dump(0)["T"], s.trs((0, 0, 0), 1, 0.0, ang, 0.0))])
    r.commit_instances()
    r.tick()
    assert r.carried_pixels() > 0
    px = r.tick_pixels()
    want = np.stack([(px >> 16) & 255, (px >> 8) & 255, px & 255], -1)
    r.close()
    assert np.array_equal(carried, want)
    assert not np.array_equal(carried, run("--spin", "20"))
    # --carry without a spin, or in whitted mode, is refused with a message, not ignored
    for args in ([exe, scene_path, str(tmp_path / "no.ppm"), str(w), str(h), "path", "2", "--carry"],
                 [exe, scene_path, str(tmp_path / "no.ppm"), str(w), str(h), "whitted", "1", "--spin", "20", "--carry"]):
        done = subprocess.run(args, capture_output=True)
        assert done.returncode == 2 and b"--carry" in done.stderr and not (tmp_path / "no.ppm").exists()
