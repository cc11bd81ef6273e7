"""Budgeted adaptive passes on the device, through host_api (include/rt_amd.h rt_select_budget / rt_download_budgets / rt_render_budget):
  1. the selection -- list, budgets, total, cap used, the fit rule's halvings and its RT_E_UNSUPPORTED -- against tests/budget_ref.py, on
     uneven statistics, and at the sizes where the compaction takes its other paths (tests/adaptive_shapes.py SIZES);
  2. count alone decides a pixel: after every budgeted pass each pixel with count n equals frames F .. F + n - 1 rendered one at a time by a
     second context (the test that catches a wrong sample -> (pixel, frame) mapping); unlisted pixels are not written;
  3. a pass at pass_cap 1 after k whole frames leaves what rt_render_active(frame_base + k, 1) leaves on the same list;
  4. check 2 on every pipeline a path batch can take, and at a frame_base whose frame numbers wrap;
  5. the plan's life (consumed, dropped by whatever changes counts or the list), the error cases, an empty selection;
  6. Renderer::Tick with adaptivePassCap set against the loop by hand, a reprojecting Tick included; adaptivePassCap 0 is today's Tick.
Every comparison is exact: np.array_equal on integers, bitwise on floats.  The classes of pixels asserted as present are the ones
tests/test_budget_cpu.py counts on the oracle's samples of the same scenes and sizes (tests/budget_shapes.py PRESENT)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import adaptive_shapes as sh  # noqa: E402
import budget_ref as br  # noqa: E402
import budget_shapes as tc  # noqa: E402
import support as sp  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
F32 = np.float32
SEED = 0x12345678


def _renderer(host_api, scenes, monkeypatch, name, env=None, w=97, h=41):
    return sp.renderer(host_api, monkeypatch, tc.scene_fn(scenes, name), w, h, env)


def _snapshots(host_api, scenes, monkeypatch, name, w, h, F, upto):
    return sp.snapshots(host_api, monkeypatch, name, tc.scene_fn(scenes, name), w, h, upto, first=F)


def _select(r, sel, cap, mps=0):
    return r.select_budget(dict(select=sel, pass_cap=cap, max_pass_samples=mps))


def _check_plan(r, stats, sel, cap, mps=0):
    """rt_select_budget on the context's statistics (= stats) against budget_ref.plan; returns the reference plan"""
    cnt, sy, syy = stats
    lst, b, total, used = br.plan(cnt, sy, syy, cap, mps, **sel)
    assert b is not None, "the reference says RT_E_UNSUPPORTED"
    n, got_total, got_cap = _select(r, sel, cap, mps)
    got_lst, n2 = r.active()
    got_b, n3 = r.budgets()
    assert n == n2 == n3 == len(lst) and (got_total, got_cap) == (total, used), (sel, cap, mps, n, len(lst), got_total, total, got_cap, used)
    assert np.array_equal(got_lst, lst) and np.array_equal(got_b, b), (sel, cap, mps)
    assert len(b) == 0 or b.min() >= 1
    return lst, b, total, used


def _uneven(r, host_api, w, h):
    """counts 4 and 7"""
    stats = sp.uneven(r, host_api, sh.seeded_list(w, h, seed=tc.UNEVEN_SEED))
    assert set(np.unique(stats[0])) == {tc.UNEVEN_WHOLE, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE}
    return stats


# ---- 1. selection ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(97, 41), (257, 3)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", list(tc.SCENES))
def test_selection_equals_the_restatement(name, size, scenes, host_api, monkeypatch):
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, name, w=w, h=h)
    stats = _uneven(r, host_api, w, h)
    present = tc.PRESENT[(name, size)]
    got = tc.classes(*stats)
    for cls in present:
        if cls != "loop_budgets_differ":
            assert got[cls] > 0, (cls, got)
    S = tc.SELECT
    distinct = set()
    for sel in (S, dict(S, max_samples=9), dict(S, threshold=0.0), dict(S, threshold=INF), dict(S, floor=0.5), tc.HALVE):
        for cap in (1, 7, 64):
            lst, b, total, used = _check_plan(r, stats, sel, cap)
            assert used == cap  # the context's own limit is far away
            distinct.add((len(lst), total))
            again = _check_plan(r, stats, sel, cap)  # a second selection on the same statistics: the same plan
            assert np.array_equal(again[1], b)
    assert len(distinct) >= 6, distinct  # the parameter sets really select different plans
    # a prefix of the budgets, and the list's true length
    lst, b, total, used = _check_plan(r, stats, S, 7)
    short, n = r.budgets(cap=5)
    assert n == len(lst) and np.array_equal(short, b[:5])
    # the fit rule: one halving, two halvings (7 -> 3 -> 1), and not even one sample per active pixel
    cnt, sy, syy = stats
    t7, t3, t1 = (int(br.budgets(cnt, sy, syy, cap, **tc.HALVE).sum()) for cap in (7, 3, 1))
    assert t7 > t3 > t1 == w * h
    for mps, want_cap in ((t7, 7), (t7 - 1, 3), (t3, 3), (t3 - 1, 1), (t1, 1)):
        assert _check_plan(r, stats, tc.HALVE, 7, mps)[3] == want_cap, mps
    if "clamped_by_max_samples" in present:  # budgets above 32 exist: pass_cap 64 halves once to fit total(32)
        t32 = int(br.budgets(cnt, sy, syy, 32, **S).sum())
        assert int(br.budgets(cnt, sy, syy, 64, **S).sum()) > t32
        assert _check_plan(r, stats, S, 64, t32)[3] == 32
    n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
    p = host_api.budget_params(dict(select=tc.HALVE, pass_cap=7, max_pass_samples=t1 - 1))
    assert r.rt.rt_select_budget(r.ctx, C.byref(p), C.byref(n), C.byref(total), C.byref(cap)) == host_api.RT_E_UNSUPPORTED
    assert n.value == t1
    out = np.zeros(w * h, np.uint32)
    assert r.rt.rt_download_budgets(r.ctx, out.ctypes.data_as(C.c_void_p), w * h, C.byref(n)) == host_api.RT_E_STATE  # no plan afterwards
    assert r.rt.rt_render_budget(r.ctx, 0, SEED, 4) == host_api.RT_E_STATE
    got_lst, k = r.active()                                                                                         # the list is installed
    assert k == t1 and np.array_equal(got_lst, ar.active_list(cnt, sy, syy, **tc.HALVE))
    r.render_active(tc.UNEVEN_WHOLE + tc.UNEVEN_MORE, 1)                                                            # ... and rt_render_active serves it
    assert np.array_equal(r.stats()[0], cnt + 1)
    r.close()


SHAPE_SELECT = dict(min_samples=4, max_samples=12, threshold=0.05, floor=1e-3)
RENDERED_SHAPES = [s for s in sh.SIZES if s[0] * s[1] <= 641 * 409]  # the two largest frames: the selection alone


@pytest.mark.parametrize("size", list(sh.SIZES), ids=lambda s: "%dx%d" % s)
def test_selection_at_the_compaction_edges(size, scenes, host_api, monkeypatch):
    """One lane, one wave, one block, ragged frames, more blocks than the scan has lanes: counts 3 (below min_samples) and 5 (noisy or
    not), the plan against the restatement at pass_cap 1 and 7; every pixel (b = 12 - count, capped) and no pixel; and, up to 641 x 409,
    a pass at pass_cap 7 against frames rendered one at a time -- the offsets and the records of every block and scan lane."""
    w, h = size
    n = w * h
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.stats_enable(True)
    r.clear()
    r.render(PATH, 0, 3)
    on = np.random.default_rng(9).random(n) < 0.3  # about 30 % of the pixels, the first and the last among them
    on[0] = on[n - 1] = True
    r.set_active(np.flatnonzero(on).astype(np.uint32))
    r.render_active(3, 2)
    stats = r.stats()
    assert set(np.unique(stats[0])) <= {3, 5} and (stats[0] == 5).any()
    for cap in (1, 7):
        lst, b, total, used = _check_plan(r, stats, SHAPE_SELECT, cap)
        assert (stats[0].reshape(-1)[lst] == 3).sum() == (stats[0] == 3).sum()  # everything below min_samples is listed
    everything = dict(SHAPE_SELECT, min_samples=12)
    lst, b, total, used = _check_plan(r, stats, everything, 7)
    assert len(lst) == n and total == 7 * n
    nothing = dict(min_samples=2, max_samples=1024, threshold=INF, floor=1e-3)
    assert _check_plan(r, stats, nothing, 7)[2] == 0
    before = sp.state(r)
    r.render_budget(0)  # an empty plan: RT_OK, nothing touched
    assert sp.same_state(sp.state(r), before)
    if size in RENDERED_SHAPES:
        snaps = _snapshots(host_api, scenes, monkeypatch, "mixed_small", w, h, 0, 12)
        assert sp.differs_from_snapshot_of_its_count(before, snaps) is None  # the starting state is frames 0 .. count - 1 already
        lst, b, total, used = _check_plan(r, stats, SHAPE_SELECT, 7)
        r.render_budget(0)
        after = sp.state(r)
        want = stats[0].reshape(-1).copy()
        want[lst] += b
        assert np.array_equal(after[1].reshape(-1), want)
        assert sp.differs_from_snapshot_of_its_count(after, snaps) is None
        lst, b, total, used = _check_plan(r, r.stats(), everything, 7)  # every pixel, first frames 3 .. 11 by now
        r.render_budget(0)
        assert sp.differs_from_snapshot_of_its_count(sp.state(r), snaps) is None
    r.close()


# ---- 2. / 4. count alone decides a pixel ---------------------------------------------------------------------------------------------------
def _count_decides(host_api, scenes, monkeypatch, name, w, h, F, env=None, differ=False):
    P, cap = tc.LOOP, tc.LOOP_CAP
    snaps = _snapshots(host_api, scenes, monkeypatch, name, w, h, F, P["max_samples"])
    r = _renderer(host_api, scenes, monkeypatch, name, env, w=w, h=h)
    r.stats_enable(True)
    r.clear()
    for k in range(tc.LOOP_PASSES):
        before = sp.state(r)
        lst, b, total, used = _check_plan(r, before[1:], P, cap)
        assert used == cap and len(lst) > 0
        r.render_budget(F, SEED, 4)
        after = sp.state(r)
        on = np.zeros(w * h, bool)
        on[lst] = True
        on = on.reshape(h, w)
        want = before[1].reshape(-1).copy()
        want[lst] += b
        assert np.array_equal(after[1].reshape(-1), want), k
        assert all(sp.same(x[~on], y[~on]) for x, y in zip(after, before)), "pass %d wrote an unlisted pixel" % k
        assert sp.differs_from_snapshot_of_its_count(after, snaps) is None, k
        if k == 0:
            assert len(lst) == w * h and np.all(b == min(P["min_samples"], cap))
        else:
            assert len(lst) < w * h
        if k == 1 and differ:
            assert len(np.unique(b)) >= 4, np.unique(b, return_counts=True)  # budgets differ across pixels (test_budget_cpu: all of 1 .. 7)
    assert after[1].max() <= P["max_samples"]
    # the plan is consumed
    assert r.rt.rt_render_budget(r.ctx, F, SEED, 4) == host_api.RT_E_STATE
    r.close()


@pytest.mark.parametrize("size", [(97, 41), (257, 3)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2", "shiny"])
def test_count_alone_decides_a_pixel(name, size, scenes, host_api, monkeypatch):
    """Three passes from rt_clear at pass_cap 7, frame_base 100, max_samples 20 (shiny: the general kernel)."""
    differ = "loop_budgets_differ" in tc.PRESENT[(name, size)]
    _count_decides(host_api, scenes, monkeypatch, name, size[0], size[1], 100, differ=differ)


PIPELINES = [{"RT_STREAM": "0"}, {"RT_SLOTS": "777"}, {"RT_PRIMARY_TABLE": "0"}, {"RT_FUSE": "0"}, {"RT_FUSE": "1"}, {"RT_FUSE": "2"},
             {"RT_DEFER_GAMMA": "0"}, {"RT_WIDE": "1"}]


@pytest.mark.parametrize("env", PIPELINES, ids=sp.env_id)
def test_count_decides_on_every_pipeline(env, scenes, host_api, monkeypatch):
    """RT_SLOTS=777: the first pass has 15,908 samples for 777 slots (the slot wavefront hands slots on)."""
    _count_decides(host_api, scenes, monkeypatch, "mixed_small", 97, 41, 100, env=env)


def test_count_decides_at_a_frame_base_that_wraps(scenes, host_api, monkeypatch):
    _count_decides(host_api, scenes, monkeypatch, "mixed_small", 97, 41, 0xFFFFFFF0)


# ---- 3. the new path and the old ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2", "shiny"])
def test_a_pass_at_cap_1_is_render_active(name, scenes, host_api, monkeypatch):
    w, h, F, k = 97, 41, 10, 5
    PATH = host_api.RT_MODE_PATH
    sel = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    r = _renderer(host_api, scenes, monkeypatch, name, w=w, h=h)
    r.stats_enable(True)
    r.clear()
    r.render(PATH, F, k)
    lst, b, total, used = _check_plan(r, r.stats(), sel, 1)
    assert 0 < len(lst) < w * h and total == len(lst) and np.all(b == 1)
    r.render_budget(F)
    new = sp.state(r)
    r.clear()
    r.render(PATH, F, k)
    r.set_active(lst)
    r.render_active(F + k, 1)
    assert sp.same_state(sp.state(r), new)
    r.close()


# ---- 5. state and errors -----------------------------------------------------------------------------------------------------------------
def test_plan_state_and_errors(scenes, host_api, monkeypatch):
    w, h = 96, 64
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    L, ctx = r.rt, r.ctx
    ARG, STATE, UNSUP = host_api.RT_E_ARG, host_api.RT_E_STATE, host_api.RT_E_UNSUPPORTED
    n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
    buf = np.zeros(w * h, np.uint32)
    px = buf.ctypes.data_as(C.c_void_p)
    sel0 = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)

    def sel(select=None, pass_cap=7, mps=0, outs=None):
        p = host_api.budget_params(dict(select=dict(sel0, **(select or {})), pass_cap=pass_cap, max_pass_samples=mps))
        a, b, c = outs or (C.byref(n), C.byref(total), C.byref(cap))
        return L.rt_select_budget(ctx, C.byref(p), a, b, c)

    def render():
        return L.rt_render_budget(ctx, 0, SEED, 4)

    # statistics off
    assert sel() == STATE and render() == STATE and L.rt_download_budgets(ctx, px, w * h, C.byref(n)) == STATE
    r.stats_enable(True)
    r.render(PATH, 0, 5)
    # no plan yet
    assert render() == STATE and L.rt_download_budgets(ctx, px, w * h, C.byref(n)) == STATE
    # arguments: everything rt_select_active refuses, pass_cap outside 1 .. 1024, null pointers -- and a refused call installs nothing
    for bad in (dict(min_samples=1), dict(min_samples=0), dict(min_samples=8, max_samples=7), dict(threshold=float("nan")), dict(threshold=-0.5),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan"))):
        assert sel(bad) == ARG, bad
    for bad in (0, -1, 1025, 2 ** 20):
        assert sel(pass_cap=bad) == ARG, bad
    assert sel(outs=(None, C.byref(total), C.byref(cap))) == ARG and sel(outs=(C.byref(n), None, C.byref(cap))) == ARG and sel(outs=(C.byref(n), C.byref(total), None)) == ARG
    p = host_api.budget_params(dict(select=sel0))
    assert L.rt_select_budget(None, C.byref(p), C.byref(n), C.byref(total), C.byref(cap)) == ARG and L.rt_render_budget(None, 0, SEED, 4) == ARG
    assert (n.value, total.value, cap.value) == (-7, 7, -7) and render() == STATE
    assert L.rt_download_active(ctx, px, w * h, C.byref(n)) == STATE  # ... not even a list
    n.value = -7
    assert sel(pass_cap=1) == 0 and sel(pass_cap=1024) == 0 and cap.value == 1024
    assert L.rt_download_budgets(ctx, None, 3, C.byref(n)) == ARG and L.rt_download_budgets(ctx, px, -1, C.byref(n)) == ARG and L.rt_download_budgets(ctx, px, 3, None) == ARG
    # the library's defaults when params is NULL
    cnt, sy, syy = r.stats()
    want = br.plan(cnt, sy, syy, 64, 0, **ar.DEFAULTS)
    assert r.select_budget(None) == (len(want[0]), want[2], 64) and np.array_equal(r.budgets()[0], want[1])
    # the plan is consumed by its pass
    assert sel() == 0 and n.value > 0
    assert render() == 0 and render() == STATE and L.rt_download_budgets(ctx, px, w * h, C.byref(n)) == STATE
    assert L.rt_download_active(ctx, px, w * h, C.byref(n)) == 0  # (the list stays)
    # ... and dropped by whatever changes the counts or the list
    r.render_aovs(0.001)
    r.history_capture()
    some = np.array([3, 9, 10, w * h - 1], np.uint32)
    droppers = dict(render=lambda: r.render(PATH, 9, 1), render_rows=lambda: r.render_rows(PATH, 9, 1, 1, 2, 3), render_active=lambda: r.render_active(9, 1),
                    clear=r.clear, stats_enable=lambda: r.stats_enable(True), reproject=lambda: r.reproject(None), set_active=lambda: r.set_active(some),
                    select_active=lambda: r.select_active(sel0))
    for what, call in droppers.items():
        if what == "reproject":  # (the history is the statistics': captured again after the clears above)
            r.render(PATH, 0, 5)
            r.render_aovs(0.001)
            r.history_capture()
        assert sel() == 0, what
        call()
        assert render() == STATE, what
        assert L.rt_download_budgets(ctx, px, w * h, C.byref(n)) == STATE, what
    r.clear()
    r.render(PATH, 0, 5)
    # the Q-learning sampler: rt_render_active's rule; the plan waits
    assert sel() == 0 and n.value > 0
    r.qlearn_enable(4, (-3, -1, -3), (3, 4, 5))
    assert render() == UNSUP
    r.qlearn_disable()
    before = r.stats()[0]
    budgets = r.budgets()[0]
    lst = r.active()[0]
    assert render() == 0
    want = before.reshape(-1).copy()
    want[lst] += budgets
    assert np.array_equal(r.stats()[0].reshape(-1), want)
    # an empty selection: a plan of no samples -- RT_OK without a launch, nothing touched, consumed like any other
    assert sel(dict(min_samples=2, threshold=INF)) == 0 and (n.value, total.value, cap.value) == (0, 0, 7)
    assert r.budgets()[1] == 0
    state = sp.state(r)
    assert render() == 0 and sp.same_state(sp.state(r), state) and render() == STATE
    # statistics switched off under a plan
    assert sel() == 0
    r.stats_enable(False)
    assert render() == STATE
    r.close()


# ---- 6. Renderer::Tick -------------------------------------------------------------------------------------------------------------------
def test_tick_with_a_pass_cap_equals_the_loop_by_hand(scenes, host_api, monkeypatch):
    w, h, cap = 97, 41, 7
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    RP = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=16, carry_view_dependent=0)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.set_adaptive(True, P)
    r.set_reproject(True, RP)
    r.set_adaptive_budget(cap)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    cam = r.camera()
    hand.set_camera(*cam)
    hand.stats_enable(True)
    hand.clear()
    base, taken, MOVE_AT = 0, [], 5
    for t in range(8):
        if t == MOVE_AT:  # a camera move: the samples are carried, and frame_base becomes the frame of the carry
            cam = (np.asarray(cam, F32) + np.array((0.05, 0.0, 0.0), F32)).astype(F32)
            r.set_camera(*cam)
            hand.render_aovs(0.001)
            hand.history_capture()
            hand.set_camera(*cam)
            hand.render_aovs(0.001)
            carried = hand.reproject(RP)
            base = t
        r.tick()
        n, total, used = _select(hand, P, cap)
        hand.render_budget(base, SEED, 4)
        assert (r.active_pixels(), r.pass_samples()) == (n, total) and used == cap, t
        if t == MOVE_AT:
            assert r.carried_pixels() == carried > 0
        if t == 0:
            assert n == w * h and total == min(P["min_samples"], cap) * w * h  # no whole-frame phase: every pixel is below min_samples
        taken.append(total)
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
    assert 0 < taken[1] < taken[0] and len(np.unique(r.stats()[0])) > 3
    r.close()
    hand.close()


def test_tick_with_pass_cap_0_is_the_adaptive_tick_of_before(scenes, host_api, monkeypatch):
    w, h = 97, 41
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.set_adaptive(True, P)
    r.set_adaptive_budget(7)
    r.set_adaptive_budget(0)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    hand.set_camera(*r.camera())
    hand.stats_enable(True)
    hand.clear()
    for t in range(8):
        r.tick()
        if t < P["min_samples"]:
            hand.render(host_api.RT_MODE_PATH, t, 1)
            n = w * h
        else:
            n = hand.select_active(P)
            hand.render_active(t, 1)
        assert r.active_pixels() == r.pass_samples() == n, t
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
    r.close()
    hand.close()
