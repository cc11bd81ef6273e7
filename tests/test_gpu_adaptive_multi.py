"""Adaptive sampling over several contexts on the device, through host_api (include/rt_amd.h rt_select_active_rows, rt_select_budget_rows,
rt_gather_stats_rows, rt_gather_active; rapt::Renderer::Tick with 'adaptive' and several contexts):
  1. a shard's selection is tests/adaptive_ref.py's list restricted to its rows, and the shards of a split concatenate to rt_select_active's
     list, at the sizes where the compaction takes its other paths through the row map;
  2. a shard's budgets, total and cap are tests/budget_ref.py's on the shard taken as a row_count x width frame, its own fit rule included,
     and rt_render_budget on a shard plan leaves every listed pixel equal to whole frames of its count and every other pixel unwritten;
  3. rt_gather_stats_rows moves the accumulator and the three statistics arrays of the rows it names, in either direction, and nothing else;
  4. rt_gather_active moves the four arrays at the listed pixels and writes no other pixel, after either kind of pass;
  5. adaptive Ticks over [0, 0], [0, 0, 0] and [0, 1] equal the one-context Ticks: frame-by-frame, budgeted, across a reprojection carry
     and with the variance-guided denoiser.
Every comparison is exact: np.array_equal on integers, bitwise on floats.  Tests 1-5 need entry points the parent commit does not have,
and its Tick throws with 'adaptive' and several contexts."""
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

F32 = np.float32
SEED = 0x12345678
# (width, height) -> the splits run at that size: what each is here for is the table of tests/test_adaptive_rows_cpu.py
SPLITS = {(97, 41): (2, 3), (257, 3): (2,), (64, 5): (4,), (1, 7): (3,), (641, 409): (2,)}


def _renderer(host_api, scenes, monkeypatch, name, w, h, devices=None, **kw):
    return sp.renderer(host_api, monkeypatch, lambda b: tc.scene_fn(scenes, name)(b, **kw), w, h, devices=devices)


def _shard(h, r, n):
    """(row_first, row_stride, row_count) of rank r of n"""
    return r, n, (h - r + n - 1) // n


def _shard_pixels(w, h, r, n):
    return np.concatenate([np.arange(y * w, (y + 1) * w) for y in range(r, h, n)])


def _uneven(r, host_api, w, h):
    """counts 4 and 7 (one count where the seeded list is the frame)"""
    return sp.uneven(r, host_api, sh.seeded_list(w, h, seed=tc.UNEVEN_SEED))


def _snapshots(host_api, scenes, monkeypatch, w, h, upto):
    return sp.snapshots(host_api, monkeypatch, "mixed_small", scenes.mixed_small, w, h, upto)


# ---- 1. shard selection --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SPLITS), ids=lambda s: "%dx%d" % s)
def test_shard_selection_equals_the_restatement(size, scenes, host_api, monkeypatch):
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    cnt, sy, syy = _uneven(r, host_api, w, h)
    want = ar.active_list(cnt, sy, syy, **tc.SELECT)
    assert r.select_active(tc.SELECT) == len(want) and np.array_equal(r.active()[0], want)
    if size == (97, 41):
        assert 0.05 * w * h < len(want) < 0.95 * w * h, len(want)  # nothing passes vacuously (tests/budget_shapes.py PRESENT)
    for n in SPLITS[size]:
        lists = []
        for k in range(n):
            first, stride, count = _shard(h, k, n)
            mine = want[np.isin(want, _shard_pixels(w, h, k, n))]
            got_n = r.select_active_rows(first, stride, count, tc.SELECT)
            got, n2 = r.active()
            assert got_n == n2 == len(mine) and np.array_equal(got, mine), (n, k)
            lists.append(got)
        assert np.array_equal(np.sort(np.concatenate(lists)), want), n
    assert r.select_active_rows(0, 1, h, tc.SELECT) == len(want) and np.array_equal(r.active()[0], want)  # the whole frame as a row set
    # a row set outside the frame: rt_gather_rows' rule
    out = C.c_int(-7)
    p = host_api.adaptive_params(tc.SELECT)
    for rows in ((-1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 1, h + 1), (h, 1, 1), (1, 2, h // 2 + 1)):
        assert r.rt.rt_select_active_rows(r.ctx, C.byref(p), rows[0], rows[1], rows[2], C.byref(out)) == host_api.RT_E_ARG, rows
        assert b"rt_select_active_rows" in r.rt.rt_last_error(r.ctx)
    r.close()


# ---- 2. shard budgets ----------------------------------------------------------------------------------------------------------------------
def _check_shard_plan(r, stats, w, h, k, n, sel, cap, mps=0):
    """rt_select_budget_rows on rank k of n against budget_ref.plan on the shard's rows taken as a frame; returns (pixels, budgets, cap used)"""
    first, stride, count = _shard(h, k, n)
    rows = np.arange(k, h, n)
    pix = _shard_pixels(w, h, k, n)
    lst, b, total, used = br.plan(*(a[rows] for a in stats), pass_cap=cap, max_pass_samples=mps, **sel)
    assert b is not None
    got = r.select_budget_rows(first, stride, count, dict(select=sel, pass_cap=cap, max_pass_samples=mps))
    got_lst, n2 = r.active()
    got_b, n3 = r.budgets()
    assert got == (len(lst), total, used) and n2 == n3 == len(lst), (k, n, cap, mps, got, len(lst), total, used)
    assert np.array_equal(got_lst, pix[lst]) and np.array_equal(got_b, b), (k, n, cap, mps)
    return pix[lst], b, used


@pytest.mark.parametrize("n", [2, 3])
def test_shard_budgets_equal_the_restatement(n, scenes, host_api, monkeypatch):
    w, h = 97, 41
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w, h)
    stats = _uneven(r, host_api, w, h)
    assert set(np.unique(stats[0])) == {tc.UNEVEN_WHOLE, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE}
    whole64 = br.budgets(*stats, 64, **tc.SELECT).reshape(-1)
    for k in range(n):
        pix, b, used = _check_shard_plan(r, stats, w, h, k, n, tc.SELECT, 64)
        assert used == 64 and np.array_equal(b, whole64[pix]) and b.max() > 7  # no cap lowered: the frame's budgets at those pixels
        # the shard's own fit rule: a limit between its totals at caps 3 and 1 halves twice
        rows = np.arange(k, h, n)
        t7, t3, t1 = (int(br.budgets(*(a[rows] for a in stats), cap, **tc.HALVE).sum()) for cap in (7, 3, 1))
        assert t7 > t3 > t1 == len(rows) * w
        assert _check_shard_plan(r, stats, w, h, k, n, tc.HALVE, 7, t3 - 1)[2] == 1
        assert _check_shard_plan(r, stats, w, h, k, n, tc.HALVE, 7, t3)[2] == 3
    # a pass on every shard's plan in turn: listed pixels hold whole frames of their count, nothing else is written
    snaps = _snapshots(host_api, scenes, monkeypatch, w, h, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE + 7)
    everything = np.ones((h, w), bool)
    assert sp.differs_from_snapshot_of_its_count(sp.state(r), snaps, everything) is None  # the starting state is frames 0 .. count - 1 already
    for k in range(n):
        before = sp.state(r)
        pix, b, used = _check_shard_plan(r, before[1:], w, h, k, n, tc.SELECT, 7)
        assert len(pix) > 0
        r.render_budget(0, SEED, 4)
        after = sp.state(r)
        on = np.zeros(w * h, bool)
        on[pix] = True
        on = on.reshape(h, w)
        want = before[1].reshape(-1).copy()
        want[pix] += b
        assert np.array_equal(after[1].reshape(-1), want), k
        assert all(sp.same(x[~on], y[~on]) for x, y in zip(after, before)), "the pass of rank %d wrote an unlisted pixel" % k
        assert sp.differs_from_snapshot_of_its_count(after, snaps, everything) is None, k
    out = [C.c_int(-7), C.c_uint32(7), C.c_int(-7)]
    p = host_api.budget_params(dict(select=tc.SELECT, pass_cap=7))
    assert r.rt.rt_select_budget_rows(r.ctx, C.byref(p), 0, 1, h + 1, *(C.byref(o) for o in out)) == host_api.RT_E_ARG
    assert r.rt.rt_select_budget_rows(r.ctx, C.byref(p), 0, 1, 0, *(C.byref(o) for o in out)) == host_api.RT_E_ARG
    r.close()


# ---- 3. / 4. the gathers -------------------------------------------------------------------------------------------------------------------
GW, GH = 96, 61


@pytest.fixture()
def pair(scenes, host_api, monkeypatch):
    """A: frame 7 everywhere (its pixels are recognisable); B: cleared.  Both with statistics, the same scene, on device 0."""
    a = _renderer(host_api, scenes, monkeypatch, "mixed_small", GW, GH)
    b = _renderer(host_api, scenes, monkeypatch, "mixed_small", GW, GH)
    for r in (a, b):
        r.stats_enable(True)
        r.clear()
    a.render(host_api.RT_MODE_PATH, 7, 1)
    yield a, b
    a.close()
    b.close()


def test_gather_stats_rows(pair, scenes, host_api, monkeypatch):
    a, b = pair
    PATH = host_api.RT_MODE_PATH
    want = sp.state(a)
    assert np.all(want[1] == 1)
    for n in (2, 3):
        for k in range(n):
            first, stride, count = _shard(GH, k, n)
            b.clear()
            b.render_rows(PATH, 0, 3, first, stride, count)
            a.gather_stats_rows(b, first, stride, count)
            src = sp.state(b)
            rows = np.arange(k, GH, n)
            assert np.all(src[1][rows] == 3)
            for x, y in zip(want, src):
                x[rows] = y[rows]
            assert sp.same_state(sp.state(a), want), (n, k)
    # the other direction, on another shard: the way reprojected rows get back to their owner
    first, stride, count = _shard(GH, 3, 4)
    before = sp.state(b)
    b.gather_stats_rows(a, first, stride, count)
    rows = np.arange(3, GH, 4)
    for x, y in zip(before, want):
        x[rows] = y[rows]
    assert sp.same_state(sp.state(b), before) and sp.same_state(sp.state(a), want)
    # errors: reported on the source
    rt, E_ARG, E_STATE = a.rt, host_api.RT_E_ARG, host_api.RT_E_STATE
    assert rt.rt_gather_stats_rows(a.ctx, a.ctx, 0, 1, GH) == 0  # dst == src
    for rows in ((-1, 1, 1), (0, 0, 1), (0, 1, 0), (0, 1, GH + 1), (1, 2, GH // 2 + 1)):
        assert rt.rt_gather_stats_rows(a.ctx, b.ctx, *rows) == E_ARG and b"rt_gather_stats_rows: rows" in rt.rt_last_error(b.ctx), rows
    small = host_api.HostRenderer(64, 40)
    small.stats_enable(True)
    assert rt.rt_gather_stats_rows(a.ctx, small.ctx, 0, 1, 40) == E_ARG and b"differ in size" in rt.rt_last_error(small.ctx)
    assert rt.rt_gather_active(a.ctx, small.ctx) == E_ARG and b"differ in size" in rt.rt_last_error(small.ctx)
    small.close()
    b.stats_enable(False)
    assert rt.rt_gather_stats_rows(a.ctx, b.ctx, 0, 1, GH) == E_STATE and b"source" in rt.rt_last_error(b.ctx)
    assert rt.rt_gather_stats_rows(b.ctx, a.ctx, 0, 1, GH) == E_STATE and b"destination" in rt.rt_last_error(a.ctx)
    assert sp.same_state(sp.state(a), want)
    assert rt.rt_gather_rows(a.ctx, b.ctx, 0, 1, GH) == 0  # the accumulator alone needs no statistics, as ever
    assert sp.same(a.accumulator(), b.accumulator()) and all(sp.same(x, y) for x, y in zip(a.stats(), want[1:]))


def _lists(w, h):
    n = w * h
    out = [("pixel_0", np.array([0], np.uint32)), ("last_pixel", np.array([n - 1], np.uint32)), ("one_row", sh.last_row_list(w, h) - np.uint32(w * (h // 2)))]
    for length in (63, 64, 65, 255, 256, 257, 1025):
        full = sh.seeded_list(w, h, seed=length)
        assert len(full) >= length
        out.append(("seeded_%d" % length, full[np.linspace(0, len(full) - 1, length).astype(np.int64)]))
    out.append(("isolated", np.arange(2, n, 5, dtype=np.uint32)))  # w % 5 == 1: no listed pixel has a listed neighbour left, right, above or below
    return out


def test_gather_active(pair, scenes, host_api, monkeypatch):
    a, b = pair
    w, h = GW, GH
    assert w % 5 == 1
    want = sp.state(a)
    frame = 0
    for name, lst in _lists(w, h):
        assert sh.acceptable(lst, w * h) and len(lst) == len(np.unique(lst)), name
        b.set_active(lst)
        b.render_active(frame, 2)
        frame += 2
        a.gather_active(b)
        src = sp.state(b)
        on = np.zeros(w * h, bool)
        on[lst] = True
        on = on.reshape(h, w)
        assert np.all(src[1][on] >= 2)
        for x, y in zip(want, src):
            x[on] = y[on]
        assert sp.same_state(sp.state(a), want), name  # B's bits at the listed pixels, A's own everywhere else
    # after a budgeted pass on a shard: the plan is consumed, the list still serves
    first, stride, count = _shard(h, 1, 2)
    sel = dict(min_samples=8, max_samples=16, threshold=0.05, floor=1e-3)
    n, total, used = b.select_budget_rows(first, stride, count, dict(select=sel, pass_cap=3))
    lst = b.active()[0]
    assert n == len(lst) > 0 and total > n
    b.render_budget(100, SEED, 4)
    out, k = np.zeros(w * h, np.uint32), C.c_int(-1)
    assert b.rt.rt_download_budgets(b.ctx, out.ctypes.data_as(C.c_void_p), w * h, C.byref(k)) == host_api.RT_E_STATE
    assert np.array_equal(b.active()[0], lst)
    a.gather_active(b)
    src = sp.state(b)
    on = np.zeros(w * h, bool)
    on[lst] = True
    on = on.reshape(h, w)
    for x, y in zip(want, src):
        x[on] = y[on]
    assert sp.same_state(sp.state(a), want)
    # an empty list: RT_OK, nothing written; dst == src: RT_OK
    b.set_active(np.zeros(0, np.uint32))
    a.gather_active(b)
    a.set_active(np.array([5], np.uint32))
    a.gather_active(a)
    assert sp.same_state(sp.state(a), want)
    # no list on the source, statistics off on either side
    rt, E_STATE = a.rt, host_api.RT_E_STATE
    fresh = host_api.HostRenderer(w, h)
    fresh.stats_enable(True)
    assert rt.rt_gather_active(a.ctx, fresh.ctx) == E_STATE and b"no active-pixel list" in rt.rt_last_error(fresh.ctx)
    fresh.close()
    b.set_active(np.array([5], np.uint32))
    b.stats_enable(False)
    assert rt.rt_gather_active(a.ctx, b.ctx) == E_STATE and b"source" in rt.rt_last_error(b.ctx)
    assert rt.rt_gather_active(b.ctx, a.ctx) == E_STATE and b"destination" in rt.rt_last_error(a.ctx)
    assert sp.same_state(sp.state(a), want)


# ---- 5. Renderer::Tick ---------------------------------------------------------------------------------------------------------------------
TW, TH = 97, 41
RP = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=16, carry_view_dependent=0)
# (scene, its keywords, pass_cap, reproject, denoiseVariance)
TICK_CASES = [("mixed_small", {}, 0, False, False), ("mixed_small", {}, tc.LOOP_CAP, False, False),
              ("tlas_test2", {}, 0, False, False), ("tlas_test2", {}, tc.LOOP_CAP, False, False),
              ("scene3", dict(force_diffuse=True), 0, True, False), ("scene3", dict(force_diffuse=True), tc.LOOP_CAP, True, False),
              ("mixed_small", {}, tc.LOOP_CAP, False, True)]


def _tick_record(r):
    return (r.tick_accumulator(),) + tuple(r.stats()) + (r.tick_pixels(), r.active_pixels(), r.pass_samples(), r.carried_pixels(), r.iteration())


def _run_ticks(host_api, scenes, monkeypatch, case, devices):
    name, kw, cap, reproject, denoise_var = case
    r = _renderer(host_api, scenes, monkeypatch, name, TW, TH, devices=devices, **kw)
    r.set_adaptive(True, tc.LOOP)
    r.set_adaptive_budget(cap)
    if reproject:
        r.set_reproject(True, RP)
    if denoise_var:
        r.set_denoise_variance(True)
    out = []
    for t in range(7 if reproject else 8):
        if reproject and t == 4:
            r.set_camera(*(r.camera() + np.array((0.05, 0.0, 0.0), F32)).astype(F32))
        r.tick()
        out.append(_tick_record(r))
    r.close()
    return out


_ONE = {}


def _one_context(host_api, scenes, monkeypatch, case):
    key = (case[0],) + case[2:]
    if key not in _ONE:
        recs = _run_ticks(host_api, scenes, monkeypatch, case, None)
        # the run is worth comparing with: some Tick sampled a proper subset, the counts differ, and the carry carried
        assert any(0 < rec[5] < TW * TH for rec in recs), [rec[5] for rec in recs]
        assert len(np.unique(recs[-1][1])) > 1
        if case[3]:
            assert recs[4][7] > 0 and recs[4][8] == 1 and all(rec[7] == recs[4][7] for rec in recs[4:])
        _ONE[key] = recs
    return _ONE[key]


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0], [0, 1]], ids=lambda d: "-".join(map(str, d)))
def test_adaptive_ticks_over_several_contexts_equal_one_context(devices, scenes, host_api, monkeypatch):
    ndev = host_api.rt_lib().rt_device_count()
    if max(devices) >= ndev:
        pytest.skip("needs %d HIP devices, %d visible" % (max(devices) + 1, ndev))
    for case in TICK_CASES:
        one = _one_context(host_api, scenes, monkeypatch, case)
        many = _run_ticks(host_api, scenes, monkeypatch, case, devices)
        for t, (x, y) in enumerate(zip(one, many)):
            for k in range(5):  # the accumulator, count, sum_y, sum_yy of context 0, the pixels
                assert sp.same(x[k], y[k]), (case, t, k)
            assert x[5:] == y[5:], (case, t, x[5:], y[5:])  # activePixels, passSamples, carriedPixels, the iteration number
