"""Dilated adaptive selection on the device, through host_api (include/rt_amd.h rt_select_active_dilated / rt_select_budget_dilated):
  1. crafted masks at the sizes where the bitmasks' words, the row clip and the compaction take their other paths (tests/dilate_shapes.py,
     checked without a device by tests/test_dilate_cpu.py): the list must equal tests/dilate_ref.py on the DOWNLOADED statistics;
  2. real statistics with uneven counts, a light in view, two thresholds, radii 1 and 3;
  3. the budget form: list, budgets, total and cap used against the restatement, one forced halving, then rt_render_budget -- every listed
     pixel equals a second context's whole frames of its count, unlisted pixels are not written;
  4. the loop to termination at radius 0 and 2: the dilated counts dominate, no raw-active pixel is left, count alone decides a pixel;
  5. Renderer::Tick with adaptiveDilate against the same C-ABI calls by hand, the refused pair and the error cases;
  6. what the feature is for: pixels that stop at min_samples with a wrong mean, on the device's own samples.
Every comparison is exact: np.array_equal on integers, bitwise on floats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import adaptive_shapes as sh  # noqa: E402
import budget_shapes as tc  # noqa: E402
import dilate_ref as dr  # noqa: E402
import dilate_shapes as ds  # noqa: E402
import support as sp  # noqa: E402
from test_adaptive_cpu import QUALITY  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")
F32 = np.float32
SEED = 0x12345678
DIL_CRAFT = dict(min_samples=2, max_samples=3, threshold=INF, floor=1.0)


def _renderer(host_api, scenes, monkeypatch, name, w=97, h=41, devices=None):
    return sp.renderer(host_api, monkeypatch, getattr(scenes, name), w, h, devices=devices)


def _snapshots(host_api, scenes, monkeypatch, name, w, h, upto):
    return sp.snapshots(host_api, monkeypatch, name, getattr(scenes, name), w, h, upto)


def _uneven(r, host_api, w, h):
    """4 whole frames, then 3 more on a seeded 30 % list: counts 4 and 7, every pixel's sample k is frame k"""
    stats = sp.uneven(r, host_api, sh.seeded_list(w, h, seed=tc.UNEVEN_SEED))
    assert set(np.unique(stats[0])) == {tc.UNEVEN_WHOLE, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE}
    return stats


# ---- 1. crafted masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(ds.SIZES), ids=lambda s: "%dx%d" % s)
def test_dilation_of_crafted_masks(size, scenes, host_api, monkeypatch):
    """Every case of dilate_shapes.cases at the size, radii 0, 1, 2 and 16 (16 exceeds the small frames).  The statistics are crafted on
    the device: the complement of the sources gets frames 0 and 1, the 'stopped' pixels frame 2 as well, so under DIL_CRAFT raw = count < 2
    and eligible = count < 3 with finite sums.  The expected list is dilate_ref's on the downloaded statistics, so a pixel that views the
    light (+inf sums) is left out by the reference too.  One context per size; a case that fails is named, and the others still run."""
    w, h = size
    n, words, blocks, per = ds.geometry(w, h)
    assert ds.CRAFT == DIL_CRAFT and ds.RADII == (0, 1, 2, 16)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.stats_enable(True)
    bad = []
    reached_inf = reached_stopped = False
    for name, src, stopped in ds.cases(w, h):
        r.clear()
        r.set_active(ds.complement_list(src))
        r.render_active(0, 2)
        if stopped is not None:
            r.set_active(np.flatnonzero(stopped.reshape(-1)).astype(np.uint32))
            r.render_active(2, 1)
        cnt, sy, syy = r.stats()
        if not np.array_equal(cnt, ds.crafted_counts(src, stopped)):
            bad.append("%s: the crafted counts are not 0 on the sources, 3 on the stopped pixels and 2 elsewhere" % name)
            continue
        raw = ar.active_mask(cnt, sy, syy, **DIL_CRAFT)
        assert np.array_equal(raw, src)
        for radius in ds.RADII:
            want = dr.dilated_list(cnt, sy, syy, radius, **DIL_CRAFT)
            got_n = r.select_active_dilated(radius, DIL_CRAFT)
            got, n2 = r.active()
            if not (got_n == n2 == len(want) and np.array_equal(got, want)):
                k = min(len(got), len(want))
                first = np.flatnonzero(got[:k] != want[:k])
                bad.append("%s, radius %d: %d listed (download says %d) of %d wanted, first difference at entry %s" % (name, radius, got_n, n2, len(want), first[:1]))
                continue
            again_n = r.select_active_dilated(radius, DIL_CRAFT)  # once more on the same statistics: nothing the first call left is a starting point
            if not (again_n == len(want) and np.array_equal(r.active()[0], want)):
                bad.append("%s, radius %d: a second call gives %d pixels, or another list" % (name, radius, again_n))
            if radius == 0 and not (r.select_active(DIL_CRAFT) == len(want) and np.array_equal(r.active()[0], want)):
                bad.append("%s: radius 0 is not rt_select_active's list" % name)
            reach = dr.window_or(raw, radius) & ~raw
            reached_inf |= bool((reach & np.isposinf(sy)).any())
            reached_stopped |= bool((reach & (cnt == 3)).any())
    r.close()
    assert not bad, "\n".join(bad)
    if size == (97, 41):  # both ineligible classes lie where a source reaches: the lists above left them out because the device did
        assert reached_inf, "no source reaches a pixel that views the light"
        assert reached_stopped, "no source reaches a pixel at max_samples"


# ---- 2. real statistics --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(97, 41), (641, 409)], ids=lambda s: "%dx%d" % s)
def test_dilated_selection_equals_the_restatement_on_real_statistics(size, scenes, host_api, monkeypatch):
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    cnt, sy, syy = _uneven(r, host_api, w, h)
    assert np.isposinf(sy).any(), "no pixel views a light"
    grew = 0
    for threshold in (0.05, 0.2):
        sel = dict(min_samples=4, max_samples=1024, threshold=threshold, floor=1e-3)
        raw = ar.active_list(cnt, sy, syy, **sel)
        assert 0 < len(raw) < w * h
        for radius in (1, 3):
            want = dr.dilated_list(cnt, sy, syy, radius, **sel)
            k = r.select_active_dilated(radius, sel)
            got, k2 = r.active()
            print("%dx%d threshold %.2f radius %d: %d raw-active, %d listed of %d" % (w, h, threshold, radius, len(raw), len(want), w * h))
            assert k == k2 == len(want), (threshold, radius, k, k2, len(want))
            assert np.array_equal(got, want), (threshold, radius)
            grew += len(want) > len(raw)
    assert grew == 4  # the dilation lists pixels the predicate alone does not, at every setting
    r.close()


# ---- 3. the budget form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(97, 41), (257, 3)], ids=lambda s: "%dx%d" % s)
def test_dilated_budgets_and_their_pass(size, scenes, host_api, monkeypatch):
    """sel A: min_samples 4 -- raw-active pixels are the noisy ones; sel B: min_samples 6 -- the pixels at count 4 are below min_samples (budget
    2).  pass_cap 7; the limit 'total at cap 3', below the total at cap 7, forces exactly one halving."""
    w, h = size
    cap = 7
    snaps = _snapshots(host_api, scenes, monkeypatch, "mixed_small", w, h, 7 + cap)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    for sel in (dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3), dict(min_samples=6, max_samples=64, threshold=0.05, floor=1e-3)):
        for radius in (1, 3):
            cnt, sy, syy = _uneven(r, host_api, w, h)
            raw = ar.active_mask(cnt, sy, syy, **sel)
            for mps in (0, None):
                if mps is None:
                    mps = int(dr.dilated_budgets(cnt, sy, syy, cap >> 1, radius, **sel).sum())
                    assert mps < int(dr.dilated_budgets(cnt, sy, syy, cap, radius, **sel).sum()), "no budget above cap / 2: nothing to halve"
                lst, b, total, used = dr.plan(cnt, sy, syy, radius, cap, mps, **sel)
                assert b is not None and used == (cap if mps == 0 else cap >> 1), (mps, used)
                got = r.select_budget_dilated(radius, dict(select=sel, pass_cap=cap, max_pass_samples=mps))
                got_lst, n2 = r.active()
                got_b, n3 = r.budgets()
                assert got == (len(lst), total, used) and n2 == n3 == len(lst), (sel, radius, mps, got, len(lst), total, used)
                assert np.array_equal(got_lst, lst) and np.array_equal(got_b, b), (sel, radius, mps)
                only = ~raw.reshape(-1)[lst]
                assert only.any() and (~only).any() and (b[only] == 1).all() and b.max() > 1  # both kinds of entry are there
            # the pass of the halved plan: listed pixels move by their budgets and equal whole frames of their count; the rest is not written
            before = sp.state(r)
            r.render_budget(0, SEED, 4)
            after = sp.state(r)
            listed = np.zeros(w * h, bool)
            listed[lst] = True
            listed = listed.reshape(h, w)
            moved = cnt.reshape(-1).copy()
            moved[lst] += b
            assert np.array_equal(after[1].reshape(-1), moved)
            assert all(sp.same(x[~listed], y[~listed]) for x, y in zip(after, before)), "an unlisted pixel was written"
            assert sp.differs_from_snapshot_of_its_count(after, snaps, listed) is None
            assert sp.differs_from_snapshot_of_its_count(after, snaps) is None
    r.close()


def test_dilated_budgets_that_do_not_fit(scenes, host_api, monkeypatch):
    w, h = 97, 41
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    sel = dict(min_samples=4, max_samples=64, threshold=0.1, floor=1e-3)
    cnt, sy, syy = _uneven(r, host_api, w, h)
    lst = dr.dilated_list(cnt, sy, syy, 2, **sel)
    p = host_api.budget_params(dict(select=sel, pass_cap=7, max_pass_samples=len(lst) - 1))
    n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
    assert r.rt.rt_select_budget_dilated(r.ctx, C.byref(p), 2, C.byref(n), C.byref(total), C.byref(cap)) == host_api.RT_E_UNSUPPORTED
    assert n.value == len(lst) and (total.value, cap.value) == (7, -7)
    assert np.array_equal(r.active()[0], lst)                      # the list stays installed, for rt_render_active
    assert r.rt.rt_render_budget(r.ctx, 0, SEED, 4) == host_api.RT_E_STATE  # ... without a plan
    r.close()


# ---- 4. loops ------------------------------------------------------------------------------------------------------------------------
def test_dilated_loop_dominates_and_count_decides(scenes, host_api, monkeypatch):
    """Passes of one sample per listed pixel (pass_cap 1: a pixel's k-th sample is frame k) from rt_clear until nothing is listed, at
    radius 0 and radius 2, max_samples 24.  A pixel's state is a function of its count and it is listed at least as long as it is
    raw-active, so count(radius 2) >= count(radius 0) everywhere; the loop ends on an empty list, which is an empty raw list."""
    w, h = 97, 41
    sel = dict(min_samples=4, max_samples=24, threshold=0.05, floor=1e-3)
    snaps = _snapshots(host_api, scenes, monkeypatch, "mixed_small", w, h, sel["max_samples"])
    counts = {}
    for radius in (0, 2):
        r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
        r.stats_enable(True)
        r.clear()
        passes = 0
        while True:
            n, total, used = r.select_budget_dilated(radius, dict(select=sel, pass_cap=1))
            if n == 0:
                break
            assert total == n and used == 1 and passes < sel["max_samples"], "the loop must end within max_samples passes"
            r.render_budget(0, SEED, 4)
            passes += 1
        assert r.select_active(sel) == 0                           # no raw-active pixel is left
        state = sp.state(r)
        assert sp.differs_from_snapshot_of_its_count(state, snaps) is None
        counts[radius] = state[1]
        assert state[1].min() >= sel["min_samples"] and state[1].max() <= sel["max_samples"]
        r.close()
    assert (counts[2] >= counts[0]).all()
    assert (counts[2] > counts[0]).any() and len(np.unique(counts[0])) > 3
    print("samples to termination: radius 0 %d, radius 2 %d" % (counts[0].sum(), counts[2].sum()))


# ---- 5. Renderer::Tick, state and errors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 5], ids=lambda c: "pass_cap_%d" % c)
def test_tick_with_adaptive_dilate_equals_the_calls_by_hand(cap, scenes, host_api, monkeypatch):
    w, h, radius = 97, 41, 2
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.set_adaptive(True, P)
    r.set_adaptive_budget(cap)
    r.set_adaptive_dilate(radius)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    hand.set_camera(*r.camera())
    hand.stats_enable(True)
    hand.clear()
    grew = False
    for t in range(9):
        r.tick()
        if cap:
            n, total, used = hand.select_budget_dilated(radius, dict(select=P, pass_cap=cap))
            hand.render_budget(0, SEED, 4)
            assert used == cap
        elif t < P["min_samples"]:
            hand.render(host_api.RT_MODE_PATH, t, 1)
            n = total = w * h
        else:
            grew |= hand.select_active(P) < hand.select_active_dilated(radius, P)
            n = total = hand.select_active_dilated(radius, P)
            hand.render_active(t, 1)
        assert (r.active_pixels(), r.pass_samples()) == (n, total), t
        assert sp.same(r.tick_accumulator(), hand.accumulator()) and sp.same_state(sp.state(r), sp.state(hand)), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
    assert cap or grew
    r.close()
    hand.close()


def test_tick_with_adaptive_dilate_0_is_the_tick_of_before(scenes, host_api, monkeypatch):
    w, h = 97, 41
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    for cap in (0, 5):
        r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
        r.set_adaptive(True, P)
        r.set_adaptive_budget(cap)
        r.set_adaptive_dilate(3)
        r.set_adaptive_dilate(0)
        hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
        hand.set_camera(*r.camera())
        hand.stats_enable(True)
        hand.clear()
        for t in range(7):
            r.tick()
            if cap:
                n = hand.select_budget(dict(select=P, pass_cap=cap))[0]
                hand.render_budget(0, SEED, 4)
            elif t < P["min_samples"]:
                hand.render(host_api.RT_MODE_PATH, t, 1)
                n = w * h
            else:
                n = hand.select_active(P)
                hand.render_active(t, 1)
            assert r.active_pixels() == n, (cap, t)
            assert sp.same_state(sp.state(r), sp.state(hand)), (cap, t)
        r.close()
        hand.close()


def test_tick_with_adaptive_dilate_on_several_contexts_throws(scenes, host_api, monkeypatch):
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=97, h=41, devices=[0, 0])
    r.set_adaptive(True, dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3))
    r.set_adaptive_dilate(1)
    with pytest.raises(RuntimeError, match="adaptiveDilate"):
        r.tick()
    r.set_adaptive_dilate(0)
    r.tick()  # the pair alone is refused
    r.close()


def test_dilated_state_and_errors(scenes, host_api, monkeypatch):
    w, h = 96, 64
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    L, ctx = r.rt, r.ctx
    ARG, STATE = host_api.RT_E_ARG, host_api.RT_E_STATE
    n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
    sel0 = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)

    def act(select=None, radius=1, out=C.byref(n), c=ctx):
        p = host_api.adaptive_params(dict(sel0, **(select or {})))
        return L.rt_select_active_dilated(c, C.byref(p), radius, out)

    def bud(select=None, radius=1, pass_cap=7, outs=None, c=ctx):
        p = host_api.budget_params(dict(select=dict(sel0, **(select or {})), pass_cap=pass_cap))
        a, b, d = outs or (C.byref(n), C.byref(total), C.byref(cap))
        return L.rt_select_budget_dilated(c, C.byref(p), radius, a, b, d)

    # statistics off
    assert act() == STATE and bud() == STATE
    # the arguments are checked before the context's state: bad ones are RT_E_ARG with statistics off too
    assert act(radius=-1) == ARG and bud(radius=17) == ARG and act(dict(min_samples=1)) == ARG
    r.stats_enable(True)
    r.render(host_api.RT_MODE_PATH, 0, 5)
    for bad in (dict(min_samples=1), dict(min_samples=0), dict(min_samples=8, max_samples=7), dict(threshold=float("nan")), dict(threshold=-0.5),
                dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan"))):
        assert act(bad) == ARG and bud(bad) == ARG, bad
    for bad in (-1, 17, 2 ** 20, -2 ** 31):
        assert act(radius=bad) == ARG and bud(radius=bad) == ARG, bad
    for bad in (0, -1, 1025):
        assert bud(pass_cap=bad) == ARG, bad
    assert act(out=None) == ARG and act(c=None) == ARG and bud(c=None) == ARG
    assert bud(outs=(None, C.byref(total), C.byref(cap))) == ARG and bud(outs=(C.byref(n), None, C.byref(cap))) == ARG and bud(outs=(C.byref(n), C.byref(total), None)) == ARG
    assert (n.value, total.value, cap.value) == (-7, 7, -7)
    buf = np.zeros(w * h, np.uint32)
    assert L.rt_download_active(ctx, buf.ctypes.data_as(C.c_void_p), w * h, C.byref(n)) == STATE  # a refused call installs nothing
    # the edges of the radius
    assert act(radius=0) == 0 and act(radius=16) == 0 and bud(radius=0) == 0 and bud(radius=16) == 0
    # the library's defaults when params is NULL
    cnt, sy, syy = r.stats()
    assert r.select_active_dilated(2, None) == len(dr.dilated_list(cnt, sy, syy, 2, **ar.DEFAULTS))
    want = dr.plan(cnt, sy, syy, 2, 64, 0, **ar.DEFAULTS)
    assert r.select_budget_dilated(2, None) == (len(want[0]), want[2], 64) and np.array_equal(r.budgets()[0], want[1])
    # both calls drop a plan; the budget form installs one, and the undilated selection drops it
    assert bud() == 0 and act() == 0 and L.rt_render_budget(ctx, 0, SEED, 4) == STATE
    assert bud() == 0 and r.select_active(sel0) >= 0 and L.rt_render_budget(ctx, 0, SEED, 4) == STATE
    assert bud() == 0 and L.rt_render_budget(ctx, 0, SEED, 4) == 0 and L.rt_render_budget(ctx, 0, SEED, 4) == STATE
    # profiling: each call is one entry of rt_profile.query
    r.set_profiling(True)
    r.profile(reset=True)
    assert act() == 0
    assert r.profile(reset=True)["query"]["launches"] == 1
    assert bud() == 0
    assert r.profile(reset=True)["query"]["launches"] == 1
    r.set_profiling(False)
    r.close()


# ---- 6. what it is for -----------------------------------------------------------------------------------------------------------------
def test_dilation_rescues_pixels_that_stopped_wrong(scenes, host_api, monkeypatch):
    """The stopped-and-wrong count of tests/test_dilate_cpu.py on the device's own samples: QUALITY's scene (config 2) at 320 x 180, 16
    samples per pixel, then passes of one sample per listed pixel at threshold 0.02 until the next would pass 32 frames' worth; against the
    device's own 256-frame mean (frames 1000 .. 1255).  A pixel counts when reference and both accumulators are finite, its count is 16 and
    max_c |mean - ref| / max(max_c ref, 1e-3) > 0.1.  Asserted: undilated >= 8 and 4 * dilated(radius 1) <= undilated (the oracle's
    samples give 20 and 0).  Measured on an MI355X: 21 undilated, 0 at radius 1 (1,840,125 and 1,842,597 of 1,843,200 samples, MSE of the
    dilated run 0.984 of the undilated one's, 38,981 finite pixels; DESIGN.md section 7, "Dilated adaptive selection")."""
    q = QUALITY
    w, h, P = q["width"], q["height"], q["params"]
    budget = q["budget_frames"] * w * h
    r = _renderer(host_api, scenes, monkeypatch, q["scene"], w=w, h=h)
    r.clear()
    r.render(host_api.RT_MODE_PATH, q["reference_frame0"], q["reference_frames"])
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
    r.stats_enable(True)
    runs = {}
    for radius in (0, 1):
        r.clear()
        total = 0
        while True:
            n, taken, used = r.select_budget_dilated(radius, dict(select=P, pass_cap=1))
            if n == 0 or total + n > budget:
                break
            r.render_budget(0, SEED, 4)
            total += n
        cnt = r.stats()[0]
        assert int(cnt.sum(dtype=np.int64)) == total <= budget
        runs[radius] = (r.accumulator()[..., :3].astype(np.float64), cnt, total)
    r.close()
    fin = np.isfinite(ref).all(-1) & np.isfinite(runs[0][0]).all(-1) & np.isfinite(runs[1][0]).all(-1)
    wrong, mse = {}, {}
    for radius, (acc, cnt, total) in runs.items():
        with np.errstate(all="ignore"):
            mean = acc / cnt[..., None]
            off = np.abs(mean - ref).max(-1) / np.maximum(ref.max(-1), 1e-3)
        wrong[radius] = int((fin & (cnt == P["min_samples"]) & (off > 0.1)).sum())
        mse[radius] = float(((mean[fin] - ref[fin]) ** 2).mean())
    print("device stopped and wrong: undilated %d, radius 1 %d; samples %d / %d of %d; MSE radius 1 / undilated %.3f; %d finite pixels"
          % (wrong[0], wrong[1], runs[0][2], runs[1][2], budget, mse[1] / mse[0], fin.sum()))
    assert wrong[0] >= 8, wrong
    assert 4 * wrong[1] <= wrong[0], wrong
