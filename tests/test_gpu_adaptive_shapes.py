"""Adaptive sampling on the device at the sizes and lists where its kernels take their other paths (tests/adaptive_shapes.py lists them
and tests/test_adaptive_cpu.py checks the lists without a device):
  1. the compaction of rt_select_active (k_select_count / k_select_scan / k_select_scatter) on crafted masks, at ragged frames, frames of
     one lane / wave / block and frames with more blocks than the scan has lanes -- the list must be np.flatnonzero of the mask;
  2. the predicate at ragged and large frames against its numpy restatement (tests/adaptive_ref.py), on statistics with uneven counts;
  3. rt_render_active against rt_render bit for bit with fewer slots than samples, calls cut into several batches, the wide any-hit
     walks, list lengths at the wave and block edges of k_accumulate<true>'s grid, lists of frame-edge pixels, a large frame0;
  4. rt_resolve_adaptive at ragged frames and row ranges;
  5. Renderer::Tick's adaptive mode at a ragged frame.
Every comparison is exact: np.array_equal on the integer lists and counts, bitwise on the floats."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import adaptive_shapes as sh  # noqa: E402
import support as sp  # noqa: E402

pytestmark = pytest.mark.gpu

INF = float("inf")


def _renderer(host_api, scenes, monkeypatch, name, env=None, w=97, h=41):
    return sp.renderer(host_api, monkeypatch, getattr(scenes, name), w, h, env, path_ticks=False)


# ---- 1. crafted masks through the compaction ---------------------------------------------------------------------------------------
def _select_mask(r, M):
    """count 2 off the mask and 0 on it, then the selection under which exactly the pixels without samples are active"""
    r.clear()
    r.set_active(sh.complement_list(M))
    r.render_active(0, 2)
    return r.select_active(sh.CRAFT)


@pytest.mark.parametrize("size", list(sh.SIZES), ids=lambda s: "%dx%d" % s)
def test_selection_of_crafted_masks(size, scenes, host_api, monkeypatch):
    """Every mask of adaptive_shapes.MASKS that is not degenerate at the size, all of them at the two largest sizes too.  One context per
    size; a mask that fails is named with what differed, and the others still run."""
    w, h = size
    n, blocks, per = sh.SIZES[size]
    # the edges this size is here for, from this file's own arithmetic: a change of the library's block sizes must show here
    assert n == w * h and blocks == -(-n // 256) and per == -(-blocks // 1024), "the size no longer reaches the edge it is listed for"
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.stats_enable(True)
    cases = sh.masks(w, h)
    names = [name for name, _ in cases]
    assert names[:2] == ["all", "none"]
    if per > 1:
        assert {"last_block", "alternate_blocks", "seeded_30", "seeded_01", "full_to_1023", "full_from_1024", "scan_lane_mid", "scan_lane_last"} <= set(names)
    bad = []
    for name, M in cases:
        want = np.flatnonzero(M).astype(np.uint32)
        k = len(want)
        got_n = _select_mask(r, M)
        cnt = r.stats()[0].reshape(-1)
        if not np.array_equal(cnt, np.where(M, 0, 2)):
            bad.append("%s: the counts rt_render_active left are not 2 off the mask and 0 on it" % name)
            continue
        got, n2 = r.active()
        if not (got_n == n2 == k and np.array_equal(got, want)):
            first = np.flatnonzero(got[:min(len(got), k)] != want[:min(len(got), k)])
            bad.append("%s: %d selected (download says %d) of %d wanted, first difference at entry %s" % (name, got_n, n2, k, first[:1]))
            continue
        # a prefix: the entries that fit and the list's true length
        short, n3 = r.active(cap=k // 2)
        if not (n3 == k and np.array_equal(short, want[:k // 2])):
            bad.append("%s: the prefix of %d entries" % (name, k // 2))
        # once more on the same statistics: the block totals the scan left in place are not a starting point
        again_n = r.select_active(sh.CRAFT)
        again, _ = r.active()
        if not (again_n == k and np.array_equal(again, want)):
            bad.append("%s: a second selection gives %d pixels, or another list" % (name, again_n))
        if name == "none":
            before = sp.state(r)
            r.render_active(2, 1)  # nothing selected: nothing rendered
            if not (r.active()[1] == 0 and all(sp.same(x, y) for x, y in zip(sp.state(r), before))):
                bad.append("none: rt_render_active over an empty selection touched the frame")
    r.close()
    assert not bad, "\n".join(bad)


# ---- 2. the predicate at ragged and large sizes ------------------------------------------------------------------------------------
# Measured on the oracle's samples of the same frames (7 frames, the lists below), pixels of each class; the device's frames agree with
# the oracle's to 1e-4, so classes of hundreds of pixels hold on the device as well:
#                            +inf sum_y     v <= 0     mean < 0.5    mean > 0.5   (uneven / sparse statistics)
#   mixed_small  97 x 41      166 / 60    1158 / 242    353 / 99     3439 / 1018
#   mixed_small 641 x 409   11488 / 4439  114042 / 27071 36306 / 10667 212539 / 63363
#   tlas_test2   97 x 41      217 / 89     162 / 33     502 / 145    3023 / 881
#   tlas_test2  641 x 409   16159 / 6142  49011 / 12607 46497 / 13379 177795 / 53020
#   257 x 3 (a strip across the middle of the view): v <= 0 on 326 / 121 and 230 / 38 pixels, no light in view and at most two means
#   below 0.5 -- so at 257 x 3 the +inf and below-the-floor classes are not asserted, the others are.  No mean is below 1e-3 anywhere:
#   "below the floor" is held by the floor of 0.5, "above" by both floors.
WITH_LIGHT_AND_DARK = ((97, 41), (641, 409))


def _classes(cnt, sy, syy):
    with np.errstate(all="ignore"):
        n = cnt.astype(np.float32)
        m = (sy / n).astype(np.float32)
        v = ((syy - (sy * m).astype(np.float32)).astype(np.float32) / (n - np.float32(1))).astype(np.float32)
    fin = np.isfinite(sy) & np.isfinite(syy) & (cnt >= 2)
    return m, v, fin


@pytest.mark.parametrize("state", ["uneven", "sparse"])
@pytest.mark.parametrize("size", [(97, 41), (257, 3), (641, 409)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_selection_equals_the_restatement_at_ragged_sizes(name, size, state, scenes, host_api, monkeypatch):
    """uneven: 4 whole frames, then 3 more on a seeded 30 % list -- counts 4 and 7.  sparse: from clear, one frame on a seeded 60 % list,
    then 4 more on every other entry of it -- counts 0, 1 and 5.  The conditions on the inputs that held (and are asserted): see the
    table above; the mid threshold 0.05 selects some but not all of the sampled pixels at every size, scene and state."""
    w, h = size
    n = w * h
    PATH = host_api.RT_MODE_PATH
    r = _renderer(host_api, scenes, monkeypatch, name, w=w, h=h)
    r.stats_enable(True)
    r.clear()
    if state == "uneven":
        r.render(PATH, 0, 4)
        r.set_active(sh.seeded_list(w, h, seed=9))
        r.render_active(4, 3)
        lo, hi = 4, 7
    else:
        lst = sh.seeded_list(w, h, seed=11, density=0.6)
        r.set_active(lst)
        r.render_active(0, 1)
        r.set_active(lst[::2])
        r.render_active(1, 4)
        lo, hi = 1, 5
    cnt, sy, syy = r.stats()
    assert set(np.unique(cnt)) == ({4, 7} if state == "uneven" else {0, 1, 5})
    m, v, fin = _classes(cnt, sy, syy)
    # the classes the parameter sets below are there for
    assert (fin & (v <= 0)).any(), "no pixel whose variance is clamped at 0"
    assert (fin & (m > 0.5)).any()
    if size in WITH_LIGHT_AND_DARK:
        assert np.isposinf(sy).any() and np.isposinf(sy[cnt >= 2]).any(), "no pixel views a light"
        assert (fin & (m < 0.5)).any(), "no mean below the floor of 0.5"
    sampled = cnt >= 2

    def check(P):
        want = ar.active_list(cnt, sy, syy, **P)
        k = r.select_active(P)
        got, k2 = r.active()
        assert k == k2 == len(want), (P, k, k2, len(want))
        assert np.array_equal(got, want), P
        return want

    base = dict(min_samples=2, max_samples=1024, threshold=0.05, floor=1e-3)
    # a mid threshold, the small floor and the floor of 0.5: some of the sampled pixels, not all
    for floor in (1e-3, 0.5):
        got = check(dict(base, floor=floor))
        k = int(sampled.reshape(-1)[got].sum())
        assert 0 < k < int((sampled & fin).sum()), (floor, k)
        assert 0 < len(got) < n
    if size in WITH_LIGHT_AND_DARK:  # the floor of 0.5 is the denominator somewhere: it takes pixels out
        assert len(check(dict(base, floor=0.5))) < len(check(base))
    # threshold 0: every finite sampled pixel below max_samples whose variance is above 0 (and every pixel below min_samples)
    noisy = fin & (ar.relative_error(cnt, sy, syy, 1e-3) > 0)
    got = check(dict(base, threshold=0.0))
    assert np.array_equal(got, np.flatnonzero(((cnt < 2) | noisy).reshape(-1)))
    assert not (noisy & (v <= 0)).any()  # a variance clamped at 0 is no error at all
    # threshold +inf: count < min_samples alone -- at 0 and 1 (sparse), at min_samples - 1, at min_samples
    for mn in (2, lo + 1, hi, hi + 1):
        got = check(dict(base, min_samples=mn, max_samples=max(mn, 1024), threshold=INF))
        assert np.array_equal(got, np.flatnonzero((cnt < mn).reshape(-1))), mn
    assert len(check(dict(base, min_samples=hi + 1, threshold=INF))) == n
    # count == max_samples: the pixels at 'hi' are out whatever their error, the others are judged
    got = check(dict(base, max_samples=hi, threshold=0.0))
    assert np.array_equal(got, np.flatnonzero(((cnt < 2) | (noisy & (cnt < hi))).reshape(-1)))
    assert not (cnt.reshape(-1)[got] == hi).any() and (cnt.reshape(-1)[got] == lo).any()
    # the crafting parameters of section 1 on rendered statistics: the pixels without two samples
    assert np.array_equal(check(sh.CRAFT), np.flatnonzero((cnt < 2).reshape(-1)))
    r.close()


# ---- 3. rt_render_active under every schedule --------------------------------------------------------------------------------------
WARM = 2     # whole frames under the list's frames: "untouched" is then a value, not zero
_reference = {}


def _whole_frames(host_api, scenes, monkeypatch, name, w, h, frame0, nframes):
    """rt_render at default knobs, once per (scene, size, frames): the state after WARM whole frames 0 .. WARM - 1, and after the
    frames [frame0, frame0 + nframes) on top of them.  Shared by the cases below and never written to."""
    key = (name, w, h, frame0, nframes)
    if key not in _reference:
        r = _renderer(host_api, scenes, monkeypatch, name, w=w, h=h)
        r.stats_enable(True)
        r.clear()
        r.render(host_api.RT_MODE_PATH, 0, WARM)
        warm = sp.state(r)
        r.render(host_api.RT_MODE_PATH, frame0, nframes)
        _reference[key] = (warm, sp.state(r))
        r.close()
        for a in warm + _reference[key][1]:
            a.setflags(write=False)
    return _reference[key]


def _check_listed(host_api, scenes, monkeypatch, name, env, w, h, lst, frame0=WARM, nframes=4):
    """The invariant of rt_render_active: after it, the listed pixels hold the bits rt_render of the same frames leaves (accumulator,
    count, sum_y, sum_yy), and every other pixel is untouched."""
    warm, full = _whole_frames(host_api, scenes, monkeypatch, name, w, h, frame0, nframes)
    r = _renderer(host_api, scenes, monkeypatch, name, env, w=w, h=h)
    r.stats_enable(True)
    r.clear()
    r.render(host_api.RT_MODE_PATH, 0, WARM)
    assert all(sp.same(x, y) for x, y in zip(sp.state(r), warm)), "the whole frames under the list differ under %s" % (env,)
    r.set_active(lst)
    r.render_active(frame0, nframes)
    got = sp.state(r)
    r.close()
    on = np.zeros(w * h, bool)
    on[lst] = True
    on = on.reshape(h, w)
    for what, g, f, b in zip(("accumulator", "count", "sum_y", "sum_yy"), got, full, warm):
        assert sp.same(g[on], f[on]), "%s of the listed pixels" % what
        assert sp.same(g[~on], b[~on]), "%s of a pixel that is not listed" % what
    assert np.all(got[1][on] == WARM + nframes) and np.all(got[1][~on] == WARM)


SHAPES = [(97, 41), (96, 64)]


@pytest.mark.parametrize("slots,nframes", [("777", 4), ("2000", 4), ("4096", 4), ("2000", 7), ("4096", 7)])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_render_active_with_fewer_slots_and_in_batches(name, size, slots, nframes, scenes, host_api, monkeypatch):
    """RT_SLOTS=777: fewer slots than listed pixels, one batch whose slots k_finish hands on.  2000: one frame of the list fits, four do
    not -- render_batches cuts the call into one-frame batches.  4096: two (96 x 64) or three (97 x 41) frames per batch, so 4 frames
    are 2 + 2 or 3 + 1 and 7 frames end on a short batch; the statistics are fed in frame order whatever the cut."""
    w, h = size
    lst = sh.seeded_list(w, h)
    k = len(lst)
    assert 0.25 < k / (w * h) < 0.35
    branch, per_batch = sh.slots_branch(int(slots), k, nframes)
    if slots == "777":
        assert branch == "recycle" and k > 777
    elif slots == "2000":
        assert branch == "own" and per_batch == 1 and k <= 2000 < 2 * k
    else:
        assert branch == "own" and per_batch == 4096 // k == (2 if size == (96, 64) else 3)
        assert 1 < per_batch < nframes and (nframes == 4 or nframes % per_batch != 0)
    _check_listed(host_api, scenes, monkeypatch, name, {"RT_SLOTS": slots}, w, h, lst, nframes=nframes)


@pytest.mark.parametrize("env", [{"RT_WIDE": "1"}, {"RT_WIDE8": "1"}, {"RT_WIDE": "1", "RT_STREAM": "0"}], ids=sp.env_id)
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_render_active_with_the_wide_walks(name, size, env, scenes, host_api, monkeypatch):
    w, h = size
    _check_listed(host_api, scenes, monkeypatch, name, env, w, h, sh.seeded_list(w, h))


@pytest.mark.parametrize("length,env", [(k, {}) for k in (1, 63, 64, 65, 255, 256, 257, 1025)] + [(k, {"RT_STREAM": "0"}) for k in (63, 65, 257)],
                         ids=lambda v: sp.env_id(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
def test_render_active_list_lengths(size, length, env, scenes, host_api, monkeypatch):
    """the first 'length' entries of the seeded list: the wave and block edges of k_accumulate<true>'s grid over the list"""
    w, h = size
    lst = sh.seeded_list(w, h)
    assert len(lst) >= length
    _check_listed(host_api, scenes, monkeypatch, "mixed_small", env, w, h, lst[:length])


@pytest.mark.parametrize("which", ["last_row", "side_columns"])
@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_render_active_frame_edge_lists(name, size, which, scenes, host_api, monkeypatch):
    """only the last row; only column 0 and column w - 1: their jittered samples reach past the frame in the primary-hit table"""
    w, h = size
    lst = sh.last_row_list(w, h) if which == "last_row" else sh.side_columns_list(w, h)
    assert sh.acceptable(lst, w * h)
    _check_listed(host_api, scenes, monkeypatch, name, {}, w, h, lst)


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["mixed_small", "tlas_test2"])
def test_render_active_at_a_large_frame0(name, size, scenes, host_api, monkeypatch):
    w, h = size
    _check_listed(host_api, scenes, monkeypatch, name, {}, w, h, sh.seeded_list(w, h), frame0=1000, nframes=3)


# ---- 4. rt_resolve_adaptive --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(257, 3), (97, 41)], ids=lambda s: "%dx%d" % s)
def test_resolve_adaptive_at_ragged_sizes(size, scenes, host_api, monkeypatch):
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.stats_enable(True)
    lst = sh.seeded_list(w, h, density=0.6)
    r.clear()
    r.set_active(lst)
    r.render_active(0, 3)
    r.set_active(lst[::2])
    r.render_active(3, 4)
    cnt = r.stats()[0]
    assert set(np.unique(cnt)) == {0, 3, 7}
    want = ar.resolve(r.accumulator(), cnt)
    got = r.resolve_adaptive()
    assert np.array_equal(got, want)
    assert np.all(got[cnt == 0] == 0) and got[cnt == 3].any() and got[cnt == 7].any()
    for y0, y1 in ((0, 1), (h - 1, h), (h // 3, h - h // 3)):
        assert 0 <= y0 < y1 <= h
        assert np.array_equal(r.resolve_adaptive(y0, y1), want[y0:y1]), (y0, y1)
    r.close()


# ---- 5. Renderer::Tick -------------------------------------------------------------------------------------------------------------
def test_tick_adaptive_equals_the_loop_by_hand_at_a_ragged_size(scenes, host_api, monkeypatch):
    w, h = 97, 41
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    r = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    r.scene.set_raytracer(False)  # Tick renders path frames
    r.set_adaptive(True, P)
    hand = _renderer(host_api, scenes, monkeypatch, "mixed_small", w=w, h=h)
    c = r.camera()
    hand.set_camera(c[0], c[1], c[2], c[3])
    hand.stats_enable(True)
    hand.clear()
    active, rendered = [], 0
    for t in range(8):
        r.tick()
        if t < P["min_samples"]:
            hand.render(host_api.RT_MODE_PATH, t, 1)
            k = w * h
        else:
            k = hand.select_active(P)
            hand.render_active(t, 1)
        assert r.active_pixels() == k, t
        active.append(k)
        rendered += k
        assert sp.same(r.tick_accumulator(), hand.accumulator()), t
        assert all(sp.same(x, y) for x, y in zip(r.stats(), hand.stats())), t
        assert np.array_equal(r.tick_pixels(), hand.resolve_adaptive()), t
    tail = active[P["min_samples"]:]
    assert all(b <= a for a, b in zip(tail, tail[1:])), active  # a static camera: pixels only ever leave the active set
    assert 0 < tail[0] < w * h
    assert int(r.stats()[0].sum(dtype=np.int64)) == rendered
    r.close()
    hand.close()
