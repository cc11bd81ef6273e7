"""The six selections of include/rt_amd.h are one list skeleton and one plan skeleton over two lane sources (a row set, the dilated masks).
Through host_api, on uneven statistics, every comparison exact:
  1. the whole frame through each source: rt_select_active / rt_select_active_rows(0, 1, h) / rt_select_active_dilated(radius 0) leave one
     list, rt_select_budget / rt_select_budget_rows(0, 1, h) / rt_select_budget_dilated(radius 0) one result, list and budgets -- those of
     tests/adaptive_ref.py and tests/budget_ref.py -- with and without a halving of the fit rule, at the sizes where the compaction
     takes its other paths;
  2. which calls are an entry of rt_profile.query with rt_set_profiling on (rt_select_budget and rt_select_budget_rows are none, on purpose:
     profiles/dilate_bench.py relies on it);
  3. a selection that does not fit, through both sources: the list alone is installed."""
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
import dilate_ref as dr  # noqa: E402
import support as sp  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x12345678
CAP = 7
NOISY = dict(min_samples=4, max_samples=64, threshold=0.1, floor=1e-3)  # both counts are at min_samples: the raw list is the noisy pixels
SIZES = {(1, 1): "one lane", (65, 1): "a wave and a lane", (257, 3): "a block and a lane, rows across blocks", (97, 41): "ragged, several blocks"}


def _renderer(host_api, scenes, monkeypatch, w, h):
    return sp.renderer(host_api, monkeypatch, scenes.mixed_small, w, h, scene_camera=False)


def _more_list(w, h):
    """the pixels that get the three extra frames: test_gpu_budget.py's seeded list; a frame of one row (where that list is the whole
    frame: its complete row) gets the two end pixels and a seeded 30 % of the rest, so that a wave holds both counts"""
    if h > 1:
        return sh.seeded_list(w, h, seed=tc.UNEVEN_SEED)
    on = np.random.default_rng(tc.UNEVEN_SEED).random(w) < 0.3
    on[0] = on[w - 1] = True
    return np.flatnonzero(on).astype(np.uint32)


def _uneven(r, host_api, w, h):
    """counts 4 and 7 (a 1 x 1 frame: 7)"""
    stats = sp.uneven(r, host_api, _more_list(w, h))
    assert set(np.unique(stats[0])) == ({tc.UNEVEN_WHOLE, tc.UNEVEN_WHOLE + tc.UNEVEN_MORE} if w * h > 1 else {tc.UNEVEN_WHOLE + tc.UNEVEN_MORE})
    return stats


# ---- 1. the forms agree, and with the restatements ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: "%dx%d" % s)
def test_whole_frame_forms_agree(size, scenes, host_api, monkeypatch):
    """tc.SELECT: counts 4 are below min_samples, counts 7 take the noisy branch; tc.HALVE: every pixel is below min_samples with budgets 8
    and 5 before the cap, so the total at cap 3 is below the total at cap 7 at every size, whatever the variances are."""
    w, h = size
    r = _renderer(host_api, scenes, monkeypatch, w, h)
    cnt, sy, syy = _uneven(r, host_api, w, h)
    for sel in (tc.SELECT, tc.HALVE):
        want = ar.active_list(cnt, sy, syy, **sel)
        if size == (97, 41):
            assert 0.05 * w * h < len(want), len(want)  # nothing passes vacuously
        for name, call in (("rt_select_active", lambda: r.select_active(sel)), ("rt_select_active_rows", lambda: r.select_active_rows(0, 1, h, sel)),
                           ("rt_select_active_dilated", lambda: r.select_active_dilated(0, sel))):
            r.set_active(np.zeros(0, np.uint32))  # (whatever the form before left is gone)
            n = call()
            got, n2 = r.active()
            assert n == n2 == len(want) and np.array_equal(got, want), (name, sel, n, len(want))
        t7, t3 = (int(br.budgets(cnt, sy, syy, cap, **sel).sum()) for cap in (CAP, CAP >> 1))
        if sel is tc.HALVE or size == (97, 41):
            assert t3 < t7, "no budget above cap / 2: nothing to halve"
        for mps in (0, t3):
            lst, b, total, used = br.plan(cnt, sy, syy, CAP, mps, **sel)
            assert b is not None and np.array_equal(lst, want) and used == (CAP >> 1 if mps and t3 < t7 else CAP), (sel, mps, used)
            P = dict(select=sel, pass_cap=CAP, max_pass_samples=mps)
            for name, call in (("rt_select_budget", lambda: r.select_budget(P)), ("rt_select_budget_rows", lambda: r.select_budget_rows(0, 1, h, P)),
                               ("rt_select_budget_dilated", lambda: r.select_budget_dilated(0, P))):
                r.set_active(np.zeros(0, np.uint32))
                got = call()
                got_lst, n2 = r.active()
                got_b, n3 = r.budgets()
                assert got == (len(lst), total, used) and n2 == n3 == len(lst), (name, sel, mps, got, len(lst), total, used)
                assert np.array_equal(got_lst, lst) and np.array_equal(got_b, b), (name, sel, mps)
    r.close()


# ---- 2. profile entries ---------------------------------------------------------------------------------------------------------------------
def test_profile_entries_of_the_forms(scenes, host_api, monkeypatch):
    w, h = 96, 64
    r = _renderer(host_api, scenes, monkeypatch, w, h)
    sel = NOISY
    cnt, sy, syy = _uneven(r, host_api, w, h)
    r.set_profiling(True)
    P = dict(select=sel, pass_cap=CAP)
    n_raw, n_dil = len(ar.active_list(cnt, sy, syy, **sel)), len(dr.dilated_list(cnt, sy, syy, 2, **sel))
    assert n_raw > 1 and n_dil > 1

    def entries(call):
        r.profile(reset=True)
        call()
        return r.profile()["query"]["launches"]

    def refused(fn, params, *args):
        p = host_api.budget_params(params)
        n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
        assert fn(r.ctx, C.byref(p), *args, C.byref(n), C.byref(total), C.byref(cap)) == host_api.RT_E_UNSUPPORTED

    assert entries(lambda: r.select_active(sel)) == 1
    assert entries(lambda: r.select_active_rows(1, 2, h // 2, sel)) == 1
    assert entries(lambda: r.select_active_dilated(2, sel)) == 1
    assert entries(lambda: r.select_budget_dilated(2, P)) == 1
    assert entries(lambda: refused(r.rt.rt_select_budget_dilated, dict(P, max_pass_samples=n_dil - 1), 2)) == 1
    assert entries(lambda: r.select_budget(P)) == 0
    assert entries(lambda: r.select_budget_rows(1, 2, h // 2, P)) == 0
    assert entries(lambda: refused(r.rt.rt_select_budget, dict(P, max_pass_samples=n_raw - 1))) == 0
    r.close()


# ---- 3. a selection that does not fit ---------------------------------------------------------------------------------------------------------
def test_selection_that_does_not_fit_through_both_sources(scenes, host_api, monkeypatch):
    w, h = 97, 41
    r = _renderer(host_api, scenes, monkeypatch, w, h)
    sel = NOISY
    cnt, sy, syy = _uneven(r, host_api, w, h)
    whole = ar.active_list(cnt, sy, syy, **sel)
    odd_rows = whole[(whole // w) % 2 == 1]  # rows 1, 3, ..., 39
    dilated = dr.dilated_list(cnt, sy, syy, 2, **sel)
    assert 1 < len(odd_rows) < len(whole) <= len(dilated)
    for want, fn, args, word in ((odd_rows, r.rt.rt_select_budget_rows, (1, 2, h // 2), b"active"), (dilated, r.rt.rt_select_budget_dilated, (2,), b"listed")):
        r.set_active(np.zeros(0, np.uint32))
        p = host_api.budget_params(dict(select=sel, pass_cap=CAP, max_pass_samples=len(want) - 1))
        n, total, cap = C.c_int(-7), C.c_uint32(7), C.c_int(-7)
        assert fn(r.ctx, C.byref(p), *args, C.byref(n), C.byref(total), C.byref(cap)) == host_api.RT_E_UNSUPPORTED
        assert b"%d %s pixels do not fit a pass of %d samples" % (len(want), word, len(want) - 1) in r.rt.rt_last_error(r.ctx)
        assert n.value == len(want) and (total.value, cap.value) == (7, -7)  # n_active is written, the other two are not
        got, n2 = r.active()
        assert n2 == len(want) and np.array_equal(got, want)                   # the list is installed, for rt_render_active
        assert r.rt.rt_render_budget(r.ctx, 0, SEED, 4) == host_api.RT_E_STATE  # ... without a plan
    r.close()
