"""CPU tier of the budgeted adaptive passes: tests/budget_ref.py (the numpy restatement of rt_select_budget / rt_render_budget) on crafted
moments that reach every branch of the budget, the fit rule on crafted totals, and the evidence for tests/test_gpu_budget.py -- every class
of pixels that file asserts as PRESENT is counted here on the oracle's samples of the same scenes, sizes and schedules (PRESENT of
tests/budget_shapes.py names them with the margin asked for; the device's frames agree with the oracle's to 1e-4, so classes of tens of pixels hold there too).
A class the oracle does not populate with that margin is not asserted on the device:
  * need < 1 on a noisy pixel (the pixel is active by a hair): 5 to 10 pixels at 97 x 41, none at 257 x 3 -- crafted moments only;
  * at 257 x 3 (a strip across the middle of the view) at most four pixels are noisy at counts 4 / 7: only 'below min_samples' and the
    totals' order (total(7) > total(3) > total(1) under HALVE, which the pixels below min_samples carry) are asserted there."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import adaptive_shapes as sh  # noqa: E402
import budget_ref as br  # noqa: E402

F32 = np.float32
INF = float("inf")

import budget_shapes as bs  # noqa: E402
from budget_shapes import (SELECT, HALVE, LOOP, LOOP_CAP, LOOP_PASSES, MARGIN, PRESENT, UNEVEN_WHOLE, UNEVEN_MORE,  # noqa: E402,F401
                           classes, oracle_stack, uneven_moments)


# ---- crafted moments --------------------------------------------------------------------------------------------------------------------
def _moments_of(values):
    v = np.asarray(values, F32)
    sy, syy = F32(0), F32(0)
    with np.errstate(over="ignore"):
        for y in v:
            sy, syy = F32(sy + y), F32(syy + F32(y * y))
    return np.uint32(len(v)), sy, syy


def _b(values, cap, **params):
    c, sy, syy = _moments_of(values)
    P = dict(min_samples=4, max_samples=1024, threshold=0.05, floor=1e-3)
    P.update(params)
    return int(br.budgets(np.array([c]), np.array([sy]), np.array([syy]), cap, **P)[0])


def test_crafted_moments_reach_every_branch():
    # below min_samples: min_samples - count, capped; a pixel without samples too
    assert _b([1.0, 2.0], 64, min_samples=16) == 14 and _b([1.0, 2.0], 5, min_samples=16) == 5 and _b([], 64, min_samples=16) == 16
    assert _b([1.0] * 15, 64, min_samples=16) == 1
    # below min_samples wins over everything: non-finite sums are active there, and the clamp by max_samples still holds
    assert _b([INF, 1.0], 64, min_samples=4) == 2 and _b([1.0, 2.0, 3.0], 64, min_samples=4, max_samples=4) == 1
    # noisy, need >= cap: samples 0 / 2 -- n = 8, m = 1, v = 8 / 7, t = v / 0.0025 = 457.1, need = 449.1
    noisy = [0.0, 2.0] * 4
    assert _b(noisy, 64) == 64 and _b(noisy, 449) == 449 and _b(noisy, 1) == 1
    # 1 <= need < cap: the ceil
    assert _b(noisy, 450) == 450 and _b(noisy, 1024) == 450
    c, sy, syy = _moments_of(noisy)
    nd = br.need(np.array([c]), np.array([sy]), np.array([syy]), 0.05, 1e-3)[0]
    assert 449 < nd < 450 and nd != np.floor(nd)
    # an integral need is its own ceil: n = 4, samples 0 0 2 2: m = 1, v = 4 / 3; threshold 0.5: g = 0.5, t = 5.333..; need = 1.333 -> 2
    assert _b([0.0, 0.0, 2.0, 2.0], 64, threshold=0.5) == 2
    # need < 1 by rounding: active by a hair (e / d just above the threshold), t - n below 1 -> 1
    vals = [1.0] * 7 + [1.5]
    c, sy, syy = _moments_of(vals)
    e = float(ar.relative_error(np.array([c]), np.array([sy]), np.array([syy]), 1e-3)[0])
    thr = float(np.nextafter(F32(e), F32(0)))  # the largest threshold under which the pixel is still active
    nd = br.need(np.array([c]), np.array([sy]), np.array([syy]), thr, 1e-3)[0]
    assert ar.active_mask(np.array([c]), np.array([sy]), np.array([syy]), 4, 1024, thr, 1e-3)[0] and nd < 1
    assert _b(vals, 64, threshold=thr) == 1
    # threshold == 0: g * g == 0, t = +inf, need = +inf >= cap
    assert _b(noisy, 64, threshold=0.0) == 64 and _b(noisy, 1024, threshold=0.0, max_samples=100) == 92
    assert _b([1.0] * 8, 64, threshold=0.0) == 0  # v == 0: e / d > 0 is false, not active (t would be 0 / 0)
    # g * g underflows to 0 on a dark, noisy pixel: t = +inf like threshold == 0.  (A NaN need cannot reach an active pixel: with finite sums
    # v <= sum_yy / (n - 1) is finite, so t is NaN only for v == 0 and g * g == 0, where e / d > threshold is false.  The ternaries still
    # send it to the last branch, which budget_ref.budgets restates with ~(need >= cap) and (need >= 1).)
    tiny = [0.0, 2e-15] * 4  # m = d = 1e-15, g = 1e-25, g * g = 0
    assert _b(tiny, 64, threshold=1e-10, floor=1e-30) == 64
    with np.errstate(all="ignore"):
        assert np.isposinf(br.need(*[np.array([x]) for x in _moments_of(tiny)], 1e-10, 1e-30)[0])
    # the max_samples - count clamp
    assert _b(noisy, 64, max_samples=10) == 2 and _b(noisy, 64, max_samples=9) == 1 and _b(noisy, 64, max_samples=8) == 0
    # non-finite sums at or above min_samples: never listed
    assert _b([INF] + [1.0] * 7, 64) == 0 and _b([1e38] * 8, 64) == 0
    # the floor is the denominator of a dark pixel: g = threshold * floor
    dark = [0.0, 2e-4] * 4
    assert _b(dark, 1024, floor=1e-3) < _b(dark, 1024, floor=1e-4)
    # budgets agree with the predicate: b > 0 exactly where the pixel is active
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, 30, 500).astype(np.uint32)
    sy = (rng.random(500) * cnt).astype(F32)
    syy = (sy * sy / np.maximum(cnt, 1) * (1 + rng.random(500) * 0.1)).astype(F32)
    for cap in (1, 7, 64, 1024):
        b = br.budgets(cnt, sy, syy, cap, min_samples=6, max_samples=25, threshold=0.05, floor=1e-3)
        assert np.array_equal(b > 0, ar.active_mask(cnt, sy, syy, 6, 25, 0.05, 1e-3))
        assert b.max() <= cap and np.all(cnt[b > 0] + b[b > 0] <= 25)


def test_fit_rule_on_crafted_totals():
    totals = {64: 1000, 32: 900, 16: 500, 8: 300, 4: 200, 2: 150, 1: 100}
    assert br.fit(totals.get, 64, 1000) == (64, 1) and br.fit(totals.get, 64, 999) == (32, 2) and br.fit(totals.get, 64, 899) == (16, 3)
    assert br.fit(totals.get, 64, 100) == (1, 7) and br.fit(totals.get, 64, 99) == (None, 7)
    t7 = {7: 50, 3: 30, 1: 10}  # 7 >> 1 = 3, 3 >> 1 = 1
    assert br.fit(t7.get, 7, 49) == (3, 2) and br.fit(t7.get, 7, 29) == (1, 3) and br.fit(t7.get, 7, 9) == (None, 3)
    assert br.fit({1: 5}.get, 1, 5) == (1, 1) and br.fit({1: 5}.get, 1, 4) == (None, 1)
    # the limit: max_pass_samples, or the sample buffer's capacity; never above 2^31 - 1
    assert br.limit_of(0) == 2 ** 28 and br.limit_of(0, sample_gib=1) == 2 ** 26 and br.limit_of(12345) == 12345
    assert br.limit_of(0, sample_gib=64) == 2 ** 31 - 1 and br.limit_of(2 ** 32 - 1) == 2 ** 31 - 1
    # plan(): unsupported keeps the list; an empty selection is a plan of no samples
    cnt, sy, syy = np.array([0, 0, 9], np.uint32), np.zeros(3, F32), np.zeros(3, F32)
    P = dict(min_samples=4, max_samples=8, threshold=0.05, floor=1e-3)
    lst, b, total, cap = br.plan(cnt, sy, syy, 7, 0, **P)
    assert list(lst) == [0, 1] and list(b) == [4, 4] and total == 8 and cap == 7
    lst, b, total, cap = br.plan(cnt, sy, syy, 7, 7, **P)
    assert list(b) == [3, 3] and total == 6 and cap == 3
    lst, b, total, cap = br.plan(cnt, sy, syy, 7, 1, **P)
    assert list(lst) == [0, 1] and b is None and total is None and cap is None
    lst, b, total, cap = br.plan(np.array([9, 9], np.uint32), np.zeros(2, F32), np.zeros(2, F32), 7, 0, **P)
    assert len(lst) == 0 and len(b) == 0 and total == 0 and cap == 7


# ---- the oracle's samples: the classes the device tests assert ----------------------------------------------------------------------
@pytest.mark.parametrize("key", list(PRESENT), ids=lambda k: "%s-%dx%d" % (k[0], k[1][0], k[1][1]))
def test_classes_asserted_on_the_device_are_populated_on_the_oracle(key, scenes, oracle_api):
    name, (w, h) = key
    S = oracle_stack(scenes, oracle_api, name, w, h)
    cnt, sy, syy = uneven_moments(S, w, h)
    assert set(np.unique(cnt)) == {UNEVEN_WHOLE, UNEVEN_WHOLE + UNEVEN_MORE}
    got = classes(cnt, sy, syy)
    print(name, w, h, got)
    for cls in PRESENT[key]:
        if cls == "loop_budgets_differ":
            continue
        assert got[cls] >= MARGIN, (cls, got)
    # test 2's loop: in pass 2 the budgets differ across pixels (every value 1 .. 7 occurs at 97 x 41)
    passes = br.budget_loop(S, LOOP_CAP, LOOP_PASSES, **LOOP)[4]
    assert len(passes) == LOOP_PASSES
    assert passes[0][:3] == (w * h, LOOP["min_samples"] * w * h, LOOP_CAP) and np.all(passes[0][3] == LOOP["min_samples"])
    for na, total, cap, b in passes[1:]:
        assert 0 < na < w * h and cap == LOOP_CAP
    if "loop_budgets_differ" in PRESENT[key]:  # pass 2 (pass 3 gives nearly every active pixel the cap: not asserted)
        values, pixels = np.unique(passes[1][3][passes[1][3] > 0], return_counts=True)
        assert len(values) >= 5 and int(pixels[values < LOOP_CAP].sum()) >= MARGIN, (values, pixels)


@pytest.mark.parametrize("name", list(bs.SCENES))
def test_budgeted_loop_on_the_oracle(name, scenes, oracle_api):
    """The loop to its end: every count <= max_samples, every pixel's sums those of its first count samples; and with pass_cap = 1 and
    equal starting counts a pass takes exactly the samples of adaptive_ref.adaptive_loop's next step."""
    w, h = 97, 41
    S = oracle_stack(scenes, oracle_api, name, w, h)
    acc, cnt, sy, syy, passes = br.budget_loop(S, LOOP_CAP, 100, **LOOP)
    assert len(passes) < 100 and not ar.active_mask(cnt, sy, syy, **LOOP).any()
    assert cnt.max() <= LOOP["max_samples"] and cnt.min() >= LOOP["min_samples"] and cnt.max() == LOOP["max_samples"]
    assert int(cnt.sum(dtype=np.int64)) == sum(p[1] for p in passes)
    for n in np.unique(cnt):  # count alone decides a pixel
        c1, y1, yy1 = ar.moments(S[:n])
        on = cnt == n
        assert np.array_equal(sy[on].view(np.uint32), y1[on].view(np.uint32)) and np.array_equal(syy[on].view(np.uint32), yy1[on].view(np.uint32))
        assert np.array_equal(acc[on], np.add.accumulate(S[:n, ..., :3].astype(np.float64), 0)[-1][on], equal_nan=True)
    # pass_cap 1 from min_samples equal counts: adaptive_loop's steps, one frame each
    K = 9
    acc1, cnt1, sy1, syy1, passes1 = br.budget_loop(S, 1, LOOP["min_samples"] + K, **LOOP)
    assert all(p[0] == p[1] and p[2] == 1 for p in passes1)
    whole = passes1[:LOOP["min_samples"]]
    assert all(p[0] == w * h for p in whole)  # one sample per pixel per pass until min_samples
    budget = LOOP["min_samples"] * w * h + sum(p[1] for p in passes1[LOOP["min_samples"]:])
    acc2, cnt2, total2 = ar.adaptive_loop(S, budget, **LOOP)
    assert total2 == budget and np.array_equal(cnt1, cnt2) and np.array_equal(acc1, acc2, equal_nan=True)
