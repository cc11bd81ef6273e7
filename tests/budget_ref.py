"""numpy restatement of the budgeted adaptive passes of include/rt_amd.h: the per-pixel budget and the fit rule of rt_select_budget and the
loop a caller of rt_select_budget / rt_render_budget runs.  A plain helper module of the test suite: tests/test_budget_cpu.py probes it on
crafted moments and runs the loop on the oracle's samples, tests/test_gpu_budget.py holds the kernels against it bit for bit.  The predicate
is adaptive_ref's (rt_select_active's).

Everything is f32, one rounding per operation, ternaries as written (a NaN falls to the last branch); n, m, v, d as in adaptive_ref:
  count < min_samples:  b = min_samples - count
  otherwise:            g = threshold d;  t = v / (g g);  need = t - n
                        b = need >= f32(cap) ? cap : (need >= 1 ? (int)ceil(need) : 1)
  both:                 b = min(b, cap);  b = min(b, max_samples - count)
  fit:                  cap = pass_cap >> k for the smallest k >= 0 whose sum of budgets is <= limit; none (n_active > limit): unsupported"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402

F32 = np.float32
PASS_SAMPLES_MAX = 2 ** 31 - 1  # the limit is never above this (sample ids are ints)


def need(count, sum_y, sum_yy, threshold, floor):
    """need = t - n of the noisy branch (f32; whatever the inputs give, NaN and inf included)"""
    count = np.asarray(count, np.uint32)
    sy, syy = np.asarray(sum_y, F32), np.asarray(sum_yy, F32)
    with np.errstate(all="ignore"):
        n = count.astype(F32)
        m = (sy / n).astype(F32)
        v = ((syy - (sy * m).astype(F32)).astype(F32) / (n - F32(1)).astype(F32)).astype(F32)
        v = np.where(v > F32(0), v, F32(0)).astype(F32)
        d = np.where(m > F32(floor), m, F32(floor)).astype(F32)
        g = (F32(threshold) * d).astype(F32)
        t = (v / (g * g).astype(F32)).astype(F32)
        return (t - n).astype(F32)


def budgets(count, sum_y, sum_yy, cap, min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3):
    """per pixel (the inputs' shape, int64): the budget at the effective cap 'cap'; 0 where the pixel is not active"""
    count = np.asarray(count, np.uint32)
    on = ar.active_mask(count, sum_y, sum_yy, min_samples, max_samples, threshold, floor)
    c = count.astype(np.int64)
    nd = need(count, sum_y, sum_yy, threshold, floor)
    with np.errstate(invalid="ignore"):
        at_cap = nd >= F32(cap)
        mid = (nd >= F32(1)) & ~at_cap  # 1 <= need < cap: the only lanes whose ceil is taken
        noisy = np.where(at_cap, cap, np.where(mid, np.ceil(np.where(mid, nd, F32(1))).astype(np.int64), 1))
    b = np.where(c < min_samples, min_samples - c, noisy)
    b = np.minimum(b, cap)
    b = np.minimum(b, max_samples - c)
    return np.where(on, b, 0).astype(np.int64)


def limit_of(max_pass_samples, sample_gib=4):
    """the fit rule's limit: max_pass_samples, or the capacity of the finished-sample buffer (16 B per sample); at most 2^31 - 1"""
    lim = int(max_pass_samples) if max_pass_samples else (int(sample_gib) << 30) // 16
    return min(lim, PASS_SAMPLES_MAX)


def fit(totals, pass_cap, limit):
    """totals: cap -> the sum of the budgets at that cap.  (cap used, attempts) for the first cap = pass_cap >> k that fits, (None,
    attempts) when not even cap = 1 does"""
    cap, tries = int(pass_cap), 0
    while cap >= 1:
        tries += 1
        if totals(cap) <= limit:
            return cap, tries
        cap >>= 1
    return None, tries


def plan(count, sum_y, sum_yy, pass_cap=64, max_pass_samples=0, sample_gib=4, **select):
    """rt_select_budget: (list, budgets in list order or None, n_samples or None, cap_used or None); None: RT_E_UNSUPPORTED (the list
    is still what rt_select_active's would be)"""
    lst = ar.active_list(count, sum_y, sum_yy, **select)
    per_cap = {}

    def totals(cap):
        per_cap[cap] = budgets(count, sum_y, sum_yy, cap, **select).reshape(-1)
        return int(per_cap[cap].sum())

    cap, _ = fit(totals, pass_cap, limit_of(max_pass_samples, sample_gib))
    if cap is None:
        return lst, None, None, None
    b = per_cap[cap][lst].astype(np.uint32)
    return lst, b, int(b.sum(dtype=np.int64)), cap


def budget_pass(samples, acc, count, sum_y, sum_yy, b):
    """rt_render_budget on a recorded [frame][pixel...][>= 3] stack whose frame k is every pixel's sample k: pixel p gets samples
    count[p] .. count[p] + b[p] - 1, one at a time in frame order.  acc is the f64 sum of adaptive_ref.adaptive_loop.  In place."""
    samples = np.asarray(samples, F32)
    b = np.asarray(b, np.int64)
    for k in range(int(b.max()) if b.size else 0):
        on = b > k
        f = count[on].astype(np.int64)  # each pixel's next frame
        s = samples[(f,) + np.nonzero(on)]
        c1, y1, yy1 = ar.moments(s[None], count[on], sum_y[on], sum_yy[on])
        count[on], sum_y[on], sum_yy[on] = c1, y1, yy1
        acc[on] += s[..., :3].astype(np.float64)


def budget_loop(samples, pass_cap, max_passes, min_samples, max_samples, threshold, floor, max_pass_samples=0):
    """The loop a caller of rt_select_budget / rt_render_budget runs from rt_clear on a recorded stack (frame k = sample k of every
    pixel): passes until nothing is active, the fit fails or max_passes have run.  Returns (acc f64, count, sum_y, sum_yy, [(n_active,
    n_samples, cap_used, budgets per pixel)] per pass)."""
    samples = np.asarray(samples, F32)
    shape = samples.shape[1:-1]
    P = dict(min_samples=min_samples, max_samples=max_samples, threshold=threshold, floor=floor)
    count, sy, syy = np.zeros(shape, np.uint32), np.zeros(shape, F32), np.zeros(shape, F32)
    acc = np.zeros(shape + (3,), np.float64)
    passes = []
    for _ in range(max_passes):
        lst, b, total, cap = plan(count, sy, syy, pass_cap, max_pass_samples, **P)
        if len(lst) == 0 or b is None:
            break
        per_pixel = budgets(count, sy, syy, cap, **P)
        assert int((count.astype(np.int64) + per_pixel).max()) <= samples.shape[0], "the loop ran out of recorded frames"
        budget_pass(samples, acc, count, sy, syy, per_pixel)
        passes.append((len(lst), total, cap, per_pixel))
    return acc, count, sy, syy, passes
