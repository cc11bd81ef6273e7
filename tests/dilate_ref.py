"""numpy restatement of the dilated adaptive selection of include/rt_amd.h (rt_select_active_dilated, rt_select_budget_dilated).  A plain
helper module of the test suite: tests/test_dilate_cpu.py holds it against a brute-force double loop and runs the loop on the oracle's
samples, tests/test_gpu_dilate.py holds the kernels against it entry for entry.  The predicate is adaptive_ref's (rt_select_active's),
the budgets and the fit rule budget_ref's (rt_select_budget's).

With raw_q the predicate on pixel q, radius r and p = (x, y), the statistics shaped (height, width):
  win(p)     = { (x + dx, y + dy) : |dx| <= r, |dy| <= r, 0 <= x + dx < width, 0 <= y + dy < height }
  eligible_p = count_p < max_samples && isfinite(sum_y_p) && isfinite(sum_yy_p)
  active_p   = raw_p || (eligible_p && OR over q in win(p) of raw_q)
  budget_p   = rt_select_budget's where raw_p, 1 where the pixel is listed by dilation alone, 0 where it is not listed"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import budget_ref as br  # noqa: E402

F32 = np.float32
MAX_RADIUS = 16  # RT_DILATE_MAX_RADIUS


def window_or(mask, radius):
    """(height, width) bool -> OR of the mask over every pixel's window, clipped to the frame per axis (slices never wrap)"""
    m = np.asarray(mask, bool)
    assert m.ndim == 2
    h, w = m.shape
    rows = m.copy()
    for d in range(1, min(radius, w - 1) + 1):
        rows[:, d:] |= m[:, :-d]   # the source d to the left
        rows[:, :-d] |= m[:, d:]   # the source d to the right
    out = rows.copy()
    for d in range(1, min(radius, h - 1) + 1):
        out[d:, :] |= rows[:-d, :]
        out[:-d, :] |= rows[d:, :]
    return out


def eligible_mask(count, sum_y, sum_yy, max_samples):
    count = np.asarray(count, np.uint32)
    return (count < np.uint32(max_samples)) & np.isfinite(np.asarray(sum_y, F32)) & np.isfinite(np.asarray(sum_yy, F32))


def dilated_mask(count, sum_y, sum_yy, radius, min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3):
    """the predicate of rt_select_active_dilated per pixel (bool, (height, width))"""
    raw = ar.active_mask(count, sum_y, sum_yy, min_samples, max_samples, threshold, floor)
    assert raw.ndim == 2 and 0 <= radius <= MAX_RADIUS
    return raw | (eligible_mask(count, sum_y, sum_yy, max_samples) & window_or(raw, radius))


def dilated_list(count, sum_y, sum_yy, radius, **params):
    """the list rt_select_active_dilated builds: pixel indices y * width + x, ascending (uint32)"""
    return np.flatnonzero(dilated_mask(count, sum_y, sum_yy, radius, **params).reshape(-1)).astype(np.uint32)


def dilated_budgets(count, sum_y, sum_yy, cap, radius, **select):
    """per pixel (int64): budget_ref's budget where the pixel is raw-active, 1 where dilation alone lists it, 0 elsewhere"""
    raw = ar.active_mask(count, sum_y, sum_yy, **select)
    on = dilated_mask(count, sum_y, sum_yy, radius, **select)
    return np.where(raw, br.budgets(count, sum_y, sum_yy, cap, **select), np.where(on, 1, 0)).astype(np.int64)


def plan(count, sum_y, sum_yy, radius, pass_cap=64, max_pass_samples=0, sample_gib=4, **select):
    """rt_select_budget_dilated: (list, budgets in list order or None, n_samples or None, cap_used or None); None: RT_E_UNSUPPORTED (the
    list is still rt_select_active_dilated's)"""
    lst = dilated_list(count, sum_y, sum_yy, radius, **select)
    per_cap = {}

    def totals(cap):
        per_cap[cap] = dilated_budgets(count, sum_y, sum_yy, cap, radius, **select).reshape(-1)
        return int(per_cap[cap].sum())

    cap, _ = br.fit(totals, pass_cap, br.limit_of(max_pass_samples, sample_gib))
    if cap is None:
        return lst, None, None, None
    b = per_cap[cap][lst].astype(np.uint32)
    return lst, b, int(b.sum(dtype=np.int64)), cap


def dilated_loop(samples, budget, radius, min_samples, max_samples, threshold, floor):
    """adaptive_ref.adaptive_loop with the dilated selection, on a recorded [frame][y][x][>= 3] stack whose frame k is every pixel's
    sample k: frames 0 .. min_samples - 1 whole; then, pass by pass, every listed pixel gets ITS next sample (frame = its count: a
    pixel's value is a function of its count, as under rt_render_budget), until the next pass would take the total past 'budget' samples
    (None: no budget) or nothing is listed.  Returns (f64 sum of the samples taken per pixel, count, total)."""
    samples = np.asarray(samples, F32)
    count, sy, syy = ar.moments(samples[:min_samples])
    acc = samples[:min_samples, ..., :3].astype(np.float64).sum(0)
    total = int(count.sum())
    P = dict(min_samples=min_samples, max_samples=max_samples, threshold=threshold, floor=floor)
    while True:
        on = dilated_mask(count, sy, syy, radius, **P)
        k = int(on.sum())
        if k == 0 or (budget is not None and total + k > budget):
            break
        assert int(count[on].max()) < samples.shape[0], "the loop ran out of recorded frames"
        br.budget_pass(samples, acc, count, sy, syy, on.astype(np.int64))
        total += k
    return acc, count, total
