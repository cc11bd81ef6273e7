"""Dilated adaptive selection without a device: the numpy restatement (tests/dilate_ref.py) against a brute-force loop over every pixel
and window, the properties of the definition, the budgets, the crafted cases of tests/dilate_shapes.py, and the dilated loop on the
oracle's own samples -- the evidence that the device tests of tests/test_gpu_dilate.py can be met and that the feature does what it is
for: pixels that stop at min_samples with a wrong mean."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402
import budget_ref as br  # noqa: E402
import dilate_ref as dr  # noqa: E402
import dilate_shapes as ds  # noqa: E402
from test_adaptive_cpu import QUALITY  # noqa: E402

F32 = np.float32
P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
RADII = (0, 1, 2, 5, 16)


def random_stats(w, h, seed):
    """(count, sum_y, sum_yy) shaped (h, w): counts below min_samples (about 1 %), at max_samples (10 %), +inf sums (5 %), and a few per cent of
    noisy pixels among quiet ones, so that a dilation neither dies out nor covers the frame"""
    rng = np.random.default_rng(seed)
    n = w * h
    count = rng.integers(P["min_samples"], P["max_samples"], n).astype(np.uint32)
    kind = rng.random(n)
    count[kind < 0.01] = rng.integers(0, P["min_samples"], int((kind < 0.01).sum()))
    count[(kind >= 0.01) & (kind < 0.11)] = P["max_samples"]
    m = rng.uniform(0.05, 1.0, n)
    noisy = rng.random(n) < 0.04
    sd = np.where(noisy, m * 2.0, m * 0.01)
    c = count.astype(np.float64)
    sy = (c * m).astype(F32)
    syy = (c * (m * m + sd * sd)).astype(F32)
    inf = (kind >= 0.11) & (kind < 0.16)
    sy[inf], syy[inf] = np.inf, np.inf
    return count.reshape(h, w), sy.reshape(h, w), syy.reshape(h, w)


def brute_force(count, sy, syy, radius):
    """the definition of include/rt_amd.h, pixel by pixel and window by window"""
    raw = ar.active_mask(count, sy, syy, **P)
    h, w = raw.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        y0, y1 = max(y - radius, 0), min(y + radius, h - 1)
        for x in range(w):
            if raw[y, x]:
                out[y, x] = True
                continue
            if not (count[y, x] < P["max_samples"] and np.isfinite(sy[y, x]) and np.isfinite(syy[y, x])):
                continue
            out[y, x] = raw[y0:y1 + 1, max(x - radius, 0):min(x + radius, w - 1) + 1].any()
    return out


def brute_force_offsets(count, sy, syy, radius):
    """the same definition, offset by offset: every (dx, dy) of the window ORs the raw mask, shifted and clipped, into the frame (the
    pixel loop above takes seconds at the largest size)"""
    raw = ar.active_mask(count, sy, syy, **P)
    h, w = raw.shape
    seen = np.zeros((h, w), bool)
    for dy in range(-min(radius, h - 1), min(radius, h - 1) + 1):
        for dx in range(-min(radius, w - 1), min(radius, w - 1) + 1):
            # pixel (x, y) sees source (x + dx, y + dy)
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            seen[yd, xd] |= raw[ys, xs]
    may = (count < P["max_samples"]) & np.isfinite(sy) & np.isfinite(syy)
    return raw | (may & seen)


@pytest.mark.parametrize("size", list(ds.SIZES), ids=lambda s: "%dx%d" % s)
def test_restatement_equals_the_brute_force(size):
    w, h = size
    count, sy, syy = random_stats(w, h, 7 + w * h)
    raw = ar.active_mask(count, sy, syy, **P)
    if w * h > 2000:  # the classes the statistics are made for
        assert 0 < raw.sum() < raw.size // 4
        assert (count[~raw] == P["max_samples"]).any() and np.isposinf(sy[~raw]).any() and (count < P["min_samples"]).any()
    for r in RADII:
        got = dr.dilated_mask(count, sy, syy, r, **P)
        assert got.dtype == bool and got.shape == (h, w)
        assert np.array_equal(got, brute_force_offsets(count, sy, syy, r)), r
        if w * h <= 5000:
            assert np.array_equal(got, brute_force(count, sy, syy, r)), r
        lst = dr.dilated_list(count, sy, syy, r, **P)
        assert lst.dtype == np.uint32 and np.array_equal(lst, np.flatnonzero(got.reshape(-1)))


@pytest.mark.parametrize("size", [(65, 4), (97, 41), (641, 409)], ids=lambda s: "%dx%d" % s)
def test_properties_of_the_definition(size):
    w, h = size
    count, sy, syy = random_stats(w, h, 99 + w)
    raw = ar.active_mask(count, sy, syy, **P)
    elig = dr.eligible_mask(count, sy, syy, P["max_samples"])
    assert np.array_equal(dr.dilated_mask(count, sy, syy, 0, **P), raw)                       # radius 0
    assert np.array_equal(dr.dilated_list(count, sy, syy, 0, **P), ar.active_list(count, sy, syy, **P))
    prev = raw
    for r in range(1, dr.MAX_RADIUS + 1):                                                     # monotone in the radius
        cur = dr.dilated_mask(count, sy, syy, r, **P)
        assert not (prev & ~cur).any(), r
        assert not (cur & ~raw & ~elig).any(), r                                              # an ineligible pixel: only when raw-active
        prev = cur
    if w * h > 2000:
        assert prev.sum() > raw.sum()
    # empty iff the raw mask is empty: no pixel below min_samples, threshold +inf
    quiet = dict(P, threshold=np.inf)
    c2 = np.maximum(count, P["min_samples"]).astype(np.uint32)
    assert not ar.active_mask(c2, sy, syy, **quiet).any()
    for r in (0, 1, 16):
        assert not dr.dilated_mask(c2, sy, syy, r, **quiet).any()
        assert dr.dilated_mask(count, sy, syy, r, **quiet).any() == ar.active_mask(count, sy, syy, **quiet).any()


@pytest.mark.parametrize("size", [(5, 40), (64, 5), (65, 4), (97, 41)], ids=lambda s: "%dx%d" % s)
def test_a_source_at_a_row_end_does_not_light_the_next_row_start(size):
    """one source at (width - 1, y), every other pixel eligible: the listed pixels are the clipped window, nothing else -- column 0 of
    row y + 1 is listed only when the window reaches it (radius >= width - 1)"""
    w, h = size
    y = h // 2
    count = np.full((h, w), 2, np.uint32)
    count[y, w - 1] = 0
    sy = np.ones((h, w), F32)
    syy = np.ones((h, w), F32)
    for r in (0, 1, 2, 5, 16):
        got = dr.dilated_mask(count, sy, syy, r, **ds.CRAFT)
        want = np.zeros((h, w), bool)
        want[max(y - r, 0):y + r + 1, max(w - 1 - r, 0):] = True
        assert np.array_equal(got, want), r
        assert got[y + 1, 0] == (r >= w - 1 and r >= 1)
        # the linear neighbours of the source that a wrapping run of bits would reach
        p = y * w + w - 1
        flat = got.reshape(-1)
        for d in range(1, r + 1):
            q = p + d
            if q < w * h and (q % w) < w - 1 - r:
                assert not flat[q], (r, d)


def test_budgets_of_the_dilated_plan():
    w, h = 97, 41
    count, sy, syy = random_stats(w, h, 5)
    raw = ar.active_mask(count, sy, syy, **P)
    for r in (0, 1, 3):
        on = dr.dilated_mask(count, sy, syy, r, **P)
        for cap in (1, 7, 64):
            b = dr.dilated_budgets(count, sy, syy, cap, r, **P)
            assert np.array_equal(b[raw], br.budgets(count, sy, syy, cap, **P)[raw]) and (b[raw] >= 1).all()
            assert (b[on & ~raw] == 1).all() and (b[~on] == 0).all()
            assert ((count.astype(np.int64) + b)[on] <= P["max_samples"]).all()               # no budget takes a pixel past max_samples
        lst, b, total, cap = dr.plan(count, sy, syy, r, pass_cap=64, **P)
        assert cap == 64 and np.array_equal(lst, np.flatnonzero(on.reshape(-1))) and total == int(b.sum())
        if r == 0:
            l0, b0, t0, c0 = br.plan(count, sy, syy, pass_cap=64, **P)
            assert np.array_equal(lst, l0) and np.array_equal(b, b0) and (total, cap) == (t0, c0)
        # a limit between the totals at cap 32 and cap 64: one halving
        t64 = int(dr.dilated_budgets(count, sy, syy, 64, r, **P).sum())
        t32 = int(dr.dilated_budgets(count, sy, syy, 32, r, **P).sum())
        assert t32 < t64
        l2, b2, total2, cap2 = dr.plan(count, sy, syy, r, pass_cap=64, max_pass_samples=t64 - 1, **P)
        assert cap2 == 32 and total2 == t32 and np.array_equal(l2, lst) and (b2 <= 32).all()
        # not even one sample per listed pixel: unsupported, the list stands
        l3, b3, total3, cap3 = dr.plan(count, sy, syy, r, pass_cap=64, max_pass_samples=len(lst) - 1, **P)
        assert b3 is None and total3 is None and cap3 is None and np.array_equal(l3, lst)


# ---- the sizes and cases of tests/test_gpu_dilate.py -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(ds.SIZES), ids=lambda s: "%dx%d" % s)
def test_shape_cases_are_what_their_names_say(size):
    w, h = size
    n, words, blocks, per = ds.geometry(w, h)
    assert n == w * h and words == -(-n // 64) and blocks == -(-n // 256) and per == -(-blocks // 1024)
    want = {(1, 1): (1, 1, 1), (63, 1): (1, 1, 1), (65, 1): (2, 1, 1), (1, 67): (2, 1, 1), (5, 40): (4, 1, 1), (64, 5): (5, 2, 1), (65, 4): (5, 2, 1),
            (257, 3): (13, 4, 1), (97, 41): (63, 16, 1), (641, 409): (4097, 1025, 2)}[size]
    assert (words, blocks, per) == want, "the size no longer reaches the edge it is listed for"
    if size in ((63, 1), (65, 1), (1, 67), (5, 40), (65, 4), (257, 3), (97, 41), (641, 409)):
        assert n % 64 != 0                                       # high bits of the last word that must stay clear
    if size in ((5, 40), (65, 4), (97, 41), (641, 409)):
        assert w % 64 != 0 and h > 1                             # rows start at uneven bits
        assert len({(y * w) % 64 for y in range(h)}) > 2
    got = ds.cases(w, h)
    names = [c[0] for c in got]
    assert names[:2] == ["none", "all"]
    assert len(set(names)) == len(names)
    if w > 1 and h > 1:
        assert {"top_left", "top_right", "bottom_left", "bottom_right", "one_row", "one_column", "stopped_ring"} <= set(names)
    if w > 1 and h >= 4:
        assert {"row_end", "row_start"} <= set(names)
    for p in (63, 64):  # under its own name, or the corner or row end it coincides with
        if p < n:
            assert any(st is None and src.sum() == 1 and src.reshape(-1)[p] for _, src, st in got), p
    if n >= 300:
        assert "seeded_01" in names
    for name, src, stopped in got:
        assert src.dtype == bool and src.shape == (h, w), name
        assert stopped is None or (stopped.shape == (h, w) and not (stopped & src).any() and stopped.any()), name
        c = ds.crafted_counts(src, stopped)
        raw = ar.active_mask(c, np.ones((h, w), F32), np.ones((h, w), F32), **ds.CRAFT)
        assert np.array_equal(raw, src), name                     # CRAFT: raw-active exactly without samples
        assert np.array_equal(dr.eligible_mask(c, np.ones((h, w), F32), np.ones((h, w), F32), 3), c < 3)
        flat = src.reshape(-1)
        if name == "row_end":
            p = int(np.flatnonzero(flat)[0])
            assert flat.sum() == 1 and p % w == w - 1 and p + 1 < n
        elif name == "row_start":
            p = int(np.flatnonzero(flat)[0])
            assert flat.sum() == 1 and p % w == 0 and p > 0
        elif name in ("pixel63", "pixel64"):
            assert flat.sum() == 1 and flat[int(name[5:])]
        elif name == "one_row":
            assert src[h // 2].all() and src.sum() == w
        elif name == "one_column":
            assert src[:, w // 2].all() and src.sum() == h
        elif name == "seeded_01":
            assert src.sum() == (n + 50) // 100 and 0.03 < stopped.mean() < 0.07
        elif name == "stopped_ring":
            assert src.sum() == 1 and src[h // 2, w // 2]
            # every stopped pixel is within radius 2 of the source: dilation reaches it and must not list it
            for r in (2, 16):
                on = dr.dilated_mask(c, np.ones((h, w), F32), np.ones((h, w), F32), r, **ds.CRAFT)
                assert dr.window_or(src, r)[stopped].all() and not on[stopped].any()
        elif name in ("top_left", "top_right", "bottom_left", "bottom_right"):
            assert flat.sum() == 1 and (flat[0] or flat[w - 1] or flat[n - w] or flat[n - 1])
        elif name == "all":
            assert flat.all()
        elif name == "none":
            assert not flat.any()
        else:
            raise AssertionError("no check for case " + name)


# ---- the loop on the oracle's samples ------------------------------------------------------------------------------------------------
def stopped_and_wrong(acc, count, samples, reference, min_samples):
    """pixels, finite in the reference and in every recorded sample, that stopped at count == min_samples with a mean more than 10 % off the
    reference: max over the channels of |mean - ref|, relative to max(max over the channels of ref, 1e-3)"""
    fin = np.isfinite(reference).all(-1) & np.isfinite(samples[..., :3]).all(-1).all(0)
    with np.errstate(all="ignore"):
        mean = acc / count[..., None]
        off = np.abs(mean - reference).max(-1) / np.maximum(reference.max(-1), 1e-3)
    return int((fin & (count == min_samples) & (off > 0.1)).sum()), fin


def mse(acc, count, reference, fin):
    with np.errstate(all="ignore"):
        mean = acc / count[..., None]
    return float(((mean[fin] - reference[fin]) ** 2).mean())


@pytest.fixture(scope="module")
def oracle_stack(scenes, oracle_api):
    """QUALITY's experiment (tests/test_adaptive_cpu.py): the oracle's samples of 96 frames, one at a time, and its 256-frame reference"""
    q = QUALITY
    w, h = q["width"], q["height"]
    o = oracle_api.OracleScene()
    getattr(scenes, q["scene"])(o)
    o.set_raytracer(False)
    r = oracle_api.OracleRenderer(o, w, h)
    S = np.zeros((q["stack_frames"], h, w, 3), F32)
    for f in range(q["stack_frames"]):
        r.clear()
        r.render(f, 1, nthreads=0)
        S[f] = r.accumulator()[..., :3]
    r.clear()
    r.render(q["reference_frame0"], q["reference_frames"], nthreads=0)
    ref = r.accumulator()[..., :3].astype(np.float64) / q["reference_frames"]
    r.close()
    o.close()
    return S, ref


def test_dilated_loop_on_the_oracle(oracle_stack):
    """The loop of rt_select_budget_dilated (pass_cap 1) / rt_render_budget in numpy on the oracle's samples of QUALITY: config 2's scene
    at 320 x 180, 16 whole frames, threshold 0.02, a pixel's k-th sample is frame k.
    To termination with max_samples 64: count_dilated >= count_undilated at every pixel (a pixel's state is a function of its count, and
    it is listed at least as long as it is raw-active), and no raw-active pixel is left.
    At the budget of 32 frames' worth of samples: pixels that stopped at count 16 with a mean more than 10 % off the 256-frame reference.
    Oracle result: 20 undilated, 0 at radius 1, 0 at radius 2.  Asserted: undilated >= 8 and 4 * dilated(r = 1) <= undilated.
    The MSE ratios dilated / undilated are printed, not asserted (0.985 at the same budget: too close to 1 to bar)."""
    q = QUALITY
    S, ref = oracle_stack
    px = q["width"] * q["height"]
    params = dict(q["params"])
    # radius 0 of the restated loop is adaptive_ref's own loop
    a0, c0, t0 = dr.dilated_loop(S, q["budget_frames"] * px, 0, **params)
    a_ref, c_ref, t_ref = ar.adaptive_loop(S, q["budget_frames"] * px, **params)
    assert np.array_equal(c0, c_ref) and t0 == t_ref and np.array_equal(a0, a_ref, equal_nan=True)
    wrong0, fin = stopped_and_wrong(a0, c0, S, ref, params["min_samples"])
    a1, c1, t1 = dr.dilated_loop(S, q["budget_frames"] * px, 1, **params)
    a2, c2, t2 = dr.dilated_loop(S, q["budget_frames"] * px, 2, **params)
    wrong1 = stopped_and_wrong(a1, c1, S, ref, params["min_samples"])[0]
    wrong2 = stopped_and_wrong(a2, c2, S, ref, params["min_samples"])[0]
    m0 = mse(a0, c0, ref, fin)
    print("stopped and wrong at %d frames' worth: undilated %d, radius 1 %d, radius 2 %d; samples %d / %d / %d; MSE %.4g, radius 1 / undilated %.3f, radius 2 / undilated %.3f"
          % (q["budget_frames"], wrong0, wrong1, wrong2, t0, t1, t2, m0, mse(a1, c1, ref, fin) / m0, mse(a2, c2, ref, fin) / m0))
    assert max(t0, t1, t2) <= q["budget_frames"] * px
    assert wrong0 >= 8, wrong0
    assert 4 * wrong1 <= wrong0, (wrong1, wrong0)
    # to termination: without a budget the loop ends only on an empty list, which is an empty raw mask
    ends = dict(params, max_samples=64)
    e0 = dr.dilated_loop(S, None, 0, **ends)
    for r in (1, 2):
        e = dr.dilated_loop(S, None, r, **ends)
        assert (e[1] >= e0[1]).all(), r
        assert e[1].max() <= 64 and e[2] >= e0[2]
        print("to the end with max_samples 64, radius %d: %d samples (undilated %d, +%.2f %%), MSE / undilated %.3f"
              % (r, e[2], e0[2], 100.0 * (e[2] - e0[2]) / e0[2], mse(e[0], e[1], ref, fin) / mse(e0[0], e0[1], ref, fin)))
