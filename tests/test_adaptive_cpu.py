"""Adaptive sampling without a device: the numpy restatement (tests/adaptive_ref.py) on crafted moments, and the adaptive loop run on
the oracle's own per-frame samples -- the evidence that the device test of the same loop (tests/test_gpu_adaptive.py) can be met."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref as ar  # noqa: E402

F32 = np.float32
# The quality experiment, fixed here on the CPU and used unchanged by tests/test_gpu_adaptive.py: BASELINE config 2's scene
# (scenes.config2: the three.obj scene, every material diffuse, one area light) at 320 x 180, default camera.
QUALITY = dict(scene="config2", width=320, height=180, stack_frames=96, budget_frames=32, reference_frames=256, reference_frame0=1000,
               params=dict(min_samples=16, max_samples=1024, threshold=0.02, floor=1e-3))


def _moments_of(values):
    """(count, sum_y, sum_yy) of one pixel that received the grey samples 'values' in order"""
    v = np.asarray(values, F32)
    s = np.repeat(v[:, None, None], 3, axis=2)  # [frame][1 pixel][rgb]
    c, sy, syy = ar.moments(s)
    return int(c[0]), sy[0], syy[0]


def test_luminance_and_moments_are_sequential_f32():
    rng = np.random.default_rng(3)
    s = rng.random((20, 7, 3)).astype(F32)
    y = ar.luminance(s)
    assert y.dtype == F32
    # the order of the three terms: (r + g) + b, every product and sum rounded to f32
    want = (F32(0.2126) * s[..., 0] + F32(0.7152) * s[..., 1]).astype(F32) + F32(0.0722) * s[..., 2]
    assert np.array_equal(y, want.astype(F32))
    c, sy, syy = ar.moments(s)
    a, b = np.zeros(7, F32), np.zeros(7, F32)
    for f in range(20):
        a, b = (a + y[f]).astype(F32), (b + (y[f] * y[f]).astype(F32)).astype(F32)
    assert np.all(c == 20) and np.array_equal(sy, a) and np.array_equal(syy, b)
    # any split of the frames gives the same bits
    c1, sy1, syy1 = ar.moments(s[:3])
    c2, sy2, syy2 = ar.moments(s[3:], c1, sy1, syy1)
    assert np.array_equal(c2, c) and np.array_equal(sy2, sy) and np.array_equal(syy2, syy)
    # +inf samples (a directly viewed light) sum to +inf, by class
    s[5, 2] = np.inf
    _, sy, syy = ar.moments(s)
    assert np.isposinf(sy[2]) and np.isposinf(syy[2]) and np.isfinite(sy[[0, 1, 3, 4, 5, 6]]).all()


def test_crafted_moments():
    P = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
    # a constant pixel: v is exactly 0 (sum_yy - sum_y * m cancels: 0.5 and its sums are exact), never active past min_samples
    c, sy, syy = _moments_of([0.5] * 8)
    assert ar.relative_error(c, sy, syy, P["floor"]) == 0 and not ar.active_mask(c, sy, syy, **P)
    assert not ar.active_mask(c, sy, syy, **dict(P, threshold=0.0))  # e / d > 0 is false for e == 0
    # count < min_samples: active whatever the moments say (a constant pixel, an infinite one, count 0 and 1)
    for k in (0, 1, 3):
        assert ar.active_mask(k, F32(0.5 * k), F32(0.25 * k), **P)
        assert ar.active_mask(k, F32(np.inf), F32(np.inf), **P)
    # a noisy pixel, and the threshold one ulp either side of its e / d
    c, sy, syy = _moments_of([0.1, 0.9, 0.2, 0.8, 0.3, 0.7, 0.5, 0.4])
    r = ar.relative_error(c, sy, syy, P["floor"])
    assert r > 0.05 and ar.active_mask(c, sy, syy, **P)
    below, above = np.nextafter(r, F32(0)), np.nextafter(r, F32(np.inf))
    assert ar.active_mask(c, sy, syy, **dict(P, threshold=below))
    assert not ar.active_mask(c, sy, syy, **dict(P, threshold=r))      # strictly greater
    assert not ar.active_mask(c, sy, syy, **dict(P, threshold=above))
    assert not ar.active_mask(c, sy, syy, **dict(P, threshold=np.inf))
    # count == max_samples: never active; one below: still active
    assert not ar.active_mask(64, sy, syy, **P)
    assert not ar.active_mask(8, sy, syy, **dict(P, max_samples=8)) and ar.active_mask(8, sy, syy, **dict(P, max_samples=9))
    # +inf and NaN sums: never active once they have min_samples
    for bad in (np.inf, -np.inf, np.nan):
        assert not ar.active_mask(8, F32(bad), F32(1.0), **P) and not ar.active_mask(8, F32(1.0), F32(bad), **P)
        assert not ar.active_mask(8, F32(bad), F32(bad), **dict(P, threshold=0.0))
    # a mean below the floor: the denominator is the floor, so a dark noisy pixel stops asking
    dark = [1e-5, 3e-5, 0.0, 2e-5, 1e-5, 4e-5, 0.0, 2e-5]
    c, sy, syy = _moments_of(dark)
    m = sy / F32(c)
    assert m < F32(1e-3)
    assert not ar.active_mask(c, sy, syy, **P)                        # e / 1e-3 is small
    assert ar.active_mask(c, sy, syy, **dict(P, floor=1e-7))          # against its own mean it is noisy
    # cancellation: sum_yy - sum_y * m slightly negative is clamped to 0 -- no NaN from the square root, not active
    found = 0
    rng = np.random.default_rng(11)
    for _ in range(4000):
        x = F32(rng.random())
        k = int(rng.integers(5, 40))
        c, sy, syy = _moments_of([x] * k)
        with np.errstate(all="ignore"):
            raw = F32(syy - F32(sy * F32(sy / F32(c))))
        if raw < 0:
            found += 1
            r = ar.relative_error(c, sy, syy, P["floor"])
            assert r == 0 and not np.isnan(r) and not ar.active_mask(c, sy, syy, **P)
    assert found > 10, found
    # the list: ascending pixel indices of the mask
    cnt = np.array([[8, 2, 8], [8, 8, 0]], np.uint32)
    sy = np.array([[4, 1, np.inf], [4, 4.2, 0]], F32)
    syy = np.array([[2, 1, np.inf], [2, 4.1, 0]], F32)
    lst = ar.active_list(cnt, sy, syy, **P)
    assert lst.dtype == np.uint32 and lst.tolist() == [1, 4, 5] and np.all(np.diff(lst.astype(np.int64)) > 0)


def test_resolve_with_per_pixel_counts():
    import resolve_ref
    rng = np.random.default_rng(2)
    acc = (rng.random((5, 6, 4)) * 40).astype(F32)
    cnt = rng.integers(0, 50, (5, 6)).astype(np.uint32)
    cnt[0, 0], cnt[4, 5] = 0, 0
    acc[1, 1, 0], acc[2, 2, 1] = np.inf, np.nan
    got = ar.resolve(acc, cnt)
    for i in np.ndindex(cnt.shape):
        want = 0 if cnt[i] == 0 else resolve_ref.resolve(acc[i], int(cnt[i]))
        assert got[i] == want, (i, got[i], want)


def quality_ratio(samples, reference):
    """MSE of the adaptive loop's means against 'reference' over MSE of the uniform render of the same budget (budget_frames whole
    frames); on the pixels whose reference and samples are finite (a directly viewed light is +inf in both renders).  Also the samples the
    adaptive loop took and the largest count."""
    q = QUALITY
    px = q["width"] * q["height"]
    acc, cnt, total = ar.adaptive_loop(samples, q["budget_frames"] * px, **q["params"])
    uni = samples[:q["budget_frames"], ..., :3].astype(np.float64).mean(0)
    fin = np.isfinite(reference).all(-1) & np.isfinite(samples[..., :3]).all(-1).all(0)
    with np.errstate(all="ignore"):
        ada = acc / cnt[..., None]
    mse_a = ((ada[fin] - reference[fin]) ** 2).mean()
    mse_u = ((uni[fin] - reference[fin]) ** 2).mean()
    return float(mse_a / mse_u), total, int(cnt.max()), int(fin.sum())


def test_adaptive_loop_beats_uniform_on_the_oracle(scenes, oracle_api):
    """The loop of rt_select_active / rt_render_active, entirely in numpy on the oracle's samples.  BASELINE config 2's scene at 320 x 180:
    96 frames rendered one at a time (clear() between, so the accumulator is that frame's sample), a reference mean of 256 further
    frames (1000 .. 1255: independent of the samples).  Adaptive: 16 whole frames, then threshold 0.02, floor 1e-3, max 1024, until the next
    frame would pass the budget of 32 frames' worth of samples (1,843,200); uniform: 32 whole frames.
    Oracle result: MSE ratio adaptive / uniform = 0.600 (99.8 % of the budget used, largest count 59 of the 96 recorded frames,
    38,596 of 57,600 pixels finite -- the rest view the area light or sum to a non-finite value in both renders).  Asserted: <= 0.8.
    Cost: about 2 s of oracle rendering for the samples, 4 s for the reference, 8 threads; nothing is cached."""
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
    ratio, total, most, finite = quality_ratio(S, ref)
    print("oracle adaptive / uniform MSE ratio %.3f, %d of %d samples, largest count %d, %d finite pixels" % (ratio, total, q["budget_frames"] * w * h, most, finite))
    assert most < q["stack_frames"], "the loop ran out of recorded frames"
    assert total <= q["budget_frames"] * w * h
    assert ratio <= 0.8, ratio


# ---- the sizes, masks and lists of tests/test_gpu_adaptive_shapes.py ---------------------------------------------------------------
import pytest  # noqa: E402

import adaptive_shapes as sh  # noqa: E402

LARGE_ONLY = ("full_to_1023", "full_from_1024", "scan_lane_mid", "scan_lane_last")


def _per(mask, unit):
    """(active pixels, pixels) of every run of 'unit' consecutive pixels (the last run may be short)"""
    n = len(mask)
    starts = np.arange(0, n, unit)
    return np.add.reduceat(mask.astype(np.int64), starts), np.minimum(unit, n - starts)


@pytest.mark.parametrize("size", list(sh.SIZES), ids=lambda s: "%dx%d" % s)
def test_shape_sizes_reach_the_edges_they_are_listed_for(size):
    w, h = size
    n, blocks, per = sh.SIZES[size]
    assert n == w * h
    assert sh.geometry(n)[:2] == (blocks, per)
    assert blocks == -(-n // 256) and per == -(-blocks // 1024)  # the library's two constants, written out
    _, _, owners, last_owns = sh.geometry(n)
    last_block = n - (blocks - 1) * 256
    want = {(1, 1): (1, 1, 1), (63, 1): (1, 1, 63), (65, 1): (1, 1, 65), (255, 1): (1, 1, 255), (257, 3): (4, 1, 3), (97, 41): (16, 1, 137),
            (641, 409): (513, 1, 25), (1280, 721): (902, 1, 256), (1279, 721): (901, 3, 47)}[size]
    assert (owners, last_owns, last_block) == want
    assert owners <= 1024 and (owners - 1) * per + last_owns == blocks
    if size == (97, 41):
        assert last_block % 64 != 0 and last_block > 64          # the last wave of the last block is partial, and not its only wave
    if per > 1:
        assert last_owns < per                                   # a last owning lane whose run is short
        assert owners < 1024                                     # lanes past the end: first and last both clamped to blocks
        assert sh.scan_lane_blocks(n, owners) == (blocks, blocks) and sh.scan_lane_blocks(n, 1023) == (blocks, blocks)
        assert sh.scan_lane_blocks(n, owners - 1) == (blocks - last_owns, blocks)
        assert sh.scan_lane_blocks(n, 64) == (64 * per, 65 * per)


@pytest.mark.parametrize("size", list(sh.SIZES), ids=lambda s: "%dx%d" % s)
def test_shape_masks_are_what_their_names_say(size):
    w, h = size
    n, blocks, per = sh.SIZES[size]
    got = dict(sh.masks(w, h))
    # which masks a size leaves out, and why: each would be another mask of the table
    absent = set(sh.MASKS) - set(got)
    want_absent = set()
    if n == 1:
        want_absent |= {"first", "last", "every_other", "seeded_30"}
    if blocks == 1:
        want_absent |= {"last_block", "all_but_last_block", "alternate_blocks"}
    if n <= 64:
        want_absent |= {"lane0"}
    if n < 64:
        want_absent |= {"lane63"}
    if h == 1:
        want_absent |= {"one_row"}
    if n < 2000:
        want_absent |= {"seeded_01"}
    if per == 1:
        want_absent |= set(LARGE_ONLY)
    assert absent == want_absent
    seen = {}
    for name, m in got.items():
        assert m.dtype == bool and m.shape == (n,), name
        key = m.tobytes()
        # no two masks of a size are the same mask; only the scan's own may repeat a block mask (1025 blocks: the block past the scan's
        # lanes is the last one; a last scan lane that owns one entry owns the last block)
        assert key not in seen or name in LARGE_ONLY, (name, seen.get(key))
        seen[key] = name
        lst = sh.complement_list(m)
        assert sh.acceptable(lst, n) and len(lst) == n - int(m.sum()), name
        assert np.array_equal(np.flatnonzero(m), np.setdiff1d(np.arange(n), lst)), name
        b, bsize = _per(m, 256)
        v, vsize = _per(m, 64)
        assert len(b) == blocks
        if name == "all":
            assert np.array_equal(b, bsize) and np.array_equal(v, vsize)
        elif name == "none":
            assert not b.any()
        elif name == "first":
            assert m[0] and m.sum() == 1
        elif name == "last":
            assert m[n - 1] and m.sum() == 1 and b[-1] == 1
        elif name == "last_block":
            assert not b[:-1].any() and b[-1] == bsize[-1] == n - (blocks - 1) * 256
        elif name == "all_but_last_block":
            assert np.array_equal(b[:-1], bsize[:-1]) and b[-1] == 0
        elif name == "alternate_blocks":
            assert np.array_equal(b[0::2], bsize[0::2]) and not b[1::2].any()
        elif name == "lane0":
            assert np.all(v == 1) and m[::64].all()
        elif name == "lane63":
            assert np.array_equal(v, (vsize == 64).astype(np.int64)) and m[63::64].all()
        elif name == "every_other":
            assert np.array_equal(v, (vsize + 1) // 2) and m[::2].all()
        elif name == "one_row":
            assert m.sum() == w and m.reshape(h, w)[h // 2].all()
        elif name == "seeded_30":
            assert 0 < m.sum() < n and abs(m.mean() - 0.3) < 4 * np.sqrt(0.21 / n)
            if blocks > 1:
                assert np.all(b[:-1] > 0) and np.all(b < bsize)  # no block empty, none full: the middling totals
        elif name == "seeded_01":
            assert m.sum() == (n + 500) // 1000
            if blocks > 16:
                assert (b == 0).mean() > 0.5                     # most blocks total 0
        elif name == "full_to_1023":
            assert np.all(b[:1024] == 256) and not b[1024:].any() and blocks > 1024
        elif name == "full_from_1024":
            assert not b[:1024].any() and np.array_equal(b[1024:], bsize[1024:])
        elif name == "scan_lane_mid":
            assert np.all(b[64 * per:65 * per] == 256) and m.sum() == 256 * per
        elif name == "scan_lane_last":
            _, _, owners, last_owns = sh.geometry(n)
            assert np.array_equal(b[blocks - last_owns:], bsize[blocks - last_owns:]) and not b[:blocks - last_owns].any()
            assert last_owns == {(641, 409): 1, (1280, 721): 1, (1279, 721): 3}[size]
        else:
            raise AssertionError("no check for mask " + name)
    # the acceptance rule itself
    assert sh.acceptable(np.zeros(0, np.uint32), n) and not sh.acceptable(np.array([n], np.uint32), n)
    assert not sh.acceptable(np.array([0, 0], np.uint32), max(n, 2)) and not sh.acceptable(np.array([1, 0], np.uint32), max(n, 2))


def test_shape_lists():
    for w, h in ((97, 41), (96, 64), (257, 3), (641, 409)):
        n = w * h
        for seed, density in ((5, 0.3), (9, 0.3), (11, 0.6)):
            lst = sh.seeded_list(w, h, seed, density)
            assert sh.acceptable(lst, n) and lst[0] == 0 and lst[-1] == n - 1
            assert abs(len(lst) / n - density) < 0.05, (w, h, len(lst) / n)
            row = np.arange((h // 3) * w, (h // 3 + 1) * w)
            assert np.isin(row, lst).all()
        row = sh.last_row_list(w, h)
        assert sh.acceptable(row, n) and len(row) == w and np.all(row // w == h - 1)
        cols = sh.side_columns_list(w, h)
        assert sh.acceptable(cols, n) and len(cols) == 2 * h and set(np.unique(cols % w)) == {0, w - 1}
    # the RT_SLOTS branches the device test asks for, from the lengths of its lists
    for w, h in ((97, 41), (96, 64)):
        k = len(sh.seeded_list(w, h))
        assert k >= 1025                                         # the list lengths the device test cuts from it
        assert sh.slots_branch(777, k, 4) == ("recycle", 4)
        assert sh.slots_branch(2000, k, 4) == ("own", 1) and sh.slots_branch(2000, k, 7) == ("own", 1)
        assert sh.slots_branch(4096, k, 4) == ("own", 2 if (w, h) == (96, 64) else 3)
        assert sh.slots_branch(4096, k, 7)[1] in (2, 3)          # 7 frames: 2 + 2 + 2 + 1, or 3 + 3 + 1
        assert sh.slots_branch(1 << 28, k, 4) == ("own", 4)
