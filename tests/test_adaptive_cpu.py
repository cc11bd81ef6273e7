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
