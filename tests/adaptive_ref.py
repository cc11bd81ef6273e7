"""numpy restatement of the adaptive-sampling definitions of include/rt_amd.h: the luminance of a sample, the per-pixel moments
k_accumulate<true> keeps, the predicate of rt_select_active and the per-count resolve of rt_resolve_adaptive.  A plain helper module of
the test suite: tests/test_adaptive_cpu.py probes it on crafted moments and runs the adaptive loop on the oracle's samples,
tests/test_gpu_adaptive.py holds the kernels against it bit for bit.

Everything is f32, one rounding per operation (numpy float32 arithmetic does exactly that; the library is built without contraction):
  y = (0.2126 r + 0.7152 g) + 0.0722 b                 of the sample as it is added to the accumulator
  count += 1, sum_y += y, sum_yy += y y                one sample at a time, in frame order
  n = f32(count); m = sum_y / n; v = (sum_yy - sum_y m) / (n - 1); v = v > 0 ? v : 0; e = sqrt(v / n); d = m > floor ? m : floor
  active = count < min_samples || (count < max_samples && isfinite(sum_y) && isfinite(sum_yy) && e / d > threshold)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resolve_ref  # noqa: E402

F32 = np.float32
DEFAULTS = dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3)


def luminance(rgb):
    """(..., >= 3) float32 samples -> float32 luminance (...)"""
    s = np.asarray(rgb, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((F32(0.2126) * s[..., 0] + F32(0.7152) * s[..., 1]).astype(F32) + F32(0.0722) * s[..., 2]).astype(F32)


def moments(samples, count=None, sum_y=None, sum_yy=None):
    """[frame][pixel...][>= 3] samples, added in frame order to (count, sum_y, sum_yy) (zeros when not given) -> the three arrays"""
    samples = np.asarray(samples, F32)
    shape = samples.shape[1:-1]
    count = np.zeros(shape, np.uint32) if count is None else np.array(count, np.uint32)
    sum_y = np.zeros(shape, F32) if sum_y is None else np.array(sum_y, F32)
    sum_yy = np.zeros(shape, F32) if sum_yy is None else np.array(sum_yy, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(samples.shape[0]):
            y = luminance(samples[f])
            sum_y = (sum_y + y).astype(F32)
            sum_yy = (sum_yy + (y * y).astype(F32)).astype(F32)
            count = count + np.uint32(1)
    return count, sum_y, sum_yy


def relative_error(count, sum_y, sum_yy, floor):
    """e / d of the predicate (f32; whatever the inputs give, NaN and inf included)"""
    count = np.asarray(count, np.uint32)
    sy, syy = np.asarray(sum_y, F32), np.asarray(sum_yy, F32)
    with np.errstate(all="ignore"):
        n = count.astype(F32)
        m = (sy / n).astype(F32)
        v = ((syy - (sy * m).astype(F32)).astype(F32) / (n - F32(1)).astype(F32)).astype(F32)
        v = np.where(v > F32(0), v, F32(0)).astype(F32)
        e = np.sqrt((v / n).astype(F32)).astype(F32)
        d = np.where(m > F32(floor), m, F32(floor)).astype(F32)
        return (e / d).astype(F32)


def active_mask(count, sum_y, sum_yy, min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3):
    """the predicate of rt_select_active per pixel (bool, the inputs' shape)"""
    count = np.asarray(count, np.uint32)
    sy, syy = np.asarray(sum_y, F32), np.asarray(sum_yy, F32)
    r = relative_error(count, sy, syy, floor)
    with np.errstate(invalid="ignore"):
        noisy = (count < np.uint32(max_samples)) & np.isfinite(sy) & np.isfinite(syy) & (r > F32(threshold))
    return (count < np.uint32(min_samples)) | noisy


def active_list(count, sum_y, sum_yy, **params):
    """the list rt_select_active builds: pixel indices y * width + x of the active pixels, ascending (uint32)"""
    return np.flatnonzero(active_mask(count, sum_y, sum_yy, **params).reshape(-1)).astype(np.uint32)


def resolve(rgba, count):
    """rt_resolve_adaptive: (..., >= 3) float32 accumulator values and their (...) uint32 counts -> uint32 pixels; count 0 is black"""
    a = np.asarray(rgba, F32)
    count = np.asarray(count, np.uint32)
    with np.errstate(all="ignore"):
        mean = (a[..., :3] / count.astype(F32)[..., None]).astype(F32)
    return np.where(count == 0, np.uint32(0), resolve_ref.resolve(mean, 1)).astype(np.uint32)


def adaptive_loop(samples, budget, min_samples, max_samples, threshold, floor):
    """The loop a caller of rt_select_active / rt_render_active runs, on a recorded [frame][pixel...][>= 3] stack of samples: frames
    0 .. min_samples - 1 whole; then, frame by frame, the active pixels get that frame's sample, until the next frame would take the
    total past 'budget' samples, nothing is active or the stack ends.  Returns (sum of the samples taken per pixel (f64), count, total)."""
    samples = np.asarray(samples, F32)
    shape = samples.shape[1:-1]
    count, sy, syy = moments(samples[:min_samples])
    acc = samples[:min_samples, ..., :3].astype(np.float64).sum(0)
    total = int(count.sum())
    for f in range(min_samples, samples.shape[0]):
        on = active_mask(count, sy, syy, min_samples, max_samples, threshold, floor)
        k = int(on.sum())
        if k == 0 or total + k > budget:
            break
        c1, y1, yy1 = moments(samples[f:f + 1][:, on], count[on], sy[on], syy[on])
        count[on], sy[on], syy[on] = c1, y1, yy1
        acc[on] += samples[f][on][..., :3].astype(np.float64)
        total += k
    assert count.shape == shape
    return acc, count, total
