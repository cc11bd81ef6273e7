"""numpy float32 restatement of the thin lens of path-mode camera samples (include/rt_amd.h rt_set_lens), on top of tests/filter_ref.py's
streams, offsets and pixel order: the lens point by rejection on the jitter stream behind the filter's draws, lam, the focal point of the
pinhole ray, the origin on the lens disk and the ray from there; rt_focus_at's distance.  No device and no product code: the tests hold
the device against this."""
import numpy as np

import filter_ref as fr

f32 = np.float32
TRIES = 16  # RT_LENS_TRIES


def dot(a, b):
    """(a.x * b.x + a.y * b.y) + a.z * b.z, float32, over the last axis"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(f32)


def normalize(v):
    """v * (1.0f / sqrtf(dot(v, v))), per component"""
    v = np.asarray(v, f32)
    inv = f32(1.0) / np.sqrt(dot(v, v))
    return (v * np.asarray(inv, f32)[..., None]).astype(f32)


def camera(cam):
    """(cam_pos, TL, TR, BL, A, B, N) as float32 vectors"""
    pos, tl, tr, bl = [np.asarray(v, f32) for v in cam]
    A, B = tr - tl, bl - tl
    return pos, tl, tr, bl, A, B, cross(A, B)


def screen_dist(cam):
    pos, tl, _, _, _, _, N = camera(cam)
    return np.abs(dot(tl - pos, N)) / np.sqrt(dot(N, N))


def lam(cam, focus):
    return f32(focus) / screen_dist(cam)


def lens_points(kind, s):
    """(a, b, fallback) of the samples with index s: pairs ca, cb = RandomFloat(js) * 2 - 1 from the jitter stream StreamSeed(~s), behind the
    two draws a BOX / TENT offset took, until ca * ca + cb * cb <= 1; fallback marks the samples refused TRIES times (a = b = 0)"""
    js = fr.stream_seed(~np.asarray(s, dtype=np.uint32))
    if kind != fr.POINT:
        js, _ = fr.random_float(js)
        js, _ = fr.random_float(js)
    a, b = np.zeros(js.shape, f32), np.zeros(js.shape, f32)
    todo = np.ones(js.shape, bool)
    for _ in range(TRIES):
        js, r1 = fr.random_float(js)
        ca = r1 * f32(2) - f32(1)
        js, r2 = fr.random_float(js)
        cb = r2 * f32(2) - f32(1)
        ok = todo & (ca * ca + cb * cb <= f32(1.0))
        a, b = np.where(ok, ca, a), np.where(ok, cb, b)
        todo &= ~ok
    return a.astype(f32), b.astype(f32), todo


def focal_points(kind, cam, w, h, frame, seed_base, focus):
    """F = cam + lam * (P - cam) of every sample of the frame, P = (TL + u * A) + v * B"""
    pos, tl, _, _, A, B, _ = camera(cam)
    x, y = fr.pixel_xy(w, h)
    dx, dy = fr.offsets(kind, fr.sample_index(w, h, frame, seed_base))
    u = ((x + dx) * (f32(1.0) / f32(w)))[:, None]
    v = ((y + dy) * (f32(1.0) / f32(h)))[:, None]
    P = (tl + u * A) + v * B
    return (pos + lam(cam, focus) * (P - pos)).astype(f32)


def rays(kind, cam, w, h, frame, seed_base, radius, focus):
    """the camera rays (O, D), float32 (w * h, 3), of one frame's samples under the lens, in pixel order"""
    pos, _, _, _, A, B, _ = camera(cam)
    radius = f32(radius)
    F = focal_points(kind, cam, w, h, frame, seed_base, focus)
    a, b, _ = lens_points(kind, fr.sample_index(w, h, frame, seed_base))
    O = ((pos + (a * radius)[:, None] * normalize(A)) + (b * radius)[:, None] * normalize(B)).astype(f32)
    return O, normalize(F - O)


def ray_fn(radius, focus):
    """the adapter filter_ref.accumulate(..., ray_fn=...) takes"""
    return lambda kind, cam, w, h, frame, seed_base: rays(kind, cam, w, h, frame, seed_base, radius, focus)


def focus_distance(cam, t, D):
    """rt_focus_at's distance of a hit at t along the unit direction D: t * (fabsf(dot(D, N)) / sqrtf(dot(N, N)))"""
    N = camera(cam)[6]
    return (np.asarray(t, f32) * (np.abs(dot(D, N)) / np.sqrt(dot(N, N)))).astype(f32)
