"""numpy float32 restatement of the shutter of path-mode camera samples (include/rt_amd.h rt_set_shutter), on top of tests/filter_ref.py's
streams, offsets and pixel order and tests/lens_ref.py's vector operations: the time tau on the jitter stream behind the filter's draws, the
camera interpolated to it float by float, the pinhole ray of that camera, or the thin-lens ray of it with lam evaluated per sample and the
rejection pairs drawn behind tau.  No device and no product code: the tests hold the device against this."""
import numpy as np

import filter_ref as fr
import lens_ref as lr

f32 = np.float32


def jitter_stream(kind, s):
    """the jitter stream StreamSeed(~s) of the samples with index s behind the filter's draws (two for BOX / TENT, none for POINT)"""
    js = fr.stream_seed(~np.asarray(s, dtype=np.uint32))
    if kind != fr.POINT:
        js, _ = fr.random_float(js)
        js, _ = fr.random_float(js)
    return js


def times(kind, s):
    """tau of the samples with index s: one RandomFloat of the jitter stream behind the filter's draws; the closed interval [0, 1]"""
    return fr.random_float(jitter_stream(kind, s))[1]


def cameras(cam_open, cam_close, tau):
    """X(tau) = X0 + tau * (X1 - X0) for the twelve floats: (cam_pos, TL, TR, BL), each float32 (n, 3)"""
    tau = np.asarray(tau, f32)[:, None]
    out = []
    for x0, x1 in zip(cam_open, cam_close):
        x0, x1 = np.asarray(x0, f32), np.asarray(x1, f32)
        out.append((x0 + tau * (x1 - x0)).astype(f32))
    return out


def lens_points(kind, s):
    """lens_ref.lens_points one draw later: the rejection pairs continue on the jitter stream behind tau; (a, b, fallback)"""
    js, _ = fr.random_float(jitter_stream(kind, s))
    a, b = np.zeros(js.shape, f32), np.zeros(js.shape, f32)
    todo = np.ones(js.shape, bool)
    for _ in range(lr.TRIES):
        js, r1 = fr.random_float(js)
        ca = r1 * f32(2) - f32(1)
        js, r2 = fr.random_float(js)
        cb = r2 * f32(2) - f32(1)
        ok = todo & (ca * ca + cb * cb <= f32(1.0))
        a, b = np.where(ok, ca, a), np.where(ok, cb, b)
        todo &= ~ok
    return a.astype(f32), b.astype(f32), todo


def rays(kind, cam_open, cam_close, w, h, frame, seed_base, radius=0, focus=1):
    """the camera rays (O, D), float32 (w * h, 3), of one frame's samples with the shutter on, in pixel order"""
    s = fr.sample_index(w, h, frame, seed_base)
    x, y = fr.pixel_xy(w, h)
    if kind == fr.POINT:
        dx = dy = np.zeros(len(s), f32)
    else:
        dx, dy = fr.offsets(kind, s)
    u = ((x + dx) * (f32(1.0) / f32(w)))[:, None]
    v = ((y + dy) * (f32(1.0) / f32(h)))[:, None]
    pos, tl, tr, bl = cameras(cam_open, cam_close, times(kind, s))
    A, B = tr - tl, bl - tl
    P = (tl + u * A) + v * B
    if not radius > 0:
        return pos.copy(), lr.normalize(P - pos)
    radius = f32(radius)
    N, E = lr.cross(A, B), tl - pos
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = f32(focus) / (np.abs(lr.dot(E, N)) / np.sqrt(lr.dot(N, N)))
    F = (pos + lam[:, None] * (P - pos)).astype(f32)
    a, b, _ = lens_points(kind, s)
    O = ((pos + (a * radius)[:, None] * lr.normalize(A)) + (b * radius)[:, None] * lr.normalize(B)).astype(f32)
    return O, lr.normalize(F - O)


def ray_fn(cam_close, radius=0, focus=1):
    """the adapter filter_ref.accumulate(..., ray_fn=...) takes: 'cam' there is the camera at shutter open"""
    return lambda kind, cam, w, h, frame, seed_base: rays(kind, cam, cam_close, w, h, frame, seed_base, radius, focus)
