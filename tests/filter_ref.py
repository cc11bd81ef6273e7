"""numpy float32 restatement of the pixel filter of path-mode camera samples (include/rt_amd.h rt_set_pixel_filter): both random streams,
the three offset rules, primary_ray_f for the pinhole camera, and the accumulation over frames through the oracle's Sample on the
restated rays.  No device and no product code: the tests hold the device against this."""
import numpy as np

REFERENCE, POINT, BOX, TENT = 0, 1, 2, 3
KINDS = {"point": POINT, "box": BOX, "tent": TENT}
GAMMA = np.float32(0.57142857142857142857143)
f32 = np.float32


def wang_hash(s):
    s = np.asarray(s, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = (s ^ np.uint32(61)) ^ (s >> np.uint32(16))
        s = s * np.uint32(9)
        s = s ^ (s >> np.uint32(4))
        s = s * np.uint32(0x27d4eb2d)
        s = s ^ (s >> np.uint32(15))
    return s


def stream_seed(index):
    """StreamSeed: InitSeed(index) = WangHash((index + 1) * 17), the zero state remapped to 0x9E3779B9"""
    index = np.asarray(index, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s = wang_hash((index + np.uint32(1)) * np.uint32(17))
    return np.where(s == 0, np.uint32(0x9E3779B9), s).astype(np.uint32)


def random_float(seed):
    """one xorshift32 step on every state: (the new states, RandomFloat = (float)state * 2^-32)"""
    s = np.asarray(seed, dtype=np.uint32).copy()
    s ^= s << np.uint32(13)
    s ^= s >> np.uint32(17)
    s ^= s << np.uint32(5)
    return s, s.astype(np.float32) * f32(2.3283064365387e-10)


def sample_index(w, h, frame, seed_base):
    """s = seed_base + pixel + frame * W * H (uint32, wrapping) for every pixel, in pixel order"""
    p = np.arange(w * h, dtype=np.uint64)
    return ((int(seed_base) + p + (int(frame) & 0xFFFFFFFF) * (w * h)) & 0xFFFFFFFF).astype(np.uint32)


def offset(kind, u):
    """the offset rule of one axis from a uniform draw u of [0, 1] (float32 in, float32 out)"""
    u = np.asarray(u, dtype=np.float32)
    if kind == POINT:
        return np.zeros_like(u)
    if kind == BOX:
        return u - f32(0.5)
    if kind == TENT:
        with np.errstate(invalid="ignore"):
            lo = np.sqrt(f32(2) * u) - f32(1)
            hi = f32(1) - np.sqrt(f32(2) - f32(2) * u)
        return np.where(u < f32(0.5), lo, hi).astype(np.float32)
    raise ValueError(kind)


def offsets(kind, s):
    """(dx, dy) of the samples with index s: the jitter stream StreamSeed(~s), two draws"""
    js = stream_seed(~np.asarray(s, dtype=np.uint32))
    js, u1 = random_float(js)
    js, u2 = random_float(js)
    return offset(kind, u1), offset(kind, u2)


def primary_ray_f(cam, w, h, fx, fy):
    """primary_ray on u = fx * (1.0f / W), v = fy * (1.0f / H): cam is (cam_pos, top_left, top_right, bottom_left); (O, D) float32 (n, 3)"""
    pos, tl, tr, bl = [np.asarray(v, dtype=np.float32) for v in cam]
    fx, fy = np.asarray(fx, dtype=np.float32), np.asarray(fy, dtype=np.float32)
    u = (fx * (f32(1.0) / f32(w)))[:, None]
    v = (fy * (f32(1.0) / f32(h)))[:, None]
    P = (tl + u * (tr - tl)) + v * (bl - tl)
    d = (P - pos).astype(np.float32)
    dot = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inv = f32(1.0) / np.sqrt(dot)
    D = (d * inv[:, None]).astype(np.float32)
    O = np.broadcast_to(pos, D.shape).astype(np.float32).copy()
    return O, D


def pixel_xy(w, h):
    p = np.arange(w * h)
    return (p % w).astype(np.float32), (p // w).astype(np.float32)


def rays(kind, cam, w, h, frame, seed_base):
    """the camera rays of one frame's samples, in pixel order"""
    x, y = pixel_xy(w, h)
    dx, dy = offsets(kind, sample_index(w, h, frame, seed_base))
    return primary_ray_f(cam, w, h, x + dx, y + dy)


def gamma(c):
    """the per-sample gamma: (float)pow((double)c, (double)GAMMA)"""
    with np.errstate(invalid="ignore"):
        return np.power(np.asarray(c, dtype=np.float32).astype(np.float64), np.float64(GAMMA)).astype(np.float32)


def accumulate(orr, kind, cam, frame0, nframes, seed_base, ray_fn=None):
    """the accumulator (h, w, 3) after frames [frame0, frame0 + nframes): per frame the oracle's Sample (depth 4, the scene at
    set_raytracer(False)) on the frame's rays in pixel order, stream i starting at StreamSeed(seed_base + f * W * H + i) with nothing
    drawn, the per-sample gamma, added in frame order"""
    w, h = orr.w, orr.hgt
    acc = np.zeros((w * h, 3), np.float32)
    for f in range(frame0, frame0 + nframes):
        O, D = (ray_fn or rays)(kind, cam, w, h, f, seed_base)
        L = orr.trace_rays(1, O, D, depth=4, seed_base=(int(seed_base) + (f & 0xFFFFFFFF) * w * h) & 0xFFFFFFFF)
        acc = acc + gamma(L)
    return acc.reshape(h, w, 3)
