"""numpy restatement of rt_reproject (include/rt_amd.h): which history pixel every pixel of the new frame takes its samples from, and the
accumulator and statistics the call leaves.  A plain helper module of the test suite: tests/test_reproject_cpu.py probes it on crafted
G-buffers and runs the experiment on the oracle, tests/test_gpu_reproject.py holds k_reproject against it bit for bit.

Everything is f32, one rounding per operation (numpy float32 arithmetic does exactly that; the library is built without contraction):
  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z,  cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
  A = TR' - TL';  B = BL' - TL';  N = cross(A, B);  E = TL' - cam';  d = x_p - cam'
  lam = dot(E, N) / dot(d, N)  (finite, > 0);  Q = lam d - E;  nn = dot(N, N);  u = dot(cross(Q, B), N) / nn;  v = dot(cross(A, Q), N) / nn
  rx = floor(u W + 0.5), ry = floor(v H + 0.5)  (0 <= rx < W, 0 <= ry < H as floats);  q = ry W + rx
  carried = eligible && count'_q > 0 && obj'_q == obj_p && mat'_q == mat_p && dist2(n_p, n'_q) <= ntol ntol
            && |dot(n'_q, x_p - x'_q)| <= ptol t_p

A G-buffer here is a dict of (H, W[, 3]) arrays: pos (f32 xyz), normal (f32 xyz), t (f32), obj (i32, -1: a miss), mat (i32).  A camera is
the (4, 3) f32 array cam_pos, top_left, top_right, bottom_left.  Materials are (type, shinieness) arrays indexed by mat."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=0, carry_view_dependent=0)
RT_MAT_DIFFUSE = 1


def _c(v):
    """the three components of (..., 3) as f32 arrays"""
    v = np.asarray(v, F32)
    return v[..., 0], v[..., 1], v[..., 2]


def dot(a, b):
    (ax, ay, az), (bx, by, bz) = a, b
    return ((ax * bx).astype(F32) + (ay * by).astype(F32)).astype(F32) + (az * bz).astype(F32)


def cross(a, b):
    (ax, ay, az), (bx, by, bz) = a, b
    return ((ay * bz).astype(F32) - (az * by).astype(F32), (az * bx).astype(F32) - (ax * bz).astype(F32), (ax * by).astype(F32) - (ay * bx).astype(F32))


def sub(a, b):
    return tuple((x - y).astype(F32) for x, y in zip(a, b))


def depth_ratio(pos, camera):
    """lam of the definition: the history screen plane's distance over the point's, along the plane's normal (f32; > 0 and finite in
    front of the history camera)"""
    cam, TL, TR, BL = (tuple(F32(c) for c in np.asarray(camera, F32)[k]) for k in range(4))
    with np.errstate(all="ignore"):
        N = cross(sub(TR, TL), sub(BL, TL))
        return (dot(sub(TL, cam), N) / dot(sub(_c(pos), cam), N)).astype(F32)


def project(pos, camera, width, height):
    """(rx, ry, ok): the f32 pixel coordinates of the points 'pos' (..., 3) on the history camera's nearest pixel, and whether the point
    lies in front of the camera and inside the frame"""
    cam, TL, TR, BL = (tuple(F32(c) for c in np.asarray(camera, F32)[k]) for k in range(4))
    with np.errstate(all="ignore"):
        A, B = sub(TR, TL), sub(BL, TL)
        N = cross(A, B)
        E = sub(TL, cam)
        d = sub(_c(pos), cam)
        lam = depth_ratio(pos, camera)
        ok = np.isfinite(lam) & (lam > F32(0))
        Q = tuple(((lam * dk).astype(F32) - ek).astype(F32) for dk, ek in zip(d, E))
        nn = dot(N, N)
        u = (dot(cross(Q, B), N) / nn).astype(F32)
        v = (dot(cross(A, Q), N) / nn).astype(F32)
        rx = np.floor(((u * F32(width)).astype(F32) + F32(0.5)).astype(F32)).astype(F32)
        ry = np.floor(((v * F32(height)).astype(F32) + F32(0.5)).astype(F32)).astype(F32)
        ok = ok & (rx >= F32(0)) & (rx < F32(width)) & (ry >= F32(0)) & (ry < F32(height))
    return rx, ry, ok


def eligible(cur, mat_type, mat_shinieness, carry_view_dependent):
    obj, mat = np.asarray(cur["obj"], np.int32), np.asarray(cur["mat"], np.int32)
    hit = obj != -1
    if carry_view_dependent:
        return hit
    mat_type, sh = np.asarray(mat_type, np.int32).reshape(-1), np.asarray(mat_shinieness, F32).reshape(-1)
    known = (mat >= 0) & (mat < len(mat_type))
    m = np.where(known, mat, 0)
    if len(mat_type) == 0:
        return np.zeros(obj.shape, bool)
    return hit & known & (mat_type[m] == RT_MAT_DIFFUSE) & (sh[m] == F32(0))


def source(cur, hist, hist_count, hist_camera, mat_type, mat_shinieness, normal_tolerance=0.25, plane_tolerance=0.01, max_history=0, carry_view_dependent=0):
    """per pixel of the current G-buffer: the history pixel index it is carried from, -1 where it is not (int64, (H, W)), and the
    eligibility mask"""
    h, w = np.asarray(cur["obj"]).shape
    el = eligible(cur, mat_type, mat_shinieness, carry_view_dependent)
    rx, ry, ok = project(cur["pos"], hist_camera, w, h)
    q = np.where(ok, np.where(ok, ry, 0).astype(np.int64) * w + np.where(ok, rx, 0).astype(np.int64), 0)
    flat = lambda a, *tail: np.asarray(a).reshape((h * w,) + tail)  # noqa: E731
    cnt_q = flat(hist_count)[q]
    obj_q, mat_q = flat(hist["obj"])[q], flat(hist["mat"])[q]
    n_q, x_q = flat(hist["normal"], 3).astype(F32)[q], flat(hist["pos"], 3).astype(F32)[q]
    with np.errstate(all="ignore"):
        dn = sub(_c(cur["normal"]), _c(n_q))
        nd = dot(dn, dn)
        ntol2 = F32(F32(normal_tolerance) * F32(normal_tolerance))
        off = sub(_c(cur["pos"]), _c(x_q))
        pd = np.abs(dot(_c(n_q), off))
        lim = (F32(plane_tolerance) * np.asarray(cur["t"], F32)).astype(F32)
        good = el & ok & (cnt_q > 0) & (obj_q == np.asarray(cur["obj"])) & (mat_q == np.asarray(cur["mat"])) & (nd <= ntol2) & (pd <= lim)
    return np.where(good, q, -1), el


def reproject(cur, hist, hist_acc, hist_count, hist_sum_y, hist_sum_yy, hist_camera, mat_type, mat_shinieness, **params):
    """rt_reproject: (acc (H, W, 4) f32, count u32, sum_y f32, sum_yy f32, n_carried, src, eligible)"""
    P = dict(DEFAULTS, **params)
    src, el = source(cur, hist, hist_count, hist_camera, mat_type, mat_shinieness, **P)
    h, w = src.shape
    on = src >= 0
    q = np.where(on, src, 0)
    acc = np.asarray(hist_acc, F32).reshape(h * w, 4)[q].copy()
    cnt = np.asarray(hist_count, np.uint32).reshape(-1)[q].copy()
    sy = np.asarray(hist_sum_y, F32).reshape(-1)[q].copy()
    syy = np.asarray(hist_sum_yy, F32).reshape(-1)[q].copy()
    mh = int(P["max_history"])
    if mh > 0:
        cap = on & (cnt > np.uint32(mh))
        with np.errstate(all="ignore"):
            f = (F32(mh) / cnt.astype(F32)).astype(F32)
            acc = np.where(cap[..., None], (acc * f[..., None]).astype(F32), acc)
            sy = np.where(cap, (sy * f).astype(F32), sy)
            syy = np.where(cap, (syy * f).astype(F32), syy)
        cnt = np.where(cap, np.uint32(mh), cnt).astype(np.uint32)
    acc[~on] = 0
    cnt[~on], sy[~on], syy[~on] = 0, 0, 0
    return acc, cnt, sy, syy, int(on.sum()), src, el


def gbuffer_of(scene, renderer, t_min=0.001):
    """the G-buffer rt_render_aovs would make, from a scene / renderer pair with primary_rays() and find_nearest() (the oracle's): the
    position is O + D * t in f32, one rounding per operation"""
    O, D = renderer.primary_rays()
    hit = scene.find_nearest(O, D, t_min=t_min)
    h, w = renderer.hgt, renderer.w
    with np.errstate(all="ignore"):
        pos = (O + (D * hit["t"][:, None]).astype(F32)).astype(F32)
    return dict(pos=pos.reshape(h, w, 3), normal=hit["normal"].reshape(h, w, 3), t=hit["t"].reshape(h, w), obj=hit["obj"].reshape(h, w), mat=hit["mat"].reshape(h, w))


class MaterialRecorder:
    """A scene builder that passes every call on to 'builder' and keeps (type, shinieness) of every material it creates, by the index the
    builder returned: the table rt_reproject's eligibility reads."""

    def __init__(self, builder):
        self._b = builder
        self._mats = {}

    def __getattr__(self, name):
        return getattr(self._b, name)

    def diffuse(self, albedo, col, ks=0.2, kd=0.8, n=2, emission=0.0, shininess=0.0, rt=True):
        i = self._b.diffuse(albedo, col, ks, kd, n, emission=emission, shininess=shininess, rt=rt)
        self._mats[int(i)] = (RT_MAT_DIFFUSE, float(shininess))
        return i

    def metal(self, *a, **k):
        i = self._b.metal(*a, **k)
        self._mats[int(i)] = (2, 0.0)
        return i

    def glass(self, *a, **k):
        i = self._b.glass(*a, **k)
        self._mats[int(i)] = (3, 0.0)
        return i

    def tables(self):
        """(type int32, shinieness f32), indexed by material"""
        n = max(self._mats) + 1 if self._mats else 0
        assert sorted(self._mats) == list(range(n)), "material indices are not 0 .. n - 1"
        return np.array([self._mats[i][0] for i in range(n)], np.int32), np.array([self._mats[i][1] for i in range(n)], F32)


# ---- what tests/test_gpu_reproject.py and tests/test_gpu_reproject_motion.py share: the moves, the parameter sets and the histories --------
ADAPTIVE = dict(min_samples=4, max_samples=64, threshold=0.05, floor=1e-3)
MOVES = dict(none=(0.0, 0.0, 0.0), small=(0.05, 0.0, 0.0), large=(0.2, 0.05, 0.1), behind=(0.0, 0.0, -20.0))  # behind: the new camera sees ground that lies behind the old one
PARAMS = dict(defaults={}, view_dependent=dict(carry_view_dependent=1), capped=dict(max_history=8), exact=dict(normal_tolerance=0.0, plane_tolerance=0.0))


def moved(camera, move):
    return (np.asarray(camera, F32) + np.array(move, F32)).astype(F32)


def list_mask(w, h, seed=5):
    """about 60 % of the pixels, never pixel 0 unless it is the only one, always the last"""
    on = np.random.default_rng(seed).random(w * h) < 0.6
    on[0] = False
    on[w * h - 1] = True
    return on


def make_history(r, host_api, kind, w, h):
    """samples for a capture, on a renderer with statistics on: 12 whole frames ('uniform'), an adaptive loop with uneven counts
    ('adaptive'), or 5 frames on list_mask's pixels alone ('list')"""
    PATH = host_api.RT_MODE_PATH
    r.clear()
    if kind == "uniform":
        r.render(PATH, 0, 12)
    elif kind == "adaptive":
        r.render(PATH, 0, ADAPTIVE["min_samples"])
        for f in range(ADAPTIVE["min_samples"], ADAPTIVE["min_samples"] + 6):
            r.select_active(ADAPTIVE)
            r.render_active(f, 1)
    else:
        r.set_active(np.flatnonzero(list_mask(w, h)).astype(np.uint32))
        r.render_active(0, 5)


def materials(r):
    """(type, shinieness) of the materials the renderer's scene uploads (rt_material: 16 words, type at 0, shinieness at 10)"""
    import ctypes as C
    from test_layout_cpu import RtSceneDesc
    d = RtSceneDesc.from_address(r.scene.describe().value)
    n = int(d.n_materials)
    words = np.ctypeslib.as_array(C.cast(d.materials, C.POINTER(C.c_uint32)), shape=(n, 16)).copy()
    return words[:, 0].view(np.int32).copy(), words[:, 10].view(F32).copy()
