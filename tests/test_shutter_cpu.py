"""The shutter of path-mode camera samples on the CPU (include/rt_amd.h rt_set_shutter): tests/shutter_ref.py's restatement draws a uniform
time of its own per sample, behind the filter's draws; a translating closing camera moves every origin of the frames the GPU tier compares bit
for bit (tests/test_gpu_shutter.py is not vacuous), an unmoved one gives the pixel filter's rays, the lens's 16-try fallback stays unused in
those frames one draw later, and the rays of a camera that translates along its screen blur a plane facing it as the geometry predicts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as fr  # noqa: E402
import lens_ref as lr  # noqa: E402
import shutter_ref as sr  # noqa: E402
import test_lens_cpu as lc  # noqa: E402

SKEWED = lc.SKEWED
W, H, FRAMES = 40, 21, 64
SEED = 0x12345678
RADIUS, FOCUS = 0.05, 3.0
MOVE = (0.25, -0.15, 0.1)  # every component >= 0.1 in magnitude
KINDS = (fr.POINT, fr.BOX, fr.TENT)
# what tests/test_gpu_shutter.py compares bit for bit: the ray cases (sizes, frames and seed bases of the lens's tier, under the default
# camera of the size, 24 x 16 under SKEWED), the parity frames 5 .. 7 and the composition's frames 3 .. 14 at 40 x 21
GPU_RAY_SIZES, GPU_RAY_FRAMES = lc.GPU_RAY_SIZES, lc.GPU_RAY_FRAMES
GPU_PARITY_SIZES, GPU_PARITY_FRAMES = [(24, 16), (65, 3)], (5, 6, 7)
GPU_COMPOSE_SIZE, GPU_COMPOSE_FRAMES = (40, 21), tuple(range(0, 15))


def open_camera(w, h):
    """the open camera of the GPU tier at a size: SKEWED at 24 x 16, Camera::Camera for the aspect otherwise"""
    return SKEWED if (w, h) == (24, 16) else lc.default_camera(w, h)


def translated(cam, move=MOVE):
    """the closing camera of a pure translation: all four points moved by 'move' (float32)"""
    return tuple(tuple((np.asarray(p, np.float32) + np.asarray(move, np.float32)).tolist()) for p in cam)


def rotated(cam, move=MOVE, angle=0.2, push=0.3):
    """a closing camera that also turns the screen rectangle: its three points are turned about cam_pos by 'angle' about the y axis and
    pushed away from cam_pos by the factor 1 + push, then everything is moved by 'move'.  The screen's distance from the camera differs at
    the two ends and in between, so lam varies with tau"""
    pos = np.asarray(cam[0], np.float64)
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = [pos + np.asarray(move, np.float64)]
    for p in cam[1:]:
        out.append(pos + (1 + push) * (R @ (np.asarray(p, np.float64) - pos)) + np.asarray(move, np.float64))
    return tuple(tuple(np.asarray(p, np.float32).tolist()) for p in out)


def gpu_cases():
    """(w, h, frame, seed_base) of every frame the GPU tier compares"""
    for w, h in GPU_RAY_SIZES:
        for f in GPU_RAY_FRAMES:
            yield w, h, f, lc.ray_seed_base(w, h)
    for w, h in GPU_PARITY_SIZES:
        for f in GPU_PARITY_FRAMES:
            yield w, h, f, SEED
    for f in GPU_COMPOSE_FRAMES:
        yield GPU_COMPOSE_SIZE + (f, SEED)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- tau ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=["point", "box", "tent"])
def test_tau_is_a_uniform_draw_of_its_own(kind):
    s = np.concatenate([fr.sample_index(W, H, f, SEED) for f in range(FRAMES)])
    tau = sr.times(kind, s).astype(np.float64)
    n = len(tau)
    assert n == 53760
    assert tau.min() >= 0.0 and tau.max() <= 1.0
    # a uniform on [0, 1]: mean 1/2 with variance 1/12; (x - 1/2)^2 has mean 1/12 and variance 1/80 - 1/144 = 1/180
    se_mean, se_var = np.sqrt(1 / 12 / n), np.sqrt(1 / 180 / n)
    mean, var = tau.mean(), ((tau - 0.5) ** 2).mean()
    print("tau over %d samples: mean %.5f (0.5 +- %.5f), variance %.5f (%.5f +- %.5f)" % (n, mean, 4 * se_mean, var, 1 / 12, 4 * se_var))
    assert abs(mean - 0.5) <= 4 * se_mean
    assert abs(var - 1 / 12) <= 4 * se_var
    # not the path stream's first draw, and not one of the filter's: two draws agree with probability about 2^-23 (RandomFloat has 2^23
    # values in [0.5, 1)), 0.006 times in n, so more than one agreement means a shared draw
    _, path_first = fr.random_float(fr.stream_seed(s))
    js, u1 = fr.random_float(fr.stream_seed(~s))
    _, u2 = fr.random_float(js)
    tau32 = sr.times(kind, s)
    assert (tau32 == path_first).sum() <= 1
    if kind != fr.POINT:
        assert (tau32 == u1).sum() <= 1 and (tau32 == u2).sum() <= 1
        _, u3 = fr.random_float(fr.random_float(js)[0])
        assert np.array_equal(tau32, u3)  # behind the filter's two draws
    else:
        assert np.array_equal(tau32, u1)  # POINT draws nothing in front of it


# ---- the GPU tier is not vacuous ----------------------------------------------------------------------------------------------------
def test_a_translating_camera_moves_every_origin_of_the_gpu_tier_s_frames():
    n = 0
    for w, h, f, seed_base in gpu_cases():
        cam = open_camera(w, h)
        for close in (translated(cam), rotated(cam)):
            for kind in KINDS:
                O, _ = sr.rays(kind, cam, close, w, h, f, seed_base)
                O_off, _ = fr.rays(kind, cam, w, h, f, seed_base)
                assert np.all(np.any(bits(O) != bits(O_off), axis=1)), (w, h, f, kind)
                O, _ = sr.rays(kind, cam, close, w, h, f, seed_base, RADIUS, FOCUS)
                O_off, _ = lr.rays(kind, cam, w, h, f, seed_base, RADIUS, FOCUS)
                assert np.all(np.any(bits(O) != bits(O_off), axis=1)), (w, h, f, kind, "lens")
                n += len(O)
    assert n > 100000


def test_an_unmoved_closing_camera_gives_the_filter_s_rays():
    for w, h, f, seed_base in gpu_cases():
        cam = open_camera(w, h)
        for kind in KINDS:
            O, D = sr.rays(kind, cam, cam, w, h, f, seed_base)
            O_ref, D_ref = fr.rays(kind, cam, w, h, f, seed_base)
            assert np.array_equal(bits(O), bits(O_ref)) and np.array_equal(bits(D), bits(D_ref)), (w, h, f, kind)
            # ... but with a lens the tau draw has moved the lens point: not the lens's rays
            if w * h > 1:
                O, _ = sr.rays(kind, cam, cam, w, h, f, seed_base, RADIUS, FOCUS)
                assert not np.array_equal(bits(O), bits(lr.rays(kind, cam, w, h, f, seed_base, RADIUS, FOCUS)[0]))


def test_the_lens_fallback_stays_unused_one_draw_later():
    n = 0
    for w, h, f, seed_base in gpu_cases():
        for kind in KINDS:
            a, b, fb = sr.lens_points(kind, fr.sample_index(w, h, f, seed_base))
            assert int(fb.sum()) == 0, (w, h, f, kind)
            assert np.all(a * a + b * b <= 1.0)
            n += len(a)
    # (a fallback has probability (1 - pi / 4)^16 = 2e-11 a sample)
    assert n > 50000


def test_lam_varies_with_tau_under_the_rotating_camera():
    """the rotating closing camera is what the GPU tier's per-sample lam is held to: the screen's distance differs along the exposure"""
    cam = open_camera(24, 16)
    tau = np.linspace(0, 1, 9, dtype=np.float32)
    d = [lr.screen_dist([c[i] for c in sr.cameras(cam, rotated(cam), tau)]) for i in range(len(tau))]
    assert np.ptp(d) > 0.1 * np.min(d)
    d = [lr.screen_dist([c[i] for c in sr.cameras(cam, translated(cam), tau)]) for i in range(len(tau))]
    assert np.ptp(d) <= 1e-5 * np.min(d)


# ---- the blur itself ----------------------------------------------------------------------------------------------------------------
def test_a_camera_that_translates_along_its_screen_blurs_a_facing_plane_as_the_geometry_predicts():
    """A rectangular screen one unit in front of the camera, 8 pixels wide; a plane four units in front of it, parallel to the screen, cut
    into texels as wide as a pixel's footprint there (1.0).  The camera moves 2.5 texels along the screen's A direction over the exposure.
    POINT samples: pixel p's ray looks at the first quarter point of texel p at tau = 0 and slides 2.5 texels to the right, so it sees texel
    p for the first 0.3 of the exposure, texel p + 1 for the next 0.4, texel p + 2 for the last 0.3, and never texel p - 1 or p + 3."""
    w, h, n = 8, 1, 256
    cam = ((0.5, 1.0, -2.0), (-0.5, 1.5, -1.0), (1.5, 1.5, -1.0), (-0.5, 0.5, -1.0))
    shift = 2.5
    close = translated(cam, (shift, 0.0, 0.0))
    plane_z, scale = 2.0, 4.0
    pos, tl, tr = (np.asarray(v, np.float64) for v in cam[:3])
    c0 = pos[0] + (tl[0] - pos[0]) * scale - 0.25            # texel 0's left edge: a quarter texel left of where pixel 0's ray meets the plane at tau = 0
    foot = (tr[0] - tl[0]) / w * scale                        # a pixel's footprint on the plane
    assert foot == 1.0
    counts = np.zeros((w, 5), int)
    for f in range(n):
        O, D = (a.astype(np.float64) for a in sr.rays(fr.POINT, cam, close, w, h, f, SEED))
        t = (plane_z - O[:, 2]) / D[:, 2]
        x = O[:, 0] + t * D[:, 0]
        k = np.floor((x - c0) / foot).astype(int) - np.arange(w)  # the texel seen, relative to the pixel's own
        assert k.min() >= -1 and k.max() <= 3
        np.add.at(counts, (np.arange(w), k + 1), 1)
    frac = counts / n
    print("share of the exposure pixel p sees texel p - 1 .. p + 3:\n%s" % np.array2string(frac, precision=3))
    for k, q in ((-1, 0.0), (0, 0.3), (1, 0.4), (2, 0.3), (3, 0.0)):
        bound = 4 * np.sqrt(q * (1 - q) / n)
        assert np.all(np.abs(frac[:, k + 1] - q) <= bound), (k, q, bound, frac[:, k + 1])
