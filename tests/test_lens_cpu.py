"""The thin lens of path-mode camera samples on the CPU (include/rt_amd.h rt_set_lens): tests/lens_ref.py's restatement is a thin lens -- its
rays pass through their focal points, its lens points cover the disk, the 16-try fallback stays unused in the frames the GPU tests
compare bit for bit, its rays are not the pinhole's -- and, through the oracle's nearest-hit query on a plane facing the camera, a point on
the focal plane is sharp, one at twice the distance is spread over the aperture, and focus_distance() recovers the plane's depth.
tests/test_gpu_lens.py reruns the plane experiment on the device (plane_scene, hit_points)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_ref as fr  # noqa: E402
import lens_ref as lr  # noqa: E402

# a skewed camera whose screen rectangle is a parallelogram: A and B are not at a right angle (cos 0.077)
SKEWED = ((0.3, 0.2, -2.0), (-1.7, 1.1, 0.1), (1.6, 1.0, -0.1), (-1.6, -0.9, 0.2))
W, H, FRAMES = 40, 21, 64
SEED = 0x12345678
RADIUS, FOCUS = 0.05, 3.0
# the (size, seed_base) pairs, frames and kinds tests/test_gpu_lens.py compares rays on bit for bit, under the default camera of the size
# (24 x 16: under test_filter_cpu.SKEWED) -- and the frames 5 .. 7 of its accumulator comparisons
GPU_RAY_SIZES = [(1, 1), (63, 1), (65, 1), (255, 1), (257, 3), (24, 16)]
GPU_RAY_FRAMES = (0, 7)
GPU_PARITY_SIZES = [(24, 16), (65, 3), (40, 21)]
GPU_PARITY_FRAMES = tuple(range(0, 16))


def ray_seed_base(w, h):
    """s = seed_base + pixel + frame * W * H wraps within the frame"""
    return 0xFFFFFFF0 if w * h > 16 else 0xFFFFFFFF


def default_camera(w, h):
    """Camera::Camera for the aspect of w x h: what a context and the oracle's renderer start with"""
    a = np.float32(w) / np.float32(h)
    return ((0.0, 1.0, -2.0), (-a, 2.0, 0.0), (a, 2.0, 0.0), (-a, 0.0, 0.0))


@pytest.fixture(scope="module")
def stack():
    """the 53,760 samples of 64 BOX frames at 40 x 21 under the skewed camera: O, D, F, a, b, fallback, computed once and left unchanged"""
    out = dict(O=[], D=[], F=[], a=[], b=[], fb=[], Dpin=[])
    for f in range(FRAMES):
        O, D = lr.rays(fr.BOX, SKEWED, W, H, f, SEED, RADIUS, FOCUS)
        a, b, fb = lr.lens_points(fr.BOX, fr.sample_index(W, H, f, SEED))
        for k, v in zip(("O", "D", "F", "a", "b", "fb", "Dpin"),
                        (O, D, lr.focal_points(fr.BOX, SKEWED, W, H, f, SEED, FOCUS), a, b, fb, fr.rays(fr.BOX, SKEWED, W, H, f, SEED)[1])):
            out[k].append(v)
    out = {k: np.concatenate(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    assert len(out["O"]) == 53760 and out["O"].dtype == np.float32 and out["D"].dtype == np.float32
    return out


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
def test_rays_pass_through_their_focal_points(stack):
    O, D, F = (stack[k].astype(np.float64) for k in ("O", "D", "F"))
    dist = np.linalg.norm(np.cross(F - O, D), axis=1) / np.linalg.norm(D, axis=1)
    print("largest distance of a ray's line from its focal point: %.3g (focus %.1f)" % (dist.max(), FOCUS))
    assert dist.max() <= 1e-5 * FOCUS
    # ... and the focal points lie on the plane parallel to the screen, focus_distance from the camera
    pos, _, _, _, _, _, N = (np.asarray(v, np.float64) for v in lr.camera(SKEWED))
    depth = np.abs((F - pos) @ (N / np.linalg.norm(N)))
    assert np.abs(depth - FOCUS).max() <= 1e-5 * FOCUS


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
def test_lens_points_cover_the_disk(stack):
    a, b = stack["a"].astype(np.float64), stack["b"].astype(np.float64)
    rho2 = a * a + b * b
    print("mean of a*a + b*b over %d samples: %.4f; largest %.6f" % (len(a), rho2.mean(), rho2.max()))
    assert rho2.max() <= 1.0
    assert abs(rho2.mean() - 0.5) <= 0.01  # uniform on the unit disk: E[rho^2] = 1/2, standard error sqrt(1/12 / n) = 0.0012
    for q, share in ((a >= 0, 0.5), (b >= 0, 0.5), ((a >= 0) & (b >= 0), 0.25)):  # no half and no quadrant is favoured (standard error 0.002)
        assert abs(q.mean() - share) <= 0.01
    # the origins lie in the screen's plane through cam_pos ...
    pos, _, _, _, A, B, N = (np.asarray(v, np.float64) for v in lr.camera(SKEWED))
    off = stack["O"].astype(np.float64) - pos
    assert np.abs(off @ (N / np.linalg.norm(N))).max() <= 1e-6 * RADIUS + 4 * np.finfo(np.float32).eps * np.abs(pos).max()
    # ... within radius * sqrt(1 + |cos(A, B)|) of it: the definition's O = cam + a r unit(A) + b r unit(B) has
    # |O - cam|^2 = r^2 (a^2 + b^2 + 2 a b cos) <= r^2 (1 + |cos|); a rectangular screen (cos = 0) gives the radius itself, below
    cos = abs(A @ B) / (np.linalg.norm(A) * np.linalg.norm(B))
    assert 0.05 < cos < 0.1
    assert np.linalg.norm(off, axis=1).max() <= RADIUS * np.sqrt(1 + cos) * (1 + 1e-6)


def test_lens_points_stay_within_the_radius_of_a_rectangular_screen():
    cam = default_camera(W, H)
    pos = np.asarray(cam[0], np.float64)
    far, rho2 = 0.0, []
    for f in range(FRAMES):
        O, _ = lr.rays(fr.BOX, cam, W, H, f, SEED, RADIUS, FOCUS)
        a, b, _ = lr.lens_points(fr.BOX, fr.sample_index(W, H, f, SEED))
        off = O.astype(np.float64) - pos
        assert np.abs(off[:, 2]).max() == 0.0  # the screen's plane is z = const
        far = max(far, np.linalg.norm(off, axis=1).max())
        rho2.append(a.astype(np.float64) ** 2 + b.astype(np.float64) ** 2)
    rho2 = np.concatenate(rho2)
    print("largest |O - cam| / radius over %d samples: %.7f; mean of a*a + b*b %.4f" % (len(rho2), far / RADIUS, rho2.mean()))
    assert far <= RADIUS * (1 + 1e-6)
    assert abs(rho2.mean() - 0.5) <= 0.01


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def test_the_fallback_stays_unused_in_the_frames_the_tests_use(stack):
    assert int(stack["fb"].sum()) == 0
    n = 0
    for kind in (fr.POINT, fr.BOX, fr.TENT):
        for w, h in GPU_RAY_SIZES:
            for f in GPU_RAY_FRAMES:
                n += int(lr.lens_points(kind, fr.sample_index(w, h, f, ray_seed_base(w, h)))[2].sum())
        for w, h in GPU_PARITY_SIZES:
            for f in GPU_PARITY_FRAMES:
                n += int(lr.lens_points(kind, fr.sample_index(w, h, f, SEED))[2].sum())
    assert n == 0


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
def test_lens_rays_are_not_the_pinhole_s(stack):
    differ = np.any(stack["D"].view(np.uint32) != stack["Dpin"].view(np.uint32), axis=1)
    print("directions that differ bitwise from filter_ref.rays: %.4f" % differ.mean())
    assert differ.mean() >= 0.99
    pos = np.asarray(SKEWED[0], np.float32)
    assert np.any(stack["O"] != pos, axis=1).mean() >= 0.99


def test_radius_zero_is_not_part_of_the_restatement():
    """radius 0 is 'off' in the library (no lens draw at all): the restatement on radius 0 still looks through cam_pos"""
    O, D = lr.rays(fr.BOX, SKEWED, 8, 5, 3, SEED, 0.0, FOCUS)
    assert np.array_equal(O, np.broadcast_to(np.float32(SKEWED[0]), O.shape))
    _, Dp = fr.rays(fr.BOX, SKEWED, 8, 5, 3, SEED)
    assert np.abs(D.astype(np.float64) - Dp).max() <= 1e-6


# ---- (e), (f): a plane facing the camera -----------------------------------------------------------------------------------------
PW, PH = 5, 3


def plane_scene(depth):
    """a builder of two large triangles in the plane z = cam.z + depth, facing the default camera (whose screen's normal is +z)"""
    def build(b):
        z, s = -2.0 + depth, 60.0
        b.sky(np.full((4, 8, 3), 128, np.uint8))
        b.area_light(11, (0.0, 3.0, -6.0), 1.0, (1, 1, 1), 0.1, (0, -1, 0))
        m = b.diffuse(0.8, (1, 1, 1), 0.0, 1.0, 4)
        b.mesh_raw(1, m, np.float32([[-s, -s, z, s, -s, z, s, s, z], [-s, -s, z, s, s, z, -s, s, z]]))
        b.build(0)
    return build


def hit_points(nearest, kind, cam, w, h, frames, radius, focus, rays_fn=None):
    """(hit points (frames, w * h, 3) in f64, every ray hit): nearest(O, D) -> t (a miss: >= 1e30) on each frame's rays"""
    pts = []
    for f in range(frames):
        O, D = (rays_fn or (lambda fr_: lr.rays(kind, cam, w, h, fr_, SEED, radius, focus)))(f)
        t = np.asarray(nearest(O, D), np.float64)
        assert np.all(t < 1e30)
        pts.append(O.astype(np.float64) + t[:, None] * D.astype(np.float64))
    return np.stack(pts)


def check_spread(at_focus, at_twice, pinhole_twice):
    """the two claims of the plane experiment, on hit points (frames, pixels, 3)"""
    spread = np.linalg.norm(at_focus[:, None] - at_focus[None, :], axis=-1).max()
    print("in focus: hit points within %.3g of each other (focus %.1f)" % (spread, FOCUS))
    assert spread <= 1e-4 * FOCUS
    far = np.linalg.norm(at_twice - pinhole_twice[None], axis=-1).max(axis=0)  # per pixel, over the frames
    print("at twice the distance: largest distance from the pinhole hit / radius %.4f .. %.4f" % (far.min() / RADIUS, far.max() / RADIUS))
    assert np.all(far >= 0.8 * RADIUS) and np.all(far <= 1.0001 * RADIUS)


@pytest.fixture(scope="module")
def planes(oracle_api):
    made = []

    def make(depth):
        o = oracle_api.OracleScene()
        plane_scene(depth)(o)
        made.append(o)
        return lambda O, D: o.find_nearest(O, D, t_min=0.001)["t"]

    yield make
    for o in made:
        o.close()


def test_a_point_on_the_focal_plane_is_sharp_and_one_behind_it_is_spread(planes):
    cam = default_camera(PW, PH)
    at_focus = hit_points(planes(FOCUS), fr.POINT, cam, PW, PH, FRAMES, RADIUS, FOCUS)
    twice = planes(2 * FOCUS)
    at_twice = hit_points(twice, fr.POINT, cam, PW, PH, FRAMES, RADIUS, FOCUS)
    pin = hit_points(twice, fr.POINT, cam, PW, PH, 1, 0, 0, rays_fn=lambda f: fr.rays(fr.POINT, cam, PW, PH, f, SEED))[0]
    check_spread(at_focus, at_twice, pin)


@pytest.mark.parametrize("depth", [FOCUS, 2 * FOCUS, 0.7])
def test_focus_distance_is_the_plane_s_depth(depth, planes):
    cam = default_camera(PW, PH)
    O, D = fr.rays(fr.POINT, cam, PW, PH, 0, SEED)
    t = planes(depth)(O, D)
    d = lr.focus_distance(cam, t, D)
    assert d.dtype == np.float32
    centre = (PH // 2) * PW + PW // 2
    assert abs(float(d[centre]) - depth) <= 1e-5 * depth
    assert np.abs(d.astype(np.float64) - depth).max() <= 1e-5 * depth  # ... and of every other pixel: the plane is parallel to the screen
