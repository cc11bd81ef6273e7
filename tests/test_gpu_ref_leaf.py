"""The device against the reference's own recorded answers (tests/golden/ref_leaf.npz, written by the reference's compiled leaf code:
tests/golden/make_ref_leaf_golden.py), DIRECTLY -- no oracle in between, and no reference on this machine: the record carries the pin.
  * Camera::GetPrimaryRay at the reference's fixed 600 x 400, pinhole and every fisheye setting of the record: rt_sample_rays under the
    POINT filter, bit for bit at the record's pixels.
  * One-primitive scenes (a single triangle as a mesh, a single sphere, a single plane).  Their BVH's root is a leaf, so bvh::Intersect /
    IsOccluded hand the ray to the leaf test alone, at the BVH's own t_min of 0.0001 whatever t_min the caller names (bvh.cpp:606-656):
    the record's rows at that t_min go through rt_intersect_batch with t_min 1e-6 and 1e-3, with and without tmax, and through
    rt_occluded_batch with tmax; hit or miss, t and the normal are the record's bits.  The host mirror's one-ray members
    (bvh::Intersect, bvh::IsOccluded) take the crafted rows one at a time.
  * Where Scene::FindNearest does hand the caller's t_min to a leaf test -- the area light's, and a sphere's or plane's tested by brute
    force beside a TLAS (template/scene.h:1257-1261) -- every row of the record goes through rt_intersect_batch at the t_min it names.
  * Scene::GetSkyColor: rt_sky_color and the host mirror's one-ray form.
Only the record's rays go to the device (finite origins and directions); the one exclusion is the CPU tier's: Triangle::IsOccluding where the
reference runs off its end (tests/test_ref_leaf_cpu.py)."""
import os

import numpy as np
import pytest

import ref_leaf_cases as rc
import support as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_leaf.npz"))
    return {k: (z[k].view(f32) if z[k].dtype == np.uint32 and not k.endswith("_seed") else z[k]) for k in z.files}


def test_camera_rays_equal_the_reference(gold, host_api, monkeypatch):
    sp.clean_env(monkeypatch)
    xs, ys, cams, want = gold["in_cam_xs"], gold["in_cam_ys"], gold["in_cam_rows"], gold["out_cam_D"]
    assert len(cams) == 15 and cams[:, 12].sum() == 13
    at = ys.astype(np.int64) * rc.CAM_W + xs
    r = host_api.HostRenderer(rc.CAM_W, rc.CAM_H)
    r.set_pixel_filter(host_api.RT_FILTER_POINT)
    for i, cam in enumerate(cams):
        r.set_camera(cam[0:3], cam[3:6], cam[6:9], cam[9:12], fisheye=bool(cam[12]), view_angle=float(cam[13]), y_angle=float(cam[14]))
        O, D = r.sample_rays(0)
        assert sp.same(O[at], np.broadcast_to(cam[:3], (len(at), 3))), i
        assert sp.same(D[at], want[i]), "camera %d: %d of %d directions differ" % (i, (sp.bits(D[at]) != sp.bits(want[i])).any(1).sum(), len(at))
    r.close()


@pytest.mark.parametrize("kind", ["tri", "sph", "pla"])
def test_one_primitive_scenes_equal_the_reference(kind, gold, host_api, monkeypatch):
    sp.clean_env(monkeypatch)
    g = lambda k: gold["out_%s_%s" % (kind, k)]
    i_ = lambda k: gold["in_%s_%s" % (kind, k)]
    prims, prim, O, D, tmax, tmin = i_("prims"), i_("prim"), i_("O"), i_("D"), i_("tmax"), i_("tmin")
    assert np.isfinite(O).all() and np.isfinite(D).all()
    undefined = gold["out_tri_occ_undefined"] if kind == "tri" else np.zeros(len(O), bool)
    crafted = np.zeros(len(O), bool)
    for name, a, b, _ in rc.all_cases()[kind]["fam"]:
        crafted[a:b] = not name.startswith("random")
    seen = 0
    for p in range(len(prims)):
        rows = np.where((prim == p) & (tmin == rc.BVH_TMIN))[0]
        far = rows[tmax[rows] == rc.FAR]
        assert len(rows) and len(far)
        r = host_api.HostRenderer(8, 8)
        rc.one_primitive(r.scene, kind, prims[p])
        r.commit()
        for t_min in (1e-6, 1e-3):  # named by the caller, used for lights only: the leaf test runs at the BVH's own
            for sel, tm in ((rows, tmax[rows]), (far, None)):
                got = r.find_nearest(O[sel], D[sel], tm, t_min=t_min)
                hit = g("hit")[sel]
                assert np.array_equal(got["obj"] != -1, hit), (kind, p, t_min)
                assert sp.same(got["t"], g("t")[sel]), (kind, p, t_min)
                assert sp.same(got["normal"][hit], g("nrm")[sel][hit]), (kind, p, t_min)
        ok = ~undefined[rows]
        assert np.array_equal(r.is_occluded(O[rows], D[rows], tmax[rows])[ok] != 0, g("occ")[rows][ok]), (kind, p)
        # the host mirror's one-ray members: one device round trip each, so the crafted rows only (at most 48 of them)
        for i in rows[crafted[rows]][:48]:
            t, obj, n = r.scene.member_intersect(0, 0, O[i], D[i], float(tmax[i]))
            assert (obj != -1) == g("hit")[i] and f32(t).view(np.uint32) == g("t")[i].view(np.uint32), (kind, p, i)
            assert not g("hit")[i] or sp.same(n, g("nrm")[i]), (kind, p, i)
            if not undefined[i]:
                assert r.scene.member_occluded(0, 0, O[i], D[i], float(tmax[i])) == bool(g("occ")[i]), (kind, p, i)
        seen += len(rows)
        r.close()
    assert seen == (tmin == rc.BVH_TMIN).sum() >= 900


def test_find_nearest_hands_the_callers_t_min_to_the_leaf(gold, host_api, monkeypatch):
    sp.clean_env(monkeypatch)

    def new_scene(build):
        r = host_api.HostRenderer(8, 8)
        build(r.scene)
        r.commit()
        return (lambda O, D, tmax, t_min: r.find_nearest(O, D, tmax, t_min=t_min)), r.close
    n = rc.check_callers_t_min(new_scene, gold)
    assert n == sum(len(gold["in_%s_O" % k]) for k in ("sph", "pla", "area"))


def test_sky_lookup_equals_the_reference(gold, host_api, monkeypatch):
    sp.clean_env(monkeypatch)
    img, D, want = gold["in_sky_img"], gold["in_sky_D"], gold["out_sky_rgb"]
    r = host_api.HostRenderer(8, 8)
    r.scene.sky(img)
    rc.one_primitive(r.scene, "pla", rc.PLA_PRIMS[0])
    r.commit()
    assert sp.same(r.sky_color(D), want)
    for i in range(0, 40):
        assert sp.same(r.scene.sky_color_one(D[i]), want[i]), i
    r.close()
