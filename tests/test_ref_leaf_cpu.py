"""The leaf functions of the path against the REFERENCE'S OWN COMPILED CODE.  oracle/ref/ref_leaf.cpp includes the reference's headers
from where they lie and exports its inline leaf code -- Triangle, Sphere, Plane, AreaLight, DirectionalLight, glass, diffuse / metal scatter,
Camera::GetPrimaryRay, Scene::GetSkyColor -- as C entry points; tests/golden/make_ref_leaf_golden.py ran the crafted inputs of
tests/ref_leaf_cases.py through it and recorded the answers in tests/golden/ref_leaf.npz.  Here, on a machine without a device:
  * where the library is built (the reference's sources are present), its live answers equal the record bit for bit;
  * the oracle's own functions (oracle_capi.cpp orc_leaf_*) answer every case with the record's bits, NaNs by class;
  * the host mirror (librapt_host.so) does for the one leaf function it computes on the host, the Triangle constructor (its one-ray
    members and its sky lookup are answered by the device: tests/test_gpu_ref_leaf.py);
  * every family of inputs reaches, in the record, the branch it is listed for.
The one named exclusion is oracle/README.md's: Triangle::IsOccluding where it runs off its end (undefined in the reference, defined as
'false' here); the record marks those cases from the reference's two builds alone, and they are capped at 2 % of the family."""
import ctypes as C
import os

import numpy as np
import ref_leaf_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_leaf.so")
f32 = np.float32


def _load():
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_leaf.npz"))
    g = {}
    for k in z.files:
        a = z[k]
        g[k] = a.view(f32) if a.dtype == np.uint32 and not k.endswith("_seed") else a
    return g


GOLD = _load()
CASES = rc.all_cases()
OUT_KEYS = sorted(k[4:] for k in GOLD if k.startswith("out_") and k != "out_tri_occ_undefined")
UNDEFINED = GOLD["out_tri_occ_undefined"]


def test_the_record_holds_these_inputs():
    """the record's inputs are the case module's, bit for bit: a change to either without the other is caught here"""
    now = rc.flat_inputs(CASES)
    assert sorted(now) == sorted(k for k in GOLD if k.startswith("in_"))
    for k, v in now.items():
        assert v.shape == GOLD[k].shape and rc.same_bits(np.asarray(v), GOLD[k]).all(), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_leaf.npz")) < 1000000


def _check(got, who):
    bad = []
    for k in OUT_KEYS:
        d = ~rc.same_bits(got[k], GOLD["out_" + k])
        if k == "tri_occ":
            d &= ~UNDEFINED
        if d.any():
            bad.append("%s: %d of %d" % (k, d.sum(), d.size))
    assert not bad, who + " differs from the reference's recorded answers: " + "; ".join(bad)


def test_live_reference_equals_the_record():
    """oracle/_ref/libref_leaf.so is built only where the reference's sources are present; the record carries the pin everywhere else"""
    if not os.path.exists(REF_SO):
        return
    L = C.CDLL(REF_SO)
    assert L.ref_leaf_libm() == 0 and L.ref_camera_width() == rc.CAM_W and L.ref_camera_height() == rc.CAM_H
    cam = np.zeros(15, f32)
    L.ref_camera_default(cam.ctypes.data_as(C.c_void_p))
    assert rc.same_bits(cam, rc.cameras()[0]).all()  # the first camera of the cases is Camera's own constructor's
    _check(rc.answers(L, "ref_", CASES), "the live library")


def test_oracle_equals_the_record(oracle_api):
    got = rc.answers(oracle_api.lib(), "orc_leaf_", CASES)
    _check(got, "the oracle")
    # the named exclusion, and nothing wider: where the reference runs off the end of Triangle::IsOccluding the oracle says 'false'
    assert not got["tri_occ"][UNDEFINED].any()
    assert 0 < UNDEFINED.mean() <= 0.02


def test_every_family_reaches_its_branch():
    g = lambda k: GOLD["out_" + k]
    for kind in ("tri", "sph", "pla", "area"):
        assert not rc.expect_ok(g(kind + "_hit"), CASES[kind]["fam"]), kind
        hit, c = g(kind + "_hit"), CASES[kind]
        assert rc.same_bits(g(kind + "_t")[~hit], c["tmax"][~hit]).all()  # a miss leaves ray.t alone
        assert len(hit) >= 2000
    fam = lambda kind: {n: slice(a, b) for n, a, b, _ in CASES[kind]["fam"]}
    # Triangle: IsOccluding agrees with Intersect wherever it is defined; every undefined case is one the edge tests let through
    assert np.array_equal(g("tri_occ")[~UNDEFINED], g("tri_hit")[~UNDEFINED]) and not g("tri_hit")[UNDEFINED].any()
    f = fam("tri")
    for name in ("t_zero", "tmax_at", "tmax_below", "tmin_at", "tmin_below", "degenerate0", "degenerate3"):
        for tm in rc.TMINS:
            assert UNDEFINED[f["%s@%g" % (name, tm)]].all(), name
    assert np.isnan(g("tri_N")[3:]).all() and np.isfinite(g("tri_N")[:3]).all()  # two equal corners: a NaN normal
    assert rc.same_bits(g("tri_N")[:2], f32([[0, 0, 1], [-1, 0, 0]])).all()
    # Sphere: the far root is taken from inside and where the near one is under t_min
    f, t = fam("sph"), g("sph_t")
    assert np.array_equal(g("sph_occ"), g("sph_hit"))
    assert (t[f["inside0@1e-06"]] < 1.3).all() and (np.abs(t[f["outside0@1e-06"]] - 2) < 1e-5).all() and (t[f["surface_in0@0.001"]] == 2).all()
    assert (t[f["first_root_small@0.001"]] > 1.9).all() and (t[f["first_root_small@1e-06"]] < 1e-3).all()
    assert rc.same_bits(g("sph_nrm")[f["outside0@1e-06"]][4], f32([0, 0, -1])).all()
    # Plane
    assert np.array_equal(g("pla_occ"), g("pla_hit"))
    # AreaLight::Intersect: the stored t is the double t - 1e-6 rounded to float, also past ray.t
    f, t, c = fam("area"), g("area_t"), CASES["area"]
    s = f["store@1e-06"]
    want = (2.0 - c["O"][s, 1].astype(np.float64) - 1e-6).astype(f32)
    assert rc.same_bits(t[s], want).all() and len(np.unique(want)) == len(want)
    assert t[f["t_equals_tmin@1e-06"]][0] < 0 and rc.same_bits(t[f["t_equals_tmin@0.001"]], f32([np.float64(f32(1e-3)) - 1e-6])).all()
    assert (t[f["rim_on_short_ray@0.001"]] > 1.5).all()
    # AreaLight::GetLightIntensityAt: +inf seen directly; the flat branch (strength * colour) below isZero's 1e-4 -- the float nearest 1e-4
    # included, which only a double comparison puts below -- and the falling-off branch above it
    f, v, c = fam("area_int"), g("area_int"), CASES["area_int"]
    assert np.isposinf(v[f["direct_view"]]).all()
    for name, flat in (("near_zero_cos_at", True), ("near_zero_cos_below", True), ("near_negative_cos", True), ("near_zero_cos_above", False), ("far_zero_cos", False)):
        s = f[name]
        assert s.stop > s.start and ((v[s] == c["prims"][c["prim"][s]][:, 3:4]).all(1) == flat).all(), name
    assert np.array_equal((v[f["at_radius"]] == 4).all(1), [True, False, True, False])
    # AreaLight::GetLightPosition: the position itself under the raytracer flag (no draw), two draws otherwise
    c = CASES["area_pos"]
    rt = c["prims"][c["prim"], 11] != 0
    assert rt.any() and (~rt).any()
    assert np.array_equal(g("area_pos_seed")[rt], c["seed"][rt]) and rc.same_bits(g("area_pos")[rt], c["prims"][c["prim"][rt], :3]).all()
    s = c["seed"][~rt].astype(np.uint64)
    for _ in range(2):
        for sh, left in ((13, True), (17, False), (5, True)):
            s = (s ^ ((s << sh) if left else (s >> sh))) & 0xFFFFFFFF
    assert np.array_equal(g("area_pos_seed")[~rt], s.astype(np.uint32))  # Marsaglia's xorshift32, twice
    assert rc.same_bits(g("area_pos")[~rt][:, 2], c["prims"][c["prim"][~rt], 2]).all() and (g("area_pos")[~rt][:, 0] != c["prims"][c["prim"][~rt], 0]).any()
    # DirectionalLight: nothing behind it, NaN at its own position, and both sides of the cone's edge
    f, v = fam("dirl"), g("dir_int")
    assert (v[f["behind"]] == 0).all() and np.isnan(v[f["at_pos"]]).all()
    edge = v[f["cone_edge"]][:, 0]
    assert (edge[:13] == 0).any() and (edge[:13] > 0).any() and edge[13] > 0 and edge[14] == 0
    assert (v[f["inside"]] > 0).all() and (v[f["outside"]] == 0).all()
    assert g("dir_sin")[4] == 0 and g("dir_sin")[0] == f32(np.sin(np.float64(f32(0.5) * f32(np.pi) / f32(2))))
    # glass::fresnel: total internal reflection (kr == 1) on one side of the critical angle only, for exactly the (ior, side) that have one
    kr = g("fresnel_kr")
    assert not rc.expect_ok(kr == 1, CASES["fresnel"]["fam"])
    f = fam("fresnel")
    for ior in rc.IORS:
        k = kr[f["cosi_-1_0_1@%g" % ior]]
        assert k[1] == 1 and k[0] == k[4] and k[2] == k[5]  # cosi == 0; the clamp of a dot product beyond +-1
        for side in (-1, 1):
            s = f["sweep%+d@%g" % (side, ior)]
            if s.stop - s.start > 24:
                near = kr[s][24:57]
                assert (near == 1).any() and (near < 1).any(), (ior, side)  # the 33 angles within 2e-6 of the critical angle
    assert ((kr >= 0) & (kr <= 1)).all()
    # glass::RefractRay: 1 - len^2 changes sign inside each sweep (the root of its absolute value comes down to ~0 and goes up again)
    f, v, c = fam("refract"), g("refract"), CASES["refract"]
    for ratio in (1.5, 2.4, 1.25):
        s = f["len_near_1@%g" % ratio]
        ln = np.abs(c["ratio"][s].astype(np.float64) * c["D"][s, 0])
        assert (ln < 1).any() and (ln > 1).any() and np.abs(v[s][:, 1]).min() < 3e-3 and np.abs(v[s][:, 1]).max() > 0.1
    assert np.isfinite(v).all()
    # diffuse::scatter: the energy survives in some cases and is zeroed in others; the specular term is there in some and 0 in others
    en, c = g("diffuse_energy"), CASES["diffuse"]
    assert ((en == 0).all(1)).sum() > 50 and ((en[:, 0] > 0)).sum() > 50
    spec = g("diffuse_att") - (c["mat"][:, :3] * c["lightInt"] * c["mat"][:, 4:5])
    assert (np.abs(spec).max(1) > 1e-3).sum() > 50 and (np.abs(spec).max(1) == 0).sum() > 50
    assert g("metal_ret").sum() > 100 and (~g("metal_ret")).sum() > 100
    # Camera: unit directions, the centre pixel of the pinhole camera looks along +z, the fisheye rows differ from the pinhole's
    D = g("cam_D")
    assert D.shape == (len(rc.cameras()), len(rc.camera_pixels()[0]), 3) and D.shape[0] == 15 and D.shape[1] <= 4096
    assert np.abs(np.sqrt((D.astype(np.float64) ** 2).sum(-1)) - 1).max() < 1e-6
    xs, ys = rc.camera_pixels()
    for corner in ((0, 0), (599, 0), (0, 399), (599, 399), (300, 200)):
        assert ((xs == corner[0]) & (ys == corner[1])).sum() == 1
    for row in (0, 199, 300, 399):
        assert (ys == row).sum() >= 75
    centre = D[0][(xs == 300) & (ys == 200)][0]
    assert centre[0] == 0 and centre[1] == 0 and centre[2] == 1
    assert all(not rc.same_bits(D[i], D[j]).all() for i in range(15) for j in range(i))
    # Scene::GetSkyColor: straight up and down are the NaN-to-int case (oracle/README.md): column 0
    c, v = CASES["sky"], g("sky_rgb")
    img = c["img"].astype(f32) / f32(255)
    assert rc.same_bits(v[0], img[0, 0]).all() and rc.same_bits(v[1], img[8, 0]).all()
    assert len(np.unique(v, axis=0)) > 100


def test_host_mirror_triangle_constructor_equals_the_record(host_api):
    """The one leaf function the host mirror computes on the host: Triangle's constructor (N, centroid), read back through the mesh dump.  Its
    one-ray members and its sky lookup are answered by the device; tests/test_gpu_ref_leaf.py holds those to the record."""
    s = host_api.HostScene()
    s.mesh_raw(1, s.diffuse(0.8, (1, 1, 1)), rc.TRI_PRIMS)
    tris, _ = s.mesh_tris(0)
    assert rc.same_bits(tris[:, :9], rc.TRI_PRIMS).all()
    assert rc.same_bits(tris[:, 9:12], GOLD["out_tri_N"]).all() and rc.same_bits(tris[:, 12:15], GOLD["out_tri_centroid"]).all()
    s.close()


def test_oracle_find_nearest_hands_the_callers_t_min_to_the_leaf(oracle_api):
    """Scene::FindNearest of the oracle, where it hands the caller's t_min on (lights; spheres and planes beside a TLAS), against the record"""
    def new_scene(build):
        o = oracle_api.OracleScene()
        build(o)
        return (lambda O, D, tmax, t_min: o.find_nearest(O, D, tmax, t_min=t_min)), o.close
    n = rc.check_callers_t_min(new_scene, GOLD)
    assert n == sum(len(CASES[k]["O"]) for k in ("sph", "pla", "area"))
