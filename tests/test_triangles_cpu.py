"""CPU tier for rt_set_triangles (include/rt_amd.h): the restatements of tests/triangles_ref.py against the host mirror -- bvh::Refit and
Triangle::update on every test mesh -- and the conditions on the GPU tests' inputs: the updated description moves the words each case is
meant to move, the deformations change what the test rays hit (on the oracle alone), and no test ray has two hits at one distance.  These
tests pass without the call: they show that the inputs reach their branches."""
import numpy as np
import pytest

import triangles_desc as td
import triangles_ref as tr

f32 = np.float32
HOWS = ("twist", "scale", "collapse")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", params=td.LAYOUT_CASES)
def case(request, scenes, host_api):
    h = host_api.HostScene()
    c = td.build_case(h, request.param, scenes)
    c.update(name=request.param, scene=h, layout0=host_api.layout(h.describe(), 1, 0, 1))
    return c


@pytest.mark.parametrize("how", HOWS)
def test_refit_restatement_equals_the_host_mirror(case, how, host_api):
    """the NumPy bvh::Refit and Triangle::update against the mirror's, bit for bit (signs of zero included), on the deformed mesh; and
    rt_layout_build of the updated description differs from the uploaded one's where it should and nowhere else"""
    h = case["scene"]
    d = td.Desc(host_api, h)
    k = case["k"]
    old = tr.v9_of(d.tris[k])
    v9, N = td.deformed(case, d, how)
    sent = d.deform(k, v9, N)
    at = 0
    for m in case["meshes"]:  # the same vertices into the mirror's meshes, then its own Refit
        n = len(h.mesh_tris(m)[0])
        h.set_mesh_vertices(m, v9[at:at + n])
        got = h.mesh_tris(m)[0]
        if N is None:
            assert np.array_equal(_bits(got[:, 9:12]), _bits(sent["N"][at:at + n])), "Triangle::update's normal"
        at += n
    assert at == len(v9)
    h.refit(case["host"])
    dump = h.bvh_dump(case["host"])
    assert np.array_equal(dump["nodes"], _bits(d.nodes[k]).reshape(-1, 8)), "bvh::Refit"
    L0, L1 = case["layout0"], host_api.layout(d.desc(), 1, 0, 1)
    p0, p1, s0, s1 = d.ranges()[k]
    for name, lo, hi in (("pairs", p0, p1), ("prims", s0, s1)):
        a, b = _bits(L0[name]).reshape(-1, 16), _bits(L1[name]).reshape(-1, 16)
        assert a.shape == b.shape
        changed = np.flatnonzero((a != b).any(1))
        if name == "prims":
            assert np.all((changed >= lo) & (changed < hi)) and len(changed) >= (hi - lo) // 2, "the BLAS's primitive records move, no others"
            assert np.array_equal(a[:, 13:15], b[:, 13:15]) and np.array_equal(a[:, 15], b[:, 15]), "objIdx, material, kind | last | type stay"
        else:
            inside = changed[(changed >= lo) & (changed < hi)]
            assert len(inside) > 0 or p1 - p0 <= 1, "the BLAS's pair boxes move"
            assert np.all((changed >= lo) & (changed < hi) | (changed >= len(a) - L1["tlasPairs"])), "only this BLAS's and the TLAS's pair records move"
            assert np.array_equal(a[lo:hi, 3], b[lo:hi, 3]) and np.array_equal(a[lo:hi, 11], b[lo:hi, 11]), "the links stay"
    if d.use_tlas:
        assert not np.array_equal(_bits(L0["reach"]), _bits(L1["reach"])) or d.n == 1, "reach moves"
        if how == "scale" and not case["name"].startswith("tri"):
            assert L1["reachOriginMax"] > 10 * L0["reachOriginMax"], "the scaled mesh moves reachOriginMax"
    for name in ("refitOrder", "refitLevelStart", "rootLink", "inst", "lights", "mats", "brute"):
        assert np.array_equal(_bits(L0[name]), _bits(L1[name])), name
    assert np.array_equal(L0["scalars"][5:], L1["scalars"][5:])
    # back to the uploaded vertices for the next deformation of this module-scoped scene
    at = 0
    for m in case["meshes"]:
        n = len(h.mesh_tris(m)[0])
        h.set_mesh_vertices(m, old[at:at + n])
        at += n
    h.refit(case["host"])


# ---- the behaviour tests' inputs -----------------------------------------------------------------------------------------------------------
def _moller(O, D, tri):
    """every (ray, triangle) hit distance in float64 (NaN: no hit): rays (n, 3), world triangles (m, 3, 3)"""
    O, D, tri = O.astype(np.float64)[:, None], D.astype(np.float64)[:, None], tri.astype(np.float64)[None]
    e1, e2 = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    h = np.cross(D, e2)
    a = (e1 * h).sum(-1)
    with np.errstate(all="ignore"):
        f = 1.0 / a
        s = O - tri[:, :, 0]
        u = f * (s * h).sum(-1)
        q = np.cross(s, e1)
        v = f * (D * q).sum(-1)
        t = f * (e2 * q).sum(-1)
    ok = (np.abs(a) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 1e-6)
    return np.where(ok, t, np.nan)


@pytest.mark.parametrize("how", HOWS)
def test_the_rays_see_the_deformation_and_have_no_ties(how, oracle_api):
    """On the oracle alone: at least a quarter of the case's rays change their hit record between the undeformed scene and a scene built
    fresh from the deformed triangles; and no ray meets two triangles of the deformed scene at one distance (the order in which a refitted
    tree and a rebuilt one find equal hits may differ)."""
    base = tr.grid_mesh()
    new = tr.BEHAVIOUR_DEFORMS[how](base)
    hits = []
    for mesh in (base, new):
        o = oracle_api.OracleScene()
        Ts = tr.spread_transforms(o, tr.BEHAVIOUR_INSTANCES)
        tr.mesh_scene(o, [tr.SMALL, mesh], Ts)
        O, D = tr.aimed_rays(tr.BEHAVIOUR_RAYS, 41, Ts[1::2], new)
        hits.append(o.find_nearest(O, D))
    a, b = hits
    changed = (a["obj"] != b["obj"]) | (_bits(a["t"]) != _bits(b["t"])) | (_bits(a["normal"]) != _bits(b["normal"])).any(1)
    assert changed.sum() >= len(O) // 4, "%d of %d rays see the deformation" % (changed.sum(), len(O))
    assert (b["obj"] >= 2000).sum() >= len(O) // 4, "the rays meet the deformed mesh"
    world = []
    for i, T in enumerate(Ts):
        M = np.asarray(T, dtype=np.float64).reshape(4, 4)
        v = (new if i & 1 else tr.SMALL).reshape(-1, 3).astype(np.float64)
        world.append((v @ M[:3, :3].T + M[:3, 3]).reshape(-1, 3, 3))
    t = np.sort(_moller(O, D, np.concatenate(world)), axis=1)  # NaNs last
    gap = (t[:, 1:] - t[:, :-1]) / np.maximum(np.abs(t[:, :-1]), 1e-30)
    with np.errstate(invalid="ignore"):
        assert not (gap < 1e-5).any(), "two hits at one distance"
