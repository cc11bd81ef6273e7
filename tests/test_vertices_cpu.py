"""CPU tier for rt_set_mesh_indices / rt_set_vertices (include/rt_amd.h): the support module tests/vertices_ref.py against itself and the
host mirror, the conditions on the GPU tests' inputs (the shared-vertex meshes share, every box extreme of a reduction-boundary mesh sits
on the one triangle it is meant for, the refusal inputs spoil a referenced vertex or an unreferenced one as they say), and the claim the
device's reduction rests on: the sign of a zero in a BLAS's object box reaches no stored byte of the layout.  No device is needed."""
import numpy as np
import pytest

import triangles_desc as td
import triangles_ref as tr
import vertices_ref as vr

f32, u32 = np.float32, np.uint32


def _bits(a):
    return np.ascontiguousarray(a).view(u32)


SOUPS = {"random": lambda: tr.random_mesh(), "sentinel": lambda: tr.sentinel_mesh(), "grid": lambda: tr.grid_mesh(), "small": lambda: tr.SMALL,
         "signed_zeros": lambda: np.array([[0.0, 0, 0, -0.0, 0, 0, 0, -0.0, 1], [-0.0, 0, 0, 0, 0, 0, 1, 1, -0.0]], f32),
         "nan": lambda: np.array([[np.nan, 0, 0, 1, 0, 0, 0, 1, 0], [np.nan, 0, 0, 0, 1, 0, 0, 0, 1]], f32)}


@pytest.mark.parametrize("name", sorted(SOUPS))
def test_assemble_inverts_weld(name):
    v9 = np.ascontiguousarray(SOUPS[name](), dtype=f32).reshape(-1, 9)
    xyz, idx = vr.weld(v9)
    assert idx.dtype == u32 and idx.shape == (len(v9), 3) and idx.max() == len(xyz) - 1
    assert np.array_equal(_bits(vr.assemble(xyz, idx)), _bits(v9))
    assert len(np.unique(_bits(xyz).reshape(-1, 3), axis=0)) == len(xyz), "no vertex twice"
    if name == "signed_zeros":
        assert len(xyz) == 4 and len(np.unique(xyz, axis=0)) == 3, "-0 and +0 are different vertices: (0, 0, 0) and (-0, 0, 0) both stay"
    if name == "grid":
        assert len(xyz) == 13 * 13 and len(xyz) < len(v9), "the height field's corners are shared"
    if name == "sentinel":
        assert len(vr.coincident_faces(xyz, idx)) == 2 and np.array_equal(vr.nan_triangles(v9), [len(v9) - 2, len(v9) - 1])


@pytest.mark.parametrize("name", sorted(vr.SHARED))
def test_the_shared_vertex_meshes_share(name):
    xyz, idx = vr.SHARED[name]()
    assert (len(xyz), len(idx)) == vr.SHARED_COUNTS[name] and len(xyz) < len(idx)
    assert vr.referenced(idx, len(xyz)).all() and idx.max() == len(xyz) - 1
    # what is degenerate in them is so by construction (eight faces of stellatedDode have two corners at one position), under every deformation
    rep = vr.coincident_faces(xyz, idx)
    assert len(rep) == (8 if name == "stellatedDode" else 0)
    for how in (None,) + tuple(vr.DEFORMS):
        v = xyz if how is None else vr.deformed(xyz, how)
        assert np.array_equal(vr.nan_triangles(vr.assemble(v, idx)), rep), how


@pytest.mark.parametrize("name", ["ico", "lowBigB", "three", "stellatedDode"])
def test_mesh_update_equals_the_restated_normals(name, host_api):
    """the host mirror's indexed Mesh::update (faces are 1-based there) against triangles_ref.normals over the assembled triangles"""
    assets = __import__("conftest").pkg("assets")
    h = host_api.HostScene()
    m = h.mesh_obj(1, assets.obj_path(name), h.diffuse(0.8, (1, 1, 1)), (0.1, 0.2, 0.3), 0.7)
    xyz, faces = h.mesh_indexed(m)
    assert (len(xyz), len(faces)) == vr.SHARED_COUNTS[name] and faces.min() == 1 and faces.max() == len(xyz)
    idx = (faces - 1).astype(u32)
    nan = vr.coincident_faces(xyz, idx)
    for how in vr.DEFORMS:
        new = vr.deformed(xyz, how)
        h.set_mesh_vertex_array(m, new)
        h.mesh_update(m)
        got = h.mesh_tris(m)[0]
        v9 = vr.assemble(new, idx)
        assert np.array_equal(_bits(got[:, :9]), _bits(v9)), "the triangles follow the vertices"
        want = tr.normals(v9)
        assert np.array_equal(vr.nan_triangles(v9), nan) and len(nan) <= 8
        ok = np.ones(len(v9), bool)
        ok[nan] = False
        assert np.array_equal(_bits(got[ok, 9:12]), _bits(want[ok])), how
        assert np.isnan(got[nan, 9:12]).all() and np.isnan(want[nan]).all()
    h.close()


@pytest.mark.parametrize("n", vr.BOUNDARY_SIZES)
def test_every_extreme_of_a_boundary_mesh_sits_on_its_triangle(n):
    base, idx = vr.boundary_mesh(n)
    assert len(idx) == n and vr.referenced(idx, len(base)).all() and len(vr.nan_triangles(vr.assemble(base, idx))) == 0
    targets = vr.boundary_targets(n)
    assert targets[0] == 0 and targets[-1] == n - 1
    for b in range(64, n, 64):
        assert b - 1 in targets and b in targets
    for t in targets:
        for e in range(6):
            xyz, intended = vr.boundary_vertices(n, e, t)
            assert intended[e] == t
            v9 = vr.assemble(xyz, idx)
            holders = vr.extreme_holders(v9)
            for k in range(6):
                assert holders[k].tolist() == [intended[k]], "n %d, extreme %d on triangle %d: extreme %d is held by %s" % (n, e, t, k, holders[k])
            v = v9.reshape(-1, 3)
            assert [v[:, 0].min(), v[:, 1].min(), v[:, 2].min(), v[:, 0].max(), v[:, 1].max(), v[:, 2].max()] == list(vr.EXTREME)
            assert len(vr.nan_triangles(v9)) == 0


def test_the_refusal_inputs_spoil_what_they_say():
    xyz, idx = vr.with_spare_vertex(*vr.grid(16, 16))
    ref = vr.referenced(idx, len(xyz))
    assert ref[:-1].all() and not ref[-1]
    for name, (v, vtx, used) in vr.refusal_inputs(xyz, idx).items():
        bad = ~(np.abs(v) <= f32(1e29))
        assert bad.sum() == 1 and bad[vtx].any() and bool(ref[vtx]) == used, name
        tris = np.flatnonzero(~(np.abs(vr.assemble(v, idx)) <= f32(1e29)).all(1))
        assert (len(tris) > 0) == used, name


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_sign_of_a_zero_on_the_box_reaches_no_stored_byte(axis, host_api):
    """two descriptions that differ only in the sign of the zeros of a mesh flattened onto a coordinate plane -- a whole face of the BLAS's
    box, which is what blas_object_box's min and max pick a zero from -- give the same reach, inst and pairs (rt_layout.h instance_reach:
    a bound enters through lo - tv, products, fabs, and lo - m with m >= 1e-20).  One instance has no translation at all (tv = 0)."""
    h = host_api.HostScene()
    Ts = tr.spread_transforms(h, 3)
    Ts[1] = h.trs((0.0, 0.0, 0.0), 1.0, 0.0, 0.0, 0.0)
    tr.mesh_scene(h, [tr.SMALL, tr.grid_mesh()], Ts)
    d = td.Desc(host_api, h)
    flat = tr.collapse(tr.grid_mesh(), axis=axis, at=0.0)
    d.deform(1, flat)
    assert not np.signbit(d.tris[1]["v0"][:, axis]).any()
    plus = host_api.layout(d.desc(), 1, 0, 1)
    for k in ("v0", "v1", "v2"):
        d.tris[1][k][:, axis] = f32(-0.0)  # the triangles alone: nodes and TLAS stay the first description's
    assert np.signbit(d.tris[1]["v0"][:, axis]).all()
    minus = host_api.layout(d.desc(), 1, 0, 1)
    assert not np.array_equal(_bits(plus["prims"]), _bits(minus["prims"])), "the two descriptions differ"
    for name in ("reach", "inst", "pairs"):
        assert np.array_equal(_bits(plus[name]), _bits(minus[name])), name
    assert np.array_equal(plus["scalars"], minus["scalars"])
    h.close()
