"""CPU tier for rt_set_lights / rt_set_materials / rt_set_sky: the cases of tests/look_cases.py are not vacuous.  On rt_layout_build, with
no device: every type edit flips bits 4-5 of the kind word of triangle, sphere, plane and brute-force records and changes no other word
of PRIMS, PAIRS, REACH or INST, and every pathUnsupported case flips scalar 11.  On the oracle: every light, material and sky edit changes
at least one pixel in eight of the 16 x 8 frame the GPU tests render.  And the host mirror's half of Scene::CommitLights / CommitMaterials
/ CommitSky -- ReplaceMaterial, the light list, the skydome -- leaves a scene whose describe() is the edited scene's built from scratch
(the device half needs a context: tests/test_gpu_look.py)."""
import ctypes as C

import numpy as np
import pytest

import look_cases as lc
import support as sp
from test_layout_cpu import RtBlas, RtSceneDesc, read_desc

KNOBS = [(-1, 0, 1), (1, 0, 0)]


def _layout(host_api, knobs=(-1, 0, 1), **kw):
    s = host_api.HostScene()
    lc.look_scene(s, **kw)
    L = host_api.layout(s.describe(), *knobs)
    s.close()
    return L


# ---- the layout -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.TYPE_EDITS)
@pytest.mark.parametrize("knobs", KNOBS)
def test_a_type_edit_flips_type_bits_and_nothing_else(name, knobs, host_api):
    e = lc.MATERIAL_EDITS[name]
    for tlas in (False, True):
        A, B = _layout(host_api, knobs, tlas=tlas, mats=e["before"]), _layout(host_api, knobs, tlas=tlas, mats=e["after"])
        for arr in ("pairs", "reach", "inst", "wide", "wide8", "leafBox", "refitOrder", "rootLink"):
            assert sp.same(A[arr], B[arr]), arr
        flipped = set()
        for arr in ("prims", "brute"):
            (ka, wa), (kb, wb) = lc.kind_words(A[arr]), lc.kind_words(B[arr])
            assert np.array_equal(wa, wb), "%s: a word other than the kind word changed" % arr
            assert np.array_equal(ka & ~np.uint32(lc.TYPE_MASK), kb & ~np.uint32(lc.TYPE_MASK)), "%s: the kind or the last bit changed" % arr
            for k in np.unique(ka[ka != kb] & 3):
                flipped.add((arr, int(k)))
            mat = wa[:, 14].view(np.int32)
            named = (mat >= e["first"]) & (mat < e["first"] + e["count"])
            assert not np.any((ka != kb) & ~named), "only records that name an edited material change"
        # kinds (csrc/rt_scene_dev.h): 0 triangle, 1 sphere, 2 plane
        want = {("prims", 0), ("brute", 1), ("brute", 2)} if tlas else {("prims", 0), ("prims", 1), ("prims", 2)}
        assert want <= flipped, (tlas, flipped)
        assert A["pathUnsupported"] == B["pathUnsupported"] == 0


def test_kind_numbers(host_api):
    """the kinds the test above names are the library's: a scene BVH of one triangle, one sphere, one plane holds one record of each"""
    L = _layout(host_api)
    kind, w = lc.kind_words(L["prims"])
    mat = w[:, 14].view(np.int32)
    assert sorted(kind & 3) == [0, 0, 0, 1, 1, 2, 2]
    # the panel's two triangles, a sphere and the wall name X (1); the type bits are X's type
    assert sorted((kind & 3)[mat == 1]) == [0, 0, 1, 2] and np.all((kind[mat == 1] & lc.TYPE_MASK) >> lc.TYPE_SHIFT == lc.DIFFUSE)


@pytest.mark.parametrize("name", ["shiny_on", "shiny_off"])
def test_path_support_flips_scalar_11(name, host_api):
    e = lc.MATERIAL_EDITS[name]
    for tlas in (False, True):
        A, B = _layout(host_api, tlas=tlas, mats=e["before"]), _layout(host_api, tlas=tlas, mats=e["after"])
        assert (int(A["scalars"][11]), int(B["scalars"][11])) == e["unsupported"] and A["pathUnsupported"] != B["pathUnsupported"]
        assert sp.same(A["prims"], B["prims"]) and sp.same(A["brute"], B["brute"]) and not sp.same(A["mats"], B["mats"])


def test_every_material_edit_changes_its_range_of_the_table_only(host_api):
    for name, e in lc.MATERIAL_EDITS.items():
        a, b = lc.scene_tables(host_api, mats=e["before"])[0], lc.scene_tables(host_api, mats=e["after"])[0]
        differs = np.array([a[i].tobytes() != b[i].tobytes() for i in range(len(a))])
        assert len(a) == len(b) == 4 and differs[e["first"]:e["first"] + e["count"]].all() and differs.sum() == e["count"], name
        assert bool((a["type"] != b["type"]).any()) == e["type"], name


def test_out_of_range_material_indices_get_no_type(host_api):
    """pack_prim's rule for an index outside the table: type bits 0, whatever the table holds"""
    import triangles_desc as td
    s = host_api.HostScene()
    lc.look_scene(s)
    d = td.Desc(host_api, s)
    base = lc.kind_words(host_api.layout(d.desc())["prims"])[0]
    d.tris[0]["material"][0], d.tris[0]["material"][1] = -1, 4
    for mats in (lc.tables(d.ptr)[0], lc.retyped(lc.tables(d.ptr)[0])):
        L = host_api.layout(lc.patch(d, mats=mats).desc())
        kind, w = lc.kind_words(L["prims"])
        mat = w[:, 14].view(np.int32)
        out = (mat < 0) | (mat >= 4)
        assert out.sum() == 2 and np.all(kind[out] & lc.TYPE_MASK == 0) and np.all(kind[~out] & lc.TYPE_MASK != 0)
    assert not np.array_equal(base, kind)
    s.close()


@pytest.mark.parametrize("n", lc.STRIP_SIZES)
def test_strip_scenes_hold_that_many_records(n, host_api):
    s = host_api.HostScene()
    lc.strip_scene(s, n)
    L = host_api.layout(s.describe())
    assert len(L["prims"]) == 16 * n and (n > 1 or L["root"] & 0x80000000), "n = 1: the root is a leaf"
    s.close()


def test_light_tables(host_api):
    for n in lc.LIGHT_TABLES:
        mats, lights, sky = lc.scene_tables(host_api, lights=lc.lights(n))
        assert len(lights) == n and (n < 2 or set(lights["kind"]) == {0, 1}), "area and directional lights"
        assert np.array_equal(lights["obj_idx"], 11 + np.arange(n))
        L = _layout(host_api, lights=lc.lights(n))
        assert len(L["lights"]) == 14 * max(n, 1)


# ---- the oracle: the edits are visible in the frame the GPU tests render ------------------------------------------------------------------------
def _frames(oracle_api, **kw):
    """(a path frame of 4 spp, a Whitted frame) of look_scene(**kw) at the GPU tests' size"""
    o = oracle_api.OracleScene()
    lc.look_scene(o, **kw)
    orr = oracle_api.OracleRenderer(o, lc.W, lc.H)
    out = []
    for whitted in (False, True):
        o.set_raytracer(whitted)
        orr.clear()
        orr.render(0, 1 if whitted else 4, nthreads=0)
        out.append(orr.accumulator()[..., :3].copy())
    orr.close(), o.close()
    return out


def _changed(a, b):
    """the share of pixels whose bits differ"""
    return float((sp.bits(a) != sp.bits(b)).any(-1).mean())


_BASE = {}


def _base(oracle_api, tlas):
    if tlas not in _BASE:
        _BASE[tlas] = _frames(oracle_api, tlas=tlas)
    return _BASE[tlas]


@pytest.mark.parametrize("tlas", [False, True], ids=["bvh", "tlas"])
def test_the_oracle_sees_every_material_edit(tlas, oracle_api):
    for name, e in lc.MATERIAL_EDITS.items():
        before = _base(oracle_api, tlas) if e["before"] == lc.MATS else _frames(oracle_api, tlas=tlas, mats=e["before"])
        after = _base(oracle_api, tlas) if e["after"] == lc.MATS else _frames(oracle_api, tlas=tlas, mats=e["after"])
        share = [_changed(x, y) for x, y in zip(before, after)]
        print("%s tlas=%d: path %.3f whitted %.3f of the pixels change" % (name, tlas, share[0], share[1]))
        assert min(share) >= 1 / 8, (name, share)


@pytest.mark.parametrize("tlas", [False, True], ids=["bvh", "tlas"])
def test_the_oracle_sees_every_light_and_sky_edit(tlas, oracle_api):
    tabs = {n: _frames(oracle_api, tlas=tlas, lights=lc.lights(n)) for n in lc.LIGHT_TABLES}
    for a, b in lc.LIGHT_TRANSITIONS + ((31, 32),):
        share = [_changed(x, y) for x, y in zip(tabs[a], tabs[b])]
        print("lights %d -> %d tlas=%d: path %.3f whitted %.3f" % (a, b, tlas, share[0], share[1]))
        assert min(share) >= 1 / 8, (a, b, share)
    for name, sky in lc.SKY_EDITS.items():
        share = [_changed(x, y) for x, y in zip(_base(oracle_api, tlas), _frames(oracle_api, tlas=tlas, sky=sky))]
        print("sky %s tlas=%d: path %.3f whitted %.3f" % (name, tlas, share[0], share[1]))
        assert min(share) >= 1 / 8, (name, share)


# ---- the host mirror -----------------------------------------------------------------------------------------------------------------------
def _described(host_api, s):
    """everything a description holds that the edits may touch or must not touch, as bytes and arrays"""
    ptr = s.describe()
    mats, lights, sky = lc.tables(ptr)
    d = read_desc(host_api, ptr)
    raw = RtSceneDesc.from_address(ptr.value)
    blas = (RtBlas * raw.n_blas).from_address(raw.blas)
    sph = [C.string_at(b.spheres, b.n_sph * 32) if b.spheres else b"" for b in blas] + [C.string_at(raw.brute_spheres, raw.n_brute_spheres * 32) if raw.brute_spheres else b""]
    pla = [C.string_at(b.planes, b.n_pla * 24) if b.planes else b"" for b in blas] + [C.string_at(raw.brute_planes, raw.n_brute_planes * 24) if raw.brute_planes else b""]
    tris = [b["tris"].tobytes() for b in d["blas"]]
    nodes = [b["nodes"].tobytes() for b in d["blas"]]
    return dict(mats=mats.tobytes(), lights=lights.tobytes(), sky=None if sky is None else (sky.shape, sky.tobytes()), sph=sph, pla=pla, tris=tris, nodes=nodes,
                inst=d["instances"].tobytes(), tlas=d["tlas"].tobytes(), counts=(raw.n_lights, raw.n_materials, raw.sky_w, raw.sky_h, raw.sky_n))


def _replace(s, index, spec):
    getattr(s, "replace_" + spec[0])(index, **spec[1])


@pytest.mark.parametrize("tlas", [False, True], ids=["bvh", "tlas"])
def test_host_edits_describe_the_edited_scene(tlas, host_api):
    def scratch(**kw):
        s = host_api.HostScene()
        lc.look_scene(s, tlas=tlas, **kw)
        out = _described(host_api, s)
        s.close()
        return out

    for name, e in lc.MATERIAL_EDITS.items():
        s = host_api.HostScene()
        lc.look_scene(s, tlas=tlas, mats=e["before"])
        s.describe()
        for i in range(e["first"], e["first"] + e["count"]):
            _replace(s, i, e["after"][i])
        assert _described(host_api, s) == scratch(mats=e["after"]), name
        s.close()
    for a, b in lc.LIGHT_TRANSITIONS:
        s = host_api.HostScene()
        lc.look_scene(s, tlas=tlas, lights=lc.lights(a))
        s.clear_lights()
        for l in lc.lights(b):
            lc.add_light(s, l)
        assert _described(host_api, s) == scratch(lights=lc.lights(b)), (a, b)
        s.close()
    for name, sky in lc.SKY_EDITS.items():
        s = host_api.HostScene()
        lc.look_scene(s, tlas=tlas)
        if sky is None:
            s.clear_sky()
        else:
            s.sky(lc.sky_image(*sky))
        got, want = _described(host_api, s), scratch(sky=sky)
        assert got == want, name
        s.close()


def test_commit_needs_a_committed_scene(host_api):
    s = host_api.HostScene()
    lc.look_scene(s)
    for commit in (s.commit_lights, s.commit_materials, s.commit_sky):
        with pytest.raises(RuntimeError, match="Commit"):
            commit()
    with pytest.raises(RuntimeError, match="no such material"):
        s.replace_metal(9, 0.1, (1, 1, 1))
    s.close()


def test_the_abi_declares_the_three_calls(host_api):
    L = host_api.rt_lib()
    for name in ("rt_set_lights", "rt_set_materials", "rt_set_sky"):
        assert name in host_api.RT_SYMBOLS and hasattr(L, name)
    # no context: refused before anything else is looked at
    assert L.rt_set_lights(None, None, 0) == host_api.RT_E_ARG and L.rt_set_materials(None, 0, 1, None) == host_api.RT_E_ARG and L.rt_set_sky(None, None, 0, 0, 0) == host_api.RT_E_ARG
