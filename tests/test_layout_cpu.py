"""CPU tier for the scene layout (csrc/rt_layout.h build_layout, through the device-free rt_layout_* entry points): what rt_upload_scene
makes of an rt_scene_desc.  test_layout_equals_parent: every array and scalar equals, bit for bit, what the commit before the split copied
to the device (profiles/upload_parent_digests.json, recorded from that commit with profiles/patches/upload_host_stub.diff).  The other
tests state the guarantees the traversal kernels rely on, from the description alone: they know nothing of the digests."""
import ctypes as C
import ctypes.util
import hashlib
import json
import os

import numpy as np
import pytest

from test_host_cpu import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [(-1, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)]  # (RT_WIDE, RT_WIDE8, RT_TLAS_LDS)
LEAF_BIT, INST_BIT, BOX_BIT, EMPTY = 0x80000000, 0x40000000, 0x20000000, 0xFFFFFFFF
# csrc/rt_scene_dev.h: RT_LDS_WORDS, RT_BLOCK, RT_STACK_ROWS_MAX, RT_STACK_ROWS_MIN
LDS_WORDS, BLOCK, ROWS_MAX, ROWS_MIN = 5120, 256, 14, 8


# ---- the description, read back through ctypes (include/rt_amd.h) -----------------------------------------
class RtBlas(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodes_used", C.c_uint32), ("prim_idx", C.c_void_p), ("n_prims", C.c_uint32), ("tris", C.c_void_p), ("n_tri", C.c_uint32),
                ("spheres", C.c_void_p), ("n_sph", C.c_uint32), ("planes", C.c_void_p), ("n_pla", C.c_uint32)]


class RtSceneDesc(C.Structure):
    _fields_ = [("use_tlas", C.c_int32), ("blas", C.c_void_p), ("n_blas", C.c_uint32), ("instances", C.c_void_p), ("n_instances", C.c_uint32),
                ("tlas_nodes", C.c_void_p), ("tlas_nodes_used", C.c_uint32), ("brute_spheres", C.c_void_p), ("n_brute_spheres", C.c_uint32),
                ("brute_planes", C.c_void_p), ("n_brute_planes", C.c_uint32), ("lights", C.c_void_p), ("n_lights", C.c_uint32),
                ("materials", C.c_void_p), ("n_materials", C.c_uint32), ("sky_pixels", C.c_void_p), ("sky_w", C.c_int32), ("sky_h", C.c_int32), ("sky_n", C.c_int32)]


TLAS_NODE = np.dtype([("aabb_min", np.float32, 3), ("left_right", np.uint32), ("aabb_max", np.float32, 3), ("blas", np.uint32)])
INSTANCE = np.dtype([("blas", np.int32), ("transform", np.float32, 16), ("inv_transform", np.float32, 16)])
MATERIAL = np.dtype([("type", np.int32), ("raytracer", np.int32), ("col", np.float32, 3), ("albedo", np.float32, 3), ("specu", np.float32), ("diffu", np.float32),
                     ("shinieness", np.float32), ("N", np.int32), ("ir", np.float32), ("absorption", np.float32, 3)])
LIGHT = np.dtype([("kind", np.int32), ("obj_idx", np.int32), ("pos", np.float32, 3), ("strength", np.float32), ("col", np.float32, 3), ("normal", np.float32, 3),
                  ("radius", np.float32), ("sin_angle", np.float32)])


def desc_array(ptr, n, dtype):
    return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype).copy() if ptr and n else np.zeros(0, dtype)


def read_desc(host_api, ptr):
    """the arrays behind an rt_scene_desc pointer, as numpy copies"""
    d = RtSceneDesc.from_address(ptr.value)
    blas = []
    for b in (RtBlas * d.n_blas).from_address(d.blas):
        blas.append(dict(nodes=desc_array(b.nodes, b.nodes_used, host_api.RT_BVH_NODE_DTYPE), prim_idx=desc_array(b.prim_idx, b.n_prims, np.dtype(np.uint32)),
                         tris=desc_array(b.tris, b.n_tri, host_api.RT_TRIANGLE_DTYPE), n_prims=b.n_prims, n_tri=b.n_tri, n_sph=b.n_sph, n_pla=b.n_pla))
    return dict(use_tlas=d.use_tlas, blas=blas, instances=desc_array(d.instances, d.n_instances, INSTANCE), tlas=desc_array(d.tlas_nodes, d.tlas_nodes_used, TLAS_NODE),
                materials=desc_array(d.materials, d.n_materials, MATERIAL))


def built(scenes, host_api, name, kw):
    h = host_api.HostScene()
    info = scenes.REGISTRY[name](h, **kw)
    return h, info


# ---- the layout equals the parent's ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parent_digests():
    return json.load(open(os.path.join(ROOT, "profiles", "upload_parent_digests.json")))["digests"]


def parent_view(L, use_tlas):
    """the layout as the commit before the split showed it: the arrays it copied, and the scalars it left in DScene and the context"""
    u32 = lambda a: np.asarray(a, dtype=np.uint32)
    wide_built = len(L["wide"]) > 0 or L["wideOK"]
    wide8_built = bool(L["wide8OK"]) and len(L["wide8"]) > 0
    out = {k: L[k] for k in ("pairs", "prims", "wide", "wide8", "leafBox", "reach", "brute", "inst", "lights", "mats", "refitOrder", "refitLevelStart",
                             "rootLink", "rootWide", "rootWide8", "scalars")}
    out["primsOrig"] = L["prims"][:L["animSlots"] * 16]
    out["blasRootWide"] = L["rootWide"] if L["wideOK"] else L["rootLink"]  # what the scoped queries enter a BLAS by
    out["dscene"] = u32([1 if use_tlas else 0, L["rootWide"][0] if wide_built else 0, L["rootWide8"][0] if wide8_built else EMPTY, len(L["wide"]) // 32,
                         len(L["mats"]) // 16, 1 if L["wideOK"] else 0, 1 if wide8_built else 0, L["nInst"] if use_tlas else 0])
    return out


@pytest.mark.parametrize("name,kw", SCENES)
def test_layout_equals_parent(name, kw, scenes, host_api, parent_digests):
    h, info = built(scenes, host_api, name, kw)
    want = parent_digests[name + json.dumps(kw, sort_keys=True)]
    for knobs in KNOBS:
        got = parent_view(host_api.layout(h.describe(), *knobs), info["tlas"])
        ref = want["%d,%d,%d" % knobs]
        assert set(got) == set(ref)
        for arr in sorted(ref):
            assert hashlib.sha256(np.ascontiguousarray(got[arr]).tobytes()).hexdigest() == ref[arr], "array %s differs from the parent's under %r" % (arr, knobs)
    h.close()


# ---- invariants, from the description alone -----------------------------------------------------------------------
INVARIANT_SCENES = [("mixed_small", {"split": 0}), ("tlas_test2", {}), ("pretty_tlas", {"n_instances": 8})]
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


@pytest.fixture(scope="module", params=INVARIANT_SCENES, ids=lambda p: p[0])
def case(request, scenes, host_api):
    """one scene: its description, its layout with both wide forms forced on, and per BLAS the offsets of its records"""
    name, kw = request.param
    h, info = built(scenes, host_api, name, kw)
    ptr = h.describe()
    d = read_desc(host_api, ptr)
    L = host_api.layout(ptr, 1, 1, 1)
    assert L["wideOK"], "the reference's trees are nested"
    # ... and bounded unless a plane's +-1e30 slab is among the boxes: then the 8-wide form is refused as a whole
    assert L["wide8OK"] == (not any(b["n_pla"] for b in d["blas"])) and (L["wide8OK"] or len(L["wide8"]) == len(L["leafBox"]) == 0)
    pair_off = np.concatenate([[0], np.cumsum([len(b["nodes"]) // 2 for b in d["blas"]])]).astype(np.int64)
    prim_off = np.concatenate([[0], np.cumsum([b["n_prims"] for b in d["blas"]])]).astype(np.int64)
    yield dict(d=d, L=L, pair_off=pair_off, prim_off=prim_off, info=info)
    h.close()


def used_nodes(b):
    """indices of the binary nodes that exist (node 1 is never written), split into leaves and inner nodes"""
    idx = np.array([i for i in range(len(b["nodes"])) if i != 1], dtype=np.int64)
    leaf = b["nodes"]["prim_count"][idx] > 0
    return idx[leaf], idx[~leaf]


def test_pairs_and_prims(case):
    d, L = case["d"], case["L"]
    pairs = L["pairs"].view(np.uint32).reshape(-1, 16)
    kind = L["prims"].view(np.uint32).reshape(-1, 16)[:, 15]
    mat = L["prims"].view(np.int32).reshape(-1, 16)[:, 14]
    last = (kind & 4) != 0
    n_leaves = 0
    for k, b in enumerate(d["blas"]):
        if b["n_prims"] == 0:
            continue
        po, so, nd = int(case["pair_off"][k]), int(case["prim_off"][k]), b["nodes"]
        leaves, inner = used_nodes(b)
        n_leaves += len(leaves)
        for i in list(leaves) + list(inner):
            if i == 0:
                link = int(L["rootLink"][k])
            else:
                link = int(pairs[po + i // 2, 3 + 8 * (i & 1)])
                assert np.array_equal(pairs[po + i // 2, 8 * (i & 1):8 * (i & 1) + 3].view(np.float32), nd["aabb_min"][i])
                assert np.array_equal(pairs[po + i // 2, 8 * (i & 1) + 4:8 * (i & 1) + 7].view(np.float32), nd["aabb_max"][i])
            lf, pc = int(nd["left_first"][i]), int(nd["prim_count"][i])
            if pc == 0:  # an inner link names a pair record of its own BLAS: the record of the node's children
                assert link == po + lf // 2 and po < link < po + len(nd) // 2
            else:        # a leaf link names a slot of its own BLAS whose run ends at the first last bit
                assert link == (LEAF_BIT | (so + lf)) and so <= so + lf and so + lf + pc <= so + b["n_prims"]
                assert not last[so + lf:so + lf + pc - 1].any() and last[so + lf + pc - 1]
    assert int(last.sum()) == n_leaves
    types = d["materials"]["type"]
    ok = (mat >= 0) & (mat < len(types))
    assert ok.all() and np.array_equal((kind[ok] >> 4) & 3, types[mat[ok]].astype(np.uint32))
    assert np.all((kind & 3) <= 2)


def leaf_slots(b, so):
    leaves, _ = used_nodes(b)
    return sorted(so + int(b["nodes"]["left_first"][i]) for i in leaves)


def test_wide_nodes(case):
    d, L = case["d"], case["L"]
    wf, wu = L["wide"].reshape(-1, 32), L["wide"].view(np.uint32).reshape(-1, 32)
    pairs = L["pairs"].reshape(-1, 16)
    link, src = wu[:, 24:28], wu[:, 28:32]
    lo, hi = wf[:, 0:12].reshape(-1, 3, 4), wf[:, 12:24].reshape(-1, 3, 4)  # [record][axis][child]
    used = link != EMPTY
    # a used child carries the box of the binary node its source names; an unused one an inverted box
    r, j = np.nonzero(used)
    s = src[r, j].astype(np.int64)
    rec, side = pairs[s // 2], (s & 1)[:, None]
    assert np.array_equal(lo[r, :, j], np.where(side == 0, rec[:, 0:3], rec[:, 8:11])) and np.array_equal(hi[r, :, j], np.where(side == 0, rec[:, 4:7], rec[:, 12:15]))
    r, j = np.nonzero(~used)
    assert np.all(lo[r, :, j] == np.float32(1e30)) and np.all(hi[r, :, j] == np.float32(-1e30)) and np.all(src[r, j] == EMPTY)
    seen_records = 0
    for k, b in enumerate(d["blas"]):
        root = int(L["rootWide"][k])
        if b["n_prims"] == 0:
            assert root == EMPTY
            continue
        found, todo = [], [root]
        while todo:
            lk = todo.pop()
            if lk & LEAF_BIT:
                found.append(lk & ~LEAF_BIT)
                continue
            seen_records += 1
            todo.extend(int(x) for x in link[lk] if x != EMPTY)
        assert sorted(found) == leaf_slots(b, int(case["prim_off"][k])), "every binary leaf's first slot is reached exactly once"
    assert seen_records == len(wf)


def fmaf(a, b, c):
    return _libm.fmaf(float(a), float(b), float(c))


def test_wide8_nodes(case):
    d, L = case["d"], case["L"]
    if not L["wide8OK"]:
        return  # (the fixture checked why, and that nothing was kept)
    w8 = L["wide8"].reshape(-1, 32)
    origin, exps = w8[:, 0:3].view(np.float32), w8[:, 3]
    q = np.ascontiguousarray(w8[:, 4:16]).view(np.uint8).reshape(-1, 6, 8)  # qlo.x qlo.y qlo.z qhi.x qhi.y qhi.z
    link = w8[:, 16:24]
    leaf_box = L["leafBox"].reshape(-1, 8)
    seen_records, seen_boxes = 0, 0
    for k, b in enumerate(d["blas"]):
        root, so, nd = int(L["rootWide8"][k]), int(case["prim_off"][k]), b["nodes"]
        if b["n_prims"] == 0:
            assert root == EMPTY
            continue
        # the binary node a subtree stands for is the one that covers the same range of slots
        span = {}
        for i in sorted((i for i in range(len(nd)) if i != 1), reverse=True):  # children have larger numbers than their parent
            lf, pc = int(nd["left_first"][i]), int(nd["prim_count"][i])
            span[i] = (so + lf, so + lf + pc) if pc else (min(span[lf][0], span[lf + 1][0]), max(span[lf][1], span[lf + 1][1]))
        node_of = {v: i for i, v in span.items()}
        assert len(node_of) == len(span)
        slot_leaf = {so + int(nd["left_first"][i]): i for i in used_nodes(b)[0]}

        def check_leaf(lk):
            rec = leaf_box[lk & ~BOX_BIT]
            slot = int(rec[3:4].view(np.uint32)[0])
            i = slot_leaf[slot]
            assert np.array_equal(rec[0:3], nd["aabb_min"][i]) and np.array_equal(rec[4:7], nd["aabb_max"][i])
            return i

        found = []

        def walk(lk):  # -> (the range of slots below the link, the binary node it stands for)
            nonlocal seen_records, seen_boxes
            if lk & BOX_BIT:
                seen_boxes += 1
                i = check_leaf(lk)
                found.append(span[i][0])
                return span[i], i
            seen_records += 1
            lo_s, hi_s = None, None
            for j in range(8):
                c = int(link[lk, j])
                if c == EMPTY:
                    assert all(q[lk, a, j] == 255 and q[lk, 3 + a, j] == 0 for a in range(3))
                    continue
                (a0, a1), i = walk(c)
                for a in range(3):  # the box the device evaluates, fma(q, 2^e, origin) in one rounding, contains the binary node's
                    sc = np.ldexp(np.float32(1), int((exps[lk] >> (8 * a)) & 255) - 128)
                    assert fmaf(q[lk, a, j], sc, origin[lk, a]) <= nd["aabb_min"][i][a] and fmaf(q[lk, 3 + a, j], sc, origin[lk, a]) >= nd["aabb_max"][i][a]
                lo_s, hi_s = (a0 if lo_s is None else min(lo_s, a0)), (a1 if hi_s is None else max(hi_s, a1))
            return (lo_s, hi_s), node_of[(lo_s, hi_s)]

        (_, _), top = walk(root)  # (recursion as deep as the 8-wide tree: a third of the binary tree's depth)
        assert top == 0 and sorted(found) == leaf_slots(b, so), "every leaf is reached exactly once"
    assert seen_records == len(w8) and seen_boxes == len(leaf_box)


def inverse3(A):
    """the inverse by cofactors, in the operation order of pack_reach (float64)"""
    det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])
    Ai = [[0.0] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            Ai[r][c] = (A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1]) / det
    return Ai


def test_reach(case):
    d, L = case["d"], case["L"]
    if not d["use_tlas"]:
        assert len(L["reach"]) == 0 and L["tlasPairs"] == 0
        return
    # world box (float64) of the vertices of every triangle a ray can hit, per instance; the object box for the origin bound
    world, extent = [], 1.0
    for inst in d["instances"]:
        t = d["blas"][inst["blas"]]["tris"]
        N = t["N"]
        keep = ~(np.all(N == 0, axis=1) | np.isnan(N).any(axis=1))
        v = np.concatenate([t["v0"][keep], t["v1"][keep], t["v2"][keep]]).astype(np.float64)
        T = inst["transform"].astype(np.float64).reshape(4, 4)
        w = v @ T[:3, :3].T + T[:3, 3]
        world.append((w.min(0), w.max(0)))
        # reachOriginMax: 64 x 3 x the largest coordinate of the object boxes' corners under the exact inverse of invTransform
        m = [float(x) for x in inst["inv_transform"]]
        Ai, tv = inverse3([[m[0], m[1], m[2]], [m[4], m[5], m[6]], [m[8], m[9], m[10]]]), [m[3], m[7], m[11]]
        lo, hi = [float(x) for x in v.min(0)], [float(x) for x in v.max(0)]
        for corner in range(8):
            l = [(hi[a] if corner >> a & 1 else lo[a]) - tv[a] for a in range(3)]
            for a in range(3):
                extent = max(extent, abs(Ai[a][0] * l[0] + Ai[a][1] * l[1] + Ai[a][2] * l[2]))
    assert np.float32(L["reachOriginMax"]) == np.float32(64.0 * 3.0 * extent)
    pairs = L["pairs"].view(np.uint32).reshape(-1, 16)
    reach = L["reach"][:L["tlasPairs"] * 12].reshape(-1, 2, 6)
    assert len(L["reach"]) == L["tlasPairs"] * 12 + 16

    def below(lk):
        if lk & INST_BIT:
            return [lk & ~INST_BIT]
        return below(int(pairs[lk, 3])) + below(int(pairs[lk, 11]))

    assert sorted(below(L["root"])) == list(range(len(d["instances"])))
    for s in range(L["tlasPairs"]):
        for h in range(2):
            for i in below(int(pairs[L["tlasBase"] + s, 3 + 8 * h])):
                assert np.all(reach[s, h, 0:3].astype(np.float64) <= world[i][0]) and np.all(reach[s, h, 3:6].astype(np.float64) >= world[i][1]), (s, h, i)


def lds_rows(pairs, instances):
    """csrc/rt_scene_dev.h: the stack rows a TLAS copy of RT_TLAS_COPY_WORDS(pairs, instances) words leaves of a block's LDS"""
    words = pairs * 28 + instances * 13
    return (LDS_WORDS - ((words + 3) & ~3)) // BLOCK - 6


# 8 instances: 8 pairs, 8 * 28 + 8 * 13 = 328 words, (5120 - 328) // 256 - 6 = 12 rows.  16 instances: 16 pairs, 656 words, (5120 - 656) // 256 - 6 = 11
# rows (csrc/rt_scene_dev.h quoted 10 for them, which no LDS size the library has had gives: 13 at the 5760 words of its first rounds, 11 since)
@pytest.mark.parametrize("name,kw,rows", [("pretty_tlas", {"n_instances": 8}, 12), ("bigb_instanced", {"n": 16}, 11)])
def test_lds_split(name, kw, rows, scenes, host_api):
    h, _ = built(scenes, host_api, name, kw)
    on, off = host_api.layout(h.describe(), -1, 0, 1), host_api.layout(h.describe(), -1, 0, 0)
    assert rows == lds_rows(on["tlasPairs"], on["nInst"]) >= ROWS_MIN and on["nInst"] == kw.get("n_instances", kw.get("n"))
    assert (on["tlasLds"], on["stackRows"]) == (1, rows)
    assert (off["tlasLds"], off["stackRows"]) == (0, ROWS_MAX)
    h.close()
    g, _ = built(scenes, host_api, "mixed_small", {"split": 0})  # no TLAS: nothing to copy, every row is a stack row
    L = host_api.layout(g.describe())
    assert (L["tlasLds"], L["stackRows"]) == (0, ROWS_MAX)
    g.close()


# ---- errors: every refusal of upload that needs no device, with the text the commit before the split reported --------------
def tiny_desc(host_api, tlas=False):
    """one triangle in a two-node tree (the root is a leaf), one material; with tlas: one instance of it under a one-node TLAS.
    Returns (desc, blas, keep): the structures to spoil, and the arrays that must stay alive."""
    nodes = np.zeros(4, dtype=host_api.RT_BVH_NODE_DTYPE)
    nodes["aabb_max"][0] = 1
    nodes["prim_count"][0] = 1
    prim_idx = np.zeros(2, dtype=np.uint32)
    tris = np.zeros(2, dtype=host_api.RT_TRIANGLE_DTYPE)
    tris["v1"][:, 0], tris["v2"][:, 1], tris["N"][:, 2] = 1, 1, 1
    spheres = np.zeros(1, dtype=host_api.RT_SPHERE_DTYPE)
    mats = np.zeros(1, dtype=MATERIAL)
    mats["type"], mats["raytracer"] = 1, 1
    lights = np.zeros(40, dtype=LIGHT)
    inst = np.zeros(1, dtype=INSTANCE)
    inst["transform"][0, [0, 5, 10, 15]] = 1
    inst["inv_transform"][0, [0, 5, 10, 15]] = 1
    tl = np.zeros(4, dtype=TLAS_NODE)
    tl["aabb_max"] = 1
    p = lambda a: a.ctypes.data
    blas = (RtBlas * 1)(RtBlas(p(nodes), 2, p(prim_idx), 1, p(tris), 1, p(spheres), 0, None, 0))
    desc = RtSceneDesc(use_tlas=int(tlas), blas=C.addressof(blas), n_blas=1, materials=p(mats), n_materials=1, lights=p(lights), n_lights=0)
    if tlas:
        desc.instances, desc.n_instances, desc.tlas_nodes, desc.tlas_nodes_used = p(inst), 1, p(tl), 1
    return desc, blas[0], dict(nodes=nodes, prim_idx=prim_idx, tris=tris, spheres=spheres, mats=mats, lights=lights, inst=inst, tl=tl, blas=blas)


def inner_root(a):
    """the tiny tree with an inner root: nodes 2 and 3 are its leaves, one triangle each"""
    a["nodes"]["prim_count"][0], a["nodes"]["left_first"][0] = 0, 2
    a["nodes"]["aabb_max"][2:4], a["nodes"]["prim_count"][2:4], a["nodes"]["left_first"][3] = 1, 1, 1
    a["prim_idx"][1] = 1


def _odd_nodes(d, b, a): b.nodes_used = 3
def _counts(d, b, a): b.n_prims = 2
def _leaf_range(d, b, a): a["nodes"]["prim_count"][0] = 2
def _child(d, b, a): a["nodes"]["prim_count"][0], a["nodes"]["left_first"][0] = 0, 3
def _prim_idx(d, b, a): a["prim_idx"][0] = 5
def _sphere(d, b, a): b.n_sph, b.n_prims = 1, 2
def _bound(d, b, a): a["nodes"]["aabb_min"][0, 0] = np.inf
def _tlas_child(d, b, a): d.tlas_nodes_used, a["tl"]["left_right"][0] = 3, 1 | (9 << 16)
def _ancestor(d, b, a): d.tlas_nodes_used, a["tl"]["left_right"][0], a["tl"]["left_right"][2] = 3, 1 | (2 << 16), 1 | (0 << 16)
def _inst_blas(d, b, a): a["inst"]["blas"][0] = 7
def _mat_type(d, b, a): a["mats"]["type"][0] = 0
def _lights(d, b, a): d.n_lights = 33


# (what is spoiled, TLAS?, the rt_status rt_upload_scene returns, the message)
ERRORS = [(_odd_nodes, False, -2, "rt_upload_scene: blas 0 has 3 nodes (expected an even count >= 2)"),
          (_counts, False, -2, "rt_upload_scene: blas 0 primitive counts disagree"),
          (_leaf_range, False, -2, "rt_upload_scene: blas 0 node 0 leaf range out of bounds"),
          (_child, False, -2, "rt_upload_scene: blas 0 node 0 child index 3 invalid"),
          (_prim_idx, False, -2, "rt_upload_scene: blas 0 prim_idx[0] = 5 out of range"),
          (_sphere, True, -4, "rt_upload_scene: blas 0 holds spheres / planes; an instanced BLAS must be triangles only"),
          (_bound, False, -4, "rt_upload_scene: blas 0 node 0 has a non-finite bound or one beyond 1e30"),
          (_tlas_child, True, -2, "rt_upload_scene: tlas node 0 child out of range"),
          (_ancestor, True, -2, "rt_upload_scene: tlas node 0 is its own ancestor"),
          (_inst_blas, True, -2, "rt_upload_scene: instance 0 blas 7 out of range"),
          (_mat_type, False, -2, "rt_upload_scene: material 0 has type 0"),
          (_lights, False, -4, "rt_upload_scene: 33 lights (limit 32)")]


@pytest.mark.parametrize("spoil,tlas,status,message", ERRORS, ids=[e[0].__name__[1:] for e in ERRORS])
def test_errors(spoil, tlas, status, message, host_api):
    desc, blas, alive = tiny_desc(host_api, tlas)
    assert host_api.layout(C.c_void_p(C.addressof(desc)))["root"] == (INST_BIT if tlas else LEAF_BIT)  # the unspoiled description is accepted
    spoil(desc, blas, alive)
    with pytest.raises(host_api.LayoutError) as e:
        host_api.layout(C.c_void_p(C.addressof(desc)))
    assert e.value.message == message  # (rt_layout_build reports a refusal as NULL + text; the status is pinned on the device: test_gpu_parity.py)


def test_tiny_inner_root(host_api):
    """the smallest tree with a pair record: both wide forms hold one record whose two used children are its leaves"""
    desc, blas, alive = tiny_desc(host_api)
    inner_root(alive)
    blas.nodes_used, blas.n_prims, blas.n_tri = 4, 2, 2
    L = host_api.layout(C.c_void_p(C.addressof(desc)), 1, 1, 1)
    assert L["root"] == 1 and L["wideOK"] and L["wide8OK"] and len(L["wide"]) == 32 and len(L["wide8"]) == 32 and len(L["leafBox"]) == 16
    assert list(L["wide"].view(np.uint32)[24:28]) == [LEAF_BIT, LEAF_BIT | 1, EMPTY, EMPTY]
    assert list(L["wide8"][16:24]) == [BOX_BIT, BOX_BIT | 1] + [EMPTY] * 6
