"""What the tests of rt_set_triangles know of the scene a context holds: the uploaded rt_scene_desc read into NumPy, and the UPDATED
description after deformations and moves -- blas[k].tris replaced, blas[k].nodes after the restated bvh::Refit (tests/triangles_ref.py),
the boxes of that BLAS's instances a fresh instance's, tlas_nodes the restated tlas::build over all boxes -- as a new rt_scene_desc that
rt_layout_build and rt_upload_scene take."""
import ctypes as C

import numpy as np

import instances_ref as ir
import triangles_ref as tr
from test_layout_cpu import INSTANCE, RtBlas, RtSceneDesc, desc_array, read_desc

f32 = np.float32


class Desc:
    def __init__(self, host_api, scene):
        self.ptr = scene.describe()
        raw = RtSceneDesc.from_address(self.ptr.value)
        self.raw = RtSceneDesc.from_buffer_copy(raw)
        self.rawblas = [RtBlas.from_buffer_copy(b) for b in (RtBlas * raw.n_blas).from_address(raw.blas)]
        d = read_desc(host_api, self.ptr)
        self.use_tlas = bool(d["use_tlas"])
        self.blas = d["blas"]
        self.tris = [np.array(b["tris"], dtype=tr.TRIANGLE) for b in self.blas]
        self.nodes = [np.array(b["nodes"], dtype=tr.BVH_NODE) for b in self.blas]
        self.spheres = [desc_array(b.spheres, b.n_sph, tr.SPHERE) for b in self.rawblas]
        self.planes = [desc_array(b.planes, b.n_pla, tr.PLANE) for b in self.rawblas]
        self.inst = np.array(d["instances"], dtype=INSTANCE)
        self.n = len(self.inst)
        self.tlas = np.ascontiguousarray(d["tlas"]).view(np.uint32).reshape(-1, 8).copy()
        self.bounds = np.zeros((self.n, 6), f32)
        for i, nd in enumerate(d["tlas"]):  # the box of an untouched instance: its leaf in the uploaded TLAS
            if nd["left_right"] == 0 and not (i == 0 and len(d["tlas"]) > 1):
                self.bounds[int(nd["blas"])] = np.concatenate([nd["aabb_min"], nd["aabb_max"]])
        # the description's other arrays, copied: the scene's own are only valid until it is described again
        own = lambda ptr, nbytes: C.create_string_buffer(C.string_at(ptr, nbytes), nbytes) if ptr and nbytes else None
        self.prim_idx = [np.ascontiguousarray(b["prim_idx"]) for b in self.blas]
        self.own = dict(brute_spheres=own(raw.brute_spheres, raw.n_brute_spheres * tr.SPHERE.itemsize), brute_planes=own(raw.brute_planes, raw.n_brute_planes * tr.PLANE.itemsize),
                        lights=own(raw.lights, raw.n_lights * 56), materials=own(raw.materials, raw.n_materials * 64),
                        sky_pixels=own(raw.sky_pixels, max(0, raw.sky_w * raw.sky_h * raw.sky_n)))
        self._keep = []

    def ranges(self):
        return tr.blas_ranges([dict(nodes=n, n_prims=b["n_prims"]) for n, b in zip(self.nodes, self.blas)])

    def deform(self, k, v9, N=None):
        """BLAS k under the vertices v9 (normals N, or Triangle::update's): the records to send; the description follows"""
        self.tris[k] = tr.triangles(self.tris[k], v9, N)
        self.nodes[k] = tr.refit(self.nodes[k], self.blas[k]["prim_idx"], self.tris[k], self.spheres[k], self.planes[k])
        if self.use_tlas:
            self.bounds = tr.updated_bounds(self.bounds, self.inst["blas"], k, self.nodes[k], self.inst["transform"])
            self.tlas = ir.tlas_build(self.bounds)
        return self.tris[k]

    def move(self, first, rec, bounds=None):
        """rt_set_instances(first, rec, bounds): the records replaced, the boxes given or a fresh instance's over the BLAS's current nodes"""
        for j in range(len(rec)):
            i = first + j
            self.inst[i] = (rec["blas"][j], rec["transform"][j], rec["inv_transform"][j])
            self.bounds[i] = bounds[j] if bounds is not None else ir.fresh_bounds(tr.local_box(self.nodes[int(rec["blas"][j])]), rec["transform"][j])
        self.tlas = ir.tlas_build(self.bounds)

    def desc(self):
        """the updated description as a pointer rt_layout_build / rt_upload_scene take (its arrays stay alive with this object)"""
        blas = (RtBlas * len(self.rawblas))()
        keep = [blas]
        for k, b in enumerate(self.rawblas):
            blas[k] = RtBlas.from_buffer_copy(b)
            t, nd = np.ascontiguousarray(self.tris[k]), np.ascontiguousarray(self.nodes[k])
            keep += [t, nd]
            blas[k].tris, blas[k].nodes, blas[k].prim_idx = t.ctypes.data, nd.ctypes.data, self.prim_idx[k].ctypes.data
            blas[k].spheres = self.spheres[k].ctypes.data if len(self.spheres[k]) else None
            blas[k].planes = self.planes[k].ctypes.data if len(self.planes[k]) else None
        d = RtSceneDesc.from_buffer_copy(self.raw)
        d.blas = C.addressof(blas)
        for name, buf in self.own.items():
            setattr(d, name, C.addressof(buf) if buf is not None else None)
        if self.use_tlas:
            inst, tl = np.ascontiguousarray(self.inst), np.ascontiguousarray(self.tlas)
            keep += [inst, tl]
            d.instances, d.tlas_nodes, d.tlas_nodes_used = inst.ctypes.data, tl.ctypes.data, len(tl)
        keep.append(d)
        self._keep.append(keep)
        return C.c_void_p(C.addressof(d))


# ---- the scenes of the layout tests --------------------------------------------------------------------------------------------------------
LAYOUT_CASES = ("tri1", "tri2", "tri17", "rand_s0", "rand_s1", "rand_s2", "rand_s3", "sentinel", "refit", "mixed_small", "refit_scene")


def build_case(b, name, scenes):
    """scene 'name' through the builder b: dict(k: the BLAS the tests deform, meshes: the builder's meshes whose triangles make it up, in
    order, host: that BLAS for the host mirror's calls (-1: the scene BVH), sentinel: the mesh ends with the two v = 999 triangles)"""
    import build_cases as bc
    if name.startswith("tri"):
        n = int(name[3:])
        ir.triangles_scene(b, ir.grid_transforms(b, n))
        k = 1 if n > 1 else 0  # (one instance: one BLAS)
        return dict(k=k, meshes=[k], host=k, sentinel=False)
    if name in ("mixed_small", "refit_scene"):
        (scenes.REGISTRY["mixed_small"] if name == "mixed_small" else bc.refit_scene)(b)
        return dict(k=0, meshes=list(range(b.n_meshes())), host=-1, sentinel=False)
    split = int(name[-1]) if name.startswith("rand_s") else (2 if name == "refit" else 0)
    mesh = tr.sentinel_mesh() if name == "sentinel" else (bc.refit_triangles() if name == "refit" else tr.random_mesh())
    tr.mesh_scene(b, [tr.SMALL, mesh], tr.spread_transforms(b, 3), split)
    return dict(k=1, meshes=[1], host=1, sentinel=name == "sentinel")


def deformed(case, d, how):
    """the vertices and normals of the case's BLAS under deformation 'how' (a sentinel mesh keeps its sentinels, with N = 0)"""
    v9 = tr.v9_of(d.tris[case["k"]])
    if not case["sentinel"]:
        return tr.DEFORMS[how](v9), None
    new = np.concatenate([tr.DEFORMS[how](v9[:-2]), v9[-2:]])
    return new, tr.sentinel_normals(new)
