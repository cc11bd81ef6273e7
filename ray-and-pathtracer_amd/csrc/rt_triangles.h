// rt_set_triangles on the device: the triangles of one BLAS replaced in place, its tree refitted (k_refit / k_refit_level of rt_kernels.h:
// bvh::Refit, the tree keeps its shape and its prim_idx order) and, under a TLAS, the box the refit leaves at the BLAS's root handed to
// k_instance_bounds (rt_instances.h).  The yardstick is rt_set_instances's: afterwards the context holds, byte for byte, what
// rt_upload_scene would hold of the updated description.  What makes that possible without a host re-layout:
//
//   1. A primitive record depends on its own primitive alone (rt_layout.h pack_prim), but for the LAST bit, which marks the end of a leaf
//      and belongs to the slot: the kernel keeps the one of the record it overwrites.  The slot of primitive p is the inverse of prim_idx,
//      kept per BLAS at upload (4 bytes per primitive).
//   2. A pair record's links never change under a refit, and its boxes are what bvh::Refit computes from the leaf records bottom-up:
//      k_refit_level / k_refit over the BLAS's own level order (rt_layout.h blas_refit_order, pair indices absolute), which
//      tests/test_gpu_build.py holds to the oracle bit for bit, signs of zero included.
//   3. Node 0 has no pair record: its box is the union of the root pair's two halves in Refit's operand order (fminf(l, r)), or the leaf's
//      own bounds when the root is a leaf; bvh::bounds is an empty box grown by that box's two corners (bvh.cpp:48-49).
//
// Plain HIP C++ only.
#pragma once
#include "rt_kernels.h"

namespace rtd {

// A lane per triangle.  tris: the staged rt_triangle records (14 words each: v0 v1 v2 N obj_idx material), read by a wave as one
// contiguous run; slotOf[p]: the absolute leaf slot of primitive p (0xFFFFFFFF: prim_idx never names it).  The record is pack_prim's:
// {v0, N.x} {v1, N.y} {v2, N.z} {d, objIdx, mat, kind | last | type}, d = -((N.x * v0.x + N.y * v0.y) + N.z * v0.z) with every operation
// rounded on its own, the material's type from the device's table.
__global__ void __launch_bounds__(256) k_set_triangles(const float2* __restrict__ tris, int nTri, const uint* __restrict__ slotOf, float4* prims,
                                                       const DMaterial* __restrict__ mats, int nMats)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= nTri) return;
	const uint slot = slotOf[p];
	if (slot == 0xFFFFFFFFu) return;
	const float2* t = tris + 7 * (size_t)p; // 56-byte records, 8-byte aligned
	const float2 a = t[0], b = t[1], c = t[2], d2 = t[3], e = t[4], f = t[5], g = t[6];
	// v0 = a.x a.y b.x, v1 = b.y c.x c.y, v2 = d2.x d2.y e.x, N = e.y f.x f.y, obj = g.x, mat = g.y
	const float s = __fadd_rn(__fadd_rn(__fmul_rn(e.y, a.x), __fmul_rn(f.x, a.y)), __fmul_rn(f.y, b.x));
	const int mat = __float_as_int(g.y);
	float4* rec = prims + 4 * (size_t)slot;
	int kl = RT_KIND_TRI | (__float_as_int(rec[3].w) & RT_LAST_BIT);
	if (mat >= 0 && mat < nMats) kl |= (mats[mat].type & 3) << RT_TYPE_SHIFT;
	rec[0] = make_float4(a.x, a.y, b.x, e.y);
	rec[1] = make_float4(b.y, c.x, c.y, f.x);
	rec[2] = make_float4(d2.x, d2.y, e.x, f.y);
	rec[3] = make_float4(-s, g.x, g.y, __int_as_float(kl));
}

// bvh::bounds of a refitted BLAS into box6Out (min.xyz, max.xyz): one lane.  rootLink: the BLAS's root as a pair link (a pair record, or
// LEAF_BIT | first slot).
__global__ void k_blas_root_box(const float4* pairs, const float4* prims, uint rootLink, float* box6Out)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	f3 lo, hi;
	if (rootLink & RT_LEAF_BIT) leaf_bounds(prims, rootLink & ~RT_LEAF_BIT, lo, hi);
	else {
		const float4* ch = pairs + 4 * (size_t)rootLink;
		lo = f3(t_fminf(ch[0].x, ch[2].x), t_fminf(ch[0].y, ch[2].y), t_fminf(ch[0].z, ch[2].z));
		hi = f3(t_fmaxf(ch[1].x, ch[3].x), t_fmaxf(ch[1].y, ch[3].y), t_fmaxf(ch[1].z, ch[3].z));
	}
	// aabb::grow(node.aabbMin), grow(node.aabbMax) from the empty box
	const float mn[3] = { lo.x, lo.y, lo.z }, mx[3] = { hi.x, hi.y, hi.z };
	for (int a = 0; a < 3; a++) {
		float l = 1e30f, h = -1e30f;
		l = t_fminf(l, mn[a]), h = t_fmaxf(h, mn[a]);
		l = t_fminf(l, mx[a]), h = t_fmaxf(h, mx[a]);
		box6Out[a] = l, box6Out[3 + a] = h;
	}
}

} // namespace rtd
