// rt_set_instances on the device: what of the traversal layout (rt_layout.h) depends on an instance's transform, rewritten in place from a
// TLAS that k_build_tlas (rt_build.h) has just built into scratch -- the TLAS pair records at the tail of pairs[], the reach[] records
// beside them, and the context's copy of the TLAS nodes.  The yardstick: afterwards inst[], pairs[], reach[] and the scalars are byte-equal
// to build_layout's on the updated description.  Three facts make that possible without a host re-layout:
//
//   1. tlas::build (tlas.cpp:13-48, k_build_tlas) numbers its nodes independently of the boxes' values: leaves are nodes 1..n (leaf i holds
//      instance i - 1), every merge appends one inner node, so inner nodes are n+1..2n-1 and a child's index is below its parent's; node 0 is
//      a copy of the last inner node (of the one leaf when n == 1).  pack_tlas gives a pair record to every node with left_right != 0, in
//      node order: node 0 gets slot 0 and node i > n slot i - n -- n records for n >= 2, none for n == 1 (the root is INST | 0).  tlasPairs,
//      tlasBase, the root link, tlasLds and stackRows follow from n alone: the host sets them without reading anything back.
//   2. pack_reach's per-instance part (rt_layout.h instance_reach) depends only on the instance's inv_transform and the object box of its
//      BLAS: it runs on the host, in f64, for the changed instances; the device receives {lo[3], hi[3], a, b} per instance and originMax.
//   3. The rest is tree-shaped: nodeReach bottom-up (f64 min / max unions in pack_reach's operand order, a and b by max; ascending node
//      order is a bottom-up order by fact 1), the records with m = a + b * originMax, the clamp at +-1e30, the conversion to f32 and one
//      step outwards -- rt_layout.h pack_reach statement by statement.  min, max and comparisons are exact in any order; the one product
//      and the sums round once each (the library is compiled with -ffp-contract=off, and the two-operation m is spelled with the
//      round-to-nearest intrinsics so that no flag can fuse it).
//
// n <= 256 (RT_TLAS_MAX): one workgroup of 256 lanes.  Plain HIP C++ only.
#pragma once
#include "rt_build.h"

namespace rtd {

struct InstReach { double lo[3], hi[3], a, b; }; // pack_reach's Reach: 8 doubles per instance, as the host uploads them

// std::nextafterf(x, -INFINITY) / (x, +INFINITY) for a finite x (here |x| <= 1e30): the neighbouring float, by the bits
__device__ __forceinline__ float next_down(float x)
{
	uint u = __float_as_uint(x);
	if ((u & 0x7FFFFFFFu) == 0) return __uint_as_float(0x80000001u); // +-0 -> the smallest negative subnormal
	return __uint_as_float((u & 0x80000000u) ? u + 1 : u - 1);
}
__device__ __forceinline__ float next_up(float x)
{
	uint u = __float_as_uint(x);
	if ((u & 0x7FFFFFFFu) == 0) return __uint_as_float(0x00000001u);
	return __uint_as_float((u & 0x80000000u) ? u - 1 : u + 1);
}

// bounds6 == NULL: the world box of a FRESH instance -- bvhInstance(blas) followed by one SetTransform (bvhInstance.cpp:37-44): the BLAS's
// local box (bvh::bounds, bvh.cpp:48-49) grown by its 8 corners under TransformPosition, corner i taking max.x / max.y / max.z with bits
// 0 / 1 / 2.  A lane per changed instance; xform: 12 floats (rows 0-2 of the transform) per changed instance, in the order of the change.
// Changed instance k is instance which[k] (which == nullptr: instance k, a contiguous run whose first instance blasOf and bounds6Out point
// at; rt_set_triangles names the instances of one BLAS, which need not be contiguous); blasOf: its BLAS.
__global__ void __launch_bounds__(RT_TLAS_MAX) k_instance_bounds(const float* xform, const int* blasOf, const float* blasBox6, int count, float* bounds6Out, const int* which)
{
	const int k = (int)threadIdx.x;
	if (k >= count) return;
	const int at = which ? which[k] : k;
	const float* bb = blasBox6 + 6 * blasOf[at];
	const f3 lo(bb[0], bb[1], bb[2]), hi(bb[3], bb[4], bb[5]);
	float mn[3] = { lo.x, lo.y, lo.z }, mx[3] = { hi.x, hi.y, hi.z };
	for (int i = 0; i < 8; i++) {
		const f3 p = xform_pos(xform + 12 * k, f3(i & 1 ? hi.x : lo.x, i & 2 ? hi.y : lo.y, i & 4 ? hi.z : lo.z));
		// aabb::grow(float3): bmin = fminf(bmin, p), bmax = fmaxf(bmax, p) (template/precomp.h:479-480 ternaries)
		mn[0] = t_fminf(mn[0], p.x), mn[1] = t_fminf(mn[1], p.y), mn[2] = t_fminf(mn[2], p.z);
		mx[0] = t_fmaxf(mx[0], p.x), mx[1] = t_fmaxf(mx[1], p.y), mx[2] = t_fmaxf(mx[2], p.z);
	}
	for (int a = 0; a < 3; a++) bounds6Out[6 * at + a] = mn[a], bounds6Out[6 * at + 3 + a] = mx[a];
}

// The commit: pair records, reach records, the context's TLAS and bounds copies, from the scratch nodes of a build that succeeded.
//   node       the 2 n nodes k_build_tlas left in scratch (fact 1's numbering)
//   in         per instance, instance_reach's result
//   pairsTlas  pairs[] from record tlasBase on; reach: reach[]; both have had room for n records (+ 16 spare words) since upload
//   nodeKeep   the context's copy of the TLAS (2 n + 1 nodes of room), for rt_download_tlas;  boundsKeep <- boundsNew: every instance's box
__global__ void __launch_bounds__(RT_TLAS_MAX) k_pack_tlas(const TlasNodeDev* node, int n, const InstReach* in, double originMax, uint tlasBase,
                                                           float4* pairsTlas, float* reach, TlasNodeDev* nodeKeep, const float* boundsNew, float* boundsKeep)
{
	__shared__ double nodeReach[2 * RT_TLAS_MAX][8]; // [node][lo.xyz hi.xyz a b]
	const int tid = (int)threadIdx.x;
	const int nT = 2 * n;
	// nodeReach, bottom-up.  Component c of a node depends on component c of its children alone (lo: min, hi / a / b: max), so lane c < 8
	// walks the whole tree for its component and reads nothing another lane wrote.
	if (tid < 8) {
		const bool isMin = tid < 3;
		for (int i = 1; i <= n; i++) { // leaves: nodeReach[i] = instReach[nd.blas]
			const InstReach& r = in[node[i].blas];
			nodeReach[i][tid] = tid < 3 ? r.lo[tid] : (tid < 6 ? r.hi[tid - 3] : (tid == 6 ? r.a : r.b));
		}
		for (int i = n + 1; i <= nT; i++) { // inner nodes in ascending order, then node 0 (i == nT stands for it)
			const int at = i == nT ? 0 : i;
			const uint lr = node[at].leftRight;
			if (lr == 0) { nodeReach[0][tid] = nodeReach[1][tid]; continue; } // n == 1: the root is the one leaf
			const double r = nodeReach[lr & 0xFFFFu][tid], o = nodeReach[lr >> 16][tid];
			nodeReach[at][tid] = isMin ? (o < r ? o : r) : (r < o ? o : r); // std::min(r, o) / std::max(r, o)
		}
	}
	__syncthreads();
	const int slots = n >= 2 ? n : 0;
	if (tid < slots) {
		const int at = tid == 0 ? 0 : n + tid; // the node of slot tid
		const uint lr = node[at].leftRight;
		const uint ch[2] = { lr & 0xFFFFu, lr >> 16 }; // slot A = leftRight & 0xFFFF: the child tlas::Intersect tests first
		const double big = 1e30;
		for (int s = 0; s < 2; s++) {
			const TlasNodeDev cn = node[ch[s]];
			const uint lk = cn.leftRight == 0 ? (RT_INST_BIT | cn.blas) : tlasBase + (ch[s] - (uint)n); // a child is never node 0
			pairsTlas[4 * tid + 2 * s] = make_float4(cn.lo[0], cn.lo[1], cn.lo[2], __uint_as_float(lk));
			pairsTlas[4 * tid + 2 * s + 1] = make_float4(cn.hi[0], cn.hi[1], cn.hi[2], 0.0f);
			const double* r = nodeReach[ch[s]];
			const double m = __dadd_rn(r[6], __dmul_rn(r[7], originMax)); // m = r.a + r.b * originMax
			float* rec = reach + 12 * tid + 6 * s; // {min.xyz, max.xyz} of child s
			for (int k = 0; k < 3; k++) {
				const double lo = __dsub_rn(r[k], m), hi = __dadd_rn(r[3 + k], m);
				rec[k] = next_down(__double2float_rn(lo < -big ? -big : lo));     // std::max(r.lo[k] - m, -big)
				rec[3 + k] = next_up(__double2float_rn(big < hi ? big : hi)); // std::min(r.hi[k] + m, big)
			}
		}
	}
	if (tid < 16) reach[12 * slots + tid] = 0.0f; // the spare words behind the records
	for (int i = tid; i <= nT; i += RT_TLAS_MAX) nodeKeep[i] = node[i];
	for (int i = tid; i < 6 * n; i += RT_TLAS_MAX) boundsKeep[i] = boundsNew[i];
}

} // namespace rtd
