// rt_set_vertices on the device: the front end rt_set_triangles has on the host.  An indexed mesh arrives as its vertex array alone; one
// launch assembles the rt_triangle records the unchanged k_set_triangles (rt_triangles.h) then reads, and reduces what the host's loop over
// the records used to find: the boxes and flags the call's checks, blas_object_box (rt_layout.h) and instance_reach are fed from.
//
//   1. Assemble.  Triangle p's corners are xyz[idx[3p]], xyz[idx[3p + 1]], xyz[idx[3p + 2]]; its normal is Triangle::update's
//      (template/scene.h:238-246) through the same normalize(cross(...)) k_animate uses; obj_idx and material are the ones the record at
//      slotOf[p] holds.  The 14 words go to the staging array in rt_triangle's order: from there on the call IS rt_set_triangles, and the
//      bytes it leaves are that call's by construction.
//   2. Reduce.  Per axis min and max over every corner (the magnitude box of the 1e29 / 1e30 checks and of blasBox6), the same over the
//      hittable triangles only (blas_object_box skips a triangle whose N is all zero or holds a NaN), whether blas_object_box's strict
//      < 1e29 test failed on one of those, and the lowest index of a triangle with a coordinate that is not <= 1e29.  Floats travel in an
//      order-preserving integer encoding (float_key), so that min and max are integer atomics and the result does not depend on arrival
//      order.  Among equal values only +0 and -0 differ in their keys: the record's zeros may carry another sign than the host loop's,
//      which no stored byte depends on ("Deforming from vertices").
//
// Plain HIP C++ only.
#pragma once
#include "rt_kernels.h"

namespace rtd {

// The record the host reads back, 56 bytes.  word[k]: 0-2 min and 3-5 max of every corner, 6-8 min and 9-11 max of the hittable triangles'
// corners (all as float_key), 12 nonzero: a hittable triangle has a coordinate that is not < 1e29, 13 the first triangle with a coordinate
// that is not <= 1e29 (0xFFFFFFFF: none).  Words 0-2, 6-8 and 13 are reduced by min, the others by max.
struct VertexVerdict { uint word[14]; };
#define RT_VERDICT_WORDS 14

// u32 keys in the order of the floats they stand for (-inf < ... < -0 < +0 < ... < +inf)
__host__ __device__ __forceinline__ uint float_key(float f)
{
	union { float f; uint u; } v;
	v.f = f;
	return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
__host__ __device__ __forceinline__ float key_float(uint k)
{
	union { float f; uint u; } v;
	v.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
	return v.f;
}
__host__ __device__ __forceinline__ bool verdict_takes_min(int k) { return k < 3 || (k >= 6 && k < 9) || k == 13; }

// A lane per triangle, 256-thread blocks.  idx: 3 nTri indices, every one below the length of xyz (checked on the host when they were
// bound); xyz: the vertices, three floats each; slotOf / prims: as k_set_triangles takes them (read only); stage: room for nTri 14-word
// records; out: the record, initialised by the host to the empty boxes.  Every lane stays to the end: the block reduces together.
__global__ void __launch_bounds__(256) k_assemble_triangles(const uint* __restrict__ idx, const float* __restrict__ xyz, int nTri, const uint* __restrict__ slotOf,
                                                            const float4* __restrict__ prims, float2* __restrict__ stage, VertexVerdict* out)
{
	const int p = blockIdx.x * 256 + threadIdx.x;
	uint w[RT_VERDICT_WORDS]; // (every loop over it unrolls: registers)
#pragma unroll
	for (int k = 0; k < RT_VERDICT_WORDS; k++) w[k] = verdict_takes_min(k) ? 0xFFFFFFFFu : 0u;
	if (p < nTri) {
		const uint* ip = idx + 3 * (size_t)p; // 12 contiguous bytes per lane
		const uint i0 = ip[0], i1 = ip[1], i2 = ip[2];
		const float* a = xyz + 3 * (size_t)i0;
		const float* b = xyz + 3 * (size_t)i1;
		const float* c = xyz + 3 * (size_t)i2;
		const f3 v0(a[0], a[1], a[2]), v1(b[0], b[1], b[2]), v2(c[0], c[1], c[2]);
		const f3 N = normalize(cross(v1 - v0, v2 - v0));
		float obj = 0.0f, mat = 0.0f; // (bit patterns of two ints; a primitive without a slot writes no record)
		const uint slot = slotOf[p];
		if (slot != 0xFFFFFFFFu) { const float4 r3 = prims[4 * (size_t)slot + 3]; obj = r3.y, mat = r3.z; }
		float2* t = stage + 7 * (size_t)p;
		t[0] = make_float2(v0.x, v0.y), t[1] = make_float2(v0.z, v1.x), t[2] = make_float2(v1.y, v1.z), t[3] = make_float2(v2.x, v2.y);
		t[4] = make_float2(v2.z, N.x), t[5] = make_float2(N.y, N.z), t[6] = make_float2(obj, mat);
		const float v[9] = { v0.x, v0.y, v0.z, v1.x, v1.y, v1.z, v2.x, v2.y, v2.z };
		const bool hittable = !((N.x == 0 && N.y == 0 && N.z == 0) || N.x != N.x || N.y != N.y || N.z != N.z);
#pragma unroll
		for (int j = 0; j < 9; j++) {
			const uint key = float_key(v[j]);
			const float m = fabsf(v[j]);
			if (!(m <= 1e29f)) w[13] = (uint)p;
			w[j % 3] = min(w[j % 3], key), w[3 + j % 3] = max(w[3 + j % 3], key);
			if (hittable) {
				w[6 + j % 3] = min(w[6 + j % 3], key), w[9 + j % 3] = max(w[9 + j % 3], key);
				if (!(m < 1e29f)) w[12] = 1u;
			}
		}
	}
	// the wave by shuffles, the block's four waves through LDS, then one atomic per word and block
#pragma unroll
	for (int off = 32; off > 0; off >>= 1)
#pragma unroll
		for (int k = 0; k < RT_VERDICT_WORDS; k++) {
			const uint o = (uint)__shfl_xor((int)w[k], off, 64);
			w[k] = verdict_takes_min(k) ? min(w[k], o) : max(w[k], o);
		}
	__shared__ uint part[4][RT_VERDICT_WORDS];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0)
		for (int k = 0; k < RT_VERDICT_WORDS; k++) part[wave][k] = w[k];
	__syncthreads();
	if (threadIdx.x < RT_VERDICT_WORDS) {
		const int k = threadIdx.x;
		const bool mn = verdict_takes_min(k);
		uint r = part[0][k];
		for (int q = 1; q < 4; q++) r = mn ? min(r, part[q][k]) : max(r, part[q][k]);
		if (mn) atomicMin(&out->word[k], r);
		else atomicMax(&out->word[k], r);
	}
}

} // namespace rtd
