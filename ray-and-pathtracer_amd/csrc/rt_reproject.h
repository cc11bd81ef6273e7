// Reprojection of the accumulator and the per-pixel statistics across a camera move (rt_reproject), across instance motion as well
// (rt_reproject_motion) and across mesh deformation on top of both (rt_reproject_deform): every pixel of the new frame either takes the samples of the history pixel that saw the same surface point, or
// starts empty.  Defined in include/rt_amd.h (rt_reproject, rt_reproject_motion) and restated in numpy in tests/reproject_ref.py and
// tests/reproject_motion_ref.py; they follow each other operation by operation (f32, IEEE division, no contraction: the library is built
// with -ffp-contract=off).
//   k_reproject  a backward gather, one lane per pixel of the NEW frame, 32 x 8 tiles like the a-trous filters: the new G-buffer's point is
//                projected through the HISTORY camera's pinhole onto its nearest pixel q, and q is accepted when it saw the same object and
//                material under the same normal and the point lies on q's tangent plane.  Neighbouring pixels land on neighbouring history
//                pixels, so a tile's gathers share lines.  The history's count, position, normal and material (40 B) are read first, its
//                accumulator and sums (24 B) only by a lane that passed; 28 B are written per pixel, carried or zero.  The carried pixels are
//                counted by a ballot per wave and one atomic add per wave that carried any (no LDS).
//   k_reproject_motion  the same gather with the other half of a motion vector in front: a pixel whose hit belongs to an instance that has
//                moved since the capture takes its point and normal back to where the capture saw them -- through the instance's CURRENT
//                inverse, then the CAPTURE's transform -- before the projection, and q must have seen the same instance.  Which instances
//                moved is decided on the host (a bitwise compare of two mirrors) and travels as 256 bits of kernel arguments, so an unmoved
//                pixel costs two more 4-byte loads (its index, the history's at q) and no arithmetic.  A moved one reads 24 floats: rows
//                0..2 of two 128-byte instance records, as six 16-byte global loads.  A 32 x 8 tile nearly always sees one or two
//                instances, so a wave's lanes ask for the same one or two records and the loads are served as broadcasts from one or two
//                cache lines each; staging the table in LDS (24 KB for 256 records, a barrier, and occupancy) would cost every block more
//                than those lines cost the few waves that need them.
//   k_reproject_deform  the motion gather with a third way back in front: a pixel whose hit is a triangle that has been rewritten since the
//                capture (rt_set_triangles, rt_set_time) takes its barycentric coordinates in the CURRENT triangle to the triangle the
//                capture saw, whose records the first rewrite copied aside (rt_ctx.h History).  Every lane pays one more 4-byte load (its
//                leaf slot) and, on a hit, the per-BLAS table lookup (8 bytes, one or two distinct entries per tile); a lane on a BLAS
//                with a kept copy reads 48 bytes of each of the two records as 16-byte loads and compares 12 words, and only a lane
//                whose words differ runs the ~60 flops.  A tile's lanes mostly share one or two triangles, so these loads are broadcasts
//                of a few lines like the instance records above, and for the same reason nothing is staged in LDS: the records a tile needs
//                are known only per lane, after the G-buffer load, and there are as many distinct ones as the tile sees triangles.
#pragma once
#include "rt_denoise.h" // the tile, dist2
#include "rt_kernels.h" // PixelStats, DMaterial, DInstance
#include "rt_build.h"   // RT_TLAS_MAX
#include "../../include/rt_amd.h" // RT_MAT_DIFFUSE

namespace rtd {

struct ReprojectArgs {
	const float4* nrm; const float4* pos; const float4* alb;    // the current G-buffer
	const float4* hNrm; const float4* hPos; const float4* hAlb; // the history's
	const float4* hAcc; PixelStats hSt;                         // the history's accumulator and statistics
	float4* acc; PixelStats St;                                 // what is rewritten
	const DMaterial* mats; int nMats;
	float cam[3], TL[3], TR[3], BL[3];                          // the history camera
	int width, height;
	float normalTol2, planeTol;                                 // normal_tolerance * normal_tolerance (f32), plane_tolerance
	int maxHistory, carryViewDependent;
	int* nCarried;
};

// what k_reproject_motion reads beyond that
struct ReprojectMotionArgs : ReprojectArgs {
	const int* inst; const int* hInst;           // the hit's instance per pixel (-1: none): the current G-buffer's, the history's
	const DInstance* cur; const DInstance* hXf;  // the instance records: the scene's (invT_k is read from here), the capture's (T'_k)
	uint moved[RT_TLAS_MAX / 32];                // bit k: one of instance k's 24 words (T and invT, rows 0..2) differs from the capture's
};

// ... and k_reproject_deform beyond that
struct ReprojectDeformArgs : ReprojectMotionArgs {
	const int* prim;             // the hit's leaf slot per pixel (-1: none): the current G-buffer's
	const float4* prims;         // the scene's primitive records, 4 float4 per slot
	const long long* keptDelta;  // per BLAS: the distance in bytes from a current record to the capture's kept copy of it, 0: none kept
	const int* blasOf;           // under a TLAS: the BLAS of instance k
	int useTLAS, blas0Slots;     // without a TLAS the BLAS of a slot below blas0Slots is 0
};

__device__ __forceinline__ float rp_dot(const f3& a, const f3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 rp_cross(const f3& a, const f3& b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// bit k of the 256 (k < 0: not an instance's hit).  The words are kernel arguments, i.e. scalar registers: a select chain, not an indexed
// array (which would be copied to scratch first)
__device__ __forceinline__ bool instance_moved(const ReprojectMotionArgs& R, int k)
{
	if (k < 0) return false;
	uint w = R.moved[0];
#pragma unroll
	for (int j = 1; j < RT_TLAS_MAX / 32; j++) w = (k >> 5) == j ? R.moved[j] : w;
	return ((w >> (k & 31)) & 1u) != 0;
}
__device__ __forceinline__ void load_rows(const float* rec, float* out12) // rows 0..2 of a matrix of a DInstance: 48 bytes, 16-byte aligned
{
	const float4* r = (const float4*)rec;
	const float4 a = r[0], b = r[1], c = r[2];
	out12[0] = a.x, out12[1] = a.y, out12[2] = a.z, out12[3] = a.w, out12[4] = b.x, out12[5] = b.y, out12[6] = b.z, out12[7] = b.w;
	out12[8] = c.x, out12[9] = c.y, out12[10] = c.z, out12[11] = c.w;
}

__device__ __forceinline__ bool same_bits(const float4& a, const float4& b)
{
	return ((__float_as_int(a.x) ^ __float_as_int(b.x)) | (__float_as_int(a.y) ^ __float_as_int(b.y)) | (__float_as_int(a.z) ^ __float_as_int(b.z)) |
	        (__float_as_int(a.w) ^ __float_as_int(b.w))) == 0;
}

enum { RP_CAMERA = 0, RP_MOTION = 1, RP_DEFORM = 2 };

// include/rt_amd.h rt_reproject (RP_MOTION: rt_reproject_motion, RP_DEFORM: rt_reproject_deform), line by line: the history pixel that pixel
// p (records np, xp, material mat) takes its samples from, or -1; count is that pixel's sample count (read once: the first thing the gather
// needs and the last thing it copies)
template <int MODE, typename Args>
__device__ __forceinline__ int reproject_source(const Args& R, int p, const float4& np, const float4& xp, int mat, uint& count)
{
	constexpr bool MOTION = MODE >= RP_MOTION;
	if (__float_as_int(xp.w) == -1) return -1;
	if (!R.carryViewDependent) {
		if (mat < 0 || mat >= R.nMats) return -1;
		if (R.mats[mat].type != RT_MAT_DIFFUSE || !(R.mats[mat].shinieness == 0.0f)) return -1;
	}
	float4 nm = np, xm = xp; // the point and its normal as the capture saw them (w: t_p and the object, untouched)
	int k = -1;
	if constexpr (MOTION) {
		k = R.inst[p];
		bool deformed = false;
		if constexpr (MODE == RP_DEFORM) {
			const int s = R.prim[p];
			long long delta = 0; // to the capture's copy of record s; 0: its BLAS has none
			if (s >= 0) {
				if (R.useTLAS) { if (k >= 0) delta = R.keptDelta[R.blasOf[k]]; }
				else if (s < R.blas0Slots) delta = R.keptDelta[0];
			}
			if (delta != 0) {
				// {v0, N.x} {v1, N.y} {v2, N.z} of both records, as named vectors (an indexed array would go to scratch)
				const float4* cur = R.prims + 4 * (size_t)s;
				const float4* old = (const float4*)((const char*)cur + delta);
				const float4 c0 = cur[0], c1 = cur[1], c2 = cur[2], o0 = old[0], o1 = old[1], o2 = old[2];
				if (!(same_bits(c0, o0) && same_bits(c1, o1) && same_bits(c2, o2)) && (__float_as_int(cur[3].w) & 3) == RT_KIND_TRI) {
					deformed = true;
					f3 xo = xyz(xp);
					if (k >= 0) { float invT[12]; load_rows(R.cur[k].invT, invT); xo = xform_pos(invT, xo); }
					const f3 v0 = xyz(c0), e1 = xyz(c1) - v0, e2 = xyz(c2) - v0, w = xo - v0;
					const float d11 = rp_dot(e1, e1), d12 = rp_dot(e1, e2), d22 = rp_dot(e2, e2), w1 = rp_dot(w, e1), w2 = rp_dot(w, e2);
					const float den = d11 * d22 - d12 * d12;
					const float bu = (d22 * w1 - d12 * w2) / den, bv = (d11 * w2 - d12 * w1) / den;
					const f3 h0 = xyz(o0), h1 = xyz(o1) - h0, h2 = xyz(o2) - h0;
					f3 x((h0.x + bu * h1.x) + bv * h2.x, (h0.y + bu * h1.y) + bv * h2.y, (h0.z + bu * h1.z) + bv * h2.z);
					f3 n(o0.w, o1.w, o2.w);
					if (k >= 0) { float Tc[12]; load_rows(R.hXf[k].T, Tc); x = xform_pos(Tc, x), n = normalize(xform_vec(Tc, n)); }
					xm = mk4(x, xp.w), nm = mk4(n, np.w);
				}
			}
		}
		if (!deformed && instance_moved(R, k)) { // (k < nInst: a G-buffer's index names an instance of the scene both tables describe)
			float invT[12], Tc[12];
			load_rows(R.cur[k].invT, invT), load_rows(R.hXf[k].T, Tc);
			const f3 x = xform_pos(Tc, xform_pos(invT, xyz(xp)));
			const f3 n = normalize(xform_vec(Tc, xform_vec(invT, xyz(np))));
			xm = mk4(x, xp.w), nm = mk4(n, np.w);
		}
	}
	const float4 &nh = MOTION ? nm : np, &xh = MOTION ? xm : xp;
	const f3 cam(R.cam[0], R.cam[1], R.cam[2]), TL(R.TL[0], R.TL[1], R.TL[2]), TR(R.TR[0], R.TR[1], R.TR[2]), BL(R.BL[0], R.BL[1], R.BL[2]);
	const f3 A = TR - TL, B = BL - TL, N = rp_cross(A, B), E = TL - cam, x(xh.x, xh.y, xh.z), d = x - cam;
	const float lam = rp_dot(E, N) / rp_dot(d, N);
	if (!isfinite(lam) || !(lam > 0.0f)) return -1;
	const f3 Q(lam * d.x - E.x, lam * d.y - E.y, lam * d.z - E.z);
	const float nn = rp_dot(N, N);
	const float u = rp_dot(rp_cross(Q, B), N) / nn, v = rp_dot(rp_cross(A, Q), N) / nn;
	const float rx = floorf(u * (float)R.width + 0.5f), ry = floorf(v * (float)R.height + 0.5f);
	if (!(rx >= 0.0f && rx < (float)R.width && ry >= 0.0f && ry < (float)R.height)) return -1; // (NaN fails)
	const int q = (int)ry * R.width + (int)rx; // inside the history's frame: 0 <= rx < width, 0 <= ry < height
	count = R.hSt.count[q];
	if (count == 0) return -1;
	const float4 xq = R.hPos[q];
	if (__float_as_int(xq.w) != __float_as_int(xp.w)) return -1;
	if (__float_as_int(R.hAlb[q].w) != mat) return -1;
	if constexpr (MOTION) {
		if (R.hInst[q] != k) return -1;
	}
	const float4 nq = R.hNrm[q];
	if (!(dist2(nh, nq) <= R.normalTol2)) return -1;
	const f3 off(xh.x - xq.x, xh.y - xq.y, xh.z - xq.z);
	if (!(fabsf(rp_dot(f3(nq.x, nq.y, nq.z), off)) <= R.planeTol * np.w)) return -1;
	return q;
}

// one lane's pixel: the gather, the max_history rescale, the 28 bytes written, the ballot count
template <int MODE, typename Args>
__device__ __forceinline__ void reproject_pixel(const Args& R)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	const bool inside = x < R.width && y < R.height; // (no lane leaves before the ballot)
	const int p = y * R.width + x;
	int q = -1;
	uint count = 0;
	if (inside) q = reproject_source<MODE>(R, p, R.nrm[p], R.pos[p], __float_as_int(R.alb[p].w), count);
	if (inside) {
		float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (q < 0) count = 0;
		float sy = 0.0f, syy = 0.0f;
		if (q >= 0) {
			a = R.hAcc[q], sy = R.hSt.sumY[q], syy = R.hSt.sumYY[q];
			if (R.maxHistory > 0 && count > (uint)R.maxHistory) {
				const float f = (float)R.maxHistory / (float)count;
				a = make_float4(a.x * f, a.y * f, a.z * f, a.w * f);
				sy = sy * f, syy = syy * f;
				count = (uint)R.maxHistory;
			}
		}
		R.acc[p] = a;
		R.St.count[p] = count, R.St.sumY[p] = sy, R.St.sumYY[p] = syy;
	}
	const unsigned long long carried = __ballot(q >= 0);
	const uint lane = (threadIdx.y * RT_DENOISE_TX + threadIdx.x) & 63u;
	if (lane == 0 && carried != 0) atomicAdd(R.nCarried, (int)__popcll(carried));
}

__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_reproject(ReprojectArgs R) { reproject_pixel<RP_CAMERA>(R); }
__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_reproject_motion(ReprojectMotionArgs R) { reproject_pixel<RP_MOTION>(R); }
__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_reproject_deform(ReprojectDeformArgs R) { reproject_pixel<RP_DEFORM>(R); }

} // namespace rtd
