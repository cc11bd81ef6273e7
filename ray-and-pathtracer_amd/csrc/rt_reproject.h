// Reprojection of the accumulator and the per-pixel statistics across a camera move (rt_reproject): every pixel of the new frame either
// takes the samples of the history pixel that saw the same surface point, or starts empty.  Defined in include/rt_amd.h (rt_reproject)
// and restated in numpy in tests/reproject_ref.py; the two follow each other operation by operation (f32, IEEE division, no contraction:
// the library is built with -ffp-contract=off).
//   k_reproject  a backward gather, one lane per pixel of the NEW frame, 32 x 8 tiles like the a-trous filters: the new G-buffer's point is
//                projected through the HISTORY camera's pinhole onto its nearest pixel q, and q is accepted when it saw the same object and
//                material under the same normal and the point lies on q's tangent plane.  Neighbouring pixels land on neighbouring history
//                pixels, so a tile's gathers share lines.  The history's count, position, normal and material (40 B) are read first, its
//                accumulator and sums (24 B) only by a lane that passed; 28 B are written per pixel, carried or zero.  The carried pixels are
//                counted by a ballot per wave and one atomic add per wave that carried any (no LDS).
#pragma once
#include "rt_denoise.h" // the tile, dist2
#include "rt_kernels.h" // PixelStats, DMaterial
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

__device__ __forceinline__ float rp_dot(const f3& a, const f3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 rp_cross(const f3& a, const f3& b) { return f3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// include/rt_amd.h rt_reproject, line by line: the history pixel that pixel p (records np, xp, material mat) takes its samples from, or -1;
// count is that pixel's sample count (read once: the first thing the gather needs and the last thing it copies)
__device__ __forceinline__ int reproject_source(const ReprojectArgs& R, const float4& np, const float4& xp, int mat, uint& count)
{
	if (__float_as_int(xp.w) == -1) return -1;
	if (!R.carryViewDependent) {
		if (mat < 0 || mat >= R.nMats) return -1;
		if (R.mats[mat].type != RT_MAT_DIFFUSE || !(R.mats[mat].shinieness == 0.0f)) return -1;
	}
	const f3 cam(R.cam[0], R.cam[1], R.cam[2]), TL(R.TL[0], R.TL[1], R.TL[2]), TR(R.TR[0], R.TR[1], R.TR[2]), BL(R.BL[0], R.BL[1], R.BL[2]);
	const f3 A = TR - TL, B = BL - TL, N = rp_cross(A, B), E = TL - cam, x(xp.x, xp.y, xp.z), d = x - cam;
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
	const float4 nq = R.hNrm[q];
	if (!(dist2(np, nq) <= R.normalTol2)) return -1;
	const f3 off(xp.x - xq.x, xp.y - xq.y, xp.z - xq.z);
	if (!(fabsf(rp_dot(f3(nq.x, nq.y, nq.z), off)) <= R.planeTol * np.w)) return -1;
	return q;
}

__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_reproject(ReprojectArgs R)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	const bool inside = x < R.width && y < R.height; // (no lane leaves before the ballot)
	const int p = y * R.width + x;
	int q = -1;
	uint count = 0;
	if (inside) q = reproject_source(R, R.nrm[p], R.pos[p], __float_as_int(R.alb[p].w), count);
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

} // namespace rtd
