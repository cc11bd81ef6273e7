// Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over the accumulator's mean, guided by the G-buffer of
// k_primary_aovs.  One launch per iteration i (step s = 2^i), 256-lane blocks as 32 x 8 pixel tiles, one pixel per lane: a tile's 25 taps
// of a given offset are 25 shifted copies of the tile, so neighbouring lanes read neighbouring 16-byte records and the taps of one
// iteration share L1 lines (direct loads, no LDS: at s >= 8 a tile's taps hardly overlap anyway).
// The filter is defined in include/rt_amd.h (rt_denoise) and restated in numpy in tests/denoise_ref.py; the two follow each other term by
// term:
//   c_p = accum_p.xyz / it on the first iteration (k_resolve's f32 division), the previous iteration's output after that
//   a non-finite c_p is passed through and is no tap of any neighbour
//   w = h[dx] h[dy] exp(-(|c_p - c_q|^2 kc + |n_p - n_q|^2 kn + |x_p - x_q|^2 / t_p^2 kx + |a_p - a_q|^2 ka)), a zero k drops its term
//   (sigma = inf), an overflowing k is FLT_MAX (kc, kn, kx, ka on the host, kx / t_p^2 here), two misses compare colour only, a hit and a miss do not mix (w = 0); out = sum w c_q / sum w, w channel 0
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace rtd {

#define RT_DENOISE_TX 32
#define RT_DENOISE_TY 8

struct DenoiseArgs {
	const float4* in;   // colour: the accumulator (FIRST) or the previous iteration's output
	const float4* nrm;  // normal xyz, w = t
	const float4* pos;  // position xyz, w = objIdx bits (-1: a miss)
	const float4* alb;  // albedo rgb, w = material bits
	float4* out;
	int width, height, step;
	float it;           // the accumulator's frame count (FIRST only)
	float kc, kn, kx, ka;
};

__device__ __forceinline__ bool finite4(const float4& c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }
__device__ __forceinline__ float dist2(const float4& a, const float4& b)
{
	const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
	return dx * dx + dy * dy + dz * dz;
}

template <bool FIRST>
__device__ __forceinline__ float4 denoise_color(const DenoiseArgs& A, int i)
{
	float4 c = A.in[i];
	if (FIRST) c = make_float4(c.x / A.it, c.y / A.it, c.z / A.it, 0.0f);
	return c;
}

template <bool FIRST>
__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_denoise_atrous(DenoiseArgs A)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	if (x >= A.width || y >= A.height) return;
	const int p = y * A.width + x;
	const float4 cp = denoise_color<FIRST>(A, p);
	if (!finite4(cp)) { A.out[p] = make_float4(cp.x, cp.y, cp.z, 0.0f); return; }
	const float4 xp = A.pos[p], np = A.nrm[p], ap = A.alb[p];
	const bool hitP = __float_as_int(xp.w) != -1;
	// the position term's scale 1 / t_p^2 is the centre's alone: folded into its k once, clamped like every k (a tiny t_p overflows it)
	const float kxp = A.kx != 0.0f ? fminf(A.kx / (np.w * np.w), FLT_MAX) : 0.0f;
	const float h[5] = { 1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16 };
	float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
	for (int dy = -2; dy <= 2; dy++) {
		const int qy = y + dy * A.step;
		if (qy < 0 || qy >= A.height) continue;
#pragma unroll
		for (int dx = -2; dx <= 2; dx++) {
			const int qx = x + dx * A.step;
			if (qx < 0 || qx >= A.width) continue;
			const int q = qy * A.width + qx;
			const float4 xq = A.pos[q];
			const bool hitQ = __float_as_int(xq.w) != -1;
			if (hitQ != hitP) continue;
			const float4 cq = denoise_color<FIRST>(A, q);
			if (!finite4(cq)) continue;
			float e = A.kc != 0.0f ? dist2(cp, cq) * A.kc : 0.0f;
			if (hitP) {
				const float4 nq = A.nrm[q], aq = A.alb[q];
				if (A.kn != 0.0f) e = e + dist2(np, nq) * A.kn;
				if (kxp != 0.0f) e = e + dist2(xp, xq) * kxp;
				if (A.ka != 0.0f) e = e + dist2(ap, aq) * A.ka;
			}
			const float w = h[dx + 2] * h[dy + 2] * expf(-e);
			sw = sw + w;
			sx = sx + w * cq.x, sy = sy + w * cq.y, sz = sz + w * cq.z;
		}
	}
	A.out[p] = make_float4(sx / sw, sy / sw, sz / sw, 0.0f);
}

} // namespace rtd
