// Variance-guided a-trous filter for an adaptively sampled frame (the spatial half of SVGF: Schied et al. 2017): k_denoise_atrous's
// taps, h and G-buffer terms, with the colour term replaced by a luminance difference scaled by the local standard deviation of the mean
// (a 3 x 3 prefilter of the variance), and the variance filtered along with the colour.  Defined in include/rt_amd.h
// (rt_denoise_variance) and restated in numpy in tests/denoise_var_ref.py; the three follow each other operation by operation.
//   k_denoise_var_init    accumulator + count + sum_y + sum_yy (28 B per pixel) -> one float4 record (c, v) per pixel.  A pixel that is
//                         not filtered and is no tap (count 0: colour 0; a non-finite mean or sum: the mean as it is) has v = -1, a
//                         filtered one v >= 0: the tap loop learns a tap's validity from the 16 bytes it loads anyway.
//   k_denoise_var_atrous  one launch per iteration, 32 x 8 tiles, one pixel per lane, direct 16-byte loads (rt_denoise.h explains why).
//                         The prefilter runs inside the iteration: eight more records and eight more 4-byte hit classes (pos.w) at one
//                         pixel's distance, all in lines the centre's row and its two neighbours already bring in (measured against a
//                         prefilter pass of its own, profiles/patches/denoise_var_prefilter_pass.diff: 1.18 against 1.27 ms at 1080p).
//                         The last iteration writes w = 0 instead of the marker.
#pragma once
#include "rt_denoise.h"
#include "rt_kernels.h" // PixelStats

namespace rtd {

#define RT_DENOISE_VAR_INVALID (-1.0f)

struct DenoiseVarArgs {
	const float4* in;   // (c, v) records: k_denoise_var_init's or the previous iteration's
	const float4* nrm;  // the G-buffer, as DenoiseArgs
	const float4* pos;
	const float4* alb;
	float4* out;
	int width, height, step;
	int last;           // the final iteration: an unfiltered pixel's w is written as 0, not as the marker
	float sl, eps;      // sigma_luminance (+inf: the term is dropped), epsilon
	float kn, kx, ka;
};

// the statistics' luminance: k_accumulate<true>'s own function (rt_kernels.h)
__device__ __forceinline__ float denoise_luminance(const float4& c) { return sample_luminance(c.x, c.y, c.z); }
__device__ __forceinline__ bool denoise_var_valid(const float4& c) { return !(c.w < 0.0f); }

__global__ void __launch_bounds__(256) k_denoise_var_init(const float4* accum, PixelStats St, int nPixels, float4* out)
{
	const int p = blockIdx.x * 256 + threadIdx.x;
	if (p >= nPixels) return;
	const uint count = St.count[p];
	if (count == 0) { out[p] = make_float4(0.0f, 0.0f, 0.0f, RT_DENOISE_VAR_INVALID); return; }
	const float4 a = accum[p];
	const float sumY = St.sumY[p], sumYY = St.sumYY[p];
	const float n = (float)count;
	float4 c = make_float4(a.x / n, a.y / n, a.z / n, RT_DENOISE_VAR_INVALID);
	if (finite4(c) && isfinite(sumY) && isfinite(sumYY)) {
		if (count >= 2) { // rt_select_active's operations, stopping before the square root
			const float m = sumY / n;
			float s = (sumYY - sumY * m) / (n - 1);
			s = s > 0 ? s : 0;
			c.w = s / n;
		} else {
			const float y = denoise_luminance(c);
			c.w = y * y;
		}
		c.w = fminf(c.w, FLT_MAX); // clamped like every k of rt_denoise: a tap of weight 0 then adds 0, not 0 x inf = NaN
	}
	out[p] = c;
}

__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_denoise_var_atrous(DenoiseVarArgs A)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	if (x >= A.width || y >= A.height) return;
	const int p = y * A.width + x;
	const float4 cp = A.in[p];
	if (!denoise_var_valid(cp)) { A.out[p] = make_float4(cp.x, cp.y, cp.z, A.last ? 0.0f : RT_DENOISE_VAR_INVALID); return; }
	const float4 xp = A.pos[p], np = A.nrm[p], ap = A.alb[p];
	const int classP = __float_as_int(xp.w) != -1;
	const bool hitP = classP != 0;
	// the prefilter of the variance: 3 x 3 at ONE pixel's distance, valid taps of p's hit class, normalised by the weights used
	float kl = 0.0f;
	if (A.sl < INFINITY) {
		const float k3[3] = { 0.25f, 0.5f, 0.25f };
		float gw = 0.0f, gv = 0.0f;
#pragma unroll
		for (int dy = -1; dy <= 1; dy++) {
			const int qy = y + dy;
			if (qy < 0 || qy >= A.height) continue;
#pragma unroll
			for (int dx = -1; dx <= 1; dx++) {
				const int qx = x + dx;
				if (qx < 0 || qx >= A.width) continue;
				const int q = qy * A.width + qx;
				float vq = cp.w;
				if (dx != 0 || dy != 0) {
					if ((__float_as_int(A.pos[q].w) != -1) != hitP) continue;
					vq = A.in[q].w;
					if (vq < 0.0f) continue;
				}
				const float k = k3[dx + 1] * k3[dy + 1];
				gw = gw + k;
				gv = gv + k * vq;
			}
		}
		kl = fminf(1.0f / (A.sl * sqrtf(gv / gw) + A.eps), FLT_MAX); // (a tiny epsilon on a zero variance: the centre tap's zero difference must add 0)
	}
	const float yp = denoise_luminance(cp);
	const float kxp = A.kx != 0.0f ? fminf(A.kx / (np.w * np.w), FLT_MAX) : 0.0f;
	const float h[5] = { 1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16 };
	float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
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
			const float4 cq = A.in[q];
			if (!denoise_var_valid(cq)) continue;
			float e = kl != 0.0f ? fabsf(yp - denoise_luminance(cq)) * kl : 0.0f;
			if (hitP) {
				const float4 nq = A.nrm[q], aq = A.alb[q];
				if (A.kn != 0.0f) e = e + dist2(np, nq) * A.kn;
				if (kxp != 0.0f) e = e + dist2(xp, xq) * kxp;
				if (A.ka != 0.0f) e = e + dist2(ap, aq) * A.ka;
			}
			const float w = h[dx + 2] * h[dy + 2] * expf(-e);
			sw = sw + w;
			sx = sx + w * cq.x, sy = sy + w * cq.y, sz = sz + w * cq.z;
			sv = sv + (w * w) * cq.w;
		}
	}
	A.out[p] = make_float4(sx / sw, sy / sw, sz / sw, fminf(sv / (sw * sw), FLT_MAX));
}

} // namespace rtd
