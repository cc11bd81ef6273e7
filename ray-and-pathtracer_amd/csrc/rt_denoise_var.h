// Variance-guided a-trous filter for an adaptively sampled frame (the spatial half of SVGF: Schied et al. 2017): k_denoise_atrous's
// tap loop (atrous_taps of rt_denoise.h: the taps, h, the G-buffer terms), with a luminance difference scaled by the local standard
// deviation of the mean (a 3 x 3 prefilter of the variance) as its colour term, and the variance filtered along with the colour.  Defined in include/rt_amd.h
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

struct DenoiseVarArgs : AtrousArgs { // in: (c, v) records, k_denoise_var_init's or the previous iteration's
	int last;           // the final iteration: an unfiltered pixel's w is written as 0, not as the marker
	float sl, eps;      // sigma_luminance (+inf: the term is dropped), epsilon
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

// the prefilter of the variance, as the luminance term's k: 3 x 3 at ONE pixel's distance, valid taps of p's hit class, normalised by the weights used
__device__ __forceinline__ float denoise_var_kl(const DenoiseVarArgs& A, int x, int y, const float4& cp, bool hitP)
{
	if (!(A.sl < INFINITY)) return 0.0f;
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
	return fminf(1.0f / (A.sl * sqrtf(gv / gw) + A.eps), FLT_MAX); // (a tiny epsilon on a zero variance: the centre tap's zero difference must add 0)
}
// rt_denoise_variance's colour term: |y_p - y_q| kl over the records init marked valid, and the variance filtered along: sum w^2 v_q
struct LuminanceTerm {
	const float4* in; float yp, kl;
	float sv;
	__device__ __forceinline__ float4 load(int q) const { return in[q]; }
	__device__ __forceinline__ bool valid(const float4& c) const { return denoise_var_valid(c); }
	__device__ __forceinline__ float distance(const float4& cq) const { return kl != 0.0f ? fabsf(yp - denoise_luminance(cq)) * kl : 0.0f; }
	__device__ __forceinline__ void add(float w, const float4& cq) { sv = sv + (w * w) * cq.w; }
};

__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_denoise_var_atrous(DenoiseVarArgs A)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	if (x >= A.width || y >= A.height) return;
	const int p = y * A.width + x;
	const float4 cp = A.in[p];
	if (!denoise_var_valid(cp)) { A.out[p] = make_float4(cp.x, cp.y, cp.z, A.last ? 0.0f : RT_DENOISE_VAR_INVALID); return; }
	const float4 xp = A.pos[p], np = A.nrm[p], ap = A.alb[p];
	const float kl = denoise_var_kl(A, x, y, cp, __float_as_int(xp.w) != -1);
	LuminanceTerm T{ A.in, denoise_luminance(cp), kl, 0.0f };
	const float4 s = atrous_taps(A, x, y, xp, np, ap, T);
	A.out[p] = make_float4(s.x / s.w, s.y / s.w, s.z / s.w, fminf(T.sv / (s.w * s.w), FLT_MAX));
}

} // namespace rtd
