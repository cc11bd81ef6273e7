// Edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010) over the accumulator's mean, guided by the G-buffer of
// k_primary_aovs.  One launch per iteration i (step s = 2^i), 256-lane blocks as 32 x 8 pixel tiles, one pixel per lane: a tile's 25 taps
// of a given offset are 25 shifted copies of the tile, so neighbouring lanes read neighbouring 16-byte records and the taps of one
// iteration share L1 lines (direct loads, no LDS: at s >= 8 a tile's taps hardly overlap anyway).
// The tap loop (atrous_taps) is written once, for this filter and rt_denoise_var.h's: a filter is its centre set-up and a colour term object.
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

// what both a-trous kernels' launches share: the ping-pong pair of one iteration, the G-buffer that guides it and its three terms
struct AtrousArgs {
	const float4* in;   // colour records (see the two argument structs)
	const float4* nrm;  // normal xyz, w = t
	const float4* pos;  // position xyz, w = objIdx bits (-1: a miss)
	const float4* alb;  // albedo rgb, w = material bits
	float4* out;
	int width, height, step;
	float kn, kx, ka;
};
struct DenoiseArgs : AtrousArgs { // in: the accumulator (FIRST) or the previous iteration's output
	float it, kc;       // the accumulator's frame count (FIRST only); the colour term's k
};

__device__ __forceinline__ bool finite4(const float4& c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }
__device__ __forceinline__ float dist2(const float4& a, const float4& b)
{
	const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
	return dx * dx + dy * dy + dz * dz;
}

// The 25 taps of pixel (x, y) with G-buffer records xp, np, ap: the one tap loop of k_denoise_atrous and k_denoise_var_atrous.  Returns
// (sum w c_q, sum w).  What a tap's colour is belongs to the term object T, in the idiom of the traversal policies:
//   load(q)       tap q's colour record
//   valid(c)      whether a record is a tap at all
//   distance(cq)  the colour side of the exponent (0: the term is dropped)
//   add(w, cq)    the term's own sums, after the shared ones
template <class Term>
__device__ __forceinline__ float4 atrous_taps(const AtrousArgs& A, int x, int y, const float4& xp, const float4& np, const float4& ap, Term& T)
{
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
			const float4 cq = T.load(q);
			if (!T.valid(cq)) continue;
			float e = T.distance(cq);
			if (hitP) {
				const float4 nq = A.nrm[q], aq = A.alb[q];
				if (A.kn != 0.0f) e = e + dist2(np, nq) * A.kn;
				if (kxp != 0.0f) e = e + dist2(xp, xq) * kxp;
				if (A.ka != 0.0f) e = e + dist2(ap, aq) * A.ka;
			}
			const float w = h[dx + 2] * h[dy + 2] * expf(-e);
			sw = sw + w;
			sx = sx + w * cq.x, sy = sy + w * cq.y, sz = sz + w * cq.z;
			T.add(w, cq);
		}
	}
	return make_float4(sx, sy, sz, sw);
}

template <bool FIRST>
__device__ __forceinline__ float4 denoise_color(const DenoiseArgs& A, int i)
{
	float4 c = A.in[i];
	if (FIRST) c = make_float4(c.x / A.it, c.y / A.it, c.z / A.it, 0.0f);
	return c;
}
// rt_denoise's colour term: |c_p - c_q|^2 kc over finite colours
template <bool FIRST>
struct ColorTerm {
	const DenoiseArgs& A; float4 cp; float kc;
	__device__ __forceinline__ float4 load(int q) const { return denoise_color<FIRST>(A, q); }
	__device__ __forceinline__ bool valid(const float4& c) const { return finite4(c); }
	__device__ __forceinline__ float distance(const float4& cq) const { return kc != 0.0f ? dist2(cp, cq) * kc : 0.0f; }
	__device__ __forceinline__ void add(float, const float4&) {}
};

template <bool FIRST>
__global__ void __launch_bounds__(RT_DENOISE_TX * RT_DENOISE_TY) k_denoise_atrous(DenoiseArgs A)
{
	const int x = blockIdx.x * RT_DENOISE_TX + threadIdx.x, y = blockIdx.y * RT_DENOISE_TY + threadIdx.y;
	if (x >= A.width || y >= A.height) return;
	const int p = y * A.width + x;
	const float4 cp = denoise_color<FIRST>(A, p);
	if (!finite4(cp)) { A.out[p] = make_float4(cp.x, cp.y, cp.z, 0.0f); return; }
	const float4 xp = A.pos[p], np = A.nrm[p], ap = A.alb[p];
	ColorTerm<FIRST> T{ A, cp, A.kc };
	const float4 s = atrous_taps(A, x, y, xp, np, ap, T);
	A.out[p] = make_float4(s.x / s.w, s.y / s.w, s.z / s.w, 0.0f);
}

} // namespace rtd
