// The shade step of Renderer::Trace / Renderer::Sample at a hit (renderer.cpp:21-236), ONCE: the lights, diffuse::scatter, and what each
// material makes of a hit -- the next ray and its weight -- as functions on values.  Every pipeline calls them (k_shade / k_light,
// k_shade_s / k_light_s, the two general kernels, the Whitted policies of rt_mega.h) and keeps what is its own: which array a value is
// stored to, class bytes, pending branches, rewards, frames.  The expressions are the reference's, parenthesised as it writes them: under
// -ffp-contract=off a caller gets the bits it got while the expression stood in its own body.  Where Trace and Sample differ, the
// helper takes a parameter or the caller keeps the difference.  nD may be the variable D came from and nW the one W came from (the
// general kernels step their ray in place): the statement that writes one of them is the last that reads it.
#pragma once
#include "rt_scene_dev.h"

namespace rtd {

__device__ __forceinline__ f3 sky_color(const DScene& S, const f3& D); // rt_kernels.h

// ---- lights (template/scene.h:121-137, 152-165) -----------------------------------------------
__device__ __forceinline__ f3 light_intensity(const DLight& L, const f3& p, const f3& n, const f3& from)
{
	const f3 col(L.col[0], L.col[1], L.col[2]);
	if (L.kind == 0) {
		float dis = length(from - p);
		f3 dir = from - p;
		float cos_ang = dot(normalize(n), normalize(dir));
		float relStr = 1 / (dis * RT_PI) * L.strength;
		// isZero(float3) compares each component '< 1e-4' in double (template/precomp.h:885)
		if (dis <= L.radius && ((double)cos_ang < 1e-4)) return L.strength * col;
		return relStr * col;
	}
	if (L.kind == 1) {
		const f3 pos(L.pos[0], L.pos[1], L.pos[2]), normal(L.normal[0], L.normal[1], L.normal[2]);
		f3 dir = p - pos;
		float sTheta = length(cross(dir, normal)) / length(dir) * length(normal);
		if (dot(dir, normal) < 0) return f3(0.0f);
		float dis = length(dir);
		float str = L.sinAngle - sTheta > 0 ? x_asinf(L.sinAngle) - x_asinf(sTheta) : 0;
		return f3(1 / dis * str * L.strength);
	}
	return f3(1.0f);
}
__device__ __forceinline__ f3 light_position(const DLight& L, bool raytracer, uint& seed)
{
	const f3 pos(L.pos[0], L.pos[1], L.pos[2]);
	if (L.kind != 0 || raytracer) return pos;
	float newRad = L.radius * sqrtf(RandomFloat(seed));
	float theta = RandomFloat(seed) * 2 * RT_PI;
	return f3(pos.x + newRad * x_cosf(theta), pos.y + newRad * x_sinf(theta), pos.z);
}
// the shadow ray from the hit point I towards a sampled light position (renderer.cpp:93-99 / :161-165)
__device__ __forceinline__ void shadow_ray(const f3& I, const f3& pickedPos, f3& O, f3& D, float& tmax)
{
	f3 dir = pickedPos - I;
	const float len2 = dot(dir, dir);
	dir = normalize(dir);
	O = I + dir * 1e-4f, D = dir, tmax = sqrtf(len2);
}

// Trace / Sample return at a ray that hit nothing (the sky, renderer.cpp:26 / :134) or a light (:27-28 / :135-137); false: a surface
__device__ __forceinline__ bool terminal_radiance(const DScene& S, int objIdx, const f3& I, const f3& normal, const f3& D, f3& out)
{
	if (objIdx == -1) { out = sky_color(S, D); return true; }
	if (objIdx >= 11 && objIdx < 11 + S.nLights) { out = light_intensity(S.lights[objIdx - 11], I, normal, I); return true; }
	return false;
}
// what a child at depth - 1 that cannot trace adds in path mode: Sample(depth < 0) = 0.05 (renderer.cpp:129)
__device__ __forceinline__ f3 untraced_child(const f3& W) { return W * f3(0.05f); }
// Russian roulette on the largest colour component (renderer.cpp:33-43 / :143-153; the survivor's f = f * (1 / p) is never read)
__device__ __forceinline__ bool roulette_survives(const f3& col, int depth, uint& seed)
{
	const double p = col.x > col.y && col.x > col.z ? col.x : col.y > col.z ? col.y : col.z;
	return depth < 5 || !p ? (double)RandomFloat(seed) < p : true;
}

// ---- DIFFUSE (renderer.cpp:87-122 / :156-191) -------------------------------------------------
// diffuse::scatter (template/scene.h:605-620): att out, energy in/out
__device__ __forceinline__ f3 diffuse_scatter(const DMaterial& m, const f3& rayD, const f3& lightDir, const f3& lightIntensity, const f3& normal, f3& energy)
{
	const f3 albedo(m.albedo[0], m.albedo[1], m.albedo[2]);
	f3 reflectionDirection = reflect(-lightDir, normal);
	f3 specularColor = x_powf(libm_fmaxf(0.0f, -dot(reflectionDirection, rayD)), (float)m.N) * lightIntensity;
	f3 att = albedo * lightIntensity * m.diffu + specularColor * m.specu;
	f3 retention = f3(1.0f) - albedo;
	f3 newEnergy = energy - retention;
	energy = newEnergy.x > 0 ? newEnergy : f3(0.0f);
	return att;
}
// one visible light's direct term, and the weight of its mirror branch (renderer.cpp:100-104 / :170-175)
__device__ __forceinline__ f3 direct_term(const DMaterial& m, const f3& col, const f3& att, const f3& E) { return (1 - m.shinieness) * col * att * E; }
__device__ __forceinline__ f3 mirror_weight(const DMaterial& m, const f3& col, const f3& E) { return (m.shinieness * col) * E; }
// path mode: the direct part of (direct * INVPI + 2 * indirect) * albedo (renderer.cpp:187-190) ...
__device__ __forceinline__ f3 path_direct(const f3& direct, const f3& albedo) { return (direct * RT_INVPI) * albedo; }
// ... and the indirect part: one uniform hemisphere sample from the hit point, weighted with the child's coefficient (:181-186)
__device__ __forceinline__ void hemisphere_bounce(uint& seed, const f3& normal, const f3& col, const f3& albedo, const f3& W, f3& nD, f3& nW)
{
	const f3 rayToHemi = RandomInHemisphere(seed, normal);
	const f3 cos_i(dot(rayToHemi, normal));
	nD = rayToHemi;
	nW = W * ((2 * (col * cos_i)) * albedo);
}

// ---- METAL (renderer.cpp:81-86 / :192-197, metal::scatter template/scene.h:630-635) -------------
// Sample weighs the mirror ray with col, Trace with col * energy
__device__ __forceinline__ void metal_bounce(bool path, const f3& col, const f3& I, const f3& D, const f3& normal, const f3& W, const f3& E, f3& nO, f3& nD, f3& nW)
{
	nO = I + normal * 0.001f, nD = reflect(D, normal);
	nW = path ? W * col : W * (col * E);
}

// ---- GLASS (renderer.cpp:45-80 / :198-233) ----------------------------------------------------
// What both children of a glass hit share; the absorption along the segment goes into E when the ray arrives from outside.  Sample
// takes ONE child (refraction when kr < RandomFloat), Trace the reflection always and the refraction when kr < 1, so the children
// are two functions and a caller computes only what it takes (k_shade_s is held to five waves by its registers).
struct GlassHit { float kr; bool outside; f3 norm, bias; };
__device__ __forceinline__ GlassHit glass_hit(const DMaterial& m, const f3& D, const f3& normal, float t, f3& E)
{
	const float kr = glass_fresnel(normalize(D), normalize(normal), m.ir);
	const bool outside = dot(D, normal) < 0;
	const f3 bias = 0.0001f * normal;
	const f3 norm = outside ? normal : -normal;
	if (outside) {
		// exp(+-0) is exactly 1 and x * 1 is x: a glass without absorption (every glass of the reference's scenes
		// but one) skips three double-precision exp calls; NaN / inf exponents still take them
		const float ax = m.absorption[0] * -t, ay = m.absorption[1] * -t, az = m.absorption[2] * -t;
		if (ax != 0) E.x *= x_expf(ax);
		if (ay != 0) E.y *= x_expf(ay);
		if (az != 0) E.z *= x_expf(az);
	}
	return GlassHit{ kr, outside, norm, bias };
}
__device__ __forceinline__ void glass_refracted(const GlassHit& g, const DMaterial& m, const f3& I, const f3& D, const f3& W, const f3& E, f3& nO, f3& nD, f3& nW)
{
	const f3 col(m.col[0], m.col[1], m.col[2]);
	const float r = !g.outside ? m.ir : (1 / m.ir);
	nD = normalize(glass_refract(D, g.norm, r));
	nO = g.outside ? I - g.bias : I + g.bias;
	const f3 tempCol = col * E;
	nW = W * (tempCol * (1 - g.kr));
}
__device__ __forceinline__ void glass_reflected(const GlassHit& g, const DMaterial& m, const f3& I, const f3& D, const f3& W, f3& nO, f3& nD, f3& nW)
{
	const f3 col(m.col[0], m.col[1], m.col[2]);
	nD = normalize(reflect(D, g.norm));
	nO = g.outside ? I + g.bias : I - g.bias;
	nW = W * (col * g.kr);
}

} // namespace rtd
