// The path integrator's wavefront in DENSE form (Renderer::Sample, renderer.cpp:128-236, for batches that give every
// sample an entry of its own: the bench workloads, Renderer::Tick in path mode, rt_trace_batch).
//
// rt_kernels.h keeps one slot per sample for the whole batch and a status byte per slot; after the first bounce most
// slots are dead (the bench frame: 50 % after round 0, 87 % after round 1), so every later kernel reads and writes
// 16-byte elements scattered over mostly dead 128-byte lines -- measured round 2: k_shade moves its ~250 B per live slot
// at 0.42 of the HBM peak.  Compacting afterwards would pay for the same sparse lines once more.  Here nothing is ever
// written sparse: the entries of round r + 1 are the survivors of round r in order, and every producer writes its
// output straight to the position the survivor will have.  That position has to be known before shade runs, and it
// is: whether a path continues is decided by WHAT it hit (miss / light: no; a surface: yes until the last round; a
// diffuse surface also gets a shadow record), so the kernel that finds the hit -- extend, or the producer of a ray whose
// hit it could decide itself, see ray_decided() -- leaves a class byte per entry, and one scan (k_assign) turns the
// class bytes into positions.  Per round:
//   compact   cls -> queue of the entries that still need a traversal                        (1 B per entry)
//   extend    Scene::FindNearest for those; hit record + class byte per entry                (persistent, the dominant kernel)
//   assign    exclusive scans of the CONT and SHADOW class bits -> pos[e / 64] = (position in round r + 1, shadow position) of the group's first entry
//   shade     the body of Sample at the hit: reads entry e, writes the continuation (next ray, W, E, L) at its
//             position in the other buffer of a ping-pong pair and the shadow record at its shadow position; a path
//             that ends stores its finished sample.  Nothing else is written.
//   connect   Scene::IsOccluded per (shadow record, light)                                    } on a second stream,
//   light     the direct terms of the shadow records, in light order; updates E and L of the   } beside the next
//             continuation entry (or stores the sample in the last round)                       } round's extend
// Path depth is the same for every entry of a round (depth = start depth - round), so "last round" is a launch
// argument and W.w is free.  The order of entries is the order of samples (frame-major, then pixels) with holes
// closed: neighbours stay neighbours, which is all the coherence the later rounds have.
//
// Producer-side decisions (ray_decided): a kernel that creates a ray (generate, shade) already runs the head tests of
// Scene::FindNearest on it (lights, brute-force primitives).  It now also makes the FIRST step extend would make -- the
// root pair of the TLAS with its reach boxes, or the root pair of the scene BVH -- and when that step leaves nothing to
// visit the query is answered: the hit is the head candidate.  Such an entry gets its hit record and class from the
// producer and never enters the traversal queue; a camera ray that leaves the scene this way (sky or a light) is
// finished inside generate and never becomes an entry at all.  On the bench frame two thirds of the camera rays and
// 59 % of the first-bounce rays are of this kind (profiles/r02_step_histogram_spp8.txt: "0 instance entries"); each used
// to cost a queue slot, a refill in the 42 %-lane traversal kernel, and a ray load + hit store at random addresses.
// The step is the one trace_persistent makes, on the same operands, so results are identical by construction.
#pragma once
#include "rt_kernels.h"
#include "rt_qlearn.h"

namespace rtd {

#define CL_TRACE 1  // the entry's ray still needs Scene::FindNearest's traversal (extend)
#define CL_LIVE 2   // the entry holds a path (round 0 only: entries of samples finished inside generate are not live)
#define CL_CONT 4   // the path continues: shade writes a continuation entry at pos.x
#define CL_SHADOW 8 // diffuse hit with lights: shade writes a shadow record at pos.y

// counts[] of a StreamState
#define SC_N 0       // [3] entries of round r at [r % 3]
#define SC_FLAG 3    // overflow / debug flag (as Queues::counts[3])
#define SC_SHADOW 4  // [3] shadow records of round r at [r % 3]
#define SC_TRACE 7   // length of the traversal queue
#define SC_LEFTOVER 8 // shadow rays the 4-wide walk handed back
#define SC_DECIDED 9 // rays answered by their producer (counting launches)

struct StreamState {
	float4* O[2];     // ray origin xyz, w = ray.t after the head tests        } entry e of round parity p
	float4* D[2];     // ray direction xyz, w = head candidate (pack_head)     }
	float4* hitN[2];  // hit normal xyz, w = t
	int2* hitId[2];   // objIdx, material
	float4* W[2];     // path weight xyz
	float4* E[2];     // energy xyz, w = RNG state
	float4* L[2];     // radiance so far xyz, w = sample id
	unsigned char* cls[2]; // CL_* bits
	int2* pos;        // current round, per GROUP of 64 entries: x = entry in the next round of the group's first CL_CONT entry, y = shadow record of its first CL_SHADOW entry (k_assign; k_shade_s counts inside the group)
	// A shadow record holds what exists nowhere else, and references into its round for the rest: the hit's normal, D, W and
	// material stay in entry e of buffer p = round & 1 until shade(r + 1) writes that buffer, and shade(r + 1) starts only after
	// light(r) on every schedule of run_rounds_stream.  light rebuilds the sampled light positions from the seed: it runs shade's
	// loop of light_position calls again on the same operands, so the replay is bit for bit.  connect reads them from shP:
	// replayed there, its double-precision cos / sin cost it more than the 16-B load (profiles/FINDINGS.md, finding 93).
	float4* shI;      // shadow record: ray.IntersectionPoint() xyz, w = RNG state before the light loop (bits)
	int2* shX;        //                x = entry e of round r, y = continuation entry (holds this path's E and L)
	float4* shP;      // [light][cap]   sampled light position xyz: connect's alone (light replays the draws)
	unsigned char* vis; // [light][cap] 1: occluded
	uint* traceQ;     // entries with CL_TRACE, in order
	uint* leftover;   // connect work items the 4-wide walk handed back
	int* heads;       // work heads: extend [0, RT_HEADS), connect [RT_HEADS, 2 RT_HEADS)
	int* counts;
	int cap;          // entries the arrays hold
};

// what the hit decides about the path (path mode; 'last': the round whose hits are at depth 0, renderer.cpp:129)
// matType: the material type the primitive record carried (resolve_hit), 0 = look it up
__device__ __forceinline__ int hit_class(const DScene& S, int objIdx, int mat, int last, int matType = 0)
{
	if (objIdx == -1) return 0;                                 // renderer.cpp:134
	if (objIdx >= 11 && objIdx < 11 + S.nLights) return 0;      // :135-137
	const int type = matType ? matType : S.mats[mat].type;
	const bool shadow = type != 3 && type != 2 && S.nLights > 0; // DIFFUSE: the light loop, :158-176
	const bool cont = !last || shadow; // every material scatters one ray while depth lasts; in the last round a diffuse hit
	                                   // still needs a continuation entry: light() finds the path's E and L there
	return (cont ? CL_CONT : 0) | (shadow ? CL_SHADOW : 0);
}

// Does the first step of the traversal already end it?  (trace_persistent: link = S.rootLink, one pair step, stack empty.)
// Same operands, same tests: the reference's boxes with the clean / exact slab test, and at the TLAS level the reach
// boxes under the same guard.  All loads are wave-uniform.
__device__ __forceinline__ bool ray_decided(const DScene& S, const f3& O, const f3& D, float rayT)
{
	const uint root = S.rootLink;
	if (root == RT_EMPTY) return true;
	if (root & (RT_LEAF_BIT | RT_INST_BIT)) return false; // a single leaf / a single instance: extend's business
	const f3 rD = rcp3(D);
	const bool clean = ray_is_clean(O, D, rD);
	const float4* p = S.pairs + 4 * (size_t)root;
	const float4 a0 = p[0], a1 = p[1], b0 = p[2], b1 = p[3];
	float dist1, dist2;
	if (clean) dist1 = intersect_aabb_clean(O, rD, rayT, xyz(a0), xyz(a1)), dist2 = intersect_aabb_clean(O, rD, rayT, xyz(b0), xyz(b1));
	else dist1 = intersect_aabb_exact(O, rD, rayT, xyz(a0), xyz(a1)), dist2 = intersect_aabb_exact(O, rD, rayT, xyz(b0), xyz(b1));
	if (S.useTLAS && clean && fabsf(O.x) + fabsf(O.y) + fabsf(O.z) <= S.reachOriginMax) {
		const float4* q = S.reach + 3 * (size_t)(root - S.tlasBase);
		const float4 r0 = q[0], r1 = q[1], r2 = q[2];
		if (!box_reachable(O, rD, rayT, xyz(r0), f3(r0.w, r1.x, r1.y))) dist1 = 1e30f;
		if (!box_reachable(O, rD, rayT, f3(r1.z, r1.w, r2.x), f3(r2.y, r2.z, r2.w))) dist2 = 1e30f;
	}
	return dist1 == 1e30f && dist2 == 1e30f;
}

// A new ray for entry e of the round with parity p: head tests (as emit_ray), then the decision above.  Returns the class
// byte of the entry; a decided ray gets its hit record here.  'last': the round this ray is traced in is the last one.
// finishNoHit (generate): a decided ray that hit nothing or a light is not stored at all (the caller finishes the sample).
struct NewRay { unsigned char cls; bool decided; float t; int objIdx, mat; f3 normal; };
__device__ __forceinline__ NewRay emit_ray_s(const DScene& S, const StreamState& T, int p, int e, const f3& O, const f3& D, float t_min, int last, bool finishNoHit, bool decide)
{
	NewRay r;
	float rayT = 1e34f; // Ray constructor default (template/scene.h:42)
	HitRef head;
	head.kind = -1, head.inst = -1, head.prim = 0, head.t = 0;
	LaneCounters unused;
	find_nearest_head<false>(S, O, D, t_min, rayT, head, unused);
	r.cls = CL_LIVE | CL_TRACE, r.decided = false, r.t = rayT, r.objIdx = -1, r.mat = -1, r.normal = f3(0.0f);
	if (decide && ray_decided(S, O, D, rayT)) {
		r.decided = true;
		head.t = rayT;
		int matType;
		resolve_hit(S, head, O, D, r.objIdx, r.mat, r.normal, &matType);
		const int hc = hit_class(S, r.objIdx, r.mat, last, matType);
		// nothing hit, or a light: Sample() returns at renderer.cpp:134 / :135-137 (in the last round a glass or metal hit has class 0 too)
		if (finishNoHit && (r.objIdx == -1 || (r.objIdx >= 11 && r.objIdx < 11 + S.nLights))) { r.cls = 0; return r; }
		T.hitN[p][e] = mk4(r.normal, rayT);
		T.hitId[p][e] = make_int2(r.objIdx, r.mat);
		r.cls = (unsigned char)(CL_LIVE | hc);
	}
	T.O[p][e] = mk4(O, rayT);
	T.D[p][e] = mk4(D, __uint_as_float(pack_head(head)));
	return r;
}

// counting launches: rays answered by their producer are Scene::FindNearest calls like any other.  A thread tallies its
// own, the block adds them to counts[SC_DECIDED] with one atomic at its end (same-address atomics retire at ~88 per
// microsecond: one per wave of a 2 M-wave launch would take longer than the launch), k_fold_decided moves the batch's
// total into the counters.
__device__ __forceinline__ void flush_decided(int* counts, uint mine)
{
	__shared__ uint blockDecided;
	if (threadIdx.x == 0) blockDecided = 0;
	__syncthreads();
	uint x = mine;
	for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
	if ((threadIdx.x & 63) == 0 && x) atomicAdd(&blockDecided, x);
	__syncthreads();
	if (threadIdx.x == 0 && blockDecided) atomicAdd(&counts[SC_DECIDED], (int)blockDecided);
}
__global__ void k_fold_decided(DScene S, int* counts, DCounters* counters)
{
	const unsigned long long nd = (unsigned long long)(uint)counts[SC_DECIDED];
	counts[SC_DECIDED] = 0;
	counters->rays_nearest += nd, counters->light_tests += nd * (unsigned)S.nLights;
	if (S.useTLAS) counters->brute_tests += nd * (unsigned)(S.nBruteSph + S.nBrutePla);
}

// Round bookkeeping without launches of its own.  Round r reads its entry count at counts[SC_N + r % 3]; assign(r) adds up the
// next round's at [(r + 1) % 3] and this round's shadow records at [SC_SHADOW + r % 3].  Whatever round r + 1 needs zeroed is
// zeroed by ONE thread of shade(r) (and by generate for round 0): the traversal queue's length and extend's work heads
// (compact(r) and extend(r) are over), the entry count of round r + 2 (its slot last held round r - 1's, which nobody reads any
// more), the shadow count of round r + 1 (its slot held round r - 2's: connect / light of that round ended before shade(r - 1)
// was allowed to start), and connect's heads for connect(r) (connect(r - 1) ended before this kernel was allowed to start).
__device__ __forceinline__ void prepare_round(const StreamState& T, int next /* the round being prepared */, int n0)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	if (n0 >= 0) T.counts[SC_N + next % 3] = n0; // generate: the batch's samples are round 0's entries
	T.counts[SC_TRACE] = 0, T.counts[SC_N + (next + 1) % 3] = 0, T.counts[SC_SHADOW + next % 3] = 0;
	for (int h = 0; h < RT_HEADS; h++) T.heads[h * RT_HEAD_STRIDE] = 0;
	// connect of the round before 'next' (it starts after the kernel this runs in)
	T.counts[SC_LEFTOVER] = 0;
	for (int h = RT_HEADS; h < 2 * RT_HEADS; h++) T.heads[h * RT_HEAD_STRIDE] = 0;
}
// connect's work heads alone: the leftover launch of the 4-wide walk goes through its own list with them
__global__ void k_stream_begin(StreamState T)
{
	for (int h = RT_HEADS; h < 2 * RT_HEADS; h++) T.heads[h * RT_HEAD_STRIDE] = 0;
}

__global__ void __launch_bounds__(RT_COMPACT_BLOCK) k_compact_s(StreamState T, int round)
{
	compact_body(T.cls[round & 1], T.counts[SC_N + round % 3], CL_TRACE, T.traceQ, &T.counts[SC_TRACE]);
}

// generate: camera sample e of the batch (renderer.cpp:263-278) -> entry e of round 0.  A sample whose camera ray
// provably leaves the scene (or ends on a light) is finished here: Sample() returns at :134 / :135-137.
__global__ void __launch_bounds__(RT_BLOCK) k_generate_s(DScene S, DCamera C, RenderParams R, StreamState T, int last, int decide, int counting)
{
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	const bool valid = e < (int)R.nSamples;
	bool decided = false;
	prepare_round(T, 0, (int)R.nSamples);
	if (valid) {
		const uint sid = R.sampleFirst + (uint)e;
		f3 O, D;
		uint seed = 0;
		if (R.customO) {
			O = f3(R.customO[3 * sid], R.customO[3 * sid + 1], R.customO[3 * sid + 2]);
			D = f3(R.customD[3 * sid], R.customD[3 * sid + 1], R.customD[3 * sid + 2]);
		} else sample_primary(C, R, sid, O, D, seed);
		const NewRay nr = emit_ray_s(S, T, 0, e, O, D, mode_t_min(1), last, (decide & 2) == 0, decide != 0);
		decided = nr.decided;
		if (nr.cls == 0) {
			// what the first shade would do with Lsum = 0 and W = 1 (0 + 1 * x is x, bit for bit)
			f3 Lsum(0.0f);
			const f3 W(1.0f);
			const unsigned char* texel = nullptr;
			if (nr.objIdx == -1) {
				texel = sky_texel(S, D);
				if (texel) Lsum = Lsum + W * (f3((float)texel[0], (float)texel[1], (float)texel[2]) / 255);
			} else {
				const f3 I = O + nr.t * D;
				Lsum = Lsum + W * light_intensity(S.lights[nr.objIdx - 11], I, nr.normal, I);
			}
			// the sample is a sky texel: 0 + 1 * (b / 255) is b / 255, and its gamma-corrected value one of 256 numbers the
			// device computed with the same pow (three double-precision pow calls per finished sample are most of this kernel otherwise)
			if (texel && !R.customOut && S.gammaLut) R.samples[sid] = make_float4(S.gammaLut[texel[0]], S.gammaLut[texel[1]], S.gammaLut[texel[2]], 0.0f);
			else store_sample(R, sid, Lsum);
		}
		T.cls[0][e] = nr.cls;
	}
	if (counting) flush_decided(T.counts, decided ? 1u : 0u);
}

// ---- the primary-hit table ---------------------------------------------------------------------------------------------
// sample_primary truncates the jittered pixel to ints before it builds the ray (renderer.cpp:276-278), so every camera ray of a
// batch is the ray of an INTEGER pixel of [-1, width] x [-1, height] (sample_primary_pixel), and Scene::FindNearest of it --
// head tests, the walk, resolve_hit -- is a function of that pixel, the camera and the scene alone.  A 64-frame batch asks
// the same ~2 M queries 64 times each.  The table holds their answers; round 0 of a batch reads them (k_generate_t) and has no
// traversal queue, no compaction and no extend launch.  Everything from assign(0) on sees what generate + extend(0) would have left.
//   A   a surface hit: hit normal xyz, w = t (the entry's hitN).  Nothing / a light: the finished sample's radiance xyz, the
//       Lsum k_generate_s hands to store_sample, computed once by the same expressions
//   B   x objIdx, y material (the entry's hitId), z PT_* bits | hit_class of the hit for a round that is not the last (bits 0-3)
//       and for one that is (bits 4-7), w the sky texel's bytes r | g << 8 | b << 16 (PT_TEXEL: generate's gamma table takes them)
struct PrimaryTable {
	float4* A;
	int4* B;
	int w, h; // (width + 2) x (height + 2) records, record (px + 1) + (py + 1) * w
};
#define PT_FINISHED 0x100 // the ray hits nothing or a light: Sample() returns at renderer.cpp:134 / :135-137
#define PT_TEXEL 0x200    // ... nothing, and the scene has a sky texture
struct TablePolicy {
	const DScene& S; const DCamera& C; const PrimaryTable& P; float t_min;
	__device__ __forceinline__ int slot_of(int i) const { return i; }
	__device__ __forceinline__ void ray(int i, f3& O, f3& D) const { primary_ray(C, i % P.w - 1, i / P.w - 1, O, D); } // the call sample_primary makes, on the same ints
	__device__ __forceinline__ bool load(int i, f3& O, f3& D, float& tm, HitRef& head) const
	{
		ray(i, O, D);
		tm = 1e34f; // Ray constructor default, as emit_ray_s
		LaneCounters unused;
		find_nearest_head<false>(S, O, D, t_min, tm, head, unused);
		return true;
	}
	__device__ __forceinline__ void store(int i, const HitRef& hit, const f3&, const f3&) const
	{
		f3 O, D;
		ray(i, O, D);
		int objIdx, mat, matType;
		f3 normal;
		resolve_hit(S, hit, O, D, objIdx, mat, normal, &matType);
		int flags = hit_class(S, objIdx, mat, 0, matType) | (hit_class(S, objIdx, mat, 1, matType) << 4);
		float4 a = mk4(normal, hit.t);
		int texelBits = 0;
		const bool none = objIdx == -1;
		if (none || (objIdx >= 11 && objIdx < 11 + S.nLights)) {
			// k_generate_s's finish of such a sample (the first shade with Lsum = 0 and W = 1)
			f3 Lsum(0.0f);
			const f3 W(1.0f);
			flags |= PT_FINISHED;
			if (none) {
				const unsigned char* texel = sky_texel(S, D);
				if (texel) {
					Lsum = Lsum + W * (f3((float)texel[0], (float)texel[1], (float)texel[2]) / 255);
					flags |= PT_TEXEL, texelBits = (int)texel[0] | ((int)texel[1] << 8) | ((int)texel[2] << 16);
				}
			} else {
				const f3 I = O + hit.t * D;
				Lsum = Lsum + W * light_intensity(S.lights[objIdx - 11], I, normal, I);
			}
			a = mk4(Lsum, 0.0f);
		}
		P.A[i] = a;
		P.B[i] = make_int4(objIdx, mat, flags, texelBits);
	}
};
// One launch per (camera, scene): its walk tallies go to the counters of a counting launch that happens to build; the queries themselves
// are tallied by the samples that read the table (k_generate_t), so lc.light / lc.brute stay 0 here and no ray is counted.
template <bool COUNT>
__global__ void __launch_bounds__(RT_BLOCK) k_primary_table(DScene S, DCamera C, PrimaryTable P, float t_min, int tuning, uint* spill, int* heads, int* flag, DCounters* counters)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	TablePolicy pol{ S, C, P, t_min };
	trace_persistent<false, COUNT, false>(S, pol, P.w * P.h, heads, t_min, tuning, ldsStack, spill, flag, lc, rays);
	if (COUNT) flush_counters(counters, lc, 0, 0);
}

// ---- the bounce table: one round further --------------------------------------------------------------------------------
// The ray Sample scatters at a METAL hit takes no random draw, and at a GLASS hit a draw only chooses between two rays (the
// weights carry E, W and the draw; nO and nD depend on O, D, the normal, t and the material alone).  So the round-1 ray of
// every sample whose camera ray hits glass or metal is one of at most two rays per primary record, and Scene::FindNearest of it
// one of 2 (width + 2)(height + 2) answers.  Record i of branch b sits at b * n + i:
//   branch 0   the metal mirror ray / the glass refraction (built only when kr < 1: Sample takes it only when kr < RandomFloat <= 1)
//   branch 1   the glass reflection
//   A   hit normal xyz, w = t (the entry's hitN)
//   B   x objIdx, y material (the entry's hitId), z BT_PRESENT | hit_class of the hit for a round that is not the last (bits 0-3)
//       and for one that is (bits 4-7); z == 0: no such ray, or nobody traced it
// The build runs k_shade_s's own functions on the operands k_shade_s has in round 0 -- primary_ray on the same ints, normal and t
// from the primary record, the material record -- so the ray it traces is the ray shade(0) would hand to emit_ray_s, bit for bit.
struct BounceTable {
	float4* A;
	int4* B;
	int n, w; // primary records (2 n records here) and the primary table's row length
};
#define BT_PRESENT 0x100
// the ray a glass or metal hit (material m, normal, t) of the ray (O, D) scatters on 'branch': false when there is none (the hit is
// diffuse, or no sample can take the branch)
__device__ __forceinline__ bool specular_ray(const DMaterial& m, const f3& O, const f3& D, const f3& normal, float t, int branch, f3& nO, f3& nD)
{
	if (m.type != 3 && m.type != 2) return false;
	const f3 I = O + t * D; // ray.IntersectionPoint(), as k_shade_s
	const f3 W(1.0f);
	f3 E(1.0f), nW, o(0.0f), d(0.0f);
	bool have = false;
	if (m.type == 2) {
		const f3 col(m.col[0], m.col[1], m.col[2]);
		if (branch == 0) metal_bounce(true, col, I, D, normal, W, E, o, d, nW), have = true;
	} else {
		const GlassHit g = glass_hit(m, D, normal, t, E);
		if (branch != 0) glass_reflected(g, m, I, D, W, o, d, nW), have = true;
		else if (g.kr < 1.0f) glass_refracted(g, m, I, D, W, E, o, d, nW), have = true;
	}
	if (have) nO = o, nD = d;
	return have;
}
// the ray of (record i, branch): false when there is none (the primary ray ends, its hit is diffuse, or no sample can take the branch)
__device__ __forceinline__ bool bounce_ray(const DScene& S, const DCamera& C, const PrimaryTable& P, int i, int branch, f3& nO, f3& nD)
{
	const int4 b = P.B[i];
	if (b.z & PT_FINISHED) return false;
	const DMaterial m = S.mats[b.y];
	if (m.type != 3 && m.type != 2) return false;
	const float4 a = P.A[i];
	f3 O, D;
	primary_ray(C, i % P.w - 1, i / P.w - 1, O, D);
	return specular_ray(m, O, D, xyz(a), a.w, branch, nO, nD);
}
struct BouncePolicy {
	const DScene& S; const DCamera& C; const PrimaryTable& P; const BounceTable& Bt; float t_min; int* flag;
	__device__ __forceinline__ int slot_of(int w) const { return w; }
	__device__ __forceinline__ bool load(int w, f3& O, f3& D, float& tm, HitRef& head) const
	{
		const int branch = w >= Bt.n ? 1 : 0, i = w - branch * Bt.n;
		RT_CHECK(i >= 0 && i < Bt.n && Bt.n == P.w * P.h, 26, flag);
		f3 o(0.0f), d(0.0f);
		if (!bounce_ray(S, C, P, i, branch, o, d)) { Bt.B[w] = make_int4(0, 0, 0, 0); return false; }
		O = o, D = d;
		tm = 1e34f; // Ray constructor default, as emit_ray_s
		LaneCounters unused;
		find_nearest_head<false>(S, O, D, t_min, tm, head, unused);
		return true;
	}
	__device__ __forceinline__ void store(int w, const HitRef& hit, const f3&, const f3&) const
	{
		const int branch = w >= Bt.n ? 1 : 0, i = w - branch * Bt.n;
		f3 O, D;
		bounce_ray(S, C, P, i, branch, O, D); // (the walk's O and D may be an instance's)
		int objIdx, mat, matType;
		f3 normal;
		resolve_hit(S, hit, O, D, objIdx, mat, normal, &matType);
		const int flags = BT_PRESENT | hit_class(S, objIdx, mat, 0, matType) | (hit_class(S, objIdx, mat, 1, matType) << 4);
		Bt.A[w] = mk4(normal, hit.t);
		Bt.B[w] = make_int4(objIdx, mat, flags, 0);
	}
};
// One launch per (camera, scene) right after k_primary_table, whose records it reads; counting launches as there.
template <bool COUNT>
__global__ void __launch_bounds__(RT_BLOCK) k_bounce_table(DScene S, DCamera C, PrimaryTable P, BounceTable Bt, float t_min, int tuning, uint* spill, int* heads, int* flag, DCounters* counters)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	BouncePolicy pol{ S, C, P, Bt, mode_t_min(1), flag };
	trace_persistent<false, COUNT, false>(S, pol, 2 * Bt.n, heads, t_min, tuning, ldsStack, spill, flag, lc, rays);
	if (COUNT) flush_counters(counters, lc, 0, 0);
}

// ---- the chain tables: levels 2 .. RT_BOUNCE_DEPTH ----------------------------------------------------------------------
// The argument does not stop at round 1.  While every hit of a path so far was glass or metal, no draw has entered an nO or nD: the
// round-k ray is one of at most 2^k rays per primary record, and these are the long rays (58 / 47 steps per ray leaving glass / metal,
// 14 off a diffuse surface).  Level 1 is the BounceTable, dense.  A level k >= 2 is COMPACT: a record exists only for a child of a
// specular hit of level k - 1, and B.w of a record of level k >= 1 -- 0 until k_chain_link has run over its level -- is the LINK:
// 1 + the index in level k + 1 of its first child, 0 for none.  Children per specular hit: metal one; glass the refraction at the
// link's index and the reflection one behind it (the refraction's record stays absent when kr < 1 fails, as in bounce_ray).
//   A, B    as the BounceTable's, B.w the link
//   RO, RD  (build only) the record's world ray: load writes it, store hands it to resolve_hit, the next level's load starts from it
//   parent  (build only) x = the record of the level above, y = the branch; x < 0: the slot nobody got (below)
// k_chain_link hands out the indices with one atomic per block, so the order of records differs from build to build and nothing
// depends on it.  A level holds cap records; children that do not fit -- both of a glass hit or neither -- leave link 0, and shade
// traces such a ray as it always did: a missing record is never wrong, only slower.
// Bit equality, by induction on the level.  Shade of round k - 1 computes the ray of an entry answered from record r of level k - 1
// by metal_bounce / glass_hit + glass_refracted / glass_reflected on O, D (the entry's: the nO, nD the round before wrote, to the
// bit), normal and t (hitN: r's A), the material (hitId: r's B.y) and I = O + t * D.  The build's load runs the same functions
// (specular_ray, which is bounce_ray's body) on r's world ray -- level 1: bounce_ray of the primary record, which is shade(0)'s nO, nD
// by the level-1 argument above; level >= 2: RO, RD of r, which by induction is the entry's O, D -- and on r's A and B, under
// -ffp-contract=off.  W, E and the draw enter the weights only.  So the child's ray is the ray shade would hand to emit_ray_s, and
// its record what extend would have stored for it: head tests, walk and resolve_hit (on the world ray) are the same calls.
struct ChainLevel {
	float4* A;
	int4* B;
	float4* RO;
	float4* RD;
	int2* parent;
	int* count; // records handed out so far; runs past cap when children did not fit
	int cap;
};
// Links level 'up' (its B; n records, or min(*upCount, n) of a compact level) to level L: every present record whose hit is glass or
// metal gets its children's indices.  The request of a block is one atomicAdd; a record's children sit at the block's base + the
// requests of the lanes before it.  The only hole this can leave below cap is the last slot, when a glass pair started there: its
// parent is marked -1 by the lane that saw it.
__global__ void __launch_bounds__(RT_BLOCK) k_chain_link(DScene S, int4* upB, const int* upCount, int n, ChainLevel L)
{
	__shared__ int waveSum[RT_BLOCK / 64];
	__shared__ int blockBase;
	if (upCount) n = min(*upCount, n);
	const int i = (int)(blockIdx.x * RT_BLOCK + threadIdx.x);
	const int lane = (int)(threadIdx.x & 63), wib = (int)(threadIdx.x >> 6);
	int nc = 0;
	if (i < n) {
		const int4 b = upB[i];
		if ((b.z & BT_PRESENT) && (b.z & CL_CONT)) { // a surface: b.y is a material
			const int type = S.mats[b.y].type;
			nc = type == 3 ? 2 : (type == 2 ? 1 : 0);
		}
	}
	int inc = nc;
	for (int o = 1; o < 64; o <<= 1) {
		const int t = __shfl_up(inc, o);
		if (lane >= o) inc += t;
	}
	if (lane == 63) waveSum[wib] = inc;
	__syncthreads();
	if (threadIdx.x == 0) {
		int tot = 0;
		for (int w = 0; w < RT_BLOCK / 64; w++) tot += waveSum[w];
		blockBase = tot > 0 ? atomicAdd(L.count, tot) : 0;
	}
	__syncthreads();
	if (i >= n) return;
	int base = blockBase + inc - nc;
	for (int w = 0; w < wib; w++) base += waveSum[w];
	int link = 0;
	if (nc > 0) {
		if (base >= 0 && base + nc <= L.cap) {
			L.parent[base] = make_int2(i, 0);
			if (nc == 2) L.parent[base + 1] = make_int2(i, 1);
			link = base + 1;
		} else if (base >= 0 && base < L.cap) L.parent[base] = make_int2(-1, 0); // (base == cap - 1, nc == 2)
	}
	upB[i].w = link;
}
struct ChainPolicy {
	const DScene& S; const DCamera& C; const PrimaryTable& P; const BounceTable& Bt; const ChainLevel& Up; const ChainLevel& L; float t_min; int* flag;
	__device__ __forceinline__ int slot_of(int w) const { return w; }
	__device__ __forceinline__ bool load(int w, f3& O, f3& D, float& tm, HitRef& head) const
	{
		const int2 pr = L.parent[w];
		const bool from1 = Up.A == nullptr; // the level above is the bounce table
		RT_CHECK(w >= 0 && w < L.cap && pr.x < (from1 ? 2 * Bt.n : Up.cap) && (pr.y == 0 || pr.y == 1), 29, flag);
		bool have = pr.x >= 0;
		f3 o(0.0f), d(0.0f), nO(0.0f), nD(0.0f);
		if (have) {
			float4 a;
			int4 b;
			if (from1) {
				const int branch = pr.x >= Bt.n ? 1 : 0;
				have = bounce_ray(S, C, P, pr.x - branch * Bt.n, branch, o, d);
				a = Bt.A[pr.x], b = Bt.B[pr.x];
			} else {
				o = xyz(Up.RO[pr.x]), d = xyz(Up.RD[pr.x]);
				a = Up.A[pr.x], b = Up.B[pr.x];
			}
			if (have && (b.z & BT_PRESENT) && (b.z & CL_CONT)) {
				const DMaterial m = S.mats[b.y];
				have = specular_ray(m, o, d, xyz(a), a.w, pr.y, nO, nD);
			} else have = false;
		}
		if (!have) { L.B[w] = make_int4(0, 0, 0, 0); return false; }
		L.RO[w] = mk4(nO, 0.0f), L.RD[w] = mk4(nD, 0.0f);
		O = nO, D = nD;
		tm = 1e34f; // Ray constructor default, as emit_ray_s
		LaneCounters unused;
		find_nearest_head<false>(S, O, D, t_min, tm, head, unused);
		return true;
	}
	__device__ __forceinline__ void store(int w, const HitRef& hit, const f3&, const f3&) const
	{
		const f3 O = xyz(L.RO[w]), D = xyz(L.RD[w]); // (the walk's O and D may be an instance's)
		int objIdx, mat, matType;
		f3 normal;
		resolve_hit(S, hit, O, D, objIdx, mat, normal, &matType);
		const int flags = BT_PRESENT | hit_class(S, objIdx, mat, 0, matType) | (hit_class(S, objIdx, mat, 1, matType) << 4);
		L.A[w] = mk4(normal, hit.t);
		L.B[w] = make_int4(objIdx, mat, flags, 0);
	}
};
// One launch per level >= 2 right behind k_chain_link of the level above, over the records that got a parent; counting launches as
// k_primary_table.  A level whose parent level holds no specular hit finds a count of 0 and traces nothing.
template <bool COUNT>
__global__ void __launch_bounds__(RT_BLOCK) k_chain_table(DScene S, DCamera C, PrimaryTable P, BounceTable Bt, ChainLevel Up, ChainLevel L, float t_min, int tuning, uint* spill, int* heads, int* flag, DCounters* counters)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	ChainPolicy pol{ S, C, P, Bt, Up, L, mode_t_min(1), flag };
	trace_persistent<false, COUNT, false>(S, pol, min(*L.count, L.cap), heads, t_min, tuning, ldsStack, spill, flag, lc, rays);
	if (COUNT) flush_counters(counters, lc, 0, 0);
}

// generate from the table: camera sample e of the batch -> entry e of round 0 WITH its hit, or the finished sample.  The seed and
// the two draws are sample_primary's; no head test, no ray_decided, no resolve_hit and no sky lookup per sample.  Neighbouring
// lanes are neighbouring pixels of one frame: their records are neighbours too.  No entry carries CL_TRACE.  A sample whose ray
// hits nothing or a light is finished here whatever RT_DECIDE says: the value is the one shade(0) would store.
// Counting launches: every sample is a Scene::FindNearest query answered by its producer (flush_decided).
__global__ void __launch_bounds__(RT_BLOCK) k_generate_t(DScene S, DCamera C, RenderParams R, StreamState T, PrimaryTable P, int last, int counting)
{
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	const bool valid = e < (int)R.nSamples;
	prepare_round(T, 0, (int)R.nSamples);
	if (valid) {
		const uint sid = R.sampleFirst + (uint)e;
		int px, py;
		uint seed;
		sample_primary_pixel(C, R, sid, px, py, seed);
		RT_CHECK(px >= -1 && px <= C.width && py >= -1 && py <= C.height, 25, &T.counts[SC_FLAG]);
		const size_t i = (size_t)(px + 1) + (size_t)(py + 1) * (size_t)P.w;
		const int4 b = P.B[i];
		const float4 a = P.A[i];
		unsigned char cls = 0;
		if (b.z & PT_FINISHED) {
			if ((b.z & PT_TEXEL) && S.gammaLut) R.samples[sid] = make_float4(S.gammaLut[b.w & 255], S.gammaLut[(b.w >> 8) & 255], S.gammaLut[(b.w >> 16) & 255], 0.0f);
			else store_sample(R, sid, xyz(a));
		} else {
			f3 O, D;
			primary_ray(C, px, py, O, D);
			T.O[0][e] = mk4(O, a.w);  // w (ray.t) and D.w (the head candidate) are extend's: nobody reads them now
			T.D[0][e] = mk4(D, 0.0f);
			T.hitN[0][e] = a;
			T.hitId[0][e] = make_int2(b.x, b.y);
			cls = (unsigned char)(CL_LIVE | ((last ? b.z >> 4 : b.z) & 15));
		}
		T.cls[0][e] = cls;
	}
	if (counting) flush_decided(T.counts, valid ? 1u : 0u);
}
// generate for a round 0 that shades straight from the table (k_shade_s TABLE0, k_light_s TABLE0): the class byte and the finished
// samples, exactly k_generate_t's, and no entry.  O is the camera position, D a function of the integer pixel, the rest the record's:
// shade(0) runs sample_primary_pixel anyway and reads the 32-byte record itself instead of the 56 bytes of a copy of it.  A is read
// only where a finished sample is not a sky texel.  Pinhole cameras only (the host: run_rounds_stream).
__global__ void __launch_bounds__(RT_BLOCK) k_generate_c(DScene S, DCamera C, RenderParams R, StreamState T, PrimaryTable P, int last, int counting)
{
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	const bool valid = e < (int)R.nSamples;
	prepare_round(T, 0, (int)R.nSamples);
	if (valid) {
		const uint sid = R.sampleFirst + (uint)e;
		int px, py;
		uint seed;
		sample_primary_pixel(C, R, sid, px, py, seed);
		RT_CHECK(px >= -1 && px <= C.width && py >= -1 && py <= C.height, 25, &T.counts[SC_FLAG]);
		const size_t i = (size_t)(px + 1) + (size_t)(py + 1) * (size_t)P.w;
		const int4 b = P.B[i];
		unsigned char cls = 0;
		if (b.z & PT_FINISHED) {
			if ((b.z & PT_TEXEL) && S.gammaLut) R.samples[sid] = make_float4(S.gammaLut[b.w & 255], S.gammaLut[(b.w >> 8) & 255], S.gammaLut[(b.w >> 16) & 255], 0.0f);
			else store_sample(R, sid, xyz(P.A[i]));
		} else cls = (unsigned char)(CL_LIVE | ((last ? b.z >> 4 : b.z) & 15));
		T.cls[0][e] = cls;
	}
	if (counting) flush_decided(T.counts, valid ? 1u : 0u);
}

// extend: Scene::FindNearest for the entries of the traversal queue
struct StreamExtendPolicy {
	const DScene& S;
	const StreamState& T;
	int parity, last;
	int* flag;
	__device__ __forceinline__ bool load(int work, f3& O, f3& D, float& tmax, HitRef& head) const
	{
		const int e = (int)ld_stream(T.traceQ + work);
		RT_CHECK(e >= 0 && e < T.cap, 20, flag);
		const float4 o4 = ld_stream(T.O[parity] + e), d4 = ld_stream(T.D[parity] + e);
		O = xyz(o4), D = xyz(d4), tmax = o4.w;
		unpack_head(__float_as_uint(d4.w), head);
		return true;
	}
	__device__ __forceinline__ int slot_of(int work) const { return (int)T.traceQ[work]; }
	__device__ __forceinline__ void store(int work, const HitRef& hit, const f3& /*O*/, const f3& /*D*/) const
	{
		const int e = (int)ld_stream(T.traceQ + work);
		int objIdx, mat, matType;
		f3 normal;
		const StreamState& Tc = T;
		const int par = parity;
		resolve_hit_lazy(S, hit, [&](f3& o, f3& d) { o = xyz(ld_stream(Tc.O[par] + e)), d = xyz(ld_stream(Tc.D[par] + e)); }, objIdx, mat, normal, &matType);
		st_stream(T.hitN[parity] + e, mk4(normal, hit.t));
		st_stream(T.hitId[parity] + e, make_int2(objIdx, mat));
		T.cls[parity][e] = (unsigned char)(CL_LIVE | CL_TRACE | hit_class(S, objIdx, mat, last, matType)); // the record said what its material is: no second fetch
	}
};
template <bool COUNT>
__global__ void __launch_bounds__(RT_BLOCK, RT_EXTEND_WAVES) k_extend_s(DScene S, StreamState T, int parity, int last, float t_min, int tuning, uint* spill, DCounters* counters)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	StreamExtendPolicy pol{ S, T, parity, last, &T.counts[SC_FLAG] };
	trace_persistent<false, COUNT, false>(S, pol, T.counts[SC_TRACE], T.heads, t_min, tuning, ldsStack, spill, &T.counts[SC_FLAG], lc, rays);
	if (COUNT) {
		lc.light = rays * (uint)S.nLights, lc.brute = S.useTLAS ? rays * (uint)(S.nBruteSph + S.nBrutePla) : 0;
		flush_counters(counters, lc, rays, 0);
	}
}

// assign: pos[e / 64] = (number of CL_CONT entries before group e / 64, number of CL_SHADOW entries before it) + the block's bases; the
// totals become the next round's entry count and this round's shadow count.  Same shape as compact_body: a wave owns a
// contiguous range, counts it, the block reserves with one atomic per counter, then every fourth lane writes the bases of
// its group of 64 entries.  Blocks reserve in arrival order, so entry order is by block, in order within.
__global__ void __launch_bounds__(RT_COMPACT_BLOCK) k_assign(StreamState T, int round)
{
	const int parity = round & 1;
	__shared__ int waveC[RT_COMPACT_BLOCK / 64], waveS[RT_COMPACT_BLOCK / 64];
	__shared__ int baseC, baseS;
	const unsigned char* status = T.cls[parity];
	const int n = T.counts[SC_N + round % 3];
	const uint lane = threadIdx.x & 63;
	const int waves = (gridDim.x * blockDim.x) >> 6;
	const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	int per = (n + waves - 1) / waves;
	per = (per + 1023) & ~1023;
	const long long firstL = (long long)wave * per;
	const int first = firstL < n ? (int)firstL : n;
	const int last = firstL + per < n ? (int)(firstL + per) : n;
	int mineC = 0, mineS = 0;
	for (int s0 = first; s0 < last; s0 += 1024) {
		const uint4 v = status16(status, s0 + (int)lane * 16, last, (CL_CONT | CL_SHADOW) * 0x01010101u);
		const uint cm = CL_CONT * 0x01010101u, sm = CL_SHADOW * 0x01010101u;
		mineC += __popc(v.x & cm) + __popc(v.y & cm) + __popc(v.z & cm) + __popc(v.w & cm);
		mineS += __popc(v.x & sm) + __popc(v.y & sm) + __popc(v.z & sm) + __popc(v.w & sm);
	}
	int totC = mineC, totS = mineS;
	for (int o = 32; o > 0; o >>= 1) totC += __shfl_xor(totC, o), totS += __shfl_xor(totS, o);
	const int wib = threadIdx.x >> 6;
	if (lane == 0) waveC[wib] = totC, waveS[wib] = totS;
	__syncthreads();
	if (threadIdx.x == 0) {
		int sc = 0, ss = 0;
		for (int w = 0; w < RT_COMPACT_BLOCK / 64; w++) sc += waveC[w], ss += waveS[w];
		baseC = sc > 0 ? atomicAdd(&T.counts[SC_N + (round + 1) % 3], sc) : 0;
		baseS = ss > 0 ? atomicAdd(&T.counts[SC_SHADOW + round % 3], ss) : 0;
	}
	__syncthreads();
	int bc = baseC, bs = baseS;
	for (int w = 0; w < wib; w++) bc += waveC[w], bs += waveS[w];
	if (totC == 0) return; // no continuation in this wave's range: nobody reads its positions (CL_SHADOW implies CL_CONT)
	for (int s0 = first; s0 < last; s0 += 1024) {
		const int e0 = s0 + (int)lane * 16;
		const uint4 v = status16(status, e0, last, (CL_CONT | CL_SHADOW) * 0x01010101u);
		const uint cm = CL_CONT * 0x01010101u, sm = CL_SHADOW * 0x01010101u;
		const int cC = __popc(v.x & cm) + __popc(v.y & cm) + __popc(v.z & cm) + __popc(v.w & cm);
		const int cS = __popc(v.x & sm) + __popc(v.y & sm) + __popc(v.z & sm) + __popc(v.w & sm);
		int inC = cC, inS = cS;
		for (int o = 1; o < 64; o <<= 1) {
			const int tc = __shfl_up(inC, o), ts = __shfl_up(inS, o);
			if ((int)lane >= o) inC += tc, inS += ts;
		}
		// one pair of bases per GROUP of 64 entries (four lanes of this scan): a wave of the shading kernel holds exactly one group and
		// counts inside it with two ballots -- eight bytes per entry written here and read there otherwise (4.5 GB per bench step)
		const int pc = bc + inC - cC, ps = bs + inS - cS;
		if (e0 < last && (lane & 3) == 0) T.pos[e0 >> 6] = make_int2(pc, ps);
		bc += __shfl(inC, 63), bs += __shfl(inS, 63);
	}
}

// The shading kernels are bound by latency, not by HBM or the VALU (measured: waves waiting 66 % of the time, VALU pipes 30 %
// busy, 2.7 TB/s): a lane's chain is entry -> hit record -> material -> (next ray: brute-force primitive of the head
// candidate) -> sky texel, one memory round trip each.  The two tiny tables in that chain -- materials and the
// brute-force primitives -- are copied into LDS by every block (a ds_read instead of a trip to L2), and everything
// that does not depend on another load is issued before the first use.
#define RT_LDS_MATS 48   // materials / brute-force primitives a block keeps in LDS (scenes with more read them from memory)
#define RT_LDS_BRUTE 24
struct ShadeTables { uint mats[RT_LDS_MATS * 16]; float4 brute[RT_LDS_BRUTE * 4]; uint lights[RT_MAX_LIGHTS * (sizeof(DLight) / 4)]; };
__device__ __forceinline__ void load_tables(DScene& S, ShadeTables& L, int enable)
{
	const bool m = enable && S.nMats <= RT_LDS_MATS, b = enable && S.useTLAS && S.nBruteSph + S.nBrutePla <= RT_LDS_BRUTE && S.nBruteSph + S.nBrutePla > 0;
	const bool l = enable && S.nLights > 0 && S.nLights <= RT_MAX_LIGHTS; // the light loop of a diffuse hit reads every light's record: a round trip each otherwise
	if (m) for (int i = (int)threadIdx.x; i < S.nMats * 16; i += (int)blockDim.x) L.mats[i] = ((const uint*)S.mats)[i];
	if (b) for (int i = (int)threadIdx.x; i < (S.nBruteSph + S.nBrutePla) * 4; i += (int)blockDim.x) L.brute[i] = S.brute[i];
	if (l) for (int i = (int)threadIdx.x; i < S.nLights * (int)(sizeof(DLight) / 4); i += (int)blockDim.x) L.lights[i] = ((const uint*)S.lights)[i];
	if (m || b || l) __syncthreads();
	if (m) S.mats = (const DMaterial*)L.mats;
	if (b) S.brute = L.brute;
	if (l) S.lights = (const DLight*)L.lights;
}

// shade: everything Sample does at the hit of entry e except the occlusion-dependent direct terms (renderer.cpp:133-233).
// fresh: first segment of a sample (entry index = sample of the batch; W = 1, L = 0, E evaluated, nothing read).
#ifndef RT_SHADE_S_WAVES
#define RT_SHADE_S_WAVES 5
#endif
#ifndef RT_SHADE_Q_WAVES
#define RT_SHADE_Q_WAVES 5 // the Q-learning variant (it needs 117 VGPRs unbounded)
#endif
// QL: the indirect bounce of a diffuse hit is drawn from the Q table (rt_qlearn.h) and every hit pays its reward to the
// (cell, patch) that sent the ray; W.w of an entry carries that key (0: none).
// BOUNCE: round 0 of a batch whose bounce table is current.  The ray a GLASS or METAL hit scatters is then one the table has traced:
// the entry gets its hit from there, as from a producer that decided the ray, and never enters round 1's traversal queue.  The record
// is the one k_generate_t read for this sample; its index comes out of sample_primary_pixel, which this kernel runs anyway for the
// sample's seed (fresh_energy), so generate hands nothing over and stays as it is.  bounceMask (RT_BOUNCE_TABLE): bit 0 metal, bit 1 glass refraction, bit 2 glass reflection.
// TABLE0: round 0 of a batch whose generate was k_generate_c: no round-0 entry exists.  The hit is read from the sample's record of the
// primary table P (the index out of the same sample_primary_pixel call), O is the camera position and D the pinhole ray of the integer
// pixel: primary_ray_f on the ints k_primary_table and k_generate_t hand to primary_ray, so the bits are theirs.  The shadow record
// refers to the table record instead of the entry (shX.x: k_light_s TABLE0).  Always launched with round 0 and fresh set.
// CHAIN: a batch whose chain tables (ChainLevel) are current.  An entry answered from a record of level k carries that record's link as
// its key in W.w, which is free while the sampler is off (written 0 otherwise, and loaded by every later shade anyway); key 0: no table.
// With BOUNCE (round 0) the kernel only adds the key it read from the level-1 record.  Without (round r, 1 <= r < depth), Bt is level
// r + 1 with n = its capacity: a glass or metal hit of an entry with a key takes the child key - 1 + branch under the same mask bits, and a
// present child answers the ray as the bounce table does in round 0, its own link the new key; every other ray goes to emit_ray_s with key 0.
template <bool QL, bool BOUNCE = false, bool TABLE0 = false, bool CHAIN = false>
__global__ void __launch_bounds__(RT_BLOCK, QL ? RT_SHADE_Q_WAVES : RT_SHADE_S_WAVES) k_shade_s(DScene S0, DCamera C, RenderParams R, StreamState T, int round, int fresh, int last, int lastNext, int decide, int ldsTables, int counting, QTable Qt, BounceTable Bt, int bounceMask, PrimaryTable P)
{
	static_assert(!(QL && TABLE0), "the sampler's round 0 keeps its entries");
	static_assert(!(QL && CHAIN), "W.w is the sampler's key word");
	constexpr bool READ = CHAIN && !BOUNCE; // a round >= 1 that reads a chain level
	__shared__ ShadeTables tables;
	uint nDecided = 0;
	uint qOld = 0; // QL: the words this lane's rewards were added to, or-ed (q_reward: bit 31 = a count field past its limit)
	const int parity = round & 1;
	prepare_round(T, round + 1, -1);
	DScene S = S0;
	load_tables(S, tables, ldsTables);
	const int pout = 1 - parity;
	const int n = T.counts[SC_N + round % 3];
	const size_t cap = (size_t)T.cap;
	const int nIter = (n + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);
	for (int it = 0; it < nIter; it++) {
		const int e = it * (int)(gridDim.x * blockDim.x) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
		// after round 0 every entry is live: all of an entry's loads go out together, the class byte among them (round 0
		// looks at the class first: the entries of samples finished by generate hold nothing, and they come in long runs)
		const bool spec = !TABLE0 && !fresh && e < n;
		float4 o4, d4, hn, e4, w4, l4;
		int2 id;
		const int2 grp = e < n ? T.pos[e >> 6] : make_int2(0, 0); // the bases of this wave's group of 64 entries (k_assign); the same for every lane that has an entry (the grid's last iteration reaches past n, and past pos[])
		if (spec) {
			o4 = T.O[parity][e], d4 = T.D[parity][e], hn = T.hitN[parity][e], id = T.hitId[parity][e];
			e4 = T.E[parity][e], w4 = T.W[parity][e], l4 = T.L[parity][e];
		}
		const unsigned char c = e < n ? T.cls[parity][e] : 0;
		// the entry's place in the next round and its shadow record: the group's bases + the entries before it in the wave that want one
		int2 p;
		{
			const unsigned long long mC = __ballot((c & CL_CONT) != 0), mS = __ballot((c & CL_SHADOW) != 0);
			p.x = grp.x + (int)__builtin_amdgcn_mbcnt_hi((uint)(mC >> 32), __builtin_amdgcn_mbcnt_lo((uint)mC, 0u));
			p.y = grp.y + (int)__builtin_amdgcn_mbcnt_hi((uint)(mS >> 32), __builtin_amdgcn_mbcnt_lo((uint)mS, 0u));
		}
		if (c & CL_LIVE) {
			int primaryRec = -1; // BOUNCE, TABLE0: the sample's record of the primary table
			if constexpr (TABLE0) {
				int px, py;
				uint s0;
				sample_primary_pixel(C, R, R.sampleFirst + (uint)e, px, py, s0);
				primaryRec = (px + 1) + (py + 1) * P.w;
				RT_CHECK(fresh && round == 0 && primaryRec >= 0 && primaryRec < P.w * P.h && (!BOUNCE || (Bt.w == P.w && Bt.n == P.w * P.h)), 28, &T.counts[SC_FLAG]);
				hn = P.A[primaryRec];
				id = *(const int2*)(P.B + primaryRec); // x objIdx, y material
				f3 o, d;
				primary_ray_f(C, (float)px, (float)py, o, d);
				o4 = mk4(o, 0.0f), d4 = mk4(d, 0.0f);
				e4 = make_float4(1, 1, 1, __uint_as_float(s0));
				w4 = make_float4(1, 1, 1, 0);
				l4 = make_float4(0, 0, 0, __uint_as_float(R.sampleFirst + (uint)e));
			} else if (!spec) {
				o4 = T.O[parity][e], d4 = T.D[parity][e], hn = T.hitN[parity][e], id = T.hitId[parity][e];
				if constexpr (BOUNCE) {
					int px, py;
					uint s0;
					sample_primary_pixel(C, R, R.sampleFirst + (uint)e, px, py, s0); // fresh_energy's seed of such a batch, and the pixel on the way
					e4 = make_float4(1, 1, 1, __uint_as_float(s0));
					primaryRec = (px + 1) + (py + 1) * Bt.w;
				} else e4 = fresh_energy(C, R, R.sampleFirst + (uint)e);
				w4 = make_float4(1, 1, 1, 0);
				l4 = make_float4(0, 0, 0, __uint_as_float(R.sampleFirst + (uint)e));
			}
			RT_CHECK(!(c & CL_CONT) || (p.x >= 0 && p.x < T.cap && p.y >= 0 && p.y < T.cap), 21, &T.counts[SC_FLAG]);
			const f3 O = xyz(o4), D = xyz(d4), normal = xyz(hn);
			const float t = hn.w;
			f3 W = xyz(w4), E = xyz(e4), Lsum = xyz(l4);
			uint seed = __float_as_uint(e4.w), shadowSeed = 0;
			const f3 I = O + t * D; // ray.IntersectionPoint()
			const bool childTraces = !last; // Sample(depth - 1 < 0) = 0.05 (renderer.cpp:129)
			bool segmentEnds = true, wantShadow = false;
			f3 nO(0.0f), nD(0.0f), nW(0.0f);
			uint nextKey = 0;       // QL: (cell, patch) + 1 of the ray this hit scatters
			bool deadSample = false; // QL: the guided direction points below the surface: nothing to trace
			int bounceRec = -1;      // BOUNCE: the bounce table's record of the scattered ray; READ: the chain level's
			const int chainKey = READ && !fresh ? __float_as_int(w4.w) : 0; // READ: the link of the record this entry's hit came from
			// QL: the key word travels in W.w: bits 0-30 the (cell, patch) + 1 that sent this ray, bit 31 "this sample pays rewards"
			const uint keyWord = QL ? (fresh ? (((__float_as_uint(e4.w) & Qt.learnMask) == 0) ? RT_Q_LEARNER : 0u) : __float_as_uint(w4.w)) : 0u;
			const bool learner = (keyWord & RT_Q_LEARNER) != 0;
			const uint prevKey = learner ? (keyWord & ~RT_Q_LEARNER) : 0u;

			f3 term;
			if (terminal_radiance(S, id.x, I, normal, D, term)) {
				Lsum = Lsum + W * term; // renderer.cpp:134-137
				if (QL && prevKey) qOld |= q_reward(Qt, prevKey, q_lum(term));
			} else {
				const DMaterial m = S.mats[id.y];
				const f3 col(m.col[0], m.col[1], m.col[2]);
				if (QL && prevKey) {
					const bool dif = m.type != 3 && m.type != 2;
					const f3 albedoQ(m.albedo[0], m.albedo[1], m.albedo[2]);
					qOld |= q_reward(Qt, prevKey, q_expected(Qt, q_cell(Qt, I), normal, dif ? q_lum(col * albedoQ) : q_lum(col), dif));
				}
				if (m.type == 3) { // GLASS, renderer.cpp:198-233
					const GlassHit g = glass_hit(m, D, normal, t, E);
					if (g.kr < RandomFloat(seed)) {
						glass_refracted(g, m, I, D, W, E, nO, nD, nW);
						if (BOUNCE && (bounceMask & 2)) bounceRec = primaryRec;
						if (READ && (bounceMask & 2) && chainKey > 0) bounceRec = chainKey - 1;
					} else {
						glass_reflected(g, m, I, D, W, nO, nD, nW);
						if (BOUNCE && (bounceMask & 4)) bounceRec = primaryRec + Bt.n;
						if (READ && (bounceMask & 4) && chainKey > 0) bounceRec = chainKey;
					}
					if (childTraces) segmentEnds = false;
					else Lsum = Lsum + untraced_child(nW);
				} else if (m.type == 2) { // METAL, renderer.cpp:192-197
					metal_bounce(true, col, I, D, normal, W, E, nO, nD, nW);
					if (BOUNCE && (bounceMask & 1)) bounceRec = primaryRec;
					if (READ && (bounceMask & 1) && chainKey > 0) bounceRec = chainKey - 1;
					if (childTraces) segmentEnds = false;
					else Lsum = Lsum + untraced_child(nW);
				} else { // DIFFUSE, renderer.cpp:156-191
					wantShadow = S.nLights > 0;
					shadowSeed = seed; // light draws the light positions again from here
					for (int i = 0; i < S.nLights; i++) {
						const f3 pickedPos = light_position(S.lights[i], false, seed);
						T.shP[(size_t)i * cap + (size_t)p.y] = mk4(pickedPos, 0.0f); // connect's
					}
					const f3 albedo(m.albedo[0], m.albedo[1], m.albedo[2]);
					if constexpr (QL) {
						// the scattered direction from the Q table of this cell instead of the uniform hemisphere
						float P;
						int patch;
						const int cell = q_cell(Qt, I);
						const f3 dirQ = q_sample(Qt, cell, seed, P, patch);
						const float c = dot(dirQ, normal);
						nO = I, nD = dirQ;
						if (c > 0) {
							const f3 cos_i(c);
							nW = W * (((1.0f / (16.0f * P)) * (col * cos_i)) * albedo); // 1 / (pi pdf) in the place of the uniform hemisphere's 2
							nextKey = learner ? 1u + (uint)cell * RT_Q_PATCHES + (uint)patch : 0u;
						} else {
							deadSample = true; // below the surface: the patch learns a reward of 0, the path carries no weight on
							if (learner) qOld |= q_reward(Qt, 1u + (uint)cell * RT_Q_PATCHES + (uint)patch, 0.0f);
						}
					} else {
						nO = I;
						hemisphere_bounce(seed, normal, col, albedo, W, nD, nW);
					}
					if (childTraces) segmentEnds = false;
					else Lsum = Lsum + untraced_child(nW);
				}
			}
			// the class byte promised exactly these outputs
			RT_CHECK(((c & CL_SHADOW) != 0) == wantShadow && ((c & CL_CONT) != 0) == (!segmentEnds || wantShadow), 22, &T.counts[SC_FLAG]);
			if (wantShadow) {
				T.shI[p.y] = mk4(I, __uint_as_float(shadowSeed));
				T.shX[p.y] = make_int2(TABLE0 ? primaryRec : e, p.x);
			}
			if (!segmentEnds || wantShadow) {
				T.E[pout][p.x] = mk4(E, __uint_as_float(seed));
				T.L[pout][p.x] = mk4(Lsum, l4.w);
				if (!segmentEnds && deadSample) {
					// the entry the class byte promised, as a ray that hits nothing and weighs nothing: the next shade adds 0 and ends it
					T.O[pout][p.x] = mk4(nO, 1e34f), T.D[pout][p.x] = mk4(nD, 0.0f);
					T.hitN[pout][p.x] = make_float4(0, 0, 0, 1e34f), T.hitId[pout][p.x] = make_int2(-1, -1);
					T.W[pout][p.x] = make_float4(0, 0, 0, 0);
					T.cls[pout][p.x] = CL_LIVE;
				} else if (!segmentEnds) {
					int4 bb = make_int4(0, 0, 0, 0);
					if constexpr (BOUNCE) {
						RT_CHECK(fresh && primaryRec >= 0 && primaryRec < Bt.n && bounceRec < 2 * Bt.n, 27, &T.counts[SC_FLAG]);
						if (primaryRec >= 0 && primaryRec < Bt.n && bounceRec >= 0) bb = Bt.B[bounceRec]; // (bounceRec is primaryRec or primaryRec + n)
					} else if constexpr (READ) {
						RT_CHECK(!fresh && round > 0 && bounceRec < Bt.n, 30, &T.counts[SC_FLAG]);
						if (bounceRec >= 0 && bounceRec < Bt.n) bb = Bt.B[bounceRec];
					}
					if ((BOUNCE || READ) && (bb.z & BT_PRESENT)) {
						// what emit_ray_s writes for a ray it decided
						const float4 ba = Bt.A[bounceRec];
						T.hitN[pout][p.x] = ba;
						T.hitId[pout][p.x] = make_int2(bb.x, bb.y);
						T.O[pout][p.x] = mk4(nO, ba.w), T.D[pout][p.x] = mk4(nD, 0.0f); // (w: extend's, which never sees this entry)
						T.W[pout][p.x] = mk4(nW, CHAIN ? __int_as_float(bb.w) : __uint_as_float(nextKey | (keyWord & RT_Q_LEARNER)));
						T.cls[pout][p.x] = (unsigned char)(CL_LIVE | ((lastNext ? bb.z >> 4 : bb.z) & 15));
						nDecided++;
					} else {
						const NewRay nr = emit_ray_s(S, T, pout, p.x, nO, nD, mode_t_min(1), lastNext, false, decide != 0);
						T.W[pout][p.x] = mk4(nW, __uint_as_float(nextKey | (keyWord & RT_Q_LEARNER)));
						T.cls[pout][p.x] = nr.cls;
						nDecided += nr.decided ? 1u : 0u;
					}
				}
			} else store_sample(R, __float_as_uint(l4.w), Lsum);
		}
	}
	if (QL && (qOld >> 31)) *Qt.ovf = 1;
	if (counting) flush_decided(T.counts, nDecided);
}

// connect: Scene::IsOccluded from the hit point towards each sampled light position (renderer.cpp:161-165).
// Work item = light * nShadow + shadow record: consecutive items read consecutive records and aim at the same light.
struct StreamConnectPolicy {
	const StreamState& T;
	int nShadow;
	int* flag;
	__device__ __forceinline__ bool load(int work, f3& O, f3& D, float& tmax, HitRef&) const
	{
		const int li = work / nShadow, s = work - li * nShadow;
		RT_CHECK(s >= 0 && s < T.cap && li >= 0 && li < RT_MAX_LIGHTS, 23, flag);
		const f3 I = xyz(ld_stream(T.shI + s));
		const f3 pickedPos = xyz(ld_stream(T.shP + ((size_t)li * (size_t)T.cap + (size_t)s)));
		shadow_ray(I, pickedPos, O, D, tmax);
		return true;
	}
	__device__ __forceinline__ void store(int work, bool occluded) const
	{
		const int li = work / nShadow, s = work - li * nShadow;
		st_stream(T.vis + ((size_t)li * (size_t)T.cap + (size_t)s), (unsigned char)(occluded ? 1 : 0));
	}
	__device__ __forceinline__ void leftover(int work) const { T.leftover[atomicAdd(&T.counts[SC_LEFTOVER], 1)] = (uint)work; }
};
template <bool COUNT, bool WIDE = false, bool LISTED = false, bool WIDE8 = false>
__global__ void __launch_bounds__(RT_BLOCK, RT_CONNECT_WAVES) k_connect_s(DScene S, StreamState T, int round, int tuning, uint* spill, DCounters* counters)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	const int nShadow = T.counts[SC_SHADOW + round % 3];
	StreamConnectPolicy pol{ T, nShadow > 0 ? nShadow : 1, &T.counts[SC_FLAG] };
	int* heads = T.heads + RT_HEADS * RT_HEAD_STRIDE;
	if constexpr (LISTED) {
		ListedPolicy<StreamConnectPolicy> lp{ pol, T.leftover };
		trace_persistent<true, COUNT, false, ListedPolicy<StreamConnectPolicy>>(S, lp, T.counts[SC_LEFTOVER], heads, 0.0f, tuning, ldsStack, spill, &T.counts[SC_FLAG], lc, rays);
	} else
		trace_persistent<true, COUNT, false, StreamConnectPolicy, false, WIDE8 ? 8 : (WIDE ? 4 : 2)>(S, pol, nShadow * S.nLights, heads, 0.0f, tuning, ldsStack, spill, &T.counts[SC_FLAG], lc, rays);
	if (COUNT) flush_counters(counters, lc, 0, rays);
}

// traverse: extend of round r and connect of round r - 1 as ONE persistent launch over one work list (RT_FUSE=1): items
// [0, nTrace) are the traversal queue's rays (nearest hit: the long ones start first), the rest the shadow rays of the round
// before, light-major.  A lane's kind of query follows its work item (trace_persistent MIXED).  One launch has one drain where
// two have two, which is most of what a small batch's traversal costs (profiles/r03_ab_stream_fuse.txt: at the 1/8 frame an
// extend launch is busy 0.2-0.8 ms and drains for 0.5-0.7); at large batches waves that mix the two kinds cost more than the
// drains return (DESIGN.md finding 19), so this is the small batches' round loop.
struct StreamTraversePolicy {
	StreamExtendPolicy ext;
	StreamConnectPolicy con;
	int nTrace;
	__device__ __forceinline__ bool any_of(int work) const { return work >= nTrace; }
	__device__ __forceinline__ bool load(int work, f3& O, f3& D, float& tmax, HitRef& head) const
	{
		if (work < nTrace) return ext.load(work, O, D, tmax, head);
		return con.load(work - nTrace, O, D, tmax, head);
	}
	__device__ __forceinline__ void store(int work, const HitRef& hit, const f3& O, const f3& D) const { ext.store(work, hit, O, D); }
	__device__ __forceinline__ void store(int work, bool occluded) const { con.store(work - nTrace, occluded); }
};
__global__ void __launch_bounds__(RT_BLOCK, RT_TRAVERSE_WAVES) k_traverse_s(DScene S, StreamState T, int round, int last, float t_min, int tuning, uint* spill)
{
	__shared__ __attribute__((aligned(16))) uint ldsStack[RT_LDS_WORDS];
	LaneCounters lc;
	lc.clear();
	uint rays = 0;
	const int nTrace = T.counts[SC_TRACE], nShadow = T.counts[SC_SHADOW + (round + 2) % 3]; // the shadow records of round - 1
	StreamTraversePolicy pol{ { S, T, round & 1, last, &T.counts[SC_FLAG] }, { T, nShadow > 0 ? nShadow : 1, &T.counts[SC_FLAG] }, nTrace };
	trace_persistent<false, false, false, StreamTraversePolicy, true>(S, pol, nTrace + nShadow * S.nLights, T.heads, t_min, tuning, ldsStack, spill, &T.counts[SC_FLAG], lc, rays);
}

// light: the direct-light terms of a diffuse hit, in light order (renderer.cpp:158-176: occlusion test first, scatter
// only when visible), added to the radiance of the path's continuation entry; in the last round the sample is complete.
// TABLE0: light(0) behind a shade(0) that read the primary table: shX.x is the table record, the normal and the material are its
// fields and D the pinhole ray of its pixel (TablePolicy::ray's ints); W stays 1.
template <bool TABLE0>
__global__ void RT_LIGHT_BOUNDS k_light_s(DScene S0, RenderParams R, StreamState T, int round, int last, int ldsTables, DCamera C, PrimaryTable P)
{
	__shared__ ShadeTables tables;
	DScene S = S0;
	load_tables(S, tables, ldsTables);
	const int p = round & 1, pout = 1 - p;
	const int n = T.counts[SC_SHADOW + round % 3];
	const size_t cap = (size_t)T.cap;
	for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
		const float4 i4 = T.shI[s];
		const int2 x = T.shX[s];
		const int e = x.x, cp = x.y;
		RT_CHECK(e >= 0 && e < (TABLE0 ? P.w * P.h : T.cap) && cp >= 0 && cp < T.cap && (!TABLE0 || round == 0), 24, &T.counts[SC_FLAG]);
		// the hit's own fields from entry e of this round (shade(round + 1) has not run yet); a round-0 entry has no W: shade took 1 (fresh)
		float4 n4, d4;
		int mat;
		if constexpr (TABLE0) {
			n4 = P.A[e];
			mat = P.B[e].y;
			f3 o, d;
			primary_ray_f(C, (float)(e % P.w - 1), (float)(e / P.w - 1), o, d);
			d4 = mk4(d, 0.0f);
		} else n4 = T.hitN[p][e], d4 = T.D[p][e], mat = T.hitId[p][e].y;
		const f3 W = TABLE0 || round == 0 ? f3(1.0f) : xyz(T.W[p][e]);
		const float4 e4 = T.E[pout][cp], l4 = T.L[pout][cp];
		const f3 I = xyz(i4), normal = xyz(n4), D = xyz(d4);
		f3 E = xyz(e4), Lsum = xyz(l4);
		uint seed = __float_as_uint(i4.w); // shade's light loop, replayed
		const DMaterial m = S.mats[mat];
		const f3 col(m.col[0], m.col[1], m.col[2]);
		f3 direct(0.0f);
		for (int i = 0; i < S.nLights; i++) {
			const f3 pickedPos = light_position(S.lights[i], false, seed);
			const f3 lightRayDirection = normalize(pickedPos - I);
			if (T.vis[(size_t)i * cap + (size_t)s] != 0) continue;
			const f3 att = diffuse_scatter(m, D, lightRayDirection, light_intensity(S.lights[i], I, normal, pickedPos), normal, E);
			direct = direct + direct_term(m, col, att, E);
		}
		const f3 albedo(m.albedo[0], m.albedo[1], m.albedo[2]);
		Lsum = Lsum + W * path_direct(direct, albedo);
		if (last) store_sample(R, __float_as_uint(l4.w), Lsum);
		else {
			if (E.x != e4.x || E.y != e4.y || E.z != e4.z) T.E[pout][cp] = mk4(E, e4.w);
			if (Lsum.x != l4.x || Lsum.y != l4.y || Lsum.z != l4.z) T.L[pout][cp] = mk4(Lsum, l4.w);
		}
	}
}

} // namespace rtd
