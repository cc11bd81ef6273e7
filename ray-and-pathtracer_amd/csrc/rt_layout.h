// The HBM scene layout as a value, built on the host: everything rt_upload_scene (rt_api_upload.inc) copies to the device and every guarantee the
// traversal kernels of rt_scene_dev.h rely on -- nested boxes for the 4-wide walk, outward-rounded 8-wide boxes, reach[] margins, the last bits
// that let one dword name a leaf, the refit level order, the split of a block's LDS.  Host arithmetic on std::vectors only: no hip* call, no rt_ctx;
// build_layout is also what the device-free rt_layout_* entry points of include/rt_amd.h return (tests/test_layout_cpu.py).
//
// Layout (built by rt_upload_scene from the reference-shaped arrays of include/rt_amd.h):
//   pairs[]  one 64-byte record per sibling pair of BLAS nodes (the reference allocates children
//            in adjacent slots, bvh.cpp:318-319, so one inner-node visit reads exactly one record):
//              float4 {minA.xyz, linkA} {maxA.xyz, -} {minB.xyz, linkB} {maxB.xyz, -}
//            link = LEAF_BIT | first primitive slot   (leaf)
//                 = pair index of the children          (inner)
//            A lane's fetch is one aligned half cache line; a component-wise SoA would touch
//            eight lines for the same visit (gather access, not streaming).
//   prims[]  one 64-byte record per leaf slot, in leaf order (primitiveIdx already applied):
//              tri    {v0.xyz, N.x} {v1.xyz, N.y} {v2.xyz, N.z} {d, objIdx, mat, kind|last}
//              sphere {pos.xyz, r2} {invr, r, -, -} {-}          {-, objIdx, mat, kind|last}
//              plane  {N.xyz, d}    {-}            {-}          {-, objIdx, mat, kind|last}
//            'last' marks the final slot of a leaf, so a leaf is named by its first slot alone and
//            a stack entry is one dword.
//            TLAS inner nodes (tlas.h:4-11) are stored in the same form (children boxes inside the
//            parent's record, link = pair index or INST_BIT | instance), so one piece of code walks both
//            levels; tlas::Intersect tests child (leftRight & 0xFFFF) first, which is slot A here.
//   inst[]   128-byte records: invTransform rows 0-2, matTransform rows 0-2, root link.
//   reach[]  one 48-byte record per TLAS pair, beside pairs[]: {minA.xyz, maxA.x}{maxA.yz, minB.xy}{minB.z, maxB.xyz}.
//            The reference's instance bounds are the union of the BLAS's LOCAL box and its transformed
//            box (bvhInstance.h:15-30 never resets 'bounds'), so TLAS boxes overlap nearly everywhere and
//            a ray enters almost every instance only to fail the first BLAS test.  reach holds, per child,
//            the world box of what the subtree can really contain: the corners of (BLAS root's two child
//            boxes) under the exact inverse of invTransform, evaluated in double at upload, inflated by
//            a margin m = a + b * reachOriginMax that covers the float rounding of the object-space ray
//            (~500 ulps of the magnitudes involved, scaled by the transform's condition number) for every
//            ray whose world origin has |O|_1 <= reachOriginMax (64 x the extent of the instanced geometry;
//            rays from further away are not culled).  A child whose
//            inflated reach box the ray misses cannot yield a hit and is dropped; the ORDER in which the
//            remaining children are visited still comes from the reference's boxes, so the first-found
//            rule for equal t is untouched and results are identical.  Counting launches either walk like
//            the reference (no culling: the counters are the reference's tallies) or like the timed
//            kernels (RT_TUNE_CULL_COUNTED: the counters are the work actually done).
//   wide[]   4-wide nodes for occlusion queries (the reference's own 4-wide variant is bvh.cpp:335-512,
//            :658-761).  One 128-byte record = one cache line: {min.x[4]}{min.y[4]}{min.z[4]}{max.x[4]}{max.y[4]}{max.z[4]}
//            {link[4]}{source[4]}; built at upload by collapsing the reference's binary tree (a node's children are
//            expanded, largest surface first, until there are four); a child entry carries the binary node's OWN box,
//            an unused entry an inverted box.  Why this is exact for Scene::IsOccluded: the answer is "some primitive of
//            some visited leaf occludes", a leaf is visited by the reference iff every binary ancestor's box passes
//            the slab test, and for a ray that cannot produce a NaN slab product (ray_is_clean) a box that passes
//            implies every box CONTAINING it passes (rounding is monotone: (b - O) * rD keeps the order of the b's), so
//            with nested boxes -- checked at upload, parents are unions of their children after bvh::Refit -- the
//            visited leaves are exactly those whose own box passes, whichever ancestors a walk tests on the way.  Order
//            is free (a boolean).  Rays that are not clean, in world or in an instance's object space, are handed to the
//            binary walk (leftover list).  Half as many dependent fetches per ray, and each fetch is one L1 line.
//   wide8[]  8-wide nodes with QUANTISED child boxes, the re-thought form of the reference's QBVH, for occlusion
//            queries.  One 128-byte record (96 used, six dwordx4): {origin.xyz, exponents} {qlo.x[8] qlo.y[8]} {qlo.z[8] qhi.x[8]}
//            {qhi.y[8] qhi.z[8]} {link[0..3]} {link[4..7]}; a child's box is origin + q * 2^e per axis (one fma, the expression
//            the builder checked), rounded OUTWARDS at upload so that it contains the binary node's box it stands for; built
//            by collapsing the reference's binary tree (largest surface first, up to eight children).  Exactness: the argument
//            of wide[] needs the boxes a walk tests on the way to a leaf only to CONTAIN the leaf's own box (for a clean ray a
//            box that passes implies every box containing it passes), and the leaf's own, exact box to decide whether the leaf
//            is visited.  So inner entries may be quantised as long as they contain, and a leaf entry names a leafBox[] record
//            -- the reference's exact box + the first primitive slot -- that is tested (exact slab test) before any primitive:
//            visited leaves are exactly those whose own box passes, as in bvh::BIsOccluded.  A third of the dependent fetches
//            of the binary walk, half its load instructions per ray.
// All of it is read-only and a few MB at most: every XCD's 4 MiB L2 ends up holding its own copy.
// All of it is read-only and a few MB at most: every XCD's 4 MiB L2 ends up holding its own copy.
#pragma once
#include "../../include/rt_amd.h"
#include "rt_scene_dev.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace rtd;

// the three knobs (rt_ctx.h Knobs) the layout depends on
struct LayoutKnobs {
	int wide = -1;  // RT_WIDE: -1 on for a scene BVH and off with a TLAS, 0 / 1 forced
	int wide8 = 0;  // RT_WIDE8
	int tlasLds = 1; // RT_TLAS_LDS
};

struct SceneLayout {
	// device arrays, as they are copied (reach and brute carry their slack words themselves)
	std::vector<float> pairs, prims, wide, leafBox, reach, brute;
	std::vector<uint> wide8; // 32 uints per node
	std::vector<DInstance> inst;
	std::vector<DLight> lights;
	std::vector<DMaterial> mats;
	std::vector<uint> refitOrder;
	std::vector<int> refitLevelStart;
	// per BLAS: its root as a pair link, through the 4-wide nodes, through the 8-wide nodes
	std::vector<uint> rootLink, rootWide, rootWide8;
	// DScene / context scalars (in the order of RT_LAYOUT_SCALARS, include/rt_amd.h)
	uint root = RT_EMPTY; // DScene::rootLink: the scene BVH's root, or the TLAS root
	uint tlasBase = 0;
	int tlasPairs = 0, nInst = 0;
	float reachOriginMax = 0;
	int tlasLds = 0, stackRows = RT_STACK_ROWS_MAX;
	int nBruteSph = 0, nBrutePla = 0;
	bool wideOK = false, wide8OK = false;
	bool pathUnsupported = false;
	std::string pathUnsupportedWhy;
	int animSlots = 0, refitLevels = 0;
};

static int layout_fail(std::string& err, int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	err = buf;
	return code;
}

// ---- the description as a whole: what is refused before anything is built ---------------------------
static int check_desc(const rt_scene_desc* d, std::string& err)
{
	if (d->n_lights > RT_MAX_LIGHTS) return layout_fail(err, RT_E_UNSUPPORTED, "rt_upload_scene: %u lights (limit %d)", d->n_lights, RT_MAX_LIGHTS);
	if (d->n_blas < 1 || !d->blas) return layout_fail(err, RT_E_ARG, "rt_upload_scene: no bvh");
	if (d->use_tlas && (d->n_instances < 1 || d->n_instances > 256 || !d->tlas_nodes)) return layout_fail(err, RT_E_UNSUPPORTED, "rt_upload_scene: TLAS needs 1..256 instances (nodeIdx[256], tlas.cpp:16)");
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		if (m.type < 1 || m.type > 3) return layout_fail(err, RT_E_ARG, "rt_upload_scene: material %u has type %d", i, m.type);
	}
	return RT_OK;
}
static void check_path_support(const rt_scene_desc* d, SceneLayout& L)
{
	L.pathUnsupported = false;
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		if (m.type == RT_MAT_DIFFUSE && (m.shinieness != 0 || m.raytracer == 0)) {
			L.pathUnsupported = true;
			L.pathUnsupportedWhy = m.shinieness != 0 ? "a diffuse material has shinieness != 0" : "a diffuse material was built with raytracer == 0";
		}
	}
}

// ---- pair and primitive records ----------------------------------------------------------------------
// matTypes: rt_material::type per material (null: none known); the type of the primitive's material rides in bits 4-5 of the
// record's kind word, so that the kernel that resolves a hit knows what the hit means for the path without a second fetch
static void pack_prim(float* rec, const rt_blas& b, uint p, bool last, const rt_material* mats = nullptr, uint nMats = 0)
{
	memset(rec, 0, 64);
	int kind, obj, mat;
	if (p < b.n_tri) {
		const rt_triangle& t = b.tris[p];
		rec[0] = t.v0[0], rec[1] = t.v0[1], rec[2] = t.v0[2], rec[3] = t.N[0];
		rec[4] = t.v1[0], rec[5] = t.v1[1], rec[6] = t.v1[2], rec[7] = t.N[1];
		rec[8] = t.v2[0], rec[9] = t.v2[1], rec[10] = t.v2[2], rec[11] = t.N[2];
		// float d = -dot(N, v0) (template/scene.h:193), same expression tree as the per-ray evaluation
		volatile float p0 = t.N[0] * t.v0[0], p1 = t.N[1] * t.v0[1], p2 = t.N[2] * t.v0[2];
		volatile float s01 = p0 + p1;
		volatile float s = s01 + p2;
		rec[12] = -s;
		kind = RT_KIND_TRI, obj = t.obj_idx, mat = t.material;
	} else if (p < b.n_tri + b.n_sph) {
		const rt_sphere& s = b.spheres[p - b.n_tri];
		rec[0] = s.pos[0], rec[1] = s.pos[1], rec[2] = s.pos[2], rec[3] = s.r2;
		rec[4] = s.invr, rec[5] = s.r;
		kind = RT_KIND_SPHERE, obj = s.obj_idx, mat = s.material;
	} else {
		const rt_plane& q = b.planes[p - b.n_tri - b.n_sph];
		rec[0] = q.N[0], rec[1] = q.N[1], rec[2] = q.N[2], rec[3] = q.d;
		kind = RT_KIND_PLANE, obj = q.obj_idx, mat = q.material;
	}
	int kl = kind | (last ? RT_LAST_BIT : 0);
	if (mats && mat >= 0 && (uint)mat < nMats) kl |= (mats[mat].type & 3) << RT_TYPE_SHIFT;
	memcpy(rec + 13, &obj, 4), memcpy(rec + 14, &mat, 4), memcpy(rec + 15, &kl, 4);
}

// pairs + prims of BLAS k, appended; pairOffOf[k]: its first pair record
static int pack_blas(const rt_scene_desc* d, uint k, SceneLayout& L, std::vector<uint>& pairOffOf, std::string& err)
{
	std::vector<float>&pairs = L.pairs, &prims = L.prims;
	const rt_blas& b = d->blas[k];
	if (b.nodes_used < 1 || (b.nodes_used & 1) || !b.nodes) return layout_fail(err, RT_E_ARG, "rt_upload_scene: blas %u has %u nodes (expected an even count >= 2)", k, b.nodes_used);
	if (b.n_prims != b.n_tri + b.n_sph + b.n_pla) return layout_fail(err, RT_E_ARG, "rt_upload_scene: blas %u primitive counts disagree", k);
	// an instanced BLAS is a mesh (bvh(Mesh*), bvh.cpp:5-16): the instance path resolves triangle normals only
	// (bvhInstance.cpp:19), so spheres / planes below an instance are refused rather than shaded wrongly
	if (d->use_tlas && (b.n_sph > 0 || b.n_pla > 0)) return layout_fail(err, RT_E_UNSUPPORTED, "rt_upload_scene: blas %u holds spheres / planes; an instanced BLAS must be triangles only", k);
	// node boxes must be numbers within the reference's +-1e30 sentinels (bvh.cpp:96-109): the hardware min / max
	// slab test of clean rays relies on it
	for (uint i = 0; i < b.nodes_used && b.n_prims > 0; i++) {
		if (i == 1) continue;
		for (int a = 0; a < 3; a++)
			if (!(std::fabs(b.nodes[i].aabb_min[a]) <= 1e30f) || !(std::fabs(b.nodes[i].aabb_max[a]) <= 1e30f))
				return layout_fail(err, RT_E_UNSUPPORTED, "rt_upload_scene: blas %u node %u has a non-finite bound or one beyond 1e30", k, i);
	}
	const uint pairOff = (uint)(pairs.size() / 16), primOff = (uint)(prims.size() / 16);
	pairOffOf[k] = pairOff;
	std::vector<char> last(b.n_prims, 0);
	auto link_of = [&](uint i) -> uint {
		const rt_bvh_node& nd = b.nodes[i];
		if (nd.prim_count > 0) return RT_LEAF_BIT | (primOff + nd.left_first);
		return pairOff + nd.left_first / 2;
	};
	for (uint i = 0; i < b.nodes_used; i++) {
		if (i == 1) continue;
		const rt_bvh_node& nd = b.nodes[i];
		if (nd.prim_count > 0) {
			if (nd.left_first + nd.prim_count > b.n_prims) return layout_fail(err, RT_E_ARG, "rt_upload_scene: blas %u node %u leaf range out of bounds", k, i);
			last[nd.left_first + nd.prim_count - 1] = 1;
		} else if (b.n_prims > 0 && ((nd.left_first & 1) || nd.left_first < 2 || nd.left_first + 1 >= b.nodes_used)) {
			return layout_fail(err, RT_E_ARG, "rt_upload_scene: blas %u node %u child index %u invalid", k, i, nd.left_first);
		}
	}
	L.rootLink[k] = b.n_prims == 0 ? RT_EMPTY : link_of(0);
	pairs.resize(pairs.size() + (size_t)(b.nodes_used / 2) * 16, 0.0f);
	for (uint i = 2; i + 1 < b.nodes_used + 0u && b.n_prims > 0; i += 2) {
		float* rec = &pairs[(size_t)(pairOff + i / 2) * 16];
		for (int s = 0; s < 2; s++) {
			const rt_bvh_node& nd = b.nodes[i + s];
			uint lk = link_of(i + s);
			memcpy(rec + 8 * s, nd.aabb_min, 12), memcpy(rec + 8 * s + 3, &lk, 4);
			memcpy(rec + 8 * s + 4, nd.aabb_max, 12);
		}
	}
	prims.resize(prims.size() + (size_t)b.n_prims * 16);
	for (uint j = 0; j < b.n_prims; j++) {
		const uint p = b.prim_idx[j];
		if (p >= b.n_prims) return layout_fail(err, RT_E_ARG, "rt_upload_scene: blas %u prim_idx[%u] = %u out of range", k, j, p);
		pack_prim(&prims[(size_t)(primOff + j) * 16], b, p, last[j] != 0, d->materials, d->n_materials);
	}
	return RT_OK;
}

// ---- the wide collapse: 4-wide and 8-wide nodes from the binary trees --------------------------------
// nested?  (parents are unions of their children after bvh::Refit, bvh.cpp:556-594)  bounded: every box is also finite and not inverted
// (outward rounding needs finite boxes; a plane's +-1e30 slab has no useful grid)
static bool tree_nested(const rt_blas& b, bool bounded)
{
	bool ok = true;
	for (uint i = 0; i < b.nodes_used && ok; i++) {
		if (i == 1) continue;
		for (int a = 0; a < 3 && bounded; a++)
			if (!(fabsf(b.nodes[i].aabb_min[a]) < 1e29f) || !(fabsf(b.nodes[i].aabb_max[a]) < 1e29f) || !(b.nodes[i].aabb_min[a] <= b.nodes[i].aabb_max[a])) ok = false;
		if (b.nodes[i].prim_count > 0) continue;
		for (uint ci = b.nodes[i].left_first; ci < b.nodes[i].left_first + 2; ci++)
			for (int a = 0; a < 3; a++)
				if (!(b.nodes[ci].aabb_min[a] >= b.nodes[i].aabb_min[a]) || !(b.nodes[ci].aabb_max[a] <= b.nodes[i].aabb_max[a])) ok = false;
	}
	return ok;
}
static double node_area(const rt_bvh_node& n)
{
	const double ex = (double)n.aabb_max[0] - n.aabb_min[0], ey = (double)n.aabb_max[1] - n.aabb_min[1], ez = (double)n.aabb_max[2] - n.aabb_min[2];
	return ex * ey + ey * ez + ez * ex;
}
// Collapses every BLAS into W-wide records; all or nothing (one flag for the kernels): false when a tree is not nested or the writer gives
// up, and the caller drops what was emitted.  A node's children are expanded, largest surface first, until there are W; emission is depth
// first, a record is reserved when its binary node is first reached.  The Writer stores the records:
//   bounded          tree_nested's flag; with it the scan also covers a tree whose root is a leaf
//   unbuilt(k)       root[k] of a BLAS that has no records: an empty one, or one that is never reached because an earlier tree failed
//   leaf(b, node, primOff)   the link of a leaf child (and of a root that is a leaf)
//   reserve()        a new record's index
//   write(b, k, rec, ch, n, links)   record rec from the n children ch[] (binary node numbers) and their links; entries from n on are unused
template <int W, class Writer>
static bool collapse(const rt_scene_desc* d, std::vector<uint>& root, Writer& w)
{
	size_t primBase = 0;
	for (uint k = 0; k < d->n_blas; k++) {
		const rt_blas& b = d->blas[k];
		const uint primOff = (uint)primBase;
		primBase += b.n_prims;
		root[k] = w.unbuilt(k);
		if (b.n_prims == 0) continue;
		const bool leafRoot = b.nodes[0].prim_count > 0;
		if ((w.bounded || !leafRoot) && !tree_nested(b, w.bounded)) return false;
		if (leafRoot) { root[k] = w.leaf(b, 0, primOff); continue; }
		std::vector<std::pair<uint, uint>> todo; // (binary inner node, wide record)
		const uint rootRec = w.reserve();
		root[k] = rootRec;
		todo.push_back({ 0u, rootRec });
		while (!todo.empty()) {
			const uint node = todo.back().first, rec = todo.back().second;
			todo.pop_back();
			uint ch[W];
			int n = 2;
			ch[0] = b.nodes[node].left_first, ch[1] = ch[0] + 1;
			while (n < W) {
				int best = -1;
				double bestA = -1;
				for (int j = 0; j < n; j++)
					if (b.nodes[ch[j]].prim_count == 0 && node_area(b.nodes[ch[j]]) > bestA) best = j, bestA = node_area(b.nodes[ch[j]]);
				if (best < 0) break;
				const uint lf = b.nodes[ch[best]].left_first;
				for (int j = n; j > best + 1; j--) ch[j] = ch[j - 1];
				ch[best] = lf, ch[best + 1] = lf + 1;
				n++;
			}
			uint links[W];
			for (int j = 0; j < W; j++) {
				links[j] = RT_EMPTY;
				if (j >= n) continue;
				if (b.nodes[ch[j]].prim_count > 0) links[j] = w.leaf(b, ch[j], primOff);
				else { links[j] = w.reserve(); todo.push_back({ ch[j], links[j] }); }
			}
			if (!w.write(b, k, rec, ch, n, links)) return false;
		}
	}
	return true;
}

// 4-wide nodes (wide[] above): SoA boxes, link[4], source[4]; a BLAS without records keeps its pair link
struct Wide4Writer {
	std::vector<float>& wide;
	const std::vector<uint>&rootLink, &pairOffOf;
	static constexpr bool bounded = false;
	uint unbuilt(uint k) const { return rootLink[k]; }
	uint leaf(const rt_blas& b, uint node, uint primOff) const { return RT_LEAF_BIT | (primOff + b.nodes[node].left_first); }
	uint reserve() { const uint w = (uint)(wide.size() / 32); wide.resize(wide.size() + 32, 0.0f); return w; }
	bool write(const rt_blas& b, uint k, uint rec, const uint* ch, int n, const uint* links)
	{
		float* r = &wide[(size_t)rec * 32];
		for (int j = 0; j < 4; j++) {
			uint src = 0xFFFFFFFFu;
			float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f }; // inverted: never hit
			if (j < n) {
				const rt_bvh_node& c2 = b.nodes[ch[j]];
				memcpy(lo, c2.aabb_min, 12), memcpy(hi, c2.aabb_max, 12);
				src = pairOffOf[k] * 2 + ch[j]; // global binary node number: pair record (src / 2), side (src & 1)
			}
			for (int a = 0; a < 3; a++) r[4 * a + j] = lo[a], r[12 + 4 * a + j] = hi[a];
			memcpy(&r[24 + j], &links[j], 4), memcpy(&r[28 + j], &src, 4);
		}
		return true;
	}
};

// 8-wide nodes with quantised child boxes (wide8[] / leafBox[] above): each child's box rounded outwards onto the node's
// 8-bit grid; a leaf child names a leafBox[] record, and so does a root that is a leaf
struct Wide8Writer {
	std::vector<uint>& wide8;    // 32 uints per node
	std::vector<float>& leafBox; // 8 floats per leaf: {min.xyz, first slot}{max.xyz, -}
	static constexpr bool bounded = true;
	uint unbuilt(uint) const { return RT_EMPTY; }
	uint leaf(const rt_blas& b, uint node, uint primOff)
	{
		const rt_bvh_node& n = b.nodes[node];
		const uint li = (uint)(leafBox.size() / 8);
		const uint slot = primOff + n.left_first;
		float rec[8] = { n.aabb_min[0], n.aabb_min[1], n.aabb_min[2], 0, n.aabb_max[0], n.aabb_max[1], n.aabb_max[2], 0 };
		memcpy(&rec[3], &slot, 4);
		leafBox.insert(leafBox.end(), rec, rec + 8);
		return RT_BOX_BIT | li;
	}
	uint reserve() { const uint w = (uint)(wide8.size() / 32); wide8.resize(wide8.size() + 32, 0u); return w; }
	bool write(const rt_blas& b, uint, uint rec, const uint* ch, int n, const uint* links)
	{
		uint* r = &wide8[(size_t)rec * 32];
		unsigned char q[6][8]; // qlo.x qlo.y qlo.z qhi.x qhi.y qhi.z
		uint exps = 0;
		for (int a = 0; a < 3; a++) {
			float org = b.nodes[ch[0]].aabb_min[a], top = b.nodes[ch[0]].aabb_max[a];
			for (int j = 1; j < n; j++) org = std::min(org, b.nodes[ch[j]].aabb_min[a]), top = std::max(top, b.nodes[ch[j]].aabb_max[a]);
			const double extent = (double)top - (double)org;
			int e = extent > 0 ? (int)std::ceil(std::log2(extent / 255.0)) : -100;
			if (e < -100) e = -100;
			for (bool again = true; again;) {
				again = false;
				if (e > 100) return false;
				const float sc = std::ldexp(1.0f, e);
				for (int j = 0; j < 8 && !again; j++) {
					if (j >= n) { q[a][j] = 255, q[3 + a][j] = 0; continue; } // inverted: never hit (and the link says empty)
					const float lo = b.nodes[ch[j]].aabb_min[a], hi = b.nodes[ch[j]].aabb_max[a];
					int ql = (int)std::floor(((double)lo - (double)org) / (double)sc), qh = (int)std::ceil(((double)hi - (double)org) / (double)sc);
					ql = std::max(0, std::min(255, ql)), qh = std::max(0, std::min(255, qh));
					// the device's own expression must contain the box: fma(q, 2^e, origin)
					while (ql > 0 && std::fmaf((float)ql, sc, org) > lo) ql--;
					while (qh < 255 && std::fmaf((float)qh, sc, org) < hi) qh++;
					if (std::fmaf((float)ql, sc, org) > lo || std::fmaf((float)qh, sc, org) < hi) { e++; again = true; break; } // a coarser grid
					q[a][j] = (unsigned char)ql, q[3 + a][j] = (unsigned char)qh;
				}
			}
			memcpy(&r[a], &org, 4);
			exps |= (uint)(e + 128) << (8 * a);
		}
		r[3] = exps;
		for (int a = 0; a < 6; a++) memcpy(&r[4 + 2 * a], q[a], 8);
		memcpy(&r[16], links, 32);
		return true;
	}
};

// ---- TLAS pair records ---------------------------------------------------------------------------------
// TLAS inner nodes -> pair records appended to the BLAS pairs (children boxes inside the parent's
// record; child A = leftRight & 0xFFFF, the one tlas::Intersect tests first).  tlasSlots: TLAS node index of every TLAS pair record, in record order
static int pack_tlas(const rt_scene_desc* d, SceneLayout& L, std::vector<uint>& tlasSlots, std::string& err)
{
	std::vector<float>& pairs = L.pairs;
	for (uint i = 0; i < d->tlas_nodes_used; i++) {
		const rt_tlas_node& nd = d->tlas_nodes[i];
		if (nd.left_right == 0) { if (nd.blas >= d->n_instances && (i != 0 || d->tlas_nodes_used == 1)) return layout_fail(err, RT_E_ARG, "rt_upload_scene: tlas node %u instance %u out of range", i, nd.blas); }
		else if ((nd.left_right & 0xFFFF) >= d->tlas_nodes_used || (nd.left_right >> 16) >= d->tlas_nodes_used) return layout_fail(err, RT_E_ARG, "rt_upload_scene: tlas node %u child out of range", i);
	}
	for (uint i = 0; i < d->tlas_nodes_used; i++)
		for (int a = 0; a < 3; a++)
			if (!(std::fabs(d->tlas_nodes[i].aabb_min[a]) <= 1e30f) || !(std::fabs(d->tlas_nodes[i].aabb_max[a]) <= 1e30f))
				return layout_fail(err, RT_E_UNSUPPORTED, "rt_upload_scene: tlas node %u has a non-finite bound or one beyond 1e30", i);
	const uint nT = d->tlas_nodes_used;
	std::vector<uint> slotOf(nT, 0);
	uint next = (uint)(pairs.size() / 16);
	const uint tlasSlotBase = next;
	for (uint i = 0; i < nT; i++) if (d->tlas_nodes[i].left_right != 0) slotOf[i] = next++, tlasSlots.push_back(i);
	auto tlink = [&](uint i) -> uint { const rt_tlas_node& nd = d->tlas_nodes[i]; return nd.left_right == 0 ? (RT_INST_BIT | nd.blas) : slotOf[i]; };
	pairs.resize((size_t)next * 16, 0.0f);
	for (uint i = 0; i < nT; i++) {
		const rt_tlas_node& nd = d->tlas_nodes[i];
		if (nd.left_right == 0) continue;
		const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
		float* rec = &pairs[(size_t)slotOf[i] * 16];
		for (int s = 0; s < 2; s++) {
			const rt_tlas_node& cn = d->tlas_nodes[ch[s]];
			const uint lk = tlink(ch[s]);
			memcpy(rec + 8 * s, cn.aabb_min, 12), memcpy(rec + 8 * s + 3, &lk, 4);
			memcpy(rec + 8 * s + 4, cn.aabb_max, 12);
		}
	}
	L.root = tlink(0);
	L.tlasBase = (uint)tlasSlots.size() ? tlasSlotBase : 0;
	L.tlasPairs = (int)tlasSlots.size();
	L.nInst = (int)d->n_instances;
	return RT_OK;
}

// ---- instances and the brute-force primitives -------------------------------------------------------------
static int pack_instances(const rt_scene_desc* d, SceneLayout& L, std::string& err)
{
	L.inst.resize(d->n_instances);
	for (uint i = 0; i < d->n_instances; i++) {
		const rt_instance& in = d->instances[i];
		if (in.blas < 0 || (uint)in.blas >= d->n_blas) return layout_fail(err, RT_E_ARG, "rt_upload_scene: instance %u blas %d out of range", i, in.blas);
		memset(&L.inst[i], 0, sizeof(DInstance));
		memcpy(L.inst[i].invT, in.inv_transform, 48), memcpy(L.inst[i].T, in.transform, 48);
		L.inst[i].rootLink = L.rootLink[in.blas];
		L.inst[i].rootWide = L.rootWide[in.blas];
		L.inst[i].rootWide8 = L.wide8OK ? L.rootWide8[in.blas] : RT_EMPTY;
	}
	// brute-force primitives in prim-record form
	rt_blas fake;
	memset(&fake, 0, sizeof(fake));
	fake.spheres = d->brute_spheres, fake.n_sph = d->n_brute_spheres, fake.planes = d->brute_planes, fake.n_pla = d->n_brute_planes;
	const uint nb = fake.n_sph + fake.n_pla;
	L.brute.assign((size_t)nb * 16 + 16, 0.0f);
	for (uint j = 0; j < nb; j++) pack_prim(&L.brute[(size_t)j * 16], fake, j, true, d->materials, d->n_materials);
	L.nBruteSph = (int)fake.n_sph, L.nBrutePla = (int)fake.n_pla;
	return RT_OK;
}

// ---- reach[]: per TLAS pair, the world boxes its children's geometry can occupy (see above) ----------------------
// The per-instance part, in two steps that rt_set_instances (rt_api_instances.inc) repeats for a moved instance: the object box of a BLAS
// (kept per BLAS with the context at upload), and the world box of that geometry under the instance's transform with its margins.
struct Reach { double lo[3], hi[3], a, b; };
static Reach reach_unbounded()
{
	const double big = 1e30;
	Reach r;
	for (int k = 0; k < 3; k++) r.lo[k] = -big, r.hi[k] = big;
	r.a = 0, r.b = 0;
	return r;
}
struct ObjectBox { double lo[3], hi[3]; bool bounded; }; // bounded == false: whatever the transform, the instance's reach is unbounded
// object-space box of everything a ray can hit in this BLAS: triangles and spheres; a plane is
// unbounded.  Triangle::Intersect rejects a triangle with N == 0 for every ray with finite D
// (|dot(N, D)| < t_min), and one with a NaN in N for every ray (t is NaN and fails the final
// range test) -- the two sentinel triangles a .tri mesh ends with (v0 = v1 = v2 = 999) are such.
static ObjectBox blas_object_box(const rt_blas& b)
{
	const double big = 1e30;
	ObjectBox ob;
	for (int k = 0; k < 3; k++) ob.lo[k] = ob.hi[k] = 0;
	ob.bounded = false;
	if (b.n_prims == 0 || b.n_pla > 0) return ob;
	double lo[3] = { big, big, big }, hi[3] = { -big, -big, -big };
	bool finite = true;
	for (uint j = 0; j < b.n_tri; j++) {
		const rt_triangle& t = b.tris[j];
		if ((t.N[0] == 0 && t.N[1] == 0 && t.N[2] == 0) || t.N[0] != t.N[0] || t.N[1] != t.N[1] || t.N[2] != t.N[2]) continue;
		for (int k = 0; k < 3; k++) {
			lo[k] = std::min(lo[k], (double)std::min(t.v0[k], std::min(t.v1[k], t.v2[k])));
			hi[k] = std::max(hi[k], (double)std::max(t.v0[k], std::max(t.v1[k], t.v2[k])));
			if (!(std::fabs(t.v0[k]) < 1e29f && std::fabs(t.v1[k]) < 1e29f && std::fabs(t.v2[k]) < 1e29f)) finite = false;
		}
	}
	for (uint j = 0; j < b.n_sph; j++) {
		const rt_sphere& q = b.spheres[j];
		const double rr = std::max(std::fabs((double)q.r), std::sqrt(std::fabs((double)q.r2))); // r and r2 are separate inputs
		for (int k = 0; k < 3; k++) {
			lo[k] = std::min(lo[k], (double)q.pos[k] - rr), hi[k] = std::max(hi[k], (double)q.pos[k] + rr);
			if (!(std::fabs(q.pos[k]) < 1e29f && rr < 1e29)) finite = false;
		}
	}
	if (lo[0] > hi[0]) { for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0; } // nothing hittable: an empty box at the origin
	for (int k = 0; k < 3; k++) ob.lo[k] = lo[k], ob.hi[k] = hi[k];
	ob.bounded = finite;
	return ob;
}
// the world box of an object box under the exact inverse of inv_transform (rows 0-2: the float matrix the device applies), in double, and
// the margins a, b of the float rounding of the object-space ray (see reach[] above); unbounded where that cannot be bounded
static Reach instance_reach(const ObjectBox& ob, const float* m)
{
	const double big = 1e30, rel = 1.0 / 32768.0;
	Reach r = reach_unbounded();
	if (!ob.bounded) return r;
	const double* lo = ob.lo;
	const double* hi = ob.hi;
	const double A[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } }, tv[3] = { m[3], m[7], m[11] };
	const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
	                   A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
	if (!(std::fabs(det) > 1e-30) || !std::isfinite(det)) return reach_unbounded();
	double Ai[3][3];
	for (int rI = 0; rI < 3; rI++)
		for (int cI = 0; cI < 3; cI++) {
			const int r1 = (cI + 1) % 3, r2 = (cI + 2) % 3, c1 = (rI + 1) % 3, c2 = (rI + 2) % 3;
			Ai[rI][cI] = (A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1]) / det;
		}
	double nA = 0, nAi = 0, lmax = 0, wmax = 0;
	for (int rI = 0; rI < 3; rI++) {
		nA = std::max(nA, std::fabs(A[rI][0]) + std::fabs(A[rI][1]) + std::fabs(A[rI][2]));
		nAi = std::max(nAi, std::fabs(Ai[rI][0]) + std::fabs(Ai[rI][1]) + std::fabs(Ai[rI][2]));
	}
	for (int k = 0; k < 3; k++) r.lo[k] = big, r.hi[k] = -big, lmax = std::max(lmax, std::max(std::fabs(lo[k]), std::fabs(hi[k])) + std::fabs(tv[k]));
	for (int corner = 0; corner < 8; corner++) {
		const double l[3] = { (corner & 1 ? hi[0] : lo[0]) - tv[0], (corner & 2 ? hi[1] : lo[1]) - tv[1], (corner & 4 ? hi[2] : lo[2]) - tv[2] };
		for (int k = 0; k < 3; k++) {
			const double w = Ai[k][0] * l[0] + Ai[k][1] * l[1] + Ai[k][2] * l[2];
			r.lo[k] = std::min(r.lo[k], w), r.hi[k] = std::max(r.hi[k], w);
		}
	}
	for (int k = 0; k < 3; k++) wmax = std::max(wmax, std::max(std::fabs(r.lo[k]), std::fabs(r.hi[k])));
	const double cond = std::max(1.0, nA * nAi);
	r.a = rel * (cond * wmax + nAi * lmax) + 1e-20, r.b = rel * cond;
	if (!(wmax < 1e29) || !std::isfinite(r.a) || !std::isfinite(r.b) || r.a > 1e29 || r.b > 1e10) return reach_unbounded();
	return r;
}
// the boxes are stored inflated for every world origin with |O|_1 <= originMax: 64 x the extent of
// the instanced geometry (camera and bounce rays start inside that; a ray from further away is
// simply not culled)
static double reach_origin_max(const Reach* instReach, size_t n)
{
	double extent = 1.0;
	for (size_t i = 0; i < n; i++)
		if (instReach[i].b > 0) for (int k = 0; k < 3; k++) extent = std::max(extent, std::max(std::fabs(instReach[i].lo[k]), std::fabs(instReach[i].hi[k])));
	return 64.0 * 3.0 * extent;
}

static int pack_reach(const rt_scene_desc* d, SceneLayout& L, const std::vector<uint>& tlasSlots, std::string& err)
{
	const double big = 1e30;
	std::vector<ObjectBox> box(d->n_blas);
	for (uint k = 0; k < d->n_blas; k++) box[k] = blas_object_box(d->blas[k]);
	std::vector<Reach> instReach(d->n_instances);
	for (uint i = 0; i < d->n_instances; i++) instReach[i] = instance_reach(box[d->instances[i].blas], d->instances[i].inv_transform);
	const uint nT = d->tlas_nodes_used;
	std::vector<Reach> nodeReach(nT);
	std::vector<char> state(nT, 0); // 0 unseen, 1 open, 2 done
	std::vector<uint> walk;
	if (nT > 0 && d->tlas_nodes[0].left_right != 0) walk.push_back(0);
	while (!walk.empty()) {
		const uint i = walk.back();
		const rt_tlas_node& nd = d->tlas_nodes[i];
		if (nd.left_right == 0) { nodeReach[i] = nd.blas < d->n_instances ? instReach[nd.blas] : reach_unbounded(); state[i] = 2; walk.pop_back(); continue; }
		const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
		if (state[i] == 0) {
			state[i] = 1;
			for (int sI = 0; sI < 2; sI++) {
				if (state[ch[sI]] == 1) return layout_fail(err, RT_E_ARG, "rt_upload_scene: tlas node %u is its own ancestor", ch[sI]);
				if (state[ch[sI]] == 0) walk.push_back(ch[sI]);
			}
			continue;
		}
		Reach r = nodeReach[ch[0]];
		const Reach& o = nodeReach[ch[1]];
		for (int k = 0; k < 3; k++) r.lo[k] = std::min(r.lo[k], o.lo[k]), r.hi[k] = std::max(r.hi[k], o.hi[k]);
		r.a = std::max(r.a, o.a), r.b = std::max(r.b, o.b);
		nodeReach[i] = r, state[i] = 2;
		walk.pop_back();
	}
	const double originMax = reach_origin_max(instReach.data(), instReach.size());
	L.reach.assign((size_t)tlasSlots.size() * 12 + 16, 0.0f);
	for (size_t sI = 0; sI < tlasSlots.size(); sI++) {
		const rt_tlas_node& nd = d->tlas_nodes[tlasSlots[sI]];
		const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
		for (int h = 0; h < 2; h++) {
			const Reach r = state[ch[h]] == 2 ? nodeReach[ch[h]] : reach_unbounded();
			float* rec = &L.reach[sI * 12 + 6 * h]; // {min.xyz, max.xyz} of child h
			const double m = r.a + r.b * originMax;
			// round outwards: the float box must contain the inflated double one
			for (int k = 0; k < 3; k++) {
				rec[k] = std::nextafterf((float)std::max(r.lo[k] - m, -big), -INFINITY), rec[3 + k] = std::nextafterf((float)std::min(r.hi[k] + m, big), INFINITY);
			}
		}
	}
	L.reachOriginMax = (float)originMax;
	return RT_OK;
}

// ---- refit order -------------------------------------------------------------------------------------------
// rt_set_time support: the pair records of the scene BVH grouped by depth (children are deeper than their parents) for the bottom-up refit
// The order of one BLAS, appended to 'order': its pair records as ABSOLUTE indices (pairOff: the BLAS's first record in pairs[]), level by
// level from the root's; levelStart receives one entry per level boundary, as indices into 'order' (its first entry is order's size on
// entry).  A tree whose root is a leaf has no pair record and no level.  rt_set_triangles (rt_api_triangles.inc) keeps this per BLAS.
// false: more records than the BLAS has (a node that is its own ancestor); the order is then cut short and of no use.
static bool blas_refit_order(const rt_blas& b, uint pairOff, std::vector<uint>& order, std::vector<int>& levelStart)
{
	const size_t cap = order.size() + b.nodes_used / 2;
	levelStart.assign(1, (int)order.size());
	std::vector<uint> level; // pair records relative to the BLAS
	if (b.n_prims > 0 && b.nodes[0].prim_count == 0) level.push_back(b.nodes[0].left_first / 2);
	while (!level.empty()) {
		std::vector<uint> next;
		for (uint pr : level) {
			order.push_back(pairOff + pr);
			for (int sI = 0; sI < 2; sI++) { const rt_bvh_node& nd = b.nodes[2 * pr + sI]; if (nd.prim_count == 0) next.push_back(nd.left_first / 2); }
		}
		levelStart.push_back((int)order.size());
		if (order.size() > cap) return false;
		level.swap(next);
	}
	return true;
}
static void pack_refit(const rt_scene_desc* d, SceneLayout& L)
{
	const rt_blas& b = d->blas[0];
	L.refitOrder.clear();
	blas_refit_order(b, 0, L.refitOrder, L.refitLevelStart);
	L.refitLevels = (int)L.refitLevelStart.size() - 1;
	L.animSlots = (int)b.n_prims;
}

// ---- the split of a traversal block's LDS (rt_scene_dev.h RT_LDS_WORDS): as many stack rows as the TLAS copy leaves ----
static void split_lds(SceneLayout& L, const LayoutKnobs& knobs)
{
	const int words = RT_TLAS_COPY_WORDS(L.tlasPairs, L.nInst);
	const int rows = (RT_LDS_WORDS - ((words + 3) & ~3)) / RT_BLOCK - 6;
	L.tlasLds = rows >= RT_STACK_ROWS_MIN ? 1 : 0;
	L.tlasLds = L.tlasLds && knobs.tlasLds;
	if (L.tlasLds) L.stackRows = rows < RT_STACK_ROWS_MAX ? rows : RT_STACK_ROWS_MAX;
}

// ---- light and material tables ---------------------------------------------------------------------------
static void pack_tables(const rt_scene_desc* d, SceneLayout& L)
{
	L.lights.resize(d->n_lights ? d->n_lights : 1);
	for (uint i = 0; i < d->n_lights; i++) {
		const rt_light& l = d->lights[i];
		DLight& o = L.lights[i];
		o.kind = l.kind, o.objIdx = l.obj_idx, o.strength = l.strength, o.radius = l.radius, o.sinAngle = l.sin_angle;
		memcpy(o.pos, l.pos, 12), memcpy(o.col, l.col, 12), memcpy(o.normal, l.normal, 12);
	}
	L.mats.resize(d->n_materials ? d->n_materials : 1);
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		DMaterial& o = L.mats[i];
		o.type = m.type, o.raytracer = m.raytracer, o.specu = m.specu, o.diffu = m.diffu, o.shinieness = m.shinieness, o.N = m.N, o.ir = m.ir;
		memcpy(o.col, m.col, 12), memcpy(o.albedo, m.albedo, 12), memcpy(o.absorption, m.absorption, 12);
	}
}

// The whole layout of a description, in the order the guarantees build on one another.  Returns RT_OK, or the rt_status and, in err, the message
// rt_upload_scene reports.  L is what was built up to the failure (pathUnsupported is set whenever check_desc passed).
static int build_layout(const rt_scene_desc* d, const LayoutKnobs& knobs, SceneLayout& L, std::string& err)
{
	L = SceneLayout();
	int rc = check_desc(d, err);
	if (rc != RT_OK) return rc;
	check_path_support(d, L);
	// pairs + prims of every BLAS, concatenated
	std::vector<uint> pairOffOf(d->n_blas);
	L.rootLink.assign(d->n_blas, 0), L.rootWide.assign(d->n_blas, 0), L.rootWide8.assign(d->n_blas, 0);
	for (uint k = 0; k < d->n_blas; k++)
		if ((rc = pack_blas(d, k, L, pairOffOf, err)) != RT_OK) return rc;
	// 4-wide nodes.  Default: on for a scene BVH, off with a TLAS (RT_WIDE=0 / 1 forces).  Exact either way (tests/test_gpu_parity.py::
	// test_wide_walk_*).  Measured (profiles/r02_wide_by_config.txt): one big tree gains (config 4: connect 19.3 -> 16.3 ms
	// per step, config 2: 2.63 -> 2.47), instanced scenes lose or stay level (config 5: 625 -> 660 ms, config 3: 10.1 -> 10.2):
	// there the walk spends its steps on the TLAS level and the first levels of many BLASes, where a 4-wide step
	// replaces fewer binary ones than it costs (four slab tests, a sorting network and up to three pushes).
	Wide4Writer w4{ L.wide, L.rootLink, pairOffOf };
	L.wideOK = (knobs.wide >= 0 ? knobs.wide != 0 : !d->use_tlas) && collapse<4>(d, L.rootWide, w4);
	if (!L.wideOK) L.wide.clear();
	// 8-wide nodes.  RT_WIDE8=1 / 0 forces; default off
	Wide8Writer w8{ L.wide8, L.leafBox };
	L.wide8OK = knobs.wide8 != 0 && collapse<8>(d, L.rootWide8, w8);
	if (!L.wide8OK) L.wide8.clear(), L.leafBox.clear();
	L.root = L.rootLink[0];
	if (d->use_tlas) {
		std::vector<uint> tlasSlots;
		if ((rc = pack_tlas(d, L, tlasSlots, err)) != RT_OK) return rc;
		if ((rc = pack_instances(d, L, err)) != RT_OK) return rc;
		if ((rc = pack_reach(d, L, tlasSlots, err)) != RT_OK) return rc;
		split_lds(L, knobs);
	} else if (d->blas[0].n_prims > 0) pack_refit(d, L);
	pack_tables(d, L);
	return RT_OK;
}
