// The context behind the C ABI (struct rt_ctx) and what every unit of rt_api.hip shares: error reporting, device allocation pools, the
// HIP-event kernel timers, the measurement builds' probes.  rt_api.hip is ONE translation unit on purpose -- the kernels live in headers and the
// hot ones' code generation is pinned to this compilation (bench.py kernel_hash) -- cut into units by what they do:
//   rt_api.hip          context, camera, accumulator access, counters / timers, build + tuning info
//   rt_layout.h         the scene layout as a value: build_layout, host arithmetic only (no hip* call, no rt_ctx)
//   rt_api_upload.inc   rt_upload_scene: build_layout's arrays copied to the device; rt_layout_*
//   rt_api_build.inc    device builders, refit
//   rt_api_instances.inc rt_set_instances, rt_set_instance_list (kernels: rt_instances.h), rt_download_tlas, rt_scene_array
//   rt_api_triangles.inc rt_set_triangles (kernels: rt_triangles.h), rt_blas_array
//   rt_api_vertices.inc rt_set_mesh_indices, rt_set_vertices, rt_set_vertices_device (kernel: rt_vertices.h)
//   rt_api_materials.inc rt_set_lights, rt_set_materials, rt_set_sky (kernel: rt_materials.h)
//   rt_forms.h          which instantiation a launch takes, as pure functions (no hip* call, no rt_ctx); the kernel tables they index are below
//   rt_api_camera.inc   the camera-sample settings: rt_set_pixel_filter, rt_set_lens, rt_set_shutter, rt_focus_at, rt_sample_rays and their checks
//   rt_api_render.inc   rt_render*, rt_trace_batch*: round loops and batches
//   rt_api_gather.inc   rt_gather_*
//   rt_api_query.inc    batch queries
//   rt_api_qlearn.inc   rt_qlearn_*
//   rt_api_output.inc   the output stage's shared helpers: row ranges, row downloads, the resolve, the a-trous drivers' common part
//   rt_api_denoise.inc  rt_render_aovs, rt_denoise, rt_denoise_variance and their downloads
//   rt_api_adaptive.inc rt_stats_*, rt_select_active, the active-pixel list, rt_render_active, rt_resolve_adaptive
//   rt_api_reproject.inc rt_history_capture, rt_reproject, rt_reproject_motion, rt_reproject_deform, rt_download_aov_positions,
//                       rt_download_aov_instances, rt_download_aov_prims
#pragma once
#include "../../include/rt_amd.h" // first: the kernels read its enums (RT_FILTER_*)
#include "rt_kernels.h"
#include "rt_stream.h"
#include "rt_mega.h"
#include "rt_build.h"
#include "rt_instances.h"
#include "rt_triangles.h"
#include "rt_vertices.h"
#include "rt_materials.h"
#include "rt_layout.h"
#include "rt_forms.h"
#include "rt_denoise.h"
#include "rt_adaptive.h"
#include "rt_budget.h"
#include "rt_dilate.h"
#include "rt_denoise_var.h"
#include "rt_reproject.h"
#include "rt_gather.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

using namespace rtd;

// ---- the kernel families (rt_forms.h) -----------------------------------------------------------
// One table per family of instantiations that share a signature, indexed by the form rt_forms.h chooses; beside each, the context holds
// the resident grids under the same index (rt_create fills them in a loop over the table).  A combination nobody launches is a null entry.
// [COUNT]: the counting twin of a traversal kernel
static const decltype(&k_extend<false, false>) kExtend[2][2] = { { k_extend<false, false>, k_extend<false, true> }, { k_extend<true, false>, k_extend<true, true> } }; // [COUNT][DENSE]
static const decltype(&k_connect<false>) kConnect[WALK_FORMS] = { k_connect<false>, k_connect<true>, k_connect<false, true>, k_connect<false, false, true>, nullptr }; // (no 8-wide walk over slots)
static const decltype(&k_extend_s<false>) kExtendS[2] = { k_extend_s<false>, k_extend_s<true> };
static const decltype(&k_connect_s<false>) kConnectS[WALK_FORMS] = { k_connect_s<false>, k_connect_s<true>, k_connect_s<false, true>, k_connect_s<false, false, true>, k_connect_s<false, false, false, true> };
static const decltype(&k_primary_table<false>) kPrimaryTable[2] = { k_primary_table<false>, k_primary_table<true> };
static const decltype(&k_bounce_table<false>) kBounceTable[2] = { k_bounce_table<false>, k_bounce_table<true> };
static const decltype(&k_chain_table<false>) kChainTable[2] = { k_chain_table<false>, k_chain_table<true> };
static const decltype(&k_shade_s<false>) kShadeS[SHADE_FORMS] = {
	k_shade_s<false>, k_shade_s<true>,                                 // 0, QL
	k_shade_s<false, true>, nullptr,                                   // BOUNCE
	k_shade_s<false, false, true>, nullptr,                            // TABLE0
	k_shade_s<false, true, true>, nullptr,                             // BOUNCE | TABLE0
	k_shade_s<false, false, false, true>, nullptr,                     // CHAIN
	k_shade_s<false, true, false, true>, nullptr,                      // BOUNCE | CHAIN
	nullptr, nullptr,                                                  // TABLE0 | CHAIN: round 0 of a chain batch hands out keys, so it has BOUNCE
	k_shade_s<false, true, true, true>, nullptr,                       // BOUNCE | TABLE0 | CHAIN
};
static const decltype(&k_light_s<false>) kLightS[LIGHT_FORMS] = { k_light_s<false>, k_light_s<true> };
static_assert(GENERATE_C == 0 && GENERATE_T == 1, "kGenerateTab is indexed by generate_form");
static const decltype(&k_generate_c) kGenerateTab[2] = { k_generate_c, k_generate_t }; // GENERATE_C, GENERATE_T (k_generate_s reads no table: a signature of its own)
static const decltype(&k_query_nearest<false, false>) kQueryNearest[2][2] = { { k_query_nearest<false, false>, k_query_nearest<false, true> }, { k_query_nearest<true, false>, k_query_nearest<true, true> } }; // [COUNT][HEAD]
static const decltype(&k_query_occluded<false>) kQueryOccluded[WALK_FORMS] = { k_query_occluded<false>, k_query_occluded<true>, k_query_occluded<false, true>, k_query_occluded<false, false, true>, k_query_occluded<false, false, false, true> };
static const decltype(&k_primary_hits<false>) kPrimaryHits[2] = { k_primary_hits<false>, k_primary_hits<true> };

#ifndef RT_GRID_CAP
#define RT_GRID_CAP 8
#endif
static std::string g_err;

struct Timer {
	hipEvent_t a = nullptr, b = nullptr;
};

// The environment, read ONCE per context (rt_create -> read_knobs: the library's only getenv site).
struct Knobs {
	// what a user may want to set
	long slots = 0;        // RT_SLOTS: path samples in flight (default 2^28: ~67 GB of path state at the largest batches)
	long sampleGiB = 4;    // RT_SAMPLE_GIB: size of the finished-sample buffer of a batch of frames
	int exactGamma = 0;    // RT_EXACT_GAMMA=1: the gamma of a finished sample as the reference's double-precision pow (bit-equal accumulators)
	int wide = -1;         // RT_WIDE=0/1: the 4-wide any-hit walk off / on (default: on for a scene BVH, off with a TLAS)
	int wide8 = 0;         // RT_WIDE8=1: the 8-wide quantised any-hit walk
	// switches between EQUIVALENT code paths (same results: tests/test_gpu_parity.py renders every one of them against the oracle, and the
	// profiles/ A/B scripts time them); the defaults are the measured optimum, none of them is a tuning knob a user needs
	int fuse = -1;         // RT_FUSE: 0 one kernel at a time, 1 one traversal launch per round, 2 connect + light on a second stream; < 0: by batch size
	int stream = 1;        // RT_STREAM=0: the slot wavefront of rt_kernels.h instead of the dense pipeline
	int decide = 1;        // RT_DECIDE: producers answer rays whose first traversal step leaves nothing to visit
	int mega = 1, megaLpt = 1, megaLevels = 2; // RT_MEGA / RT_MEGA_LPT / RT_MEGA_LEVELS: the forms of a Whitted frame (rt_mega.h); levels: frames up to
	                       // RT_LEVEL_SAMPLES_MAX samples run one launch per tree level (1), as one launch (0), or as whichever was faster (2)
	int deferGamma = 1;    // RT_DEFER_GAMMA=0: the gamma where a sample is stored instead of in k_accumulate
	int shadeLds = 1;      // RT_SHADE_LDS=0: material / light tables from memory
	int tlasLds = 1;       // RT_TLAS_LDS=0: the TLAS from global memory even when it fits a block's LDS
	int gammaLut = 1;      // RT_GAMMA_LUT=0: no 256-entry table for finished sky samples
	int primaryTable = 1;  // RT_PRIMARY_TABLE=0: every camera ray of a dense path batch is traced (round 0 as generate + compact + extend) instead of
	                       // read from the table of the frame's distinct camera rays (rt_stream.h k_primary_table)
	int tableMin = 12;     // RT_PRIMARY_TABLE_MIN: a stale table is rebuilt once this many camera samples per table record have been asked for since it
	                       // went stale (1080p, bench scene: the build is 0.49 ms; batches that rebuild every time are level with traced ones at
	                       // 3-8 frames, 0.13 ms ahead at 12, 0.3 at 16, 2 at 32: profiles/ab_primary_table.txt)
	int bounceTable = 7;   // RT_BOUNCE_TABLE: (tests) which first-bounce rays off a glass or metal primary hit shade(0) answers from the bounce table
	                       // (rt_stream.h BounceTable) instead of tracing them: bit 0 metal, bit 1 glass refraction, bit 2 glass reflection; 0: none,
	                       // and no table is built
	int bounceDepth = 4;   // RT_BOUNCE_DEPTH: 1-4, the levels of specular bounces answered from tables: 1 the bounce table alone; d: rounds 1 .. d - 1 also read
	                       // the chain tables (rt_stream.h ChainLevel: the rays of paths whose every hit so far was glass or metal).  The same frames at
	                       // every depth; RT_BOUNCE_TABLE's mask bits mean the same at every level
	int chainMin = 1;      // RT_BOUNCE_DEPTH_MIN: levels >= 2 are built once RT_PRIMARY_TABLE_MIN times this many camera samples per primary record have
	                       // been asked for since the tables went stale (1: with the first two levels; 0 with RT_PRIMARY_TABLE_MIN=0: everything in the
	                       // first batch).  1080p, bench scene: levels 2-4 build in 1.4 ms; a batch that rebuilds everything is 1.3 ms behind depth 1
	                       // at 1-2 frames, 0.7 at 12, 0.5 at 16, 0.26 ahead at 24 (profiles/ab_chain_table.txt), and a camera at rest has the build back
	                       // eleven one-frame batches later.  A later build (2) makes what a context's counting launch tallies depend on how many
	                       // samples it rendered before, which tests/test_gpu_look.py holds equal to a fresh context's: the default keeps one rule
	long chainCap = -1;    // RT_BOUNCE_CAP: (tests) records a level >= 2 holds; default one per primary record (the bench frame uses 0.14-0.19;
	                       // a camera inside glass can ask for 2^k).  Children that do not fit are traced as at depth 1
	int round0Entries = 0; // RT_ROUND0_ENTRIES: 0 round 0 of a batch with a current primary table shades straight from the table (k_generate_c writes class
	                       // bytes only; rt_stream.h k_shade_s TABLE0), 1 generate copies the records into round-0 entries first (k_generate_t),
	                       // 2 (tests) as 0, and the entry arrays nobody may read are filled with 0xFF bytes behind every such generate
	int levelCap = 0;      // RT_LEVEL_CAP: (tests) level queues that overflow
	unsigned mixedMax = 10000000u; // RT_MIXED_MAX: batches below this many samples run one traversal launch per round
};
static void read_knobs(Knobs& k)
{
	auto num = [](const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; };
	k.slots = num("RT_SLOTS", 0), k.sampleGiB = num("RT_SAMPLE_GIB", 4) > 0 ? num("RT_SAMPLE_GIB", 4) : 4;
	k.exactGamma = num("RT_EXACT_GAMMA", 0) != 0, k.wide = (int)num("RT_WIDE", -1), k.wide8 = num("RT_WIDE8", 0) != 0;
	{ const long f = num("RT_FUSE", -1); k.fuse = f < 0 ? -1 : (f > 2 ? 2 : (int)f); }
	k.stream = num("RT_STREAM", 1) != 0, k.decide = (int)num("RT_DECIDE", 1) & 3, k.mega = num("RT_MEGA", 1) != 0, k.megaLpt = num("RT_MEGA_LPT", 1) != 0;
	k.megaLevels = (int)num("RT_MEGA_LEVELS", 2), k.deferGamma = num("RT_DEFER_GAMMA", 1) != 0, k.shadeLds = num("RT_SHADE_LDS", 1) != 0;
	k.tlasLds = num("RT_TLAS_LDS", 1) != 0, k.gammaLut = num("RT_GAMMA_LUT", 1) != 0, k.levelCap = (int)num("RT_LEVEL_CAP", 0);
	k.mixedMax = (unsigned)num("RT_MIXED_MAX", 10000000);
	k.primaryTable = num("RT_PRIMARY_TABLE", 1) != 0, k.tableMin = (int)std::max(0l, num("RT_PRIMARY_TABLE_MIN", 12));
	{ const char* e = getenv("RT_BOUNCE_TABLE"); k.bounceTable = e ? (int)atol(e) & 7 : 7; } // (a test-tier mask read beside num(): tests/support.py KNOBS is the list of the num() knobs, and tests/test_gpu_bounce_table.py clears this one itself)
	{ const char* e = getenv("RT_BOUNCE_DEPTH"); const long v = e ? atol(e) : 4; k.bounceDepth = v < 1 ? 1 : (v > 4 ? 4 : (int)v); } // (beside num() as well: tests/test_gpu_chain_table.py clears these three itself)
	{ const char* e = getenv("RT_BOUNCE_DEPTH_MIN"); k.chainMin = e ? (int)std::max(0l, atol(e)) : 1; }
	{ const char* e = getenv("RT_BOUNCE_CAP"); k.chainCap = e ? std::max(0l, atol(e)) : -1; }
	{ const char* e = getenv("RT_ROUND0_ENTRIES"); const long v = e ? atol(e) : 0; k.round0Entries = v == 1 || v == 2 ? (int)v : 0; } // (beside num() too: tests/test_gpu_round0_direct.py clears it itself)
	if (k.exactGamma) k.deferGamma = 1; // the exact form lives where samples are read (k_accumulate), not in the shading kernels
	// the scheduling thresholds are compile-time constants since round 4 (rt_scene_dev.h): a sweep script that still sets them in
	// the environment would read as a flat sweep -- say so once
	static bool warned = false;
	const char* retired[] = { "RT_REFILL", "RT_REFILL_ANY", "RT_STEPMIN", "RT_STEPMIN_ANY", "RT_STEPMIN_XFORM", "RT_PAIRAGAIN", "RT_PAIRAGAIN_ANY", "RT_DRAIN_LANES", "RT_DRAIN_LANES_ANY" };
	for (const char* name : retired)
		if (!warned && getenv(name)) { fprintf(stderr, "rt_amd: %s is a compile-time constant (rebuild with make EXTRA=-D%s=N); the environment variable is ignored\n", name, name); warned = true; }
}

template <typename T>
static hipError_t dalloc(std::vector<void*>& pool, T** p, size_t count)
{
	void* q = nullptr;
	hipError_t e = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
	if (e == hipSuccess) { pool.push_back(q); *p = (T*)q; }
	return e;
}
static void free_pool(std::vector<void*>& pool)
{
	for (void* p : pool) (void)hipFree(p);
	pool.clear();
}

struct rt_ctx {
	int device = 0, width = 0, height = 0;
	Knobs knobs;
	hipStream_t stream = nullptr;
	std::string err, tuningInfo;
	// scene
	DScene S{};
	bool sceneLoaded = false;
	std::vector<void*> sceneAllocs;
	int sceneRaytracer = -1; // rt_set_scene_raytracer: scene.raytracer as the caller's Scene holds it (-1: it follows the function called)
	bool pathUnsupported = false; // shiny or rt==0 diffuse present: path mode runs k_sample_general instead of the wavefront
	std::string pathUnsupportedWhy;
	// animation (rt_set_time): original leaf records of the scene BVH and its pair records by level
	float4* primsOrig = nullptr;
	float4* pairsMut = nullptr; float4* primsMut = nullptr;
	std::vector<uint> blasRoot, blasRootWide, blasRootWide8; int nInstances = 0; // roots for the scoped queries (rt_intersect_scope)
	float4* wideMut = nullptr; int wideNodes = 0; // 4-wide nodes: their boxes follow the pair records after a refit
	uint* refitOrder = nullptr; int* refitLevelStart = nullptr;
	int refitLevels = 0, animSlots = 0;
	std::vector<int> refitLevelHost; // levelStart[] on the host: which levels are wide enough for a launch of their own
	// rt_set_instances (rt_api_instances.inc): the part of the layout an instance's transform decides, kept where the call can rewrite it.
	// Host: a mirror of inst[], per instance its BLAS and its reach (rt_layout.h instance_reach), per BLAS its object box (f64) and its
	// local box (f32, bvh::bounds), the uploaded TLAS until the first update replaces it, the RT_LAYOUT_SCALARS words.  Device (scene
	// pool): every instance's world box and the TLAS nodes the context walks, the local boxes, and the scratch a call builds into.
	// Every per-instance array on the device has room for RT_TLAS_MAX instances: rt_set_instance_list changes their number.
	struct InstanceState {
		std::vector<DInstance> inst;
		std::vector<int> blasOf;
		std::vector<Reach> reach;
		std::vector<ObjectBox> objBox;
		std::vector<float> blasBox6;
		std::vector<uint> rootWide, rootWide8; bool wide8OK = false; // per BLAS, what pack_instances put into a record of the upload (rt_set_instance_list)
		std::vector<char> boundsKnown; // the instance had a leaf in the uploaded TLAS, or has been set since
		std::vector<rt_tlas_node> uploaded;
		bool built = false; // tlasKeep holds a tlas::build of the context's own
		DInstance* instMut = nullptr; float* reachMut = nullptr;
		float* bounds = nullptr; TlasNodeDev* tlasKeep = nullptr; float* blasBox = nullptr; int* blasOfDev = nullptr;
		float* boundsNew = nullptr; TlasNodeDev* nodesNew = nullptr; int* used = nullptr; InstReach* reachIn = nullptr; float* xform = nullptr;
		int* which = nullptr; float* boxUndo = nullptr; // rt_set_triangles: the instances of the deformed BLAS (n ints), the BLAS's local box before the call
	};
	InstanceState instances;
	// rt_set_triangles (rt_api_triangles.inc): what upload keeps per BLAS -- its pair records and leaf slots as ranges of pairs[] / prims[],
	// the slot of each of its primitives (slotOf: the inverse of prim_idx, absolute slots, all BLASes concatenated in primitive order) and
	// its refit order by level (rt_layout.h blas_refit_order: absolute pair indices in refitOrderAll, the level boundaries in
	// refitLevelAll on the device and in BlasKeep::level on the host, both as indices into refitOrderAll).  The staging array of a call's
	// triangles and the undo copies of the two record ranges are allocated by the first call that needs them and grown on demand.
	struct BlasKeep {
		uint pairFirst = 0, pairCount = 0, slotFirst = 0, slotCount = 0, nTri = 0;
		size_t levelFirst = 0;  // this BLAS's first entry of refitLevelAll
		std::vector<int> level; // its level boundaries (levels + 1 entries)
		bool refittable = true; // false: its tree is not one (a node is its own ancestor)
		// rt_set_mesh_indices (rt_api_vertices.inc): the bound index buffer, 3 nTri words in the scene pool (allocated by the first binding,
		// kept across an unbinding), and the vertex count it was checked against.  Ends with the scene, like everything above.
		uint* meshIdx = nullptr; uint nVertices = 0;
		bool idxBound = false;
	};
	std::vector<BlasKeep> blasKeep;
	uint* slotOf = nullptr; uint* refitOrderAll = nullptr; int* refitLevelAll = nullptr;
	float* triStage = nullptr; size_t triStageCap = 0;        // triangles
	float4* undoPairs = nullptr; float4* undoPrims = nullptr; // records
	size_t undoPairCap = 0, undoPrimCap = 0;
	// rt_set_vertices (rt_api_vertices.inc): the host-memory form's copy of the vertices and the reduction record k_assemble_triangles fills
	// (scene pool, allocated by the first call that needs them; the record is read back into hostCounts[16..29])
	float* vtxStage = nullptr; size_t vtxStageCap = 0;
	VertexVerdict* vtxVerdict = nullptr;
	// rt_set_lights, rt_set_materials, rt_set_sky (rt_api_materials.inc): the material table as the description gave it (check_path_support's
	// rule runs over ALL of it after an edit) and the light table on the host, what the next copy is made from; the records in prims[] of
	// all BLASes; the light table's room on the device (0 until the first rt_set_lights gives it RT_MAX_LIGHTS records); the skydome's
	// array and its size in bytes (kept while the sky is off, so that switching it on again reuses it)
	std::vector<rt_material> matsHost;
	std::vector<DLight> lightsHost;
	uint32_t nMaterials = 0, primSlots = 0;
	int lightsCap = 0;
	unsigned char* skyMut = nullptr; size_t skyCap = 0;
	uint blasPairs = 0;          // pair records in front of the TLAS's: pairs[] holds blasPairs + S.tlasPairs records
	int32_t layoutScalars[14] = { 0 }; // RT_LAYOUT_SCALARS of the loaded scene (rt_scene_array)
	// camera
	DCamera C{};
	bool cameraSet = false;
	int pixelFilter = RT_FILTER_REFERENCE; // rt_set_pixel_filter: the kind of the path-mode camera samples (RenderParams::filter of their batches)
	rt_lens lens{ 0.0f, 1.0f }; // rt_set_lens: the thin lens of the path-mode camera samples (radius 0: off); lens_params puts it into a batch's RenderParams
	// rt_set_shutter: the camera at shutter close of the path-mode camera samples (C above is the camera at shutter open).  shutterDev is
	// its twelve floats on the device (allocated by rt_create, written by rt_set_shutter on the stream); set_lens puts its address into a
	// batch's RenderParams while shutterOn
	bool shutterOn = false;
	rt_camera shutterCam{};
	ShutterCam* shutterDev = nullptr;
	// accumulator
	float4* accum = nullptr;
	bool accumOwned = true;
	// the slot wavefront of rt_kernels.h (Whitted rounds with RT_MEGA=0, path batches above the slot budget, RT_COUNT_REFERENCE
	// launches, RT_STREAM=0): slots, status bytes, queues; it runs on the context's stream
	struct SlotState {
		PathState P{};
		Queues Q{};
		int stateSlots = 0, stateLights = -1;
		bool statePend = false, stateWide = false;
		std::vector<void*> allocs;
		int gridExtend = 0, gridConnect[WALK_FORMS] = {}; // resident blocks of the persistent traversal kernels (every wave owns a first chunk: none may wait for a slot); kExtend, kConnect
		void free_state() { free_pool(allocs); stateSlots = 0; }
	};
	SlotState slot;
	// the dense path-mode pipeline (rt_stream.h): its state, and the second stream for connect + light with its spill and events
	struct DenseState {
		StreamState T{};
		std::vector<void*> allocs;
		int cap = 0, lights = -1;
		bool wide = false;
		hipStream_t side = nullptr;
		uint* sideSpill = nullptr;
		hipEvent_t fork = nullptr, join = nullptr;
		int gridExtend = 0, gridConnect[WALK_FORMS] = {}, gridTraverse = 0; // kExtendS, kConnectS, k_traverse_s
		// resident blocks of the grid-stride shading kernels (a second, partial round of blocks would run at low occupancy): kShadeS, kLightS
		int gridShade[SHADE_FORMS] = {}, gridLight[LIGHT_FORMS] = {};
		// The primary-hit table (rt_stream.h PrimaryTable): Scene::FindNearest of every distinct camera ray of the frame, which round 0 of
		// a batch fans out to its samples.  Current while tableGen == sceneGen (the G-buffer's rule below); it outlives batches and calls.
		PrimaryTable tab{};
		std::vector<void*> tabAllocs;
		unsigned long long tableGen = 0;
		unsigned long long tablePending = 0, tablePendingGen = 0; // camera samples asked for while the table was stale at generation tablePendingGen
		int gridTable = 0;
		// The bounce table (rt_stream.h BounceTable): the first bounce off the glass and metal hits of the primary table, built with it and
		// current with it (bounceGen == sceneGen); a scene without such a material has none (in tabAllocs with the primary table)
		BounceTable btab{};
		unsigned long long bounceGen = 0;
		int gridBounce = 0; // resident blocks of k_bounce_table
		// The chain tables (rt_stream.h ChainLevel): chain[k - 2] is level k = 2 .. 4, built behind the bounce table from its records once the
		// batch's samples are worth it (primary_table_for); levels 2 .. chainLevels are current while chainGen == sceneGen.  chainCount: the
		// levels' record counters on the device.  In tabAllocs with the other tables.
		ChainLevel chain[3] = {};
		int* chainCount = nullptr;
		int chainLevels = 1;
		unsigned long long chainGen = 0;
		int gridChain = 0; // resident blocks of k_chain_table
		void free_state() { free_pool(allocs); cap = 0; }
		void destroy()
		{
			free_state();
			free_pool(tabAllocs);
			if (side) { (void)hipStreamSynchronize(side); (void)hipStreamDestroy(side); }
			if (sideSpill) (void)hipFree(sideSpill);
			if (fork) (void)hipEventDestroy(fork);
			if (join) (void)hipEventDestroy(join);
		}
	};
	DenseState dense;
	// Renderer::Trace as one persistent launch per frame (rt_mega.h).  With RT_MEGA_LEVELS=2 the context times this form against the level
	// form on the first batches of a shape and keeps the faster (the frames are identical either way; deep glass trees gain 40 % by levels,
	// shallow scenes lose 10 % to the extra launches)
	struct MegaForm {
		MegaState M{};
		std::vector<void*> allocs;
		int lanes = 0, grid = 0;
		struct Auto { unsigned nSamples = 0; int depth = 0; int tried[2] = { 0, 0 }; float ms[2] = { 0, 0 }; int choice = -1; } pick; // [0] single launch, [1] levels
		hipEvent_t ev[2] = { nullptr, nullptr };
		// longest first: per-sample cost of the last Whitted launch and the tile order made from it
		std::vector<void*> orderAllocs;
		uint* cost = nullptr; uint* order = nullptr; uint* hist = nullptr;
		size_t costCap = 0;
		unsigned costSamples = 0, costFirst = 0; // the batch cost[] describes (0 samples: nothing yet)
		void free_lanes() { free_pool(allocs); lanes = 0; }
		void free_order() { free_pool(orderAllocs); costCap = 0, costSamples = 0; }
		void destroy()
		{
			free_lanes(), free_order();
			for (int k = 0; k < 2; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
		}
	};
	MegaForm mega;
	// Whitted frames by tree levels (rt_mega.h LevelState): queues, term log
	struct LevelForm {
		LevelState V{};
		std::vector<void*> allocs;
		size_t cap = 0, samples = 0;
		int levels = 0, grid = 0;
		void free_state() { free_pool(allocs); cap = 0, levels = 0, samples = 0; }
	};
	LevelForm level;
	// pushes between contexts (rt_api_gather.inc: rt_gather_rows, rt_gather_stats_rows, rt_gather_active)
	hipEvent_t gatherDone = nullptr; // a push with this context as the source: its rows or pixels have arrived at the destination
	hipEvent_t gatherReady = nullptr; // ... and, recorded on the destination's stream before the push: what the destination had queued is done
	hipEvent_t rowsFree = nullptr;    // this context as a DESTINATION: recorded by rt_gather_begin on its stream, once per frame, before its own share is queued
	// Q-learning guided sampling (rt_qlearn.h)
	QTable Qt{};
	std::vector<void*> qAllocs;
	// traversal stack spill of the context's stream (rounds and batch queries) + flags
	uint* spill = nullptr;
	int gridBlocks = 0;
	std::vector<int> matTypes; // material types of the loaded scene, as rt_set_materials has left them (the bounce table's existence; measurement builds)
	int gridQuery = 0; // resident blocks of the query kernels
	float* gammaLut = nullptr; // DScene::gammaLut
	int* flags = nullptr; // [1] the status word of the Whitted, general and query kernels, [2] the leftover count of the wide occlusion query, [16..] their work heads
	DCounters* counters = nullptr;
	int counting = 0; // 0 off, 1 the reference's walk (RT_COUNT_REFERENCE), 2 the walk the timed kernels make (RT_COUNT_EXECUTED)
	bool profiling = false;
	rt_profile prof{};
	std::vector<Timer> timers; // pending event pairs, resolved lazily
	std::vector<int> timerKind;
	int* hostCounts = nullptr; // pinned, 32 words
	uint* resolveBuf = nullptr; // rt_resolve's device pixels (width * height), allocated on first use
	// G-buffer + denoiser (rt_api_denoise.inc).  sceneGen counts what makes the G-buffer stale (rt_upload_scene, rt_set_time, a camera
	// record that differs byte-wise): the G-buffer is current while aovGen == sceneGen
	rt_camera camRec;
	unsigned long long sceneGen = 1, aovGen = 0;
	float aovTmin = 0.0f;
	int gridAovs = 0;
	std::vector<void*> denoiseAllocs;
	float4* aovNrm = nullptr; float4* aovPos = nullptr; float4* aovAlb = nullptr; // width * height each, allocated on first use
	int* aovInst = nullptr; // the hit's TLAS instance per pixel (-1: none), allocated and current with the three above
	int* aovPrim = nullptr; // the hit's leaf slot in prims[] per pixel (-1: a miss, a light, a brute-force primitive), likewise
	float4* denoiseBuf[2] = { nullptr, nullptr }; // ping-pong of the filter's iterations
	float4* denoised = nullptr; // the buffer holding the last rt_denoise result (null: none yet)
	float4* samples = nullptr; // finished samples of the current batch, [frame][tile pixel]
	size_t sampleCap = 0;
	// adaptive sampling (rt_api_adaptive.inc): per-pixel statistics kept by k_accumulate<true> while stats.count != nullptr, and the list of
	// pixels rt_render_active renders (pixel indices, strictly ascending; nActive < 0: none installed).  The list is only indices: it
	// survives rt_clear, rt_set_camera and rt_upload_scene.
	PixelStats stats{};
	std::vector<void*> adaptiveAllocs; // the statistics
	std::vector<void*> activeAllocs;   // the list, the block totals of its compaction, its length on the device, the dilation's bitmasks
	uint* activeList = nullptr; uint* selectTotals = nullptr; int* activeCount = nullptr;
	DilateMasks dilate{};              // rt_select_active_dilated / rt_select_budget_dilated (rt_dilate.h): width * height bits each
	int nActive = -1;
	// budgeted passes (rt_api_budget.inc, rt_budget.h): the plan rt_select_budget made for the installed list -- per entry a budget, a first
	// frame and an offset into the pool, per sample of the pass a (pixel, frame) record.  planSamples < 0: no plan (never made, consumed by
	// rt_render_budget, or dropped by drop_plan because the counts or the list changed).
	BudgetPlan plan{};
	std::vector<void*> planAllocs;   // the per-entry arrays, the block totals of the budgets, the 64-bit total
	std::vector<void*> recordAllocs; // the per-sample records, grown to the largest pass
	uint* budgetTotals = nullptr; unsigned long long* planTotal = nullptr;
	size_t recordCap = 0;
	long long planSamples = -1;
	// reprojection (rt_api_reproject.inc): copies of the accumulator, the statistics, the G-buffer and the camera record taken by
	// rt_history_capture, which rt_reproject gathers from.  geomGen counts what changes the surfaces (rt_upload_scene, rt_set_time) and,
	// unlike sceneGen, not the camera: the history is valid while hist.gen == geomGen (0: none; rt_stats_enable(ctx, 0) drops it).
	// rt_reproject_motion follows instance moves, so it has a level of its own: shapeGen counts what geomGen counts EXCEPT rt_set_instances,
	// and the history is valid for it while hist.gen != 0 && hist.shapeGen == shapeGen.  For that call the capture also keeps the G-buffer's
	// instance indices and the instance records of its moment: xf on the device (a copy of inst[], what the kernel reads T' from), xfHost
	// beside the host mirror InstanceState::inst (what decides, bitwise, which instances have moved).
	// rt_reproject_deform follows deformations too, the third level: topoGen counts what shapeGen counts EXCEPT rt_set_triangles and
	// rt_set_time, and the history is valid for it while hist.gen != 0 && hist.topoGen == topoGen.  What it needs of the capture's
	// triangles is kept on first write (history_keep_blas, rt_api_build.inc): the first call that rewrites the records of BLAS b after a
	// capture copies them into keptBuf[b] (history pool, grows only) and writes keptDelta[b], the kernel's table: the distance in bytes
	// from a current record of BLAS b to its kept copy, 0 while there is none.  keptMark[b] says the copy is the capture's.
	struct History {
		float4* acc; float4* nrm; float4* pos; float4* alb;
		PixelStats stats;
		int* nCarried; // rt_reproject's count of carried pixels
		rt_camera cam;
		unsigned long long gen;
		int* inst; DInstance* xf; // width * height indices; RT_TLAS_MAX records
		unsigned long long shapeGen, topoGen;
		long long* keptDelta; size_t keptDeltaCap; // one entry per BLAS (at least one)
	};
	History hist{};
	std::vector<DInstance> histXfHost; // empty: the captured scene had no TLAS
	std::vector<float4*> keptBuf; std::vector<size_t> keptCap; // per BLAS: its kept records, their capacity in slots
	std::vector<char> keptMark;
	std::vector<long long> keptDeltaHost; // what keptDelta holds (and where its updates are copied from)
	std::vector<void*> historyAllocs;
	unsigned long long geomGen = 1, shapeGen = 1, topoGen = 1;
};

// whatever changes a pixel's count or the installed list takes the budget plan made from them along (rt_api_budget.inc)
static void drop_plan(rt_ctx* c) { c->planSamples = -1; }

static int fail(rt_ctx* c, int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	if (c) c->err = buf; else g_err = buf;
	return code;
}
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(c, RT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)

// v, copied into a new array of the scene pool with 'slack' spare elements behind it: kernels may read whole vectors past the end
template <typename T>
static int scene_array(rt_ctx* c, T** p, const std::vector<T>& v, size_t slack = 0)
{
	HIPCHK(c, dalloc(c->sceneAllocs, p, v.size() + slack));
	if (!v.empty()) HIPCHK(c, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
	return RT_OK;
}

// room for 'count' elements in a scene-pool array that only grows (the old one stays in the pool until the next upload)
template <typename T>
static int grow_scene_array(rt_ctx* c, T** p, size_t& cap, size_t count)
{
	if (cap >= count) return RT_OK;
	HIPCHK(c, dalloc(c->sceneAllocs, p, count));
	cap = count;
	return RT_OK;
}

// ---- the status word ---------------------------------------------------------------------------
// Every traversal launch leaves at most one word of trouble: counts[3] of the round pipelines' queues, flags[1] of the Whitted, general and
// query kernels.  This is the one place that knows its values; 'family' names the kernels in the debug-check message.
//   1 traversal stack   2 pending Whitted branches; from a general kernel (run_general): its call-frame stack is full (a query kernel never raises 2)
//   3 a level queue is full (run_levels repeats the frame as one launch before it gets here)   199 unknown link   100+ debug check
enum StatusFamily { FAM_WAVEFRONT = 0, FAM_WHITTED, FAM_QUERY, FAM_TRACE_GENERAL, FAM_SAMPLE_GENERAL };
static int decode_status(rt_ctx* c, int f, StatusFamily family)
{
	static const char* const name[] = { "a wavefront kernel", "the Whitted kernel", "a query kernel", "the general Trace kernel", "the general Sample kernel" };
	if (f == 0) return RT_OK;
	if (f == 199) return fail(c, RT_E_STATE, "a traversal launch met a link no step understands (corrupt tree?) and dropped rays");
	if (f >= 100) return fail(c, RT_E_STATE, "debug check %d failed in %s (RT_DEBUG_CHECKS build)", f - 100, name[family]);
	if (f == 3) return fail(c, RT_E_OVERFLOW, "a Whitted level queue overflowed");
	if (f == 2 && (family == FAM_TRACE_GENERAL || family == FAM_SAMPLE_GENERAL))
		return fail(c, RT_E_OVERFLOW, "the call-frame stack of %s is full: more than %d nested call frames in one call tree (shiny diffuse or glass hits inside one another); start at a lower depth",
			name[family], family == FAM_TRACE_GENERAL ? RT_TRACE_FRAMES : RT_SAMPLE_FRAMES);
	if (f == 2 && family != FAM_QUERY) return fail(c, RT_E_OVERFLOW, "more than %d pending Whitted branches in one pixel", RT_PEND_CAP);
	return fail(c, RT_E_OVERFLOW, "traversal stack deeper than %d entries", RT_STACK_MAX);
}
// flags[1] after what is queued on the context's stream, in stream order (the pinned hostCounts, then one synchronisation)
static int read_flags(rt_ctx* c, int& f)
{
	HIPCHK(c, hipMemcpyAsync(c->hostCounts, c->flags + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	f = c->hostCounts[0];
	return RT_OK;
}
// the general and query kernels' launches: did one of them report trouble?
static int check_overflow(rt_ctx* c, StatusFamily family = FAM_QUERY)
{
	int f = 0;
	const int rc = read_flags(c, f);
	if (rc != RT_OK) return rc;
	if (f != 0) (void)hipMemset(c->flags, 0, 2 * sizeof(int));
	return decode_status(c, f, family);
}

static int tuning(const rt_ctx* c) { return c->counting == RT_COUNT_EXECUTED ? RT_TUNE_CULL_COUNTED : 0; } // the traversal kernels' one launch-time flag (the thresholds are constants: rt_scene_dev.h)

// ---- profiling helpers ---------------------------------------------------------------------
enum { K_GENERATE = 0, K_EXTEND, K_SHADE, K_CONNECT, K_QUERY };
static void prof_begin(rt_ctx* c, int kind, hipStream_t stream = nullptr)
{
	if (!c->profiling) return;
	Timer t;
	(void)hipEventCreate(&t.a);
	(void)hipEventCreate(&t.b);
	(void)hipEventRecord(t.a, stream ? stream : c->stream);
	c->timers.push_back(t);
	c->timerKind.push_back(kind);
}
static void prof_end(rt_ctx* c, hipStream_t stream = nullptr)
{
	if (!c->profiling) return;
	(void)hipEventRecord(c->timers.back().b, stream ? stream : c->stream);
}
// a call that opened an entry and then refused: the entry is taken back
static void prof_cancel(rt_ctx* c)
{
	if (!c->profiling || c->timers.empty()) return;
	(void)hipEventDestroy(c->timers.back().a);
	(void)hipEventDestroy(c->timers.back().b);
	c->timers.pop_back();
	c->timerKind.pop_back();
}
// One build of a table of the dense pipeline (primary, bounce, chain: rt_api_render.inc) on the batch's stream: the work heads reset, a grid
// for a queue of n rays, the COUNT twin on counting launches.  prof >= 0: the build opens a profile entry of that kind behind the reset (the
// caller closes it).  args: the kernel's own, between the camera and t_min.
template <class K, class... A>
static int build_table(rt_ctx* c, hipStream_t st, const K (&twins)[2], size_t n, int resident, int prof, const A&... args)
{
	HIPCHK(c, hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), st)); // work heads: every build starts them again
	if (prof >= 0) prof_begin(c, prof, st);
	hipLaunchKernelGGL(twins[c->counting ? 1 : 0], dim3(short_grid(n, resident, RT_CHUNK)), dim3(RT_BLOCK), 0, st, c->S, c->C, args..., 0.001f, tuning(c), c->spill, c->flags + 16, &c->dense.T.counts[SC_FLAG], c->counters);
	return RT_OK;
}
static void prof_collect(rt_ctx* c)
{
	if (c->timers.empty()) return;
	(void)hipStreamSynchronize(c->stream);
	rt_kernel_time* slot[5] = { &c->prof.generate, &c->prof.extend, &c->prof.shade, &c->prof.connect, &c->prof.query };
	for (size_t i = 0; i < c->timers.size(); i++) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, c->timers[i].a, c->timers[i].b);
		slot[c->timerKind[i]]->launches++;
		slot[c->timerKind[i]]->ms += ms;
		(void)hipEventDestroy(c->timers[i].a);
		(void)hipEventDestroy(c->timers[i].b);
	}
	c->timers.clear();
	c->timerKind.clear();
}

// ---- the measurement builds' probes: empty in a default build -----------------------------------
#ifdef RT_TAIL_PROBE
// measurement build only: print, per traversal launch of the plain round loop (RT_FUSE=0), how long it ran with work left in
// its queue and how long its drain was
static void tail_probe_reset(hipStream_t st)
{
	const unsigned long long init[4] = { ~0ull, ~0ull, 0ull, 0ull };
	(void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tailProbe), init, sizeof(init), 0, hipMemcpyHostToDevice, st);
}
static void tail_probe_print(hipStream_t st, const char* what, int round)
{
	unsigned long long v[4];
	(void)hipStreamSynchronize(st);
	(void)hipMemcpyFromSymbol(v, HIP_SYMBOL(g_tailProbe), sizeof(v), 0, hipMemcpyDeviceToHost);
	fprintf(stderr, "tail probe %s round %d: busy %.1f us, drain %.1f us\n", what, round, (double)(v[1] - v[0]) / 100.0, (double)(v[2] - v[1]) / 100.0);
}
#else
static inline void tail_probe_reset(hipStream_t) {}
static inline void tail_probe_print(hipStream_t, const char*, int) {}
#endif

#ifdef RT_STEP_COUNT
// measurement build only: steps per nearest-hit ray of every extend launch of the plain round loop, by the material
// type of the hit the ray left from (previous round's hit record) -- which rays are the long ones?
static uint* g_stepBuf = nullptr;
static size_t g_stepCap = 0;
static void step_count_begin(rt_ctx* c, hipStream_t st, int nSlots)
{
	if (g_stepCap < (size_t)nSlots) { if (g_stepBuf) (void)hipFree(g_stepBuf); (void)hipMalloc((void**)&g_stepBuf, (size_t)nSlots * 4); g_stepCap = (size_t)nSlots; }
	(void)hipMemsetAsync(g_stepBuf, 0xFF, (size_t)nSlots * 4, st);
	(void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_stepOut), &g_stepBuf, sizeof(g_stepBuf), 0, hipMemcpyHostToDevice, st);
}
static void step_count_print(rt_ctx* c, hipStream_t st, const PathState& P, int parity, int round, const std::vector<int>& matType)
{
	(void)hipStreamSynchronize(st);
	const int n = P.nSlots;
	std::vector<uint> steps((size_t)n);
	std::vector<int2> prevHit((size_t)n);
	(void)hipMemcpy(steps.data(), g_stepBuf, (size_t)n * 4, hipMemcpyDeviceToHost);
	(void)hipMemcpy(prevHit.data(), P.hitId[1 - parity], (size_t)n * 8, hipMemcpyDeviceToHost);
	std::vector<uint> v;
	double sum = 0;
	unsigned long long byType[8] = { 0 }, longByType[8] = { 0 }, stepsByType[8] = { 0 }, byEnt[12] = { 0 }, longByEnt[12] = { 0 }, stepsByEnt[12] = { 0 };
	for (int i = 0; i < n; i++) {
		if (steps[(size_t)i] == 0xFFFFFFFFu) continue;
		{ const uint e = std::min(11u, steps[(size_t)i] >> 16); steps[(size_t)i] &= 0xFFFFu; byEnt[e]++, stepsByEnt[e] += steps[(size_t)i]; if (steps[(size_t)i] > 150) longByEnt[e]++; }
		v.push_back(steps[(size_t)i]);
		sum += steps[(size_t)i];
		int t = 7; // 7: no previous hit record (round 0)
		if (round > 0) { const int m = prevHit[(size_t)i].y; t = m >= 0 && m < (int)matType.size() ? matType[(size_t)m] & 3 : 6; }
		byType[t]++, stepsByType[t] += steps[(size_t)i];
		if (steps[(size_t)i] > 150) longByType[t]++;
	}
	if (v.empty()) return;
	std::sort(v.begin(), v.end());
	auto q = [&](double f) { return v[(size_t)std::min<double>((double)v.size() - 1, f * (double)v.size())]; };
	fprintf(stderr, "step count extend round %d: %zu rays, mean %.1f, p50 %u p90 %u p99 %u p99.9 %u p99.99 %u max %u\n", round, v.size(), sum / (double)v.size(), q(0.5), q(0.9), q(0.99), q(0.999), q(0.9999), v.back());
	for (int e = 0; e < 12; e++)
		if (byEnt[e]) fprintf(stderr, "   %d instance entries: %llu rays (%.2f %%), mean %.1f steps, %llu with > 150 steps (%.2f %% of them)\n", e, byEnt[e], 100.0 * (double)byEnt[e] / (double)v.size(), (double)stepsByEnt[e] / (double)byEnt[e], longByEnt[e], 100.0 * (double)longByEnt[e] / (double)byEnt[e]);
	for (int t = 0; t < 8; t++)
		if (byType[t]) fprintf(stderr, "   left a surface of type %d: %llu rays (%.1f %%), mean %.1f steps, %llu with > 150 steps (%.2f %% of them)\n", t, byType[t], 100.0 * (double)byType[t] / (double)v.size(), (double)stepsByType[t] / (double)byType[t], longByType[t], 100.0 * (double)longByType[t] / (double)byType[t]);
}
#else
static inline void step_count_begin(rt_ctx*, hipStream_t, int) {}
static inline void step_count_print(rt_ctx*, hipStream_t, const PathState&, int, int, const std::vector<int>&) {}
#endif
#ifdef RT_SECTION_PROBE
// measurement build only: per traversal launch of the plain round loop, the waves' cycles by section (rt_scene_dev.h)
static void section_probe_reset(hipStream_t st)
{
	const unsigned long long zero[16] = { 0 };
	(void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_sectionProbe), zero, sizeof(zero), 0, hipMemcpyHostToDevice, st);
}
static void section_probe_print(hipStream_t st, const char* what, int round)
{
	unsigned long long v[16];
	(void)hipStreamSynchronize(st);
	(void)hipMemcpyFromSymbol(v, HIP_SYMBOL(g_sectionProbe), sizeof(v), 0, hipMemcpyDeviceToHost);
	const double tot = (double)v[7] > 0 ? (double)v[7] : 1;
	fprintf(stderr, "section probe %s round %d: refill %.1f%% (%llu, %.0f cyc)  pair wait %.1f%% rest %.1f%% (%llu steps, %.0f + %.0f cyc)  leaf wait %.1f%% rest %.1f%% (%llu, %.0f + %.0f)  enter %.1f%% (%llu, %.0f)  exit %.1f%% (%llu, %.0f)  other %.1f%%  iterations %llu (%.0f cyc)\n",
	        what, round, 100 * v[0] / tot, v[13], v[13] ? (double)v[0] / v[13] : 0, 100 * v[1] / tot, 100 * v[2] / tot, v[9], v[9] ? (double)v[1] / v[9] : 0, v[9] ? (double)v[2] / v[9] : 0,
	        100 * v[3] / tot, 100 * v[4] / tot, v[10], v[10] ? (double)v[3] / v[10] : 0, v[10] ? (double)v[4] / v[10] : 0, 100 * v[5] / tot, v[11], v[11] ? (double)v[5] / v[11] : 0,
	        100 * v[6] / tot, v[12], v[12] ? (double)v[6] / v[12] : 0, 100 * (tot - v[0] - v[1] - v[2] - v[3] - v[4] - v[5] - v[6]) / tot, v[8], v[8] ? tot / v[8] : 0);
}
#else
static inline void section_probe_reset(hipStream_t) {}
static inline void section_probe_print(hipStream_t, const char*, int) {}
#endif

