// rt_render[_rows], rt_trace_batch[_energy]: path state, the slot wavefront's round loop, Whitted frames by tree levels / as one launch, the dense
// path-mode pipeline (run_rounds_stream), the dispatcher that puts a batch of samples on one of them (trace_samples), batches of frames and
// k_accumulate.  Included by rt_api.hip.
// ---- path state -------------------------------------------------------------------------------
static int ensure_state(rt_ctx* c, int nSlots, bool pend)
{
	rt_ctx::SlotState& pl = c->slot;
	const bool wide = c->S.wide != nullptr; // the 4-wide occlusion walk hands rays back through Q.leftover: allocated only for scenes that have it
	if (pl.stateSlots >= nSlots && pl.stateLights == c->S.nLights && (pl.statePend || !pend) && (pl.stateWide || !wide)) { pl.P.nSlots = nSlots; return RT_OK; }
	HIPCHK(c, hipStreamSynchronize(c->stream));
	pl.free_state();
	PathState P{};
	const size_t n = (size_t)nSlots;
	for (int b = 0; b < 2; b++) { HIPCHK(c, dalloc(pl.allocs, &P.O[b], n)); HIPCHK(c, dalloc(pl.allocs, &P.D[b], n)); }
	for (int b = 0; b < 2; b++) { HIPCHK(c, dalloc(pl.allocs, &P.hitN[b], n)); HIPCHK(c, dalloc(pl.allocs, &P.hitId[b], n)); }
	HIPCHK(c, dalloc(pl.allocs, &P.hitP, n));
	HIPCHK(c, dalloc(pl.allocs, &P.W, n));
	HIPCHK(c, dalloc(pl.allocs, &P.E, n));
	HIPCHK(c, dalloc(pl.allocs, &P.L, n));
	HIPCHK(c, dalloc(pl.allocs, &P.sh, n * (size_t)(c->S.nLights + 1)));
	HIPCHK(c, dalloc(pl.allocs, &P.vis, n * (size_t)(c->S.nLights + 1)));
	if (pend) {
		HIPCHK(c, dalloc(pl.allocs, &P.pend, n * RT_PEND_CAP * 4));
		HIPCHK(c, dalloc(pl.allocs, &P.pendCount, n));
	}
	Queues Q{};
	HIPCHK(c, dalloc(pl.allocs, &P.status, n + 16));
	HIPCHK(c, dalloc(pl.allocs, &Q.active, n));
	HIPCHK(c, dalloc(pl.allocs, &Q.shadow, n));
	HIPCHK(c, dalloc(pl.allocs, &Q.ended, n));
	HIPCHK(c, dalloc(pl.allocs, &Q.leftover, wide ? n * (size_t)(c->S.nLights > 0 ? c->S.nLights : 1) : (size_t)4));
	HIPCHK(c, dalloc(pl.allocs, &Q.counts, 16));
	HIPCHK(c, dalloc(pl.allocs, &Q.heads, (size_t)2 * RT_HEADS * RT_HEAD_STRIDE));
	HIPCHK(c, hipMemset(Q.counts, 0, 16 * sizeof(int)));
	P.nSlots = nSlots;
	pl.P = P, pl.Q = Q;
	pl.stateSlots = nSlots, pl.stateLights = c->S.nLights, pl.statePend = pend, pl.stateWide = wide;
	return RT_OK;
}
static int ensure_samples(rt_ctx* c, size_t count)
{
	if (c->sampleCap >= count) return RT_OK;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->samples) (void)hipFree(c->samples);
	c->samples = nullptr, c->sampleCap = 0;
	HIPCHK(c, hipMalloc((void**)&c->samples, count * sizeof(float4)));
	c->sampleCap = count;
	return RT_OK;
}

static int slot_budget(const rt_ctx* c)
{
	// slots in flight.  Every round pays a fixed tail: once the work head runs dry the waves of a traversal
	// launch drain unevenly, and the longest rays finish alone at memory latency per step (0.3-0.8 ms per traversal
	// launch whatever it held, DESIGN.md finding 38).  Fewer, larger rounds win until every sample of the batch has its
	// own slot: 16M -> 64M -> 128M slots took the 1080p x 64 spp frame from 97.8 to 79.0 to 76.4 ms (round 1), and
	// 128M -> 256M takes 1080p x 256 spp from 148 to 138.5 ms and 4K x 1024 spp from 2.96 to 2.88 s (32-frame instead
	// of 16-frame batches).  ~250 B of state per slot: 256M slots = 67 GB of the 288 GB, allocated for the slots a batch
	// really has.  The shadow rays of a round are counted in an int: slots x lights stays below 2^31.  RT_SLOTS overrides.
	const long v = c ? c->knobs.slots : 0;
	long b = v > 0 ? v : (1l << 28);
	const long lights = c && c->S.nLights > 1 ? c->S.nLights : 1;
	if (b > 0x7FFFFFFFl / lights) b = 0x7FFFFFFFl / lights;
	return (int)b;
}
static int segments_per_sample(int mode, int depth, int nLights)
{
	// path: at most 5 segments (depth 4..0); Whitted: at most 2^depth - 1 glass segments, times the
	// mirror branches of shiny diffuse hits
	if (mode == RT_MODE_PATH) return depth + 1;
	return (1 << (depth < 12 ? depth : 12)) * (1 + nLights);
}

// Scene::IsOccluded for the shadow queue, by the walk rt_forms.h chooses: a wide walk is followed by the binary walk over the (normally
// empty) list of rays it handed back because they are not clean.
static void launch_connect(rt_ctx* c, hipStream_t st, const PathState& P, const Queues& Q, int parity, uint* spill)
{
	// the any-hit walk has its own thresholds (RT_REFILL_ANY, RT_STEPMIN_ANY, RT_PAIRAGAIN_ANY)
	const int tun = tuning(c);
	const int walk = any_hit_walk(c->counting != 0, c->S.wide != nullptr, false); // (no 8-wide walk over slots)
	hipLaunchKernelGGL(kConnect[walk], dim3(c->slot.gridConnect[walk]), dim3(RT_BLOCK), 0, st, c->S, P, Q, parity, tun, spill, c->counters + 1);
	if (!walk_is_wide(walk)) return;
	hipLaunchKernelGGL(k_round_begin, dim3(1), dim3(1), 0, st, Q, 0, 0, 4);
	hipLaunchKernelGGL(kConnect[WALK_LISTED], dim3(c->slot.gridConnect[WALK_LISTED]), dim3(RT_BLOCK), 0, st, c->S, P, Q, parity, tun, spill, c->counters + 1);
}
// The round loop of the slot wavefront (rt_kernels.h), shared by rt_render_rows and rt_trace_batch: Whitted rounds (RT_MEGA=0 and
// counting launches), path batches with fewer slots than samples, RT_COUNT_REFERENCE launches, RT_STREAM=0.  One kernel at a time on
// the context's stream.  (Several sample pools on separate streams, and extend(r + 1) beside connect(r) on two streams or as one
// launch, were measured on this pipeline in rounds 1-2 and superseded by the dense pipeline of rt_stream.h:
// profiles/patches/slot_pipeline_pools_and_fusing.diff.)
static int run_rounds(rt_ctx* c, const RenderParams& R, int maxRounds, int knownRounds)
{
	// knownRounds > 0: the caller knows how many rounds empty the slots (path mode with a slot per sample:
	// one round per path segment, depth + 1 of them), so no queue length is read back before the end
	if (knownRounds > 0) maxRounds = knownRounds;
	const int mode = R.mode;
	const float t_min = mode == RT_MODE_WHITTED ? (float)1e-6 : 0.001f; // renderer.cpp:24, :131
	const int grid = c->gridBlocks;
	PathState P = c->slot.P;
	if (mode != RT_MODE_WHITTED) P.pend = nullptr, P.pendCount = nullptr;
	const Queues Q = c->slot.Q;
	hipStream_t st = c->stream;
	prof_begin(c, K_GENERATE, st);
	hipLaunchKernelGGL(k_generate, dim3((P.nSlots + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, c->S, c->C, R, P, Q);
	prof_end(c, st);
	int parity = 0, rc = RT_OK;
	for (int round = 0; round < maxRounds && rc == RT_OK; round++) {
		// round 0 of a batch with a slot per sample: every slot is ACTIVE, so no queue is built and extend /
		// shade address slots directly
		const int allActive = round == 0 && R.finishInline ? P.nSlots : 0;
		hipLaunchKernelGGL(k_round_begin, dim3(1), dim3(1), 0, st, Q, P.pendCount ? 0 : 1, allActive, 3);
		if (!allActive) hipLaunchKernelGGL(k_compact, dim3(grid / 2), dim3(RT_COMPACT_BLOCK), 0, st, P, (int)ST_ACTIVE, Q.active, &Q.counts[0]);
		tail_probe_reset(st);
		section_probe_reset(st);
		step_count_begin(c, st, P.nSlots);
		prof_begin(c, K_EXTEND, st);
		{
			auto extendKernel = kExtend[c->counting ? 1 : 0][allActive ? 1 : 0];
			hipLaunchKernelGGL(extendKernel, dim3(c->slot.gridExtend), dim3(RT_BLOCK), 0, st, c->S, P, Q, parity, t_min, tuning(c), c->spill, c->counters);
		}
		prof_end(c, st);
		tail_probe_print(st, "extend", round);
		section_probe_print(st, "extend", round);
		step_count_print(c, st, P, parity, round, c->matTypes);
		prof_begin(c, K_SHADE, st);
		hipLaunchKernelGGL(k_shade, dim3(grid), dim3(RT_BLOCK), 0, st, c->S, c->C, R, P, Q, parity, round == 0 && R.finishInline ? 1 : 0);
		prof_end(c, st);
		hipLaunchKernelGGL(k_compact, dim3(grid / 2), dim3(RT_COMPACT_BLOCK), 0, st, P, (int)ST_SHADOW, Q.shadow, &Q.counts[2]);
		tail_probe_reset(st);
		section_probe_reset(st);
		prof_begin(c, K_CONNECT, st);
		launch_connect(c, st, P, Q, parity, c->spill);
		prof_end(c, st);
		tail_probe_print(st, "connect", round);
		section_probe_print(st, "connect", round);
		prof_begin(c, K_SHADE, st);
		hipLaunchKernelGGL(k_light, dim3(grid), dim3(RT_BLOCK), 0, st, c->S, R, P, Q, parity);
		if (!R.finishInline) {
			hipLaunchKernelGGL(k_compact, dim3(grid / 2), dim3(RT_COMPACT_BLOCK), 0, st, P, (int)ST_ENDED, Q.ended, &Q.counts[1]);
			hipLaunchKernelGGL(k_finish, dim3(grid), dim3(RT_BLOCK), 0, st, c->S, c->C, R, P, Q, parity);
		}
		prof_end(c, st);
		parity = 1 - parity;
		// look at the queue lengths every few rounds (one small D2H copy + sync); the loop stops when the active queue is empty
		if ((knownRounds <= 0 && (round & 3) == 3) || round + 1 == maxRounds) {
			HIPCHK(c, hipMemcpyAsync(c->hostCounts, Q.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
			HIPCHK(c, hipStreamSynchronize(st));
			const int* hc = c->hostCounts;
			if (hc[3] != 0) (void)hipMemsetAsync(Q.counts + 3, 0, sizeof(int), st);
			rc = decode_status(c, hc[3], FAM_WAVEFRONT);
			if (rc != RT_OK || hc[0] == 0 || knownRounds > 0) break;
			if (round + 1 == maxRounds) rc = fail(c, RT_E_STATE, "paths still active after %d rounds", maxRounds);
		}
	}
	if (rc != RT_OK) return rc;
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}

// ---- Whitted frames as one persistent launch (rt_mega.h) -----------------------------------------------
#define RT_LEVEL_SAMPLES_MAX (16u << 20) // larger batches keep the single launch: their drain is a small part of them, and the queues would take GBs
// the status word of a Whitted launch, read after it and cleared for the next one; 3 is run_levels' to answer
static int whitted_status(rt_ctx* c, int& f)
{
	const int rc = read_flags(c, f);
	if (rc == RT_OK && f != 0) (void)hipMemsetAsync(c->flags, 0, 2 * sizeof(int), c->stream);
	return rc;
}

// Whitted frames by tree levels (rt_mega.h): depth launches of k_whitted_level + k_whitted_reduce.  *redo: a queue overflowed.
static int run_levels(rt_ctx* c, const RenderParams& R, const MegaState& M0, int grid0, bool* redo)
{
	rt_ctx::LevelForm& lv = c->level;
	const int levels = R.maxDepth;
	const size_t cap = ((size_t)2 * R.nSamples + 65536 + 63) & ~(size_t)63;
	if (lv.cap < cap || lv.levels < levels || lv.samples < (size_t)R.nSamples) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		lv.free_state();
		LevelState V{};
		std::vector<void*>& A = lv.allocs;
		HIPCHK(c, dalloc(A, &V.seg[0], cap * 4)); HIPCHK(c, dalloc(A, &V.seg[1], cap * 4));
		HIPCHK(c, dalloc(A, &V.count, (size_t)RT_LEVEL_MAX + 2));
		HIPCHK(c, dalloc(A, &V.termKey, cap * (size_t)levels)); HIPCHK(c, dalloc(A, &V.termVal, cap * (size_t)levels));
		HIPCHK(c, dalloc(A, &V.head, (size_t)R.nSamples));
		V.cap = (int)cap;
		lv.V = V, lv.cap = cap, lv.levels = levels, lv.samples = (size_t)R.nSamples;
	}
	LevelState V = lv.V;
	V.qcap = V.cap;
	if (c->knobs.levelCap >= 64 && c->knobs.levelCap < V.cap) V.qcap = c->knobs.levelCap & ~63; // tests: queues that overflow
	(void)hipMemsetAsync(V.count, 0, (RT_LEVEL_MAX + 2) * sizeof(int), c->stream);
	(void)hipMemsetAsync(V.head, 0xFF, (size_t)R.nSamples * sizeof(int), c->stream);
	prof_begin(c, K_EXTEND);
	for (int level = 0; level < levels; level++) {
		if (level > 0) (void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
		V.level = level;
		const int grid = level == 0 ? std::min(grid0, lv.grid) : lv.grid;
		hipLaunchKernelGGL(k_whitted_level, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, R, M0, V, tuning(c), c->spill, c->flags);
	}
	hipLaunchKernelGGL(k_whitted_reduce, dim3((R.nSamples + 255) / 256), dim3(256), 0, c->stream, R, V);
	prof_end(c);
	int f = 0;
	int rc = whitted_status(c, f);
	if (rc != RT_OK) return rc;
	*redo = f == 3;
	if (f == 3) return RT_OK;
	rc = decode_status(c, f, FAM_WHITTED);
	if (rc != RT_OK) return rc;
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}

static int run_mega(rt_ctx* c, const RenderParams& R0)
{
	rt_ctx::MegaForm& mg = c->mega;
	RenderParams R = R0;
	// deal the frame out in tiles of 64 pixels from all over it (rt_mega.h sample_of): the multiplier nearest nTiles / 61 that is coprime to nTiles
	if (R.nSamples >= 16384) {
		auto gcd = [](unsigned a, unsigned b) { while (b) { const unsigned t = a % b; a = b; b = t; } return a; };
		R.permShift = 3; // tiles of 8 pixels (profiles/r03_tick_mega.txt: tile sizes 2^0 .. 2^6)
		const unsigned nTiles = (R.nSamples + (1u << R.permShift) - 1) >> R.permShift;
		unsigned p = nTiles / 61 | 1;
		while (gcd(p, nTiles) != 1) p += 2;
		R.permMul = p;
	}
	const int gridMax = mg.grid;
	const int lanes = std::max(mg.grid, c->level.grid) * RT_BLOCK; // run_levels indexes the same arrays by lane of ITS grid
	if (mg.lanes < lanes) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		mg.free_lanes();
		MegaState M{};
		std::vector<void*>& A = mg.allocs;
		const size_t n = (size_t)lanes;
		HIPCHK(c, dalloc(A, &M.O, n)); HIPCHK(c, dalloc(A, &M.D, n)); HIPCHK(c, dalloc(A, &M.W, n)); HIPCHK(c, dalloc(A, &M.E, n)); HIPCHK(c, dalloc(A, &M.L, n));
		HIPCHK(c, dalloc(A, &M.hI, n)); HIPCHK(c, dalloc(A, &M.hN, n)); HIPCHK(c, dalloc(A, &M.hA, n)); HIPCHK(c, dalloc(A, &M.hS, n));
		HIPCHK(c, dalloc(A, &M.pend, n * RT_PEND_CAP * 4));
		M.lanes = lanes;
		mg.M = M, mg.lanes = lanes;
	}
	int grid = ((int)R.nSamples + RT_SHORT_QUEUE_RAYS * 64 - 1) / (RT_SHORT_QUEUE_RAYS * 64) + 1; // a short queue does not need the whole grid
	if (grid > gridMax) grid = gridMax;
	(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
	// longest first (rt_mega.h): a Whitted launch over the samples the last one rendered deals its tiles out by what they cost then
	MegaState M = mg.M;
	M.cost = nullptr, M.order = nullptr;
	M.nWork = (int)(((R.nSamples + (1u << R.permShift) - 1) >> R.permShift) << R.permShift);
	const int megaLevels = c->knobs.megaLevels;
	bool useLevels = megaLevels && R.mode == RT_MODE_WHITTED && !R.customO && R.maxDepth >= 1 && R.maxDepth <= RT_LEVEL_MAX && R.nSamples <= RT_LEVEL_SAMPLES_MAX && c->S.nLights <= 32;
	// RT_MEGA_LEVELS=2: both forms give the same frame, so the context may simply time them -- each form twice on the first four batches
	// of a shape (the first run of a form pays its allocations and has no cost history), then whichever was faster
	int probe = -1; // the form this batch is timed as
	if (useLevels && megaLevels == 2) {
		auto& A = mg.pick;
		if (A.nSamples != R.nSamples || A.depth != R.maxDepth) A = {}, A.nSamples = R.nSamples, A.depth = R.maxDepth;
		if (A.choice < 0) {
			probe = A.tried[0] < 2 ? 0 : 1;
			if (!mg.ev[0]) { (void)hipEventCreate(&mg.ev[0]); (void)hipEventCreate(&mg.ev[1]); }
			(void)hipEventRecord(mg.ev[0], c->stream);
		}
		useLevels = A.choice >= 0 ? A.choice == 1 : probe == 1;
	}
	auto probe_end = [&]() {
		if (probe < 0) return;
		auto& A = mg.pick;
		float ms = 0;
		(void)hipEventRecord(mg.ev[1], c->stream);
		(void)hipEventSynchronize(mg.ev[1]);
		(void)hipEventElapsedTime(&ms, mg.ev[0], mg.ev[1]);
		A.ms[probe] = ms, A.tried[probe]++;
		if (A.tried[0] >= 2 && A.tried[1] >= 2) A.choice = A.ms[1] < A.ms[0] ? 1 : 0;
	};
	if (c->knobs.megaLpt && R.mode == RT_MODE_WHITTED && R.permMul && !R.customO) {
		const unsigned tilesPerHead = RT_HEADS * 8u; // sub-queues of n / RT_HEADS entries, a multiple of 64 entries = 8 tiles of 8
		const unsigned nTiles = (R.nSamples + (1u << R.permShift) - 1) >> R.permShift;
		// k_mega_order's slot mapping is a bijection only when groups = nTilesPad / 8 is a multiple of RT_HEADS: pad to 8 * RT_HEADS tiles whatever the tile size
		const unsigned unit = std::max(tilesPerHead * (64u >> R.permShift ? 64u >> R.permShift : 1u) / 8u, 8u * RT_HEADS);
		const unsigned nTilesPad = (nTiles + unit - 1) / unit * unit;
		if (mg.costCap < (size_t)R.nSamples) {
			HIPCHK(c, hipStreamSynchronize(c->stream));
			mg.free_order();
			HIPCHK(c, dalloc(mg.orderAllocs, &mg.cost, (size_t)R.nSamples));
			HIPCHK(c, dalloc(mg.orderAllocs, &mg.order, (size_t)nTilesPad + 1024));
			HIPCHK(c, dalloc(mg.orderAllocs, &mg.hist, (size_t)2 * RT_MEGA_BUCKETS));
			mg.costCap = (size_t)R.nSamples;
		}
		if (mg.costSamples == R.nSamples && mg.costFirst == R.sampleFirst) {
			(void)hipMemsetAsync(mg.hist, 0, 2 * RT_MEGA_BUCKETS * sizeof(uint), c->stream);
			const unsigned blocks = (nTilesPad + RT_MEGA_ORDER_BLOCK - 1) / RT_MEGA_ORDER_BLOCK;
			hipLaunchKernelGGL(k_mega_hist, dim3(blocks), dim3(RT_MEGA_ORDER_BLOCK), 0, c->stream, mg.cost, R.permShift, R.nSamples, nTilesPad, mg.hist);
			hipLaunchKernelGGL(k_mega_order, dim3(blocks), dim3(RT_MEGA_ORDER_BLOCK), 0, c->stream, mg.cost, R.permShift, R.nSamples, nTilesPad, mg.hist, mg.order);
			M.order = mg.order;
			M.nWork = (int)(nTilesPad << R.permShift);
		}
		M.cost = mg.cost;
		mg.costSamples = R.nSamples, mg.costFirst = R.sampleFirst;
	}
	// a flush runs the body of Trace for the lanes that finished a query: it waits for more of them than a plain store does (32 instead of 16: 5.0 -> 4.85 ms)
	if (useLevels) {
		bool redo = false;
		const int rc = run_levels(c, R, M, grid, &redo); // level 0 deals its tiles out like the single launch (M.order), and records what they cost
		if (rc != RT_OK || !redo) { probe_end(); return rc; }
		probe = -1, mg.pick.choice = 0; // this scene overflows the level queues: the single launch from now on
		// a queue overflowed (more than two live branches per sample on average): the frame again, as one launch
		(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream);
	}
	tail_probe_reset(c->stream);
	prof_begin(c, K_EXTEND);
	hipLaunchKernelGGL(k_whitted_mega, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, R, M, tuning(c), c->spill, c->flags);
	prof_end(c);
	tail_probe_print(c->stream, "mega", 0);
	int f = 0;
	int rc = whitted_status(c, f);
	if (rc == RT_OK) rc = decode_status(c, f, FAM_WHITTED);
	if (rc != RT_OK) return rc;
	HIPCHK(c, hipGetLastError());
	probe_end();
	return RT_OK;
}

// ---- the dense path-mode pipeline (rt_stream.h) ------------------------------------------------------
static int ensure_stream_state(rt_ctx* c, int n)
{
	const bool wide = c->S.wide != nullptr || c->S.wide8 != nullptr;
	if (!c->dense.side) {
		HIPCHK(c, hipStreamCreate(&c->dense.side));
		HIPCHK(c, hipMalloc((void**)&c->dense.sideSpill, (size_t)(RT_STACK_MAX - RT_STACK_ROWS_MIN) * c->gridBlocks * RT_BLOCK * sizeof(uint)));
		HIPCHK(c, hipEventCreateWithFlags(&c->dense.fork, hipEventDisableTiming));
		HIPCHK(c, hipEventCreateWithFlags(&c->dense.join, hipEventDisableTiming));
	}
	if (c->dense.cap >= n && c->dense.lights == c->S.nLights && (c->dense.wide || !wide)) return RT_OK;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipStreamSynchronize(c->dense.side));
	c->dense.free_state();
	StreamState T{};
	// k_assign writes the positions of whole 16-entry vectors and the compactions read whole 16-byte vectors of class bytes
	const size_t cap = ((size_t)n + 1023) & ~(size_t)1023;
	const size_t nl = (size_t)(c->S.nLights > 0 ? c->S.nLights : 1);
	std::vector<void*>& A = c->dense.allocs;
	for (int b = 0; b < 2; b++) {
		HIPCHK(c, dalloc(A, &T.O[b], cap)); HIPCHK(c, dalloc(A, &T.D[b], cap));
		HIPCHK(c, dalloc(A, &T.hitN[b], cap)); HIPCHK(c, dalloc(A, &T.hitId[b], cap));
		HIPCHK(c, dalloc(A, &T.W[b], cap)); HIPCHK(c, dalloc(A, &T.E[b], cap)); HIPCHK(c, dalloc(A, &T.L[b], cap));
		HIPCHK(c, dalloc(A, &T.cls[b], cap));
	}
	HIPCHK(c, dalloc(A, &T.pos, cap / 64 + 64)); // a pair of bases per group of 64 entries
	HIPCHK(c, dalloc(A, &T.shI, cap)); HIPCHK(c, dalloc(A, &T.shX, cap)); // a shadow record: 24 B ...
	HIPCHK(c, dalloc(A, &T.shP, cap * nl));                               // ... + 16 B per light for connect
	HIPCHK(c, dalloc(A, &T.vis, cap * nl));
	HIPCHK(c, dalloc(A, &T.traceQ, cap));
	HIPCHK(c, dalloc(A, &T.leftover, wide ? cap * nl : (size_t)4));
	HIPCHK(c, dalloc(A, &T.counts, 16));
	HIPCHK(c, dalloc(A, &T.heads, (size_t)2 * RT_HEADS * RT_HEAD_STRIDE));
	HIPCHK(c, hipMemset(T.counts, 0, 16 * sizeof(int)));
	T.cap = (int)cap;
	c->dense.T = T;
	c->dense.cap = (int)cap, c->dense.lights = c->S.nLights, c->dense.wide = wide;
	return RT_OK;
}
static void launch_connect_s(rt_ctx* c, hipStream_t st, const StreamState& T, int round, uint* spill)
{
	const int tun = tuning(c);
	const int walk = any_hit_walk(c->counting != 0, c->S.wide != nullptr, c->S.wide8 != nullptr);
	hipLaunchKernelGGL(kConnectS[walk], dim3(c->dense.gridConnect[walk]), dim3(RT_BLOCK), 0, st, c->S, T, round, tun, spill, c->counters + 1);
	if (!walk_is_wide(walk)) return;
	// the binary walk over the rays the wide walk handed back (not clean: normally none)
	hipLaunchKernelGGL(k_stream_begin, dim3(1), dim3(1), 0, st, T);
	hipLaunchKernelGGL(kConnectS[WALK_LISTED], dim3(c->dense.gridConnect[WALK_LISTED]), dim3(RT_BLOCK), 0, st, c->S, T, round, tun, spill, c->counters + 1);
}
// Does round 0 of this batch read the primary-hit table (rt_stream.h)?  A current table is read; a stale one is rebuilt -- on the batch's
// stream, before generate, with no synchronisation: its status word is the round pipeline's -- once the camera samples asked for since it
// went stale are worth the build: one trace of (width + 2) x (height + 2) rays, always of the whole frame, so that row shards and
// whole frames share it.  Below that a batch keeps today's round 0 (a one-frame Tick whose camera moves every call never builds).
// The table outlives batches, calls and Ticks: a static camera accumulating frames is what a path tracer does (a camera change
// resets the accumulator anyway).
// The bounce table (rt_stream.h BounceTable) is built right behind it, from its records, inside the same profile entry, and is current
// exactly when it is (*bounce); a scene without a glass or metal material has none.
// The chain tables (rt_stream.h ChainLevel), levels 2 .. RT_BOUNCE_DEPTH, are built behind the bounce table on the same stream, work heads,
// spill buffer and status word, inside the same profile entry -- at a threshold of their own, RT_BOUNCE_DEPTH_MIN times the primary table's:
// a batch that has to rebuild pays 1-3 more builds for walks that shorten only over many frames.  When the threshold is crossed after levels
// 0-1 were built, the levels are built then, as an entry of their own.  *chain: the levels a batch may read, 1 (the bounce table) .. depth.
static int build_chain_tables(rt_ctx* c, hipStream_t st)
{
	rt_ctx::DenseState& d = c->dense;
	const size_t records = (size_t)(c->width + 2) * (size_t)(c->height + 2);
	const int depth = c->knobs.bounceDepth;
	const size_t cap = c->knobs.chainCap < 0 ? records : std::min((size_t)c->knobs.chainCap, (size_t)0x3FFFFFFF);
	if (!d.chainCount) HIPCHK(c, dalloc(d.tabAllocs, &d.chainCount, (size_t)4));
	for (int k = 2; k <= depth; k++) {
		ChainLevel& L = d.chain[k - 2];
		if (L.A) continue;
		HIPCHK(c, dalloc(d.tabAllocs, &L.A, cap)); HIPCHK(c, dalloc(d.tabAllocs, &L.B, cap));
		HIPCHK(c, dalloc(d.tabAllocs, &L.RO, cap)); HIPCHK(c, dalloc(d.tabAllocs, &L.RD, cap));
		HIPCHK(c, dalloc(d.tabAllocs, &L.parent, cap));
		L.count = d.chainCount + (k - 2), L.cap = (int)cap;
	}
	HIPCHK(c, hipMemsetAsync(d.chainCount, 0, 4 * sizeof(int), st));
	// (a capacity of 0: every link of the bounce table is the 0 k_bounce_table wrote, and no level has a record)
	for (int k = 2; k <= depth && cap > 0; k++) {
		const ChainLevel& L = d.chain[k - 2];
		const ChainLevel up = k == 2 ? ChainLevel{} : d.chain[k - 3];
		const size_t nUp = k == 2 ? 2 * records : cap;
		hipLaunchKernelGGL(k_chain_link, dim3((unsigned)((nUp + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, st, c->S, k == 2 ? d.btab.B : up.B, k == 2 ? (const int*)nullptr : (const int*)up.count, (int)nUp, L);
		const int rc = build_table(c, st, kChainTable, cap, d.gridChain, -1, d.tab, d.btab, up, L);
		if (rc != RT_OK) return rc;
	}
	d.chainLevels = depth, d.chainGen = c->sceneGen;
	return RT_OK;
}
static int primary_table_for(rt_ctx* c, const RenderParams& R, hipStream_t st, bool* use, bool* bounce, int* chain)
{
	rt_ctx::DenseState& d = c->dense;
	*use = false, *bounce = false, *chain = 1;
	const bool wantChain = c->knobs.bounceDepth > 1 && c->knobs.bounceTable != 0 && !c->Qt.on; // (the sampler's shade reads no table)
	// (a filter kind: the samples of a pixel take distinct rays, which no table of the frame's integer-pixel rays holds; such a batch does
	// not count towards a rebuild either)
	if (!c->knobs.primaryTable || R.customO || R.filter != RT_FILTER_REFERENCE) return RT_OK;
	const size_t records = (size_t)(c->width + 2) * (size_t)(c->height + 2);
	const unsigned long long chainAt = (unsigned long long)c->knobs.chainMin * (unsigned long long)c->knobs.tableMin * records;
	if (d.tableGen == c->sceneGen) {
		*use = true, *bounce = d.bounceGen == c->sceneGen;
		if (*bounce && wantChain && d.chainGen != c->sceneGen) { // levels 0-1 are current, the deeper ones not yet: the samples keep counting
			d.tablePending += R.nSamples;
			if (d.tablePending >= chainAt) {
				prof_begin(c, K_QUERY, st);
				const int rc = build_chain_tables(c, st);
				prof_end(c, st);
				if (rc != RT_OK) return rc;
			}
		}
		if (*bounce && wantChain && d.chainGen == c->sceneGen) *chain = d.chainLevels;
		return RT_OK;
	}
	if (d.tablePendingGen != c->sceneGen) d.tablePendingGen = c->sceneGen, d.tablePending = 0;
	d.tablePending += R.nSamples;
	if (d.tablePending < (unsigned long long)c->knobs.tableMin * records) return RT_OK;
	if (!d.tab.A) {
		PrimaryTable P{};
		HIPCHK(c, dalloc(d.tabAllocs, &P.A, records));
		HIPCHK(c, dalloc(d.tabAllocs, &P.B, records));
		P.w = c->width + 2, P.h = c->height + 2;
		d.tab = P;
	}
	bool specular = false;
	for (int t : c->matTypes) specular = specular || t == 2 || t == 3;
	const bool withBounce = specular && c->knobs.bounceTable != 0;
	if (withBounce && !d.btab.A) {
		BounceTable B{};
		HIPCHK(c, dalloc(d.tabAllocs, &B.A, 2 * records));
		HIPCHK(c, dalloc(d.tabAllocs, &B.B, 2 * records));
		B.n = (int)records, B.w = c->width + 2;
		d.btab = B;
	}
	int brc = build_table(c, st, kPrimaryTable, records, d.gridTable, K_QUERY, d.tab); // (the profile's query slot: a build is one launch there)
	if (brc == RT_OK && withBounce) brc = build_table(c, st, kBounceTable, 2 * records, d.gridBounce, -1, d.tab, d.btab);
	if (brc != RT_OK) return brc;
	if (withBounce) {
		d.bounceGen = c->sceneGen;
		if (wantChain && d.tablePending >= chainAt) {
			const int rc = build_chain_tables(c, st);
			if (rc != RT_OK) { prof_end(c, st); return rc; }
			*chain = d.chainLevels;
		}
	}
	prof_end(c, st);
	d.tableGen = c->sceneGen;
	*use = true, *bounce = withBounce;
	return RT_OK;
}
// Path mode, an entry per sample: 'rounds' = start depth + 1 rounds, no queue length is read back.  connect(r) and light(r)
// run on the second stream beside compact / extend / assign of round r + 1 (twoStreams; light(r) is the last writer of
// the E and L that shade(r + 1) reads, so the main stream joins before shade); RT_FUSE=0 keeps one kernel at a time.
//   generate | begin compact extend(0) assign shade(0) | begin compact extend(1) assign {|| connect(0) light(0)} shade(1) | ...
// With the primary-hit table round 0 is   [table] generate_t | assign shade(0)   on all three schedules.
static int run_rounds_stream(rt_ctx* c, const RenderParams& R, int rounds)
{
	const float t_min = 0.001f; // renderer.cpp:131
	const int grid = c->gridBlocks;
	// How connect(r) + light(r) share the machine with round r + 1 (profiles/r03_ab_stream_fuse.txt, r04_ab_gate.txt): one kernel at a
	// time (RT_FUSE=0) pays every traversal launch's drain in full; both streams started together (RT_FUSE=2) make the two persistent
	// kernels share the machine for their whole length: good below ~100 M samples per batch (1/8 frame 11.0 -> 10.1 ms, 33 M samples
	// 17.1 -> 16.4), level or slightly worse above, where the default therefore keeps one kernel at a time -- every kernel's time and
	// counters are then its own, which is what the roofline block of the bench line is made of.  (Holding the second stream at a gate
	// until extend(r + 1) has found its queue dry, so that connect(r) fills that drain and nothing else, was round 3's default below
	// 100 M samples -- with a gate that never waited, ADVICE.md r3.  Made to wait, it is no better than no gate at any size
	// (10.37 against 10.10 ms, 16.36 / 16.39, 85.2 / 83.6): taken out, profiles/patches/gate.diff.)
	// Small batches (RT_FUSE=1; default below RT_MIXED_MAX samples): extend(r) and connect(r - 1) as ONE launch (k_traverse_s), one drain
	// per round instead of two.
	// Measured (profiles/r03_ab_one_launch_per_round.txt, 1080p x spp): 1: 3.73 -> 3.24 ms, 2: 4.50 -> 4.18, 4: 6.10 -> 6.02, 8: 9.00 -> 9.08, 16: 14.8 -> 15.8.
	const unsigned mixedMax = c->knobs.mixedMax;
	const bool mixed = !c->counting && (c->knobs.fuse == 1 || (c->knobs.fuse < 0 && R.nSamples < mixedMax)) &&
	                   (unsigned long long)R.nSamples * (unsigned)(c->S.nLights + 1) < 0x7FFFFFFFull;
	const bool twoStreams = !mixed && (c->knobs.fuse < 0 ? R.nSamples < 100000000u : c->knobs.fuse != 0);
	const StreamState& T = c->dense.T;
	hipStream_t st = c->stream, sb = twoStreams ? c->dense.side : c->stream;
	const int cnt = c->counting ? 1 : 0;
	const int n = (int)R.nSamples;
	bool table = false, bounce = false;
	int chain = 1;
	{
		const int rc = primary_table_for(c, R, st, &table, &bounce, &chain);
		if (rc != RT_OK) return rc;
	}
	// which instantiation each launch of the batch takes: rt_forms.h
	const DenseBatch batch{ table, bounce, chain, c->knobs.bounceTable != 0, c->knobs.round0Entries, c->Qt.on != 0, c->C.fisheye != 0, rounds };
	const bool direct = batch.direct();
	const dim3 perEntry((n + RT_BLOCK - 1) / RT_BLOCK);
	const int gen = generate_form(batch);
	prof_begin(c, K_GENERATE, st);
	if (gen == GENERATE_S) hipLaunchKernelGGL(k_generate_s, perEntry, dim3(RT_BLOCK), 0, st, c->S, c->C, R, T, rounds == 1 ? 1 : 0, c->knobs.decide, cnt);
	else hipLaunchKernelGGL(kGenerateTab[gen], perEntry, dim3(RT_BLOCK), 0, st, c->S, c->C, R, T, c->dense.tab, rounds == 1 ? 1 : 0, cnt);
	prof_end(c, st);
	if (direct && c->knobs.round0Entries == 2) { // (tests) whoever still read a round-0 entry would see NaNs and ids of -1
		HIPCHK(c, hipMemsetAsync(T.O[0], 0xFF, (size_t)n * sizeof(float4), st));
		HIPCHK(c, hipMemsetAsync(T.D[0], 0xFF, (size_t)n * sizeof(float4), st));
		HIPCHK(c, hipMemsetAsync(T.hitN[0], 0xFF, (size_t)n * sizeof(float4), st));
		HIPCHK(c, hipMemsetAsync(T.hitId[0], 0xFF, (size_t)n * sizeof(int2), st));
	}
	// light over the shadow records of round 'of'
	auto light = [&](hipStream_t on, int of, int lastArg) {
		const int f = light_form(batch, of);
		hipLaunchKernelGGL(kLightS[f], dim3(c->dense.gridLight[f]), dim3(RT_BLOCK), 0, on, c->S, R, T, of, lastArg, c->knobs.shadeLds, c->C, f ? c->dense.tab : PrimaryTable{});
	};
	bool pendingJoin = false;
	for (int round = 0; round < rounds; round++) {
		const int last = round + 1 == rounds ? 1 : 0, lastNext = round + 2 == rounds ? 1 : 0;
		if (!(table && round == 0)) { // (the table's entries come with their hits: no queue, no traversal launch)
			hipLaunchKernelGGL(k_compact_s, dim3(grid / 2), dim3(RT_COMPACT_BLOCK), 0, st, T, round);
			tail_probe_reset(st);
			prof_begin(c, K_EXTEND, st);
			if (mixed && round > 0) hipLaunchKernelGGL(k_traverse_s, dim3(c->dense.gridTraverse), dim3(RT_BLOCK), 0, st, c->S, T, round, last, t_min, tuning(c), c->spill);
			else hipLaunchKernelGGL(kExtendS[cnt], dim3(c->dense.gridExtend), dim3(RT_BLOCK), 0, st, c->S, T, round & 1, last, t_min, tuning(c), c->spill, c->counters);
			prof_end(c, st);
			tail_probe_print(st, "extend_s", round);
		}
		if (mixed && round > 0) { // the shadow answers of the round before came with this round's hits
			prof_begin(c, K_SHADE, st);
			light(st, round - 1, 0);
			prof_end(c, st);
		}
		hipLaunchKernelGGL(k_assign, dim3(grid / 2), dim3(RT_COMPACT_BLOCK), 0, st, T, round);
		if (pendingJoin) { HIPCHK(c, hipStreamWaitEvent(st, c->dense.join, 0)); pendingJoin = false; }
		// shade: the form's bits say which tables it is handed (rt_forms.h); a chain round reads level round + 1
		const int f = shade_form(batch, round), bt = shade_bt(f);
		if (!kShadeS[f]) return fail(c, RT_E_STATE, "run_rounds_stream: no k_shade_s of form %d (round %d of %d)", f, round, rounds);
		const ChainLevel& L = c->dense.chain[bt == BT_CHAIN ? round - 1 : 0];
		const BounceTable Bt = bt == BT_BOUNCE ? c->dense.btab : bt == BT_CHAIN ? BounceTable{ L.A, L.B, L.cap, 0 } : BounceTable{};
		prof_begin(c, K_SHADE, st);
		hipLaunchKernelGGL(kShadeS[f], dim3(c->dense.gridShade[f]), dim3(RT_BLOCK), 0, st, c->S, c->C, R, T, round, round == 0 ? 1 : 0, last, lastNext, c->knobs.decide, c->knobs.shadeLds, cnt, c->Qt,
		                   Bt, shade_masked(f) ? c->knobs.bounceTable : 0, shade_tab(f) ? c->dense.tab : PrimaryTable{});
		prof_end(c, st);
		if (mixed && !last) continue; // this round's shadow rays ride in the next round's traversal launch
		if (twoStreams) {
			HIPCHK(c, hipEventRecord(c->dense.fork, st));
			HIPCHK(c, hipStreamWaitEvent(sb, c->dense.fork, 0));
		}
		prof_begin(c, K_CONNECT, sb);
		launch_connect_s(c, sb, T, round, twoStreams ? c->dense.sideSpill : c->spill);
		prof_end(c, sb);
		prof_begin(c, K_SHADE, sb);
		light(sb, round, last);
		prof_end(c, sb);
		if (twoStreams) { HIPCHK(c, hipEventRecord(c->dense.join, sb)); pendingJoin = true; }
	}
	if (pendingJoin) HIPCHK(c, hipStreamWaitEvent(st, c->dense.join, 0));
	if (cnt) hipLaunchKernelGGL(k_fold_decided, dim3(1), dim3(1), 0, st, c->S, T.counts, c->counters);
	HIPCHK(c, hipMemcpyAsync(c->hostCounts, T.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
	c->hostCounts[4] = 0;
	if (c->Qt.on) {
		// the batch's packed reward words -> the wide sums, in stream order; the overflow word rides home with the round flags
		const int nq = c->Qt.grid * c->Qt.grid * c->Qt.grid * RT_Q_PATCHES;
		hipLaunchKernelGGL(k_q_fold, dim3((nq + 255) / 256), dim3(256), 0, st, c->Qt);
		HIPCHK(c, hipMemcpyAsync(c->hostCounts + 4, c->Qt.ovf, sizeof(int), hipMemcpyDeviceToHost, st));
	}
	HIPCHK(c, hipStreamSynchronize(st));
	const int* hc = c->hostCounts;
	if (hc[4] != 0) { // the sampler's own overflow word comes first
		(void)hipMemsetAsync(c->Qt.ovf, 0, sizeof(int), st);
		return fail(c, RT_E_OVERFLOW, "Q-learning sampler: more than %u rewards for one (cell, direction) within one batch of frames: render fewer frames per call", RT_Q_ACC_LIMIT);
	}
	if (hc[3] != 0) (void)hipMemsetAsync(T.counts + 3, 0, sizeof(int), st);
	const int rc = decode_status(c, hc[3], FAM_WAVEFRONT);
	if (rc != RT_OK) { c->dense.tableGen = 0, c->dense.bounceGen = 0, c->dense.chainGen = 0; return rc; } // (the trouble may have been the table build's)
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}
// the dense pipeline serves path batches with an entry per sample; RT_COUNT_REFERENCE tallies are the slot pipeline's
// (the reference's walk visits the root pair for every ray, which a producer-side decision skips)
static bool stream_eligible(const rt_ctx* c, int mode, size_t samples)
{
	return (c->knobs.stream || c->Qt.on) && mode == RT_MODE_PATH && !c->pathUnsupported && c->counting != RT_COUNT_REFERENCE && samples <= (size_t)slot_budget(c);
}

// ---- one batch of samples ---------------------------------------------------------------------------
// Trace / Sample as one lane per call tree (rt_kernels.h): the combinations the pipelines do not serve
static int run_general(rt_ctx* c, const RenderParams& R, bool whitted)
{
	if (whitted) hipLaunchKernelGGL(k_trace_general, dim3(c->gridBlocks), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, R, c->spill, c->flags + 1);
	else hipLaunchKernelGGL(k_sample_general, dim3(c->gridBlocks), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, R, c->spill, c->flags + 1);
	return check_overflow(c, whitted ? FAM_TRACE_GENERAL : FAM_SAMPLE_GENERAL);
}
// The batch R describes, on the pipeline that serves it; 'depth' is the depth its samples start at (Whitted: R.maxDepth).  Sets
// R.finishInline: whether the samples were finished where they ended (an entry or slot each) or by k_finish.
static int trace_samples(rt_ctx* c, RenderParams& R, int depth)
{
	const int mode = R.mode;
	const size_t total = R.nSamples;
	// random draws interleave with occlusion queries (shiny / raytracer == 0 diffuse): one lane per sample
	if (mode == RT_MODE_PATH && c->pathUnsupported) return run_general(c, R, false);
	if (c->knobs.mega && !c->counting && mode == RT_MODE_WHITTED) return run_mega(c, R);
	if (stream_eligible(c, mode, total)) {
		const int rc = ensure_stream_state(c, (int)total);
		if (rc != RT_OK) return rc;
		R.finishInline = 1;
		return run_rounds_stream(c, R, depth + 1); // a round per hit level
	}
	// the slot wavefront: a slot per sample while the budget lasts
	const size_t budget = (size_t)slot_budget(c);
	const int slots = std::max(1, (int)std::min(total, budget));
	const int rc = ensure_state(c, slots, mode == RT_MODE_WHITTED);
	if (rc != RT_OK) return rc;
	const int seg = segments_per_sample(mode, depth, c->S.nLights);
	const int maxRounds = (int)((total + slots) / slots) * seg + seg + 4;
	const bool direct = mode == RT_MODE_PATH && (size_t)slots >= total;
	R.finishInline = direct ? 1 : 0;
	return run_rounds(c, R, maxRounds, direct ? seg : 0);
}

// the statistics' share of rt_clear (rt_api_adaptive.inc holds the rest of them)
static int stats_clear(rt_ctx* c)
{
	drop_plan(c); // the counts a budget plan was made from are gone
	if (!c->stats.count) return RT_OK;
	const size_t n = (size_t)c->width * c->height;
	HIPCHK(c, hipMemsetAsync(c->stats.count, 0, n * sizeof(uint), c->stream));
	HIPCHK(c, hipMemsetAsync(c->stats.sumY, 0, n * sizeof(float), c->stream));
	HIPCHK(c, hipMemsetAsync(c->stats.sumYY, 0, n * sizeof(float), c->stream));
	return RT_OK;
}

// Frames [frame0, frame0 + nframes) of one tile of pixels -- tilePixels of them: the rows row_first + k * row_stride of rt_render_rows, or
// the entries of pixelList (rt_render_active) -- in batches of frames: the finished samples of a batch live in a [frame][tile pixel]
// buffer (<= 4 GiB), which k_accumulate adds to the accumulator (and, with rt_stats_enable, to the pixels' statistics) in frame order.
static int render_batches(rt_ctx* c, int mode, uint32_t frame0, int nframes, uint32_t seed_base, int row_first, int row_stride, size_t tilePixels, const uint* pixelList, int max_depth, const char* fn)
{
	float lam = 0.0f;
	if (mode == RT_MODE_PATH) {
		const int rc = filter_check(c, fn, &lam);
		if (rc != RT_OK) return rc;
		drop_plan(c); // the batch moves the counts a budget plan was made from
	}
	const size_t sampleGiB = (size_t)c->knobs.sampleGiB;
	int batchFrames = (int)((sampleGiB << 30) / (tilePixels * sizeof(float4)));
	if (batchFrames < 1) batchFrames = 1;
	if (batchFrames > nframes) batchFrames = nframes;
	// path mode: keep a batch within the slot budget when a frame fits, so that every sample has its own slot
	// (exactly depth + 1 rounds, finished samples stored by shade / light, no finish pass; 4K: 16-frame batches)
	if (mode == RT_MODE_PATH && tilePixels <= (size_t)slot_budget(c) && (size_t)batchFrames * tilePixels > (size_t)slot_budget(c))
		batchFrames = (int)((size_t)slot_budget(c) / tilePixels);
	int rc = ensure_samples(c, tilePixels * batchFrames);
	if (rc != RT_OK) return rc;
	for (int f = 0; f < nframes; f += batchFrames) {
		const int bf = nframes - f < batchFrames ? nframes - f : batchFrames;
		const size_t total = tilePixels * bf;
		RenderParams R;
		memset(&R, 0, sizeof(R));
		R.mode = mode, R.frame0 = frame0 + (uint)f, R.nSamples = (uint)total, R.tilePixels = (uint)tilePixels, R.samples = c->samples;
		R.seedBase = seed_base, R.rowFirst = row_first, R.rowStride = row_stride, R.maxDepth = max_depth, R.accum = c->accum;
		R.pixelList = pixelList;
		R.filter = mode == RT_MODE_PATH ? c->pixelFilter : RT_FILTER_REFERENCE;
		set_lens(c, R, lam); // (lam is 0 in Whitted mode)
		R.deferGamma = mode == RT_MODE_PATH ? c->knobs.deferGamma : 0;
		R.sceneRt = -1; // (rt_render is Tick's loop: the flag is what the mode says)
		if (mode == RT_MODE_PATH && c->Qt.on && !c->pathUnsupported && !stream_eligible(c, mode, total))
			return fail(c, RT_E_UNSUPPORTED, "rt_render: the Q-learning sampler needs a path batch with an entry per sample (within the slot budget, no RT_COUNT_REFERENCE)");
		rc = trace_samples(c, R, mode == RT_MODE_PATH ? 4 : max_depth); // Sample starts at depth 4 (renderer.cpp:278): five hit levels
		if (rc != RT_OK) return rc;
		const dim3 grid((unsigned)((tilePixels + 255) / 256));
		if (mode == RT_MODE_PATH && c->stats.count) hipLaunchKernelGGL(k_accumulate<true>, grid, dim3(256), 0, c->stream, c->C, R, bf, c->stats);
		else hipLaunchKernelGGL(k_accumulate<false>, grid, dim3(256), 0, c->stream, c->C, R, bf, c->stats);
	}
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}

int rt_render_rows(rt_ctx* c, int mode, uint32_t frame0, int nframes, uint32_t seed_base, int row_first, int row_stride, int row_count, int max_depth)
{
	if (!c) return RT_E_ARG;
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_render: no scene uploaded");
	if (mode != RT_MODE_WHITTED && mode != RT_MODE_PATH) return fail(c, RT_E_ARG, "rt_render: mode %d", mode);
	if (row_first < 0 || row_stride < 1 || row_count < 1 || row_first + (row_count - 1) * row_stride >= c->height)
		return fail(c, RT_E_ARG, "rt_render: rows %d + k*%d (k < %d) outside 0..%d", row_first, row_stride, row_count, c->height);
	if (nframes < 1 || (mode == RT_MODE_WHITTED && nframes != 1)) return fail(c, RT_E_ARG, "rt_render: nframes %d (Whitted frames overwrite the accumulator: 1 only)", nframes);
	HIPCHK(c, hipSetDevice(c->device));
	if (mode == RT_MODE_WHITTED && max_depth <= 0) { // Trace(depth <= 0) returns black without tracing
		for (int k = 0; k < row_count; k++)
			HIPCHK(c, hipMemsetAsync(c->accum + (size_t)(row_first + k * row_stride) * c->width, 0, (size_t)c->width * sizeof(float4), c->stream));
		return RT_OK;
	}
	return render_batches(c, mode, frame0, nframes, seed_base, row_first, row_stride, (size_t)c->width * row_count, nullptr, max_depth, "rt_render / rt_render_rows");
}

int rt_render(rt_ctx* c, int mode, uint32_t frame0, int nframes, uint32_t seed_base, int y0, int y1, int max_depth)
{
	if (!c) return RT_E_ARG;
	if (y0 < 0 || y1 > c->height || y0 >= y1) return fail(c, RT_E_ARG, "rt_render: rows [%d,%d) outside 0..%d", y0, y1, c->height);
	return rt_render_rows(c, mode, frame0, nframes, seed_base, y0, 1, y1 - y0, max_depth);
}

int rt_trace_batch(rt_ctx* c, int mode, int n, const float* O, const float* D, int depth, uint32_t seed_base, float* rgb_out)
{
	const float one[3] = { 1, 1, 1 };
	return rt_trace_batch_energy(c, mode, n, O, D, depth, seed_base, one, rgb_out);
}

int rt_trace_batch_energy(rt_ctx* c, int mode, int n, const float* O, const float* D, int depth, uint32_t seed_base, const float* energy, float* rgb_out)
{
	if (!energy) return fail(c, RT_E_ARG, "rt_trace_batch: null energy");
	if (!c || !O || !D || !rgb_out || n < 0) return fail(c, RT_E_ARG, "rt_trace_batch: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_trace_batch: no scene uploaded");
	if (n == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	if ((mode == RT_MODE_WHITTED && depth <= 0) || (mode == RT_MODE_PATH && depth < 0)) {
		const float v = mode == RT_MODE_WHITTED ? 0.0f : 0.05f; // renderer.cpp:23, :129
		for (int i = 0; i < 3 * n; i++) rgb_out[i] = v;
		return RT_OK;
	}
	// the slot wavefront has no guided sampling (rt_render's rule, render_batches)
	if (mode == RT_MODE_PATH && c->Qt.on && !c->pathUnsupported && c->sceneRaytracer != 1 && !stream_eligible(c, mode, (size_t)n))
		return fail(c, RT_E_UNSUPPORTED, "rt_trace_batch: the Q-learning sampler needs a path batch with an entry per sample (within the slot budget, no RT_COUNT_REFERENCE)");
	int rc = RT_OK;
	float *dO = nullptr, *dD = nullptr;
	float4* dOut = nullptr;
	std::vector<void*> tmp;
	struct Guard { rt_ctx* c; std::vector<void*>& v; ~Guard() { (void)hipStreamSynchronize(c->stream); free_pool(v); } } guard{ c, tmp }; // every return path frees
	HIPCHK(c, dalloc(tmp, &dO, (size_t)3 * n));
	HIPCHK(c, dalloc(tmp, &dD, (size_t)3 * n));
	HIPCHK(c, dalloc(tmp, &dOut, (size_t)n));
	HIPCHK(c, hipMemcpyAsync(dO, O, (size_t)12 * n, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipMemcpyAsync(dD, D, (size_t)12 * n, hipMemcpyHostToDevice, c->stream));
	RenderParams R;
	memset(&R, 0, sizeof(R));
	R.mode = mode, R.nSamples = (uint)n, R.tilePixels = (uint)n, R.seedBase = seed_base, R.maxDepth = depth, R.accum = c->accum;
	R.customO = dO, R.customD = dD, R.customOut = dOut, R.customDepth = depth;
	R.customE[0] = energy[0], R.customE[1] = energy[1], R.customE[2] = energy[2];
	R.sceneRt = -1;
	// the two combinations Tick never makes (renderer.cpp:33-43, 107-121, 143-153): one lane per call tree
	const bool traceUnflagged = mode == RT_MODE_WHITTED && c->sceneRaytracer == 0, sampleFlagged = mode == RT_MODE_PATH && c->sceneRaytracer == 1;
	if (traceUnflagged || sampleFlagged) {
		if (c->Qt.on) return fail(c, RT_E_UNSUPPORTED, "rt_trace_batch: the Q-learning sampler is defined for Sample as Tick calls it only");
		R.sceneRt = c->sceneRaytracer;
		rc = run_general(c, R, traceUnflagged);
	} else rc = trace_samples(c, R, depth);
	if (rc == RT_OK) {
		std::vector<float> out4((size_t)4 * n);
		hipError_t e = hipMemcpy(out4.data(), dOut, (size_t)16 * n, hipMemcpyDeviceToHost);
		if (e != hipSuccess) rc = fail(c, RT_E_HIP, "rt_trace_batch: copy back failed: %s", hipGetErrorString(e));
		else for (int i = 0; i < n; i++) { rgb_out[3 * i] = out4[4 * i], rgb_out[3 * i + 1] = out4[4 * i + 1], rgb_out[3 * i + 2] = out4[4 * i + 2]; }
	}
	return rc;
}
