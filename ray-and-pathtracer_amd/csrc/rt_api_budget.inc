// Budgeted adaptive passes: rt_select_budget, rt_select_budget_rows, rt_select_budget_dilated, rt_download_budgets, rt_render_budget.  Included by
// rt_api.hip after rt_api_adaptive.inc (the list's storage, ensure_active_list, what a selection walks and its shared steps are its).  The kernels
// are rt_budget.h's, over the dilated masks rt_dilate.h's; the batch itself runs on whichever round pipeline
// trace_samples (rt_api_render.inc) picks for that many samples -- a plan only changes which (pixel, frame) a sample id names.
// The plan is dropped (drop_plan, rt_ctx.h) by whatever moves the counts or the list: a path-mode render_batches, stats_clear,
// rt_reproject, rt_select_active, rt_set_active_pixels.

// the per-entry arrays (an entry per pixel at most), the block totals of the budgets, the 64-bit total
static int ensure_plan(rt_ctx* c)
{
	if (c->plan.budget) return RT_OK;
	const size_t n = (size_t)c->width * c->height;
	BudgetPlan B{};
	uint* totals = nullptr;
	unsigned long long* total = nullptr;
	hipError_t e = dalloc(c->planAllocs, &B.budget, n);
	if (e == hipSuccess) e = dalloc(c->planAllocs, &B.first, n);
	if (e == hipSuccess) e = dalloc(c->planAllocs, &B.offset, n);
	if (e == hipSuccess) e = dalloc(c->planAllocs, &totals, (n + RT_SELECT_BLOCK - 1) / RT_SELECT_BLOCK);
	if (e == hipSuccess) e = dalloc(c->planAllocs, &total, (size_t)1);
	if (e != hipSuccess) { free_pool(c->planAllocs); return fail(c, RT_E_HIP, "budget plan: %s", hipGetErrorString(e)); }
	c->plan = B, c->budgetTotals = totals, c->planTotal = total;
	return RT_OK;
}
// the per-sample records of a pass of 'count' samples (the caller has synchronised the stream: nothing reads the old ones)
static int ensure_records(rt_ctx* c, size_t count)
{
	if (c->recordCap >= count) return RT_OK;
	free_pool(c->recordAllocs);
	c->plan.records = nullptr, c->recordCap = 0;
	const hipError_t e = dalloc(c->recordAllocs, &c->plan.records, count);
	if (e != hipSuccess) return fail(c, RT_E_HIP, "budget plan: %zu sample records: %s", count, hipGetErrorString(e));
	c->recordCap = count;
	return RT_OK;
}

#define RT_PASS_SAMPLES_MAX 0x7FFFFFFFull // sample ids are ints on the round pipelines

// rt_select_budget, rt_select_budget_rows, rt_select_budget_dilated (what = the caller's name): select_list's list (rt_api_adaptive.inc)
// and, per entry, the plan
static int select_plan(rt_ctx* c, const char* what, const rt_budget_params* params, const SelectOver& over, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out)
{
	const rt_budget_params B = params ? *params : rt_budget_params RT_BUDGET_DEFAULTS;
	int rc = adaptive_params_ok(c, what, B.select);
	if (rc != RT_OK) return rc;
	if (B.pass_cap < 1 || B.pass_cap > 1024) return fail(c, RT_E_ARG, "%s: pass_cap %d (1..1024)", what, B.pass_cap);
	if (!c || !n_active_out || !n_samples_out || !cap_used_out) return fail(c, RT_E_ARG, "%s: null argument", what);
	RowMap M;
	rc = select_over_ok(c, what, over, M);
	if (rc != RT_OK) return rc;
	if (!c->stats.count) return fail(c, RT_E_STATE, "%s: statistics are off (rt_stats_enable)", what);
	HIPCHK(c, hipSetDevice(c->device));
	rc = ensure_active_list(c);
	if (rc == RT_OK) rc = ensure_plan(c);
	if (rc != RT_OK) return rc;
	const AdaptiveArgs A = adaptive_args(B.select);
	const int n = M.nPixels, blocks = select_blocks(M);
	unsigned long long limit = B.max_pass_samples ? (unsigned long long)B.max_pass_samples : ((unsigned long long)c->knobs.sampleGiB << 30) / sizeof(float4);
	if (limit > RT_PASS_SAMPLES_MAX) limit = RT_PASS_SAMPLES_MAX;
	c->nActive = -1; // no list until the count has come home
	drop_plan(c);
	struct Entry { rt_ctx* c; ~Entry() { if (c) prof_end(c); } } entry{ over.planEntry ? c : nullptr }; // (over.planEntry: every way out ends the entry)
	if (over.planEntry) prof_begin(c, K_QUERY);
	if (over.dilated) launch_dilate_masks(c, A, over.radius, M); // once: the masks do not depend on the cap
	// the fit rule: the largest cap = pass_cap >> k whose total fits; the list does not depend on the cap
	int cap = B.pass_cap, got = 0;
	unsigned long long total = 0;
	for (;; cap >>= 1) {
		if (over.dilated) hipLaunchKernelGGL(k_dilate_budget_count, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate, c->stats, A, cap, n, c->selectTotals, c->budgetTotals);
		else hipLaunchKernelGGL(k_budget_count, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, cap, M, c->selectTotals, c->budgetTotals);
		hipLaunchKernelGGL(k_budget_scan, dim3(1), dim3(RT_SELECT_SCAN_BLOCK), 0, c->stream, c->selectTotals, c->budgetTotals, blocks, c->activeCount, c->planTotal);
		HIPCHK(c, hipGetLastError());
		rc = read_selected(c, got, &total); // the call's only synchronisation, once per cap tried
		if (rc != RT_OK) return rc;
		if (got < 0 || got > n || total < (unsigned long long)got || total > (unsigned long long)got * (unsigned)cap)
			return fail(c, RT_E_STATE, "%s: %d pixels of %d selected, %llu samples at cap %d", what, got, n, total, cap);
		if (total <= limit || cap == 1) break;
	}
	*n_active_out = got;
	if (total > limit) {
		// not even one sample per listed pixel fits: the list alone, for rt_render_active (selectTotals holds the pixels' prefix sums)
		launch_list_scatter(c, over, A, M);
		HIPCHK(c, hipGetLastError());
		c->nActive = got;
		return fail(c, RT_E_UNSUPPORTED, "%s: %d %s pixels do not fit a pass of %llu samples", what, got, over.dilated ? "listed" : "active", limit);
	}
	if (got > 0) {
		rc = ensure_records(c, (size_t)total);
		if (rc != RT_OK) return rc;
		if (over.dilated) hipLaunchKernelGGL(k_dilate_budget_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate, c->stats, A, cap, n, c->selectTotals, c->budgetTotals, c->activeList, c->plan);
		else hipLaunchKernelGGL(k_budget_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, cap, M, c->selectTotals, c->budgetTotals, c->activeList, c->plan);
		HIPCHK(c, hipGetLastError());
	}
	c->nActive = got, c->planSamples = (long long)total;
	*n_samples_out = (uint32_t)total, *cap_used_out = cap;
	return RT_OK;
}

int rt_select_budget(rt_ctx* c, const rt_budget_params* params, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out)
{
	return select_plan(c, "rt_select_budget", params, over_rows(0, 1, c ? c->height : 1), n_active_out, n_samples_out, cap_used_out);
}

int rt_select_budget_rows(rt_ctx* c, const rt_budget_params* params, int row_first, int row_stride, int row_count, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out)
{
	return select_plan(c, "rt_select_budget_rows", params, over_rows(row_first, row_stride, row_count), n_active_out, n_samples_out, cap_used_out);
}

int rt_select_budget_dilated(rt_ctx* c, const rt_budget_params* params, int radius, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out)
{
	return select_plan(c, "rt_select_budget_dilated", params, over_dilated(radius, true), n_active_out, n_samples_out, cap_used_out);
}

int rt_download_budgets(rt_ctx* c, uint32_t* out, int cap, int* n_out)
{
	if (!c || cap < 0 || (cap > 0 && !out) || !n_out) return fail(c, RT_E_ARG, "rt_download_budgets: bad argument");
	if (c->planSamples < 0 || c->nActive < 0) return fail(c, RT_E_STATE, "rt_download_budgets: no budget plan (rt_select_budget)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const int n = std::min(cap, c->nActive);
	if (n > 0) HIPCHK(c, hipMemcpy(out, c->plan.budget, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	*n_out = c->nActive;
	return RT_OK;
}

int rt_render_budget(rt_ctx* c, uint32_t frame_base, uint32_t seed_base, int max_depth)
{
	if (!c) return RT_E_ARG;
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_render_budget: no scene uploaded");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_render_budget: statistics are off (rt_stats_enable)");
	if (c->Qt.on) return fail(c, RT_E_UNSUPPORTED, "rt_render_budget: not with the Q-learning sampler on"); // rt_render_active's rule
	float lam = 0.0f;
	{
		const int frc = filter_check(c, "rt_render_budget", &lam);
		if (frc != RT_OK) return frc;
	}
	if (c->planSamples < 0 || c->nActive < 0) return fail(c, RT_E_STATE, "rt_render_budget: no budget plan (rt_select_budget; a plan serves one pass, and a render, a clear, a reprojection or a new list drops it)");
	const size_t total = (size_t)c->planSamples;
	drop_plan(c); // consumed: the counts move
	if (total == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = ensure_samples(c, total);
	if (rc != RT_OK) return rc;
	RenderParams R;
	memset(&R, 0, sizeof(R));
	R.mode = RT_MODE_PATH, R.frame0 = frame_base, R.nSamples = (uint)total, R.tilePixels = (uint)total, R.samples = c->samples;
	R.seedBase = seed_base, R.rowFirst = 0, R.rowStride = 1, R.maxDepth = max_depth, R.accum = c->accum;
	R.filter = c->pixelFilter;
	set_lens(c, R, lam);
	R.plan = c->plan.records; // sample sid is (pixel, frame_base + first + k) of its entry; the pool is entry-major
	R.deferGamma = c->knobs.deferGamma;
	R.sceneRt = -1;
	rc = trace_samples(c, R, 4); // Sample starts at depth 4 (renderer.cpp:278)
	if (rc != RT_OK) return rc;
	hipLaunchKernelGGL(k_accumulate_budget, dim3((unsigned)((c->nActive + 255) / 256)), dim3(256), 0, c->stream, R, c->activeList, c->plan, c->nActive, c->stats);
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}
