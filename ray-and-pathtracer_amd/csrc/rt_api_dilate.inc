// Dilated adaptive selection: rt_select_active_dilated, rt_select_budget_dilated.  Included by rt_api.hip after rt_api_adaptive.inc and
// rt_api_budget.inc: the list, its block totals, the plan and the fit rule are theirs, and so is everything that serves the result
// (rt_download_active, rt_render_active, rt_download_budgets, rt_render_budget, rt_gather_active).  The kernels are rt_dilate.h's, the two
// scans rt_adaptive.h's and rt_budget.h's own.  Whole frame only: a context that holds one row shard has no statistics for its
// neighbours' rows.

// what both calls refuse before they look at the context: rt_select_active's rules and the radius
static int dilate_args_ok(rt_ctx* c, const char* what, const rt_adaptive_params& P, int radius)
{
	if (P.min_samples < 2 || P.max_samples < P.min_samples) return fail(c, RT_E_ARG, "%s: min_samples %d (>= 2), max_samples %d (>= min_samples)", what, P.min_samples, P.max_samples);
	if (!(P.threshold >= 0.0f) || !(P.floor > 0.0f)) return fail(c, RT_E_ARG, "%s: threshold must be >= 0 and floor > 0 (neither NaN)", what);
	if (radius < 0 || radius > RT_DILATE_MAX_RADIUS) return fail(c, RT_E_ARG, "%s: radius %d (0..%d)", what, radius, RT_DILATE_MAX_RADIUS);
	return RT_OK;
}

// the three mask launches: c->dilate.listed and, in c->selectTotals, the listed pixels of every block
static void launch_dilate_masks(rt_ctx* c, const AdaptiveArgs& A, int radius, int n, int blocks)
{
	const DilateMasks& D = c->dilate;
	hipLaunchKernelGGL(k_dilate_mask, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, n, D.raw, D.eligible);
	hipLaunchKernelGGL(k_dilate_rows, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, D.raw, n, c->width, radius, D.rows);
	hipLaunchKernelGGL(k_dilate_cols, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, D, n, c->width, c->height, radius, c->selectTotals);
}

int rt_select_active_dilated(rt_ctx* c, const rt_adaptive_params* params, int radius, int* n_active_out)
{
	const char* what = "rt_select_active_dilated";
	const rt_adaptive_params P = params ? *params : rt_adaptive_params RT_ADAPTIVE_DEFAULTS;
	int rc = dilate_args_ok(c, what, P, radius);
	if (rc != RT_OK) return rc;
	if (!c || !n_active_out) return fail(c, RT_E_ARG, "%s: null argument", what);
	if (!c->stats.count) return fail(c, RT_E_STATE, "%s: statistics are off (rt_stats_enable)", what);
	HIPCHK(c, hipSetDevice(c->device));
	rc = ensure_active_list(c);
	if (rc != RT_OK) return rc;
	AdaptiveArgs A;
	A.minSamples = P.min_samples, A.maxSamples = P.max_samples, A.threshold = P.threshold, A.floor = P.floor;
	const int n = c->width * c->height, blocks = (n + RT_SELECT_BLOCK - 1) / RT_SELECT_BLOCK;
	c->nActive = -1; // no list until the count has come home
	drop_plan(c);
	prof_begin(c, K_QUERY); // (with rt_set_profiling on: the five launches are one entry of rt_profile.query)
	launch_dilate_masks(c, A, radius, n, blocks);
	hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(RT_SELECT_SCAN_BLOCK), 0, c->stream, c->selectTotals, blocks, c->activeCount);
	hipLaunchKernelGGL(k_dilate_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate.listed, n, c->selectTotals, c->activeList);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	// the only synchronisation of the call: the selected count (rt_select_active's pinned word)
	HIPCHK(c, hipMemcpyAsync(c->hostCounts + 8, c->activeCount, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const int got = c->hostCounts[8];
	if (got < 0 || got > n) return fail(c, RT_E_STATE, "%s: %d pixels selected of %d", what, got, n);
	c->nActive = got;
	*n_active_out = got;
	return RT_OK;
}

// select_budget_rows (rt_api_budget.inc) over the listed mask: the same fit rule, read-backs and plan
int rt_select_budget_dilated(rt_ctx* c, const rt_budget_params* params, int radius, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out)
{
	const char* what = "rt_select_budget_dilated";
	const rt_budget_params B = params ? *params : rt_budget_params RT_BUDGET_DEFAULTS;
	const rt_adaptive_params& P = B.select;
	int rc = dilate_args_ok(c, what, P, radius);
	if (rc != RT_OK) return rc;
	if (B.pass_cap < 1 || B.pass_cap > 1024) return fail(c, RT_E_ARG, "%s: pass_cap %d (1..1024)", what, B.pass_cap);
	if (!c || !n_active_out || !n_samples_out || !cap_used_out) return fail(c, RT_E_ARG, "%s: null argument", what);
	if (!c->stats.count) return fail(c, RT_E_STATE, "%s: statistics are off (rt_stats_enable)", what);
	HIPCHK(c, hipSetDevice(c->device));
	rc = ensure_active_list(c);
	if (rc == RT_OK) rc = ensure_plan(c);
	if (rc != RT_OK) return rc;
	AdaptiveArgs A;
	A.minSamples = P.min_samples, A.maxSamples = P.max_samples, A.threshold = P.threshold, A.floor = P.floor;
	const int n = c->width * c->height, blocks = (n + RT_SELECT_BLOCK - 1) / RT_SELECT_BLOCK;
	unsigned long long limit = B.max_pass_samples ? (unsigned long long)B.max_pass_samples : ((unsigned long long)c->knobs.sampleGiB << 30) / sizeof(float4);
	if (limit > RT_PASS_SAMPLES_MAX) limit = RT_PASS_SAMPLES_MAX;
	c->nActive = -1; // no list until the count has come home
	drop_plan(c);
	// (with rt_set_profiling on: the whole call, its read-backs included, is one entry of rt_profile.query)
	struct Entry { rt_ctx* c; ~Entry() { prof_end(c); } };
	prof_begin(c, K_QUERY);
	Entry entry{ c };
	launch_dilate_masks(c, A, radius, n, blocks); // once: the masks do not depend on the cap
	int cap = B.pass_cap, got = 0;
	unsigned long long total = 0;
	for (;; cap >>= 1) {
		hipLaunchKernelGGL(k_dilate_budget_count, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate, c->stats, A, cap, n, c->selectTotals, c->budgetTotals);
		hipLaunchKernelGGL(k_budget_scan, dim3(1), dim3(RT_SELECT_SCAN_BLOCK), 0, c->stream, c->selectTotals, c->budgetTotals, blocks, c->activeCount, c->planTotal);
		HIPCHK(c, hipGetLastError());
		HIPCHK(c, hipMemcpyAsync(c->hostCounts + 8, c->activeCount, sizeof(int), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipMemcpyAsync(c->hostCounts + 10, c->planTotal, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		got = c->hostCounts[8];
		memcpy(&total, c->hostCounts + 10, sizeof(total));
		if (got < 0 || got > n || total < (unsigned long long)got || total > (unsigned long long)got * (unsigned)cap)
			return fail(c, RT_E_STATE, "%s: %d pixels of %d selected, %llu samples at cap %d", what, got, n, total, cap);
		if (total <= limit || cap == 1) break;
	}
	*n_active_out = got;
	if (total > limit) {
		// not even one sample per listed pixel fits: the list alone, for rt_render_active (selectTotals holds the pixels' prefix sums)
		hipLaunchKernelGGL(k_dilate_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate.listed, n, c->selectTotals, c->activeList);
		HIPCHK(c, hipGetLastError());
		c->nActive = got;
		return fail(c, RT_E_UNSUPPORTED, "%s: %d listed pixels do not fit a pass of %llu samples", what, got, limit);
	}
	if (got > 0) {
		rc = ensure_records(c, (size_t)total);
		if (rc != RT_OK) return rc;
		hipLaunchKernelGGL(k_dilate_budget_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate, c->stats, A, cap, n, c->selectTotals, c->budgetTotals, c->activeList, c->plan);
		HIPCHK(c, hipGetLastError());
	}
	c->nActive = got, c->planSamples = (long long)total;
	*n_samples_out = (uint32_t)total, *cap_used_out = cap;
	return RT_OK;
}
