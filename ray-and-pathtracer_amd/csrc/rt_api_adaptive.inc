// Adaptive sampling: rt_stats_enable, rt_download_stats, rt_select_active, rt_select_active_rows, rt_select_active_dilated, rt_set_active_pixels,
// rt_download_active, rt_render_active, rt_resolve_adaptive.  Included by rt_api.hip.  The statistics are kept by k_accumulate<true> (rt_kernels.h;
// launched by render_batches of rt_api_render.inc while they are on), the selection and the per-count resolve are the kernels of rt_adaptive.h,
// the dilated selection's those of rt_dilate.h.
int rt_stats_enable(rt_ctx* c, int on)
{
	if (!c) return RT_E_ARG;
	HIPCHK(c, hipSetDevice(c->device));
	if (!on) {
		c->hist.gen = 0; // a captured history (rt_history_capture) belongs to the statistics it was taken with
		if (!c->stats.count) return RT_OK;
		HIPCHK(c, hipStreamSynchronize(c->stream));
		// ... and goes with them, the triangles it kept included (up to a copy of every deformed BLAS's records)
		free_pool(c->historyAllocs);
		c->hist = rt_ctx::History{};
		c->keptBuf.clear(), c->keptCap.clear(), c->keptMark.clear(), c->keptDeltaHost.clear();
		free_pool(c->adaptiveAllocs);
		c->stats = PixelStats{};
		return RT_OK;
	}
	if (!c->stats.count) {
		const size_t n = (size_t)c->width * c->height;
		PixelStats St{};
		hipError_t e = dalloc(c->adaptiveAllocs, &St.count, n);
		if (e == hipSuccess) e = dalloc(c->adaptiveAllocs, &St.sumY, n);
		if (e == hipSuccess) e = dalloc(c->adaptiveAllocs, &St.sumYY, n);
		if (e != hipSuccess) { free_pool(c->adaptiveAllocs); return fail(c, RT_E_HIP, "rt_stats_enable: %s", hipGetErrorString(e)); }
		c->stats = St;
	}
	return stats_clear(c);
}

int rt_download_stats(rt_ctx* c, int y0, int y1, uint32_t* count, float* sum_y, float* sum_yy)
{
	if (!rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_stats: bad argument");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_download_stats: statistics are off (rt_stats_enable)");
	return download_rows(c, y0, y1, { { c->stats.count, count, sizeof(uint) }, { c->stats.sumY, sum_y, sizeof(float) }, { c->stats.sumYY, sum_yy, sizeof(float) } });
}

// the list's device storage: width * height indices, a total per block of the selection, the selected count, and the four bitmasks of
// the dilated selection (rt_dilate.h: a bit per pixel each, 259 KB at 1080p)
static int ensure_active_list(rt_ctx* c)
{
	if (c->activeList) return RT_OK;
	const size_t n = (size_t)c->width * c->height;
	uint *list = nullptr, *totals = nullptr;
	int* count = nullptr;
	hipError_t e = dalloc(c->activeAllocs, &list, n);
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &totals, (n + RT_SELECT_BLOCK - 1) / RT_SELECT_BLOCK);
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &count, (size_t)1);
	DilateMasks D{};
	const size_t words = (n + 63) / 64;
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &D.raw, words);
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &D.eligible, words);
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &D.rows, words);
	if (e == hipSuccess) e = dalloc(c->activeAllocs, &D.listed, words);
	if (e != hipSuccess) { free_pool(c->activeAllocs); return fail(c, RT_E_HIP, "active-pixel list: %s", hipGetErrorString(e)); }
	c->activeList = list, c->selectTotals = totals, c->activeCount = count, c->dilate = D;
	return RT_OK;
}

// ---- the selection: one list skeleton here, one plan skeleton in rt_api_budget.inc, six entry points that say what is walked -------
// What a selection walks: a row set (rt_adaptive.h RowMap; the whole frame is the rows (0, 1, height)), or the whole frame through the
// dilated masks of rt_dilate.h at 'radius' (whole frame only: a context that holds one row shard has no statistics for its neighbours'
// rows).  The entry points fill it with their arguments as they came; select_over_ok checks them.
struct SelectOver {
	bool dilated;
	int rowFirst, rowStride, rowCount; // !dilated
	int radius;                        // dilated
	bool planEntry; // select_plan brackets the whole call, read-backs included, as one entry of rt_profile.query.  Only rt_select_budget_dilated
	                // does: rt_select_budget and rt_select_budget_rows have no entry at all (profiles/dilate_bench.py relies on both).
};
static SelectOver over_rows(int row_first, int row_stride, int row_count) { return SelectOver{ false, row_first, row_stride, row_count, 0, false }; }
static SelectOver over_dilated(int radius, bool plan_entry) { return SelectOver{ true, 0, 0, 0, radius, plan_entry }; }

// the rules of rt_adaptive_params, for every selection
static int adaptive_params_ok(rt_ctx* c, const char* what, const rt_adaptive_params& P)
{
	if (P.min_samples < 2 || P.max_samples < P.min_samples) return fail(c, RT_E_ARG, "%s: min_samples %d (>= 2), max_samples %d (>= min_samples)", what, P.min_samples, P.max_samples);
	if (!(P.threshold >= 0.0f) || !(P.floor > 0.0f)) return fail(c, RT_E_ARG, "%s: threshold must be >= 0 and floor > 0 (neither NaN)", what);
	return RT_OK;
}
// the radius, or the row set (row_set_ok: rt_gather_rows' rule for what lies in the frame); M: the lanes of the launches as the kernels take them
static int select_over_ok(rt_ctx* c, const char* what, const SelectOver& over, RowMap& M)
{
	if (over.dilated) {
		if (over.radius < 0 || over.radius > RT_DILATE_MAX_RADIUS) return fail(c, RT_E_ARG, "%s: radius %d (0..%d)", what, over.radius, RT_DILATE_MAX_RADIUS);
		M.rowFirst = 0, M.rowStride = 1, M.width = c->width, M.nPixels = c->width * c->height;
		return RT_OK;
	}
	if (!row_set_ok(c, over.rowFirst, over.rowStride, over.rowCount))
		return fail(c, RT_E_ARG, "%s: rows %d + k*%d (k < %d) outside 0..%d", what, over.rowFirst, over.rowStride, over.rowCount, c->height);
	M.rowFirst = over.rowFirst, M.rowStride = over.rowStride, M.width = c->width, M.nPixels = over.rowCount * c->width;
	return RT_OK;
}
static AdaptiveArgs adaptive_args(const rt_adaptive_params& P)
{
	AdaptiveArgs A;
	A.minSamples = P.min_samples, A.maxSamples = P.max_samples, A.threshold = P.threshold, A.floor = P.floor;
	return A;
}
static int select_blocks(const RowMap& M) { return (M.nPixels + RT_SELECT_BLOCK - 1) / RT_SELECT_BLOCK; }

// the three mask launches: c->dilate.listed and, in c->selectTotals, the listed pixels of every block
static void launch_dilate_masks(rt_ctx* c, const AdaptiveArgs& A, int radius, const RowMap& M)
{
	const DilateMasks& D = c->dilate;
	const int n = M.nPixels, blocks = select_blocks(M);
	hipLaunchKernelGGL(k_dilate_mask, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, n, D.raw, D.eligible);
	hipLaunchKernelGGL(k_dilate_rows, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, D.raw, n, c->width, radius, D.rows);
	hipLaunchKernelGGL(k_dilate_cols, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, D, n, c->width, c->height, radius, c->selectTotals);
}
// the list alone, from the prefix sums of the listed pixels in c->selectTotals (dilated: and the listed mask)
static void launch_list_scatter(rt_ctx* c, const SelectOver& over, const AdaptiveArgs& A, const RowMap& M)
{
	const int blocks = select_blocks(M);
	if (over.dilated) hipLaunchKernelGGL(k_dilate_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->dilate.listed, M.nPixels, c->selectTotals, c->activeList);
	else hipLaunchKernelGGL(k_select_scatter, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, M, c->selectTotals, c->activeList);
}
// The totals come home, in stream order behind what is queued: the selected count (c->activeCount) and, for a plan, the 64-bit total of its
// budgets (c->planTotal).  Pinned words 8 and 10..11 (the round pipelines use 0..4, rt_reproject 9), then the only synchronisation of
// a list call, of a plan call the one of this cap.
static int read_selected(rt_ctx* c, int& got, unsigned long long* total)
{
	HIPCHK(c, hipMemcpyAsync(c->hostCounts + 8, c->activeCount, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	if (total) HIPCHK(c, hipMemcpyAsync(c->hostCounts + 10, c->planTotal, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	got = c->hostCounts[8];
	if (total) memcpy(total, c->hostCounts + 10, sizeof(*total));
	return RT_OK;
}

// rt_select_active, rt_select_active_rows, rt_select_active_dilated (what = the caller's name)
static int select_list(rt_ctx* c, const char* what, const rt_adaptive_params* params, const SelectOver& over, int* n_active_out)
{
	const rt_adaptive_params P = params ? *params : rt_adaptive_params RT_ADAPTIVE_DEFAULTS;
	int rc = adaptive_params_ok(c, what, P);
	if (rc != RT_OK) return rc;
	if (!c || !n_active_out) return fail(c, RT_E_ARG, "%s: null argument", what);
	RowMap M;
	rc = select_over_ok(c, what, over, M);
	if (rc != RT_OK) return rc;
	if (!c->stats.count) return fail(c, RT_E_STATE, "%s: statistics are off (rt_stats_enable)", what);
	HIPCHK(c, hipSetDevice(c->device));
	rc = ensure_active_list(c);
	if (rc != RT_OK) return rc;
	const AdaptiveArgs A = adaptive_args(P);
	const int n = M.nPixels, blocks = select_blocks(M);
	c->nActive = -1; // no list until the count has come home
	drop_plan(c);
	prof_begin(c, K_QUERY); // (with rt_set_profiling on: the launches, three or five, are one entry of rt_profile.query)
	if (over.dilated) launch_dilate_masks(c, A, over.radius, M);
	else hipLaunchKernelGGL(k_select_count, dim3(blocks), dim3(RT_SELECT_BLOCK), 0, c->stream, c->stats, A, M, c->selectTotals);
	hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(RT_SELECT_SCAN_BLOCK), 0, c->stream, c->selectTotals, blocks, c->activeCount);
	launch_list_scatter(c, over, A, M);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	int got = 0;
	rc = read_selected(c, got, nullptr);
	if (rc != RT_OK) return rc;
	if (got < 0 || got > n) return fail(c, RT_E_STATE, "%s: %d pixels selected of %d", what, got, n);
	c->nActive = got;
	*n_active_out = got;
	return RT_OK;
}

int rt_select_active(rt_ctx* c, const rt_adaptive_params* params, int* n_active_out)
{
	return select_list(c, "rt_select_active", params, over_rows(0, 1, c ? c->height : 1), n_active_out);
}

int rt_select_active_rows(rt_ctx* c, const rt_adaptive_params* params, int row_first, int row_stride, int row_count, int* n_active_out)
{
	return select_list(c, "rt_select_active_rows", params, over_rows(row_first, row_stride, row_count), n_active_out);
}

int rt_select_active_dilated(rt_ctx* c, const rt_adaptive_params* params, int radius, int* n_active_out)
{
	return select_list(c, "rt_select_active_dilated", params, over_dilated(radius, false), n_active_out);
}

int rt_set_active_pixels(rt_ctx* c, const uint32_t* pixels, int n)
{
	if (!c || n < 0 || (n > 0 && !pixels)) return fail(c, RT_E_ARG, "rt_set_active_pixels: bad argument");
	// refused before anything is uploaded: the list a batch walks must name every pixel once (two samples of one pixel in one
	// k_accumulate launch would race) and inside the frame
	const uint32_t limit = (uint32_t)c->width * (uint32_t)c->height;
	for (int i = 0; i < n; i++) {
		if (pixels[i] >= limit) return fail(c, RT_E_ARG, "rt_set_active_pixels: entry %d is pixel %u of %u", i, pixels[i], limit);
		if (i > 0 && pixels[i] <= pixels[i - 1]) return fail(c, RT_E_ARG, "rt_set_active_pixels: entry %d (%u) does not ascend from entry %d (%u)", i, pixels[i], i - 1, pixels[i - 1]);
	}
	HIPCHK(c, hipSetDevice(c->device));
	const int rc = ensure_active_list(c);
	if (rc != RT_OK) return rc;
	drop_plan(c); // a plan belongs to the list it was made with
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (a batch over the list it replaces may still be accumulating)
	if (n > 0) HIPCHK(c, hipMemcpy(c->activeList, pixels, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
	c->nActive = n;
	return RT_OK;
}

int rt_download_active(rt_ctx* c, uint32_t* out, int cap, int* n_out)
{
	if (!c || cap < 0 || (cap > 0 && !out) || !n_out) return fail(c, RT_E_ARG, "rt_download_active: bad argument");
	if (c->nActive < 0) return fail(c, RT_E_STATE, "rt_download_active: no active-pixel list (rt_select_active, rt_set_active_pixels)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const int n = std::min(cap, c->nActive);
	if (n > 0) HIPCHK(c, hipMemcpy(out, c->activeList, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	*n_out = c->nActive; // the list's true length, whatever fitted
	return RT_OK;
}

int rt_render_active(rt_ctx* c, uint32_t frame0, int nframes, uint32_t seed_base, int max_depth)
{
	if (!c) return RT_E_ARG;
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_render_active: no scene uploaded");
	if (nframes < 1) return fail(c, RT_E_ARG, "rt_render_active: nframes %d", nframes);
	if (c->nActive < 0) return fail(c, RT_E_STATE, "rt_render_active: no active-pixel list (rt_select_active, rt_set_active_pixels)");
	// the rewards of a pixel subset are a different table from the whole frame's: not defined here
	if (c->Qt.on) return fail(c, RT_E_UNSUPPORTED, "rt_render_active: not with the Q-learning sampler on");
	if (c->nActive == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	return render_batches(c, RT_MODE_PATH, frame0, nframes, seed_base, 0, 1, (size_t)c->nActive, c->activeList, max_depth, "rt_render_active");
}

int rt_resolve_adaptive(rt_ctx* c, int y0, int y1, uint32_t* rgb8_out)
{
	if (!rgb8_out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_resolve_adaptive: bad argument");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_resolve_adaptive: statistics are off (rt_stats_enable)");
	return resolve_rows(c, c->accum, c->stats.count, 0, y0, y1, rgb8_out);
}
