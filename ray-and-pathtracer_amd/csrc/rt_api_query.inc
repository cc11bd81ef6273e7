// Batch queries: Scene::FindNearest / IsOccluded / GetSkyColor and the members below scene level for n caller rays, primary-hit maps.  Included by rt_api.hip.
// ---- batch queries -------------------------------------------------------------------------------
static int query_grid(rt_ctx* c, int n) { return short_grid((size_t)n, c->gridQuery, RT_CHUNK); }

// the scene as a query of the given scope sees it: rooted at the accelerator, one BLAS or one instance
static int scoped_scene(rt_ctx* c, int scope, int index, DScene& S, const char* who)
{
	S = c->S;
	if (scope == RT_SCOPE_SCENE || scope == RT_SCOPE_ACCEL) return RT_OK;
	if (scope == RT_SCOPE_BLAS) {
		if (index < 0 || index >= (int)c->blasRoot.size()) return fail(c, RT_E_ARG, "%s: blas %d of %d", who, index, (int)c->blasRoot.size());
		S.useTLAS = 0, S.tlasLds = 0, S.rootLink = c->blasRoot[(size_t)index], S.rootWide = c->blasRootWide[(size_t)index], S.rootWide8 = S.wide8 ? c->blasRootWide8[(size_t)index] : RT_EMPTY, S.nBruteSph = S.nBrutePla = 0;
		return RT_OK;
	}
	if (scope == RT_SCOPE_INSTANCE) {
		if (!c->S.useTLAS || index < 0 || index >= c->nInstances) return fail(c, RT_E_ARG, "%s: instance %d of %d", who, index, c->S.useTLAS ? c->nInstances : 0);
		S.rootLink = RT_INST_BIT | (uint)index;
		return RT_OK;
	}
	return fail(c, RT_E_ARG, "%s: scope %d", who, scope);
}

int rt_intersect_batch(rt_ctx* c, int n, const float* O, const float* D, const float* tmax, float t_min, rt_hit* out)
{
	return rt_intersect_scope(c, RT_SCOPE_SCENE, 0, n, O, D, tmax, t_min, out);
}

int rt_intersect_scope(rt_ctx* c, int scope, int index, int n, const float* O, const float* D, const float* tmax, float t_min, rt_hit* out)
{
	if (!c || !O || !D || !out || n < 0) return fail(c, RT_E_ARG, "rt_intersect_batch: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_intersect_batch: no scene uploaded");
	DScene S;
	{ const int src = scoped_scene(c, scope, index, S, "rt_intersect_scope"); if (src != RT_OK) return src; }
	if (n == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<void*> tmp;
	float *dO = nullptr, *dD = nullptr, *dT = nullptr;
	QueryHit* dH = nullptr;
	int rc = RT_OK;
	hipError_t e = dalloc(tmp, &dO, (size_t)3 * n);
	if (e == hipSuccess) e = dalloc(tmp, &dD, (size_t)3 * n);
	if (e == hipSuccess && tmax) e = dalloc(tmp, &dT, (size_t)n);
	if (e == hipSuccess) e = dalloc(tmp, &dH, (size_t)n);
	if (e == hipSuccess) e = hipMemcpyAsync(dO, O, (size_t)12 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, (size_t)12 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess && tmax) e = hipMemcpyAsync(dT, tmax, (size_t)4 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) {
		(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
		section_probe_reset(c->stream);
		prof_begin(c, K_QUERY);
		hipLaunchKernelGGL(kQueryNearest[c->counting ? 1 : 0][scope == RT_SCOPE_SCENE ? 1 : 0], dim3(query_grid(c, n)), dim3(RT_BLOCK), 0, c->stream, S, n, dO, dD, dT, t_min, tuning(c), dH, c->spill, c->flags, c->counters);
		prof_end(c);
		if (!c->counting) section_probe_print(c->stream, "query", n);
		e = hipStreamSynchronize(c->stream);
	}
	static_assert(sizeof(QueryHit) == sizeof(rt_hit), "rt_hit layout");
	if (e == hipSuccess) e = hipMemcpy(out, dH, (size_t)n * sizeof(rt_hit), hipMemcpyDeviceToHost);
	if (e != hipSuccess) rc = fail(c, RT_E_HIP, "rt_intersect_batch: %s", hipGetErrorString(e));
	free_pool(tmp);
	if (rc == RT_OK) rc = check_overflow(c);
	return rc;
}

int rt_occluded_batch(rt_ctx* c, int n, const float* O, const float* D, const float* tmax, uint8_t* out)
{
	return rt_occluded_scope(c, RT_SCOPE_SCENE, 0, n, O, D, tmax, out);
}

int rt_sky_color_batch(rt_ctx* c, int n, const float* D, float* rgb_out)
{
	if (!c || !D || !rgb_out || n < 0) return fail(c, RT_E_ARG, "rt_sky_color_batch: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_sky_color_batch: no scene uploaded");
	if (n == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<void*> tmp;
	struct Guard { std::vector<void*>& v; ~Guard() { free_pool(v); } } guard{ tmp };
	float *dD = nullptr, *dC = nullptr;
	HIPCHK(c, dalloc(tmp, &dD, (size_t)3 * n));
	HIPCHK(c, dalloc(tmp, &dC, (size_t)3 * n));
	HIPCHK(c, hipMemcpyAsync(dD, D, (size_t)12 * n, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_sky_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, n, dD, dC);
	HIPCHK(c, hipMemcpyAsync(rgb_out, dC, (size_t)12 * n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}

int rt_occluded_scope(rt_ctx* c, int scope, int index, int n, const float* O, const float* D, const float* tmax, uint8_t* out)
{
	if (!c || !O || !D || !out || n < 0) return fail(c, RT_E_ARG, "rt_occluded_batch: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_occluded_batch: no scene uploaded");
	DScene S;
	{ const int src = scoped_scene(c, scope, index, S, "rt_occluded_scope"); if (src != RT_OK) return src; }
	if (n == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<void*> tmp;
	float *dO = nullptr, *dD = nullptr, *dT = nullptr;
	unsigned char* dR = nullptr;
	uint* dL = nullptr;
	int rc = RT_OK;
	const int walk = any_hit_walk(c->counting != 0, c->S.wide != nullptr, S.wide8 != nullptr); // (the context's 4-wide nodes, the scope's 8-wide ones: DESIGN.md section 3)
	const bool wideWalk = walk_is_wide(walk);
	hipError_t e = dalloc(tmp, &dO, (size_t)3 * n);
	if (e == hipSuccess) e = dalloc(tmp, &dD, (size_t)3 * n);
	if (e == hipSuccess && tmax) e = dalloc(tmp, &dT, (size_t)n);
	if (e == hipSuccess) e = dalloc(tmp, &dR, (size_t)n);
	if (e == hipSuccess && wideWalk) e = dalloc(tmp, &dL, (size_t)n);
	if (e == hipSuccess) e = hipMemcpyAsync(dO, O, (size_t)12 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(dD, D, (size_t)12 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess && tmax) e = hipMemcpyAsync(dT, tmax, (size_t)4 * n, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess) {
		(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
		prof_begin(c, K_QUERY);
		if (wideWalk) (void)hipMemsetAsync(c->flags + 2, 0, sizeof(int), c->stream);
		hipLaunchKernelGGL(kQueryOccluded[walk], dim3(query_grid(c, n)), dim3(RT_BLOCK), 0, c->stream, S, n, dO, dD, dT, tuning(c), dR, c->spill, c->flags, c->counters + 1, dL);
		if (wideWalk) {
			// the binary walk over the rays the wide walk handed back (not clean: normally none)
			(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream);
			hipLaunchKernelGGL(kQueryOccluded[WALK_LISTED], dim3(query_grid(c, n)), dim3(RT_BLOCK), 0, c->stream, S, n, dO, dD, dT, tuning(c), dR, c->spill, c->flags, c->counters + 1, dL);
		}
		prof_end(c);
		e = hipStreamSynchronize(c->stream);
	}
	if (e == hipSuccess) e = hipMemcpy(out, dR, (size_t)n, hipMemcpyDeviceToHost);
	if (e != hipSuccess) rc = fail(c, RT_E_HIP, "rt_occluded_batch: %s", hipGetErrorString(e));
	free_pool(tmp);
	if (rc == RT_OK) rc = check_overflow(c);
	return rc;
}

int rt_primary_hits(rt_ctx* c, float t_min, int32_t* obj_out, float* t_out)
{
	if (!c || !obj_out || !t_out) return fail(c, RT_E_ARG, "rt_primary_hits: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_primary_hits: no scene uploaded");
	HIPCHK(c, hipSetDevice(c->device));
	const int n = c->width * c->height;
	std::vector<void*> tmp;
	int* dO = nullptr;
	float* dT = nullptr;
	int rc = RT_OK;
	hipError_t e = dalloc(tmp, &dO, (size_t)n);
	if (e == hipSuccess) e = dalloc(tmp, &dT, (size_t)n);
	if (e == hipSuccess) {
		(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
		prof_begin(c, K_QUERY);
		hipLaunchKernelGGL(kPrimaryHits[c->counting ? 1 : 0], dim3(query_grid(c, n)), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, t_min, tuning(c), dO, dT, c->spill, c->flags, c->counters);
		prof_end(c);
		e = hipStreamSynchronize(c->stream);
	}
	if (e == hipSuccess) e = hipMemcpy(obj_out, dO, (size_t)n * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(t_out, dT, (size_t)n * 4, hipMemcpyDeviceToHost);
	if (e != hipSuccess) rc = fail(c, RT_E_HIP, "rt_primary_hits: %s", hipGetErrorString(e));
	free_pool(tmp);
	if (rc == RT_OK) rc = check_overflow(c);
	return rc;
}

