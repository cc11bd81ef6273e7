// G-buffer (primary-hit AOVs) and the edge-avoiding a-trous denoiser: rt_render_aovs, rt_download_aovs, rt_denoise, rt_download_denoised,
// rt_resolve_denoised.  Included by rt_api.hip.  The kernels are k_primary_aovs (rt_kernels.h) and k_denoise_atrous (rt_denoise.h).
static bool aovs_current(const rt_ctx* c) { return c->aovNrm && c->aovGen == c->sceneGen; }

int rt_render_aovs(rt_ctx* c, float t_min)
{
	if (!c || !(t_min == t_min)) return fail(c, RT_E_ARG, "rt_render_aovs: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_render_aovs: no scene uploaded");
	if (aovs_current(c) && memcmp(&c->aovTmin, &t_min, sizeof(float)) == 0) return RT_OK; // nothing changed since the last pass
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * c->height;
	if (!c->aovNrm) {
		float4 *nrm = nullptr, *pos = nullptr, *alb = nullptr; // (what was allocated before a failure is freed by rt_destroy)
		hipError_t e = dalloc(c->denoiseAllocs, &nrm, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &pos, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &alb, n);
		if (e != hipSuccess) return fail(c, RT_E_HIP, "rt_render_aovs: %s", hipGetErrorString(e));
		c->aovNrm = nrm, c->aovPos = pos, c->aovAlb = alb;
	}
	c->aovGen = 0; // not current until the pass has finished
	(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
	const int grid = std::min(query_grid(c, (int)n), c->gridAovs);
	prof_begin(c, K_QUERY);
	if (c->counting) hipLaunchKernelGGL(k_primary_aovs<true>, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, t_min, tuning(c), c->aovNrm, c->aovPos, c->aovAlb, c->spill, c->flags, c->counters);
	else hipLaunchKernelGGL(k_primary_aovs<false>, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, t_min, tuning(c), c->aovNrm, c->aovPos, c->aovAlb, c->spill, c->flags, c->counters);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const int rc = check_overflow(c);
	if (rc != RT_OK) return rc;
	c->aovGen = c->sceneGen, c->aovTmin = t_min;
	return RT_OK;
}

int rt_download_aovs(rt_ctx* c, int y0, int y1, rt_hit* hits_out, float* albedo_rgb_out)
{
	if (!c || y0 < 0 || y1 > c->height || y0 >= y1) return fail(c, RT_E_ARG, "rt_download_aovs: bad argument");
	if (!c->aovNrm || c->aovGen == 0) return fail(c, RT_E_STATE, "rt_download_aovs: no G-buffer (rt_render_aovs)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const size_t first = (size_t)y0 * c->width, n = (size_t)(y1 - y0) * c->width;
	std::vector<float4> nrm(n), pos(hits_out ? n : 0), alb(n);
	HIPCHK(c, hipMemcpy(nrm.data(), c->aovNrm + first, n * sizeof(float4), hipMemcpyDeviceToHost));
	HIPCHK(c, hipMemcpy(alb.data(), c->aovAlb + first, n * sizeof(float4), hipMemcpyDeviceToHost));
	if (hits_out) HIPCHK(c, hipMemcpy(pos.data(), c->aovPos + first, n * sizeof(float4), hipMemcpyDeviceToHost));
	for (size_t i = 0; i < n; i++) {
		if (hits_out) {
			rt_hit& h = hits_out[i];
			h.t = nrm[i].w, h.normal[0] = nrm[i].x, h.normal[1] = nrm[i].y, h.normal[2] = nrm[i].z;
			memcpy(&h.obj_idx, &pos[i].w, 4), memcpy(&h.material, &alb[i].w, 4);
		}
		if (albedo_rgb_out) albedo_rgb_out[3 * i] = alb[i].x, albedo_rgb_out[3 * i + 1] = alb[i].y, albedo_rgb_out[3 * i + 2] = alb[i].z;
	}
	return RT_OK;
}

// 1 / sigma^2 in f32; sigma = +inf gives 0 (the term is dropped), a k that overflows is FLT_MAX (so a zero distance adds 0, not 0 x inf = NaN)
static float denoise_k_clamp(float k) { return std::min(k, FLT_MAX); }
static float denoise_k(float sigma) { return denoise_k_clamp(1.0f / (sigma * sigma)); }
static bool denoise_sigma_ok(float sigma) { return sigma > 0.0f; } // (false for NaN)

int rt_denoise(rt_ctx* c, int iteration, const rt_denoise_params* params)
{
	// the arguments are checked before the context (a null context reports them through rt_last_error(NULL))
	const rt_denoise_params P = params ? *params : rt_denoise_params RT_DENOISE_DEFAULTS;
	if (iteration < 1) return fail(c, RT_E_ARG, "rt_denoise: iteration %d (>= 1)", iteration);
	if (P.iterations < 1 || P.iterations > 8) return fail(c, RT_E_ARG, "rt_denoise: %d iterations (1..8)", P.iterations);
	if (!denoise_sigma_ok(P.sigma_color) || !denoise_sigma_ok(P.sigma_normal) || !denoise_sigma_ok(P.sigma_position) || !denoise_sigma_ok(P.sigma_albedo))
		return fail(c, RT_E_ARG, "rt_denoise: every sigma must be > 0 (+inf drops its term)");
	if (!c) return fail(c, RT_E_ARG, "rt_denoise: null context");
	if (!aovs_current(c)) return fail(c, RT_E_STATE, "rt_denoise: the G-buffer is %s (rt_render_aovs)", c->aovNrm ? "stale" : "missing");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * c->height;
	if (!c->denoiseBuf[0]) {
		float4 *b0 = nullptr, *b1 = nullptr;
		hipError_t e = dalloc(c->denoiseAllocs, &b0, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &b1, n);
		if (e != hipSuccess) return fail(c, RT_E_HIP, "rt_denoise: %s", hipGetErrorString(e));
		c->denoiseBuf[0] = b0, c->denoiseBuf[1] = b1;
	}
	DenoiseArgs A;
	A.nrm = c->aovNrm, A.pos = c->aovPos, A.alb = c->aovAlb;
	A.width = c->width, A.height = c->height;
	A.it = (float)iteration;
	A.kn = denoise_k(P.sigma_normal), A.kx = denoise_k(P.sigma_position), A.ka = denoise_k(P.sigma_albedo);
	const float kc0 = denoise_k(P.sigma_color);
	const dim3 grid((c->width + RT_DENOISE_TX - 1) / RT_DENOISE_TX, (c->height + RT_DENOISE_TY - 1) / RT_DENOISE_TY), block(RT_DENOISE_TX, RT_DENOISE_TY);
	for (int i = 0; i < P.iterations; i++) {
		A.in = i == 0 ? c->accum : c->denoiseBuf[(i - 1) & 1];
		A.out = c->denoiseBuf[i & 1];
		A.step = 1 << i;
		A.kc = denoise_k_clamp(kc0 * (float)(1 << (2 * i))); // sigma_c halves every iteration (exact: a power of two, until it overflows)
		if (i == 0) hipLaunchKernelGGL(k_denoise_atrous<true>, grid, block, 0, c->stream, A);
		else hipLaunchKernelGGL(k_denoise_atrous<false>, grid, block, 0, c->stream, A);
	}
	HIPCHK(c, hipGetLastError());
	c->denoised = c->denoiseBuf[(P.iterations - 1) & 1];
	return RT_OK;
}

int rt_download_denoised(rt_ctx* c, int y0, int y1, float* out)
{
	if (!c || !out || y0 < 0 || y1 > c->height || y0 >= y1) return fail(c, RT_E_ARG, "rt_download_denoised: bad argument");
	if (!c->denoised) return fail(c, RT_E_STATE, "rt_download_denoised: nothing denoised (rt_denoise)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(out, c->denoised + (size_t)y0 * c->width, (size_t)(y1 - y0) * c->width * sizeof(float4), hipMemcpyDeviceToHost));
	return RT_OK;
}

int rt_resolve_denoised(rt_ctx* c, int y0, int y1, uint32_t* rgb8_out)
{
	if (!c || !rgb8_out || y0 < 0 || y1 > c->height || y0 >= y1) return fail(c, RT_E_ARG, "rt_resolve_denoised: bad argument");
	if (!c->denoised) return fail(c, RT_E_STATE, "rt_resolve_denoised: nothing denoised (rt_denoise)");
	HIPCHK(c, hipSetDevice(c->device));
	const int n = (y1 - y0) * c->width;
	if (!c->resolveBuf) HIPCHK(c, hipMalloc((void**)&c->resolveBuf, (size_t)c->width * c->height * 4));
	hipLaunchKernelGGL(k_resolve, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->denoised, y0 * c->width, n, 1, c->resolveBuf);
	HIPCHK(c, hipMemcpyAsync(rgb8_out, c->resolveBuf, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return RT_OK;
}
