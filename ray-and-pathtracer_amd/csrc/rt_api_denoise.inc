// G-buffer (primary-hit AOVs) and the two edge-avoiding a-trous denoisers: rt_render_aovs, rt_download_aovs, rt_denoise, rt_denoise_variance,
// rt_download_denoised, rt_resolve_denoised.  Included by rt_api.hip after rt_api_output.inc (the helpers they share).  The kernels are
// k_primary_aovs (rt_kernels.h), k_denoise_atrous (rt_denoise.h) and k_denoise_var_init, k_denoise_var_atrous (rt_denoise_var.h).

int rt_render_aovs(rt_ctx* c, float t_min)
{
	if (!c || !(t_min == t_min)) return fail(c, RT_E_ARG, "rt_render_aovs: bad argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_render_aovs: no scene uploaded");
	if (aovs_current(c) && memcmp(&c->aovTmin, &t_min, sizeof(float)) == 0) return RT_OK; // nothing changed since the last pass
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * c->height;
	if (!c->aovNrm) {
		float4 *nrm = nullptr, *pos = nullptr, *alb = nullptr; // (what was allocated before a failure is freed by rt_destroy)
		int *inst = nullptr, *prim = nullptr;
		hipError_t e = dalloc(c->denoiseAllocs, &nrm, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &pos, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &alb, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &inst, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &prim, n);
		if (e != hipSuccess) return fail(c, RT_E_HIP, "rt_render_aovs: %s", hipGetErrorString(e));
		c->aovNrm = nrm, c->aovPos = pos, c->aovAlb = alb, c->aovInst = inst, c->aovPrim = prim;
	}
	c->aovGen = 0; // not current until the pass has finished
	(void)hipMemsetAsync(c->flags + 16, 0, RT_HEADS * RT_HEAD_STRIDE * sizeof(int), c->stream); // work heads
	const int grid = std::min(query_grid(c, (int)n), c->gridAovs);
	prof_begin(c, K_QUERY);
	if (c->counting) hipLaunchKernelGGL(k_primary_aovs<true>, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, t_min, tuning(c), c->aovNrm, c->aovPos, c->aovAlb, c->aovInst, c->aovPrim, c->spill, c->flags, c->counters);
	else hipLaunchKernelGGL(k_primary_aovs<false>, dim3(grid), dim3(RT_BLOCK), 0, c->stream, c->S, c->C, t_min, tuning(c), c->aovNrm, c->aovPos, c->aovAlb, c->aovInst, c->aovPrim, c->spill, c->flags, c->counters);
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
	if (!rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_aovs: bad argument");
	if (!c->aovNrm || c->aovGen == 0) return fail(c, RT_E_STATE, "rt_download_aovs: no G-buffer (rt_render_aovs)");
	const size_t n = (size_t)(y1 - y0) * c->width;
	std::vector<float4> nrm(n), pos(hits_out ? n : 0), alb(n);
	const int rc = download_rows(c, y0, y1, { { c->aovNrm, nrm.data(), sizeof(float4) }, { c->aovAlb, alb.data(), sizeof(float4) }, { c->aovPos, hits_out ? pos.data() : nullptr, sizeof(float4) } });
	if (rc != RT_OK) return rc;
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

int rt_denoise(rt_ctx* c, int iteration, const rt_denoise_params* params)
{
	const rt_denoise_params P = params ? *params : rt_denoise_params RT_DENOISE_DEFAULTS;
	if (iteration < 1) return fail(c, RT_E_ARG, "rt_denoise: iteration %d (>= 1)", iteration);
	int rc = atrous_check(c, "rt_denoise", P.iterations, P.sigma_color, P.sigma_normal, P.sigma_position, P.sigma_albedo);
	if (rc != RT_OK) return rc;
	if (!c) return fail(c, RT_E_ARG, "rt_denoise: null context");
	DenoiseArgs A;
	rc = atrous_begin(c, "rt_denoise", A, P.sigma_normal, P.sigma_position, P.sigma_albedo);
	if (rc != RT_OK) return rc;
	A.it = (float)iteration;
	const float kc0 = denoise_k(P.sigma_color);
	return atrous_run(c, A, P.iterations, c->accum, [&](int i, dim3 grid, dim3 block) {
		A.kc = denoise_k_clamp(kc0 * (float)(1 << (2 * i))); // sigma_c halves every iteration (exact: a power of two, until it overflows)
		if (i == 0) hipLaunchKernelGGL(k_denoise_atrous<true>, grid, block, 0, c->stream, A);
		else hipLaunchKernelGGL(k_denoise_atrous<false>, grid, block, 0, c->stream, A);
	});
}

// the variance-guided filter of an adaptively sampled frame: init writes buffer 1, the iterations follow; served like rt_denoise's result
int rt_denoise_variance(rt_ctx* c, const rt_denoise_var_params* params)
{
	const rt_denoise_var_params P = params ? *params : rt_denoise_var_params RT_DENOISE_VAR_DEFAULTS;
	int rc = atrous_check(c, "rt_denoise_variance", P.iterations, P.sigma_luminance, P.sigma_normal, P.sigma_position, P.sigma_albedo);
	if (rc != RT_OK) return rc;
	if (!(P.epsilon > 0.0f)) return fail(c, RT_E_ARG, "rt_denoise_variance: epsilon must be > 0");
	if (!c) return fail(c, RT_E_ARG, "rt_denoise_variance: null context");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_denoise_variance: statistics are off (rt_stats_enable)");
	DenoiseVarArgs A;
	rc = atrous_begin(c, "rt_denoise_variance", A, P.sigma_normal, P.sigma_position, P.sigma_albedo);
	if (rc != RT_OK) return rc;
	A.sl = P.sigma_luminance, A.eps = P.epsilon;
	const int n = c->width * c->height;
	hipLaunchKernelGGL(k_denoise_var_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->accum, c->stats, n, c->denoiseBuf[1]);
	return atrous_run(c, A, P.iterations, c->denoiseBuf[1], [&](int i, dim3 grid, dim3 block) {
		A.last = i == P.iterations - 1;
		hipLaunchKernelGGL(k_denoise_var_atrous, grid, block, 0, c->stream, A);
	});
}

int rt_download_denoised(rt_ctx* c, int y0, int y1, float* out)
{
	if (!out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_denoised: bad argument");
	if (!c->denoised) return fail(c, RT_E_STATE, "rt_download_denoised: nothing denoised (rt_denoise)");
	return download_rows(c, y0, y1, { { c->denoised, out, sizeof(float4) } });
}

int rt_resolve_denoised(rt_ctx* c, int y0, int y1, uint32_t* rgb8_out)
{
	if (!rgb8_out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_resolve_denoised: bad argument");
	if (!c->denoised) return fail(c, RT_E_STATE, "rt_resolve_denoised: nothing denoised (rt_denoise)");
	return resolve_rows(c, c->denoised, nullptr, 1, y0, y1, rgb8_out);
}
