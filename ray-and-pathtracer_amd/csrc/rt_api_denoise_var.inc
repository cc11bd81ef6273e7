// The variance-guided denoiser of an adaptively sampled frame: rt_denoise_variance.  Included by rt_api.hip after rt_api_denoise.inc
// (the G-buffer, the ping-pong buffers, the k helpers) and rt_api_adaptive.inc (the statistics).  The kernels are k_denoise_var_init and
// k_denoise_var_atrous (rt_denoise_var.h); the result is served by rt_download_denoised / rt_resolve_denoised.
int rt_denoise_variance(rt_ctx* c, const rt_denoise_var_params* params)
{
	// the arguments are checked before the context (a null context reports them through rt_last_error(NULL))
	const rt_denoise_var_params P = params ? *params : rt_denoise_var_params RT_DENOISE_VAR_DEFAULTS;
	if (P.iterations < 1 || P.iterations > 8) return fail(c, RT_E_ARG, "rt_denoise_variance: %d iterations (1..8)", P.iterations);
	if (!denoise_sigma_ok(P.sigma_luminance) || !denoise_sigma_ok(P.sigma_normal) || !denoise_sigma_ok(P.sigma_position) || !denoise_sigma_ok(P.sigma_albedo))
		return fail(c, RT_E_ARG, "rt_denoise_variance: every sigma must be > 0 (+inf drops its term)");
	if (!(P.epsilon > 0.0f)) return fail(c, RT_E_ARG, "rt_denoise_variance: epsilon must be > 0");
	if (!c) return fail(c, RT_E_ARG, "rt_denoise_variance: null context");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_denoise_variance: statistics are off (rt_stats_enable)");
	if (!aovs_current(c)) return fail(c, RT_E_STATE, "rt_denoise_variance: the G-buffer is %s (rt_render_aovs)", c->aovNrm ? "stale" : "missing");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * c->height;
	if (!c->denoiseBuf[0]) {
		float4 *b0 = nullptr, *b1 = nullptr;
		hipError_t e = dalloc(c->denoiseAllocs, &b0, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &b1, n);
		if (e != hipSuccess) return fail(c, RT_E_HIP, "rt_denoise_variance: %s", hipGetErrorString(e));
		c->denoiseBuf[0] = b0, c->denoiseBuf[1] = b1;
	}
	// init writes buffer 1; iteration i reads (i + 1) & 1 and writes i & 1
	hipLaunchKernelGGL(k_denoise_var_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->accum, c->stats, (int)n, c->denoiseBuf[1]);
	DenoiseVarArgs A;
	A.nrm = c->aovNrm, A.pos = c->aovPos, A.alb = c->aovAlb;
	A.width = c->width, A.height = c->height;
	A.sl = P.sigma_luminance, A.eps = P.epsilon;
	A.kn = denoise_k(P.sigma_normal), A.kx = denoise_k(P.sigma_position), A.ka = denoise_k(P.sigma_albedo);
	const dim3 grid((c->width + RT_DENOISE_TX - 1) / RT_DENOISE_TX, (c->height + RT_DENOISE_TY - 1) / RT_DENOISE_TY), block(RT_DENOISE_TX, RT_DENOISE_TY);
	for (int i = 0; i < P.iterations; i++) {
		A.in = c->denoiseBuf[(i + 1) & 1];
		A.out = c->denoiseBuf[i & 1];
		A.step = 1 << i;
		A.last = i == P.iterations - 1;
		hipLaunchKernelGGL(k_denoise_var_atrous, grid, block, 0, c->stream, A);
	}
	HIPCHK(c, hipGetLastError());
	c->denoised = c->denoiseBuf[(P.iterations - 1) & 1];
	return RT_OK;
}
