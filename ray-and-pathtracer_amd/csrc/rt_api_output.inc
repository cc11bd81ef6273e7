// The host helpers of the stage between the accumulator and the screen, written once for the four row downloads, the three resolves and
// the two a-trous drivers (rt_denoise, rt_denoise_variance).  Included by rt_api.hip before the first of them.
static bool rows_ok(const rt_ctx* c, int y0, int y1) { return c && y0 >= 0 && y1 <= c->height && y0 < y1; } // rows [y0, y1) of c's frame
// rows row_first + k*row_stride, k < row_count, of c's frame: the one rule of rt_gather_rows, rt_gather_stats_rows and the _rows selections
static bool row_set_ok(const rt_ctx* c, int row_first, int row_stride, int row_count)
{
	return c && row_first >= 0 && row_stride >= 1 && row_count >= 1 && (long long)row_first + (long long)(row_count - 1) * row_stride < c->height;
}

// rows [y0, y1) of frame-sized device arrays, after everything the stream has queued; a null dst is an output the caller did not ask for
struct RowCopy { const void* src; void* dst; size_t elem; };
static int download_rows(rt_ctx* c, int y0, int y1, std::initializer_list<RowCopy> copies)
{
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const size_t first = (size_t)y0 * c->width, n = (size_t)(y1 - y0) * c->width;
	for (const RowCopy& r : copies) if (r.dst) HIPCHK(c, hipMemcpy(r.dst, (const char*)r.src + first * r.elem, n * r.elem, hipMemcpyDeviceToHost));
	return RT_OK;
}

// rows [y0, y1) of src as RGB8: divided by the pixel's own count where there is one (k_resolve_adaptive), by it otherwise (k_resolve)
static int resolve_rows(rt_ctx* c, const float4* src, const uint* count, int it, int y0, int y1, uint32_t* rgb8_out)
{
	HIPCHK(c, hipSetDevice(c->device));
	const int first = y0 * c->width, n = (y1 - y0) * c->width;
	// one frame-sized pixel buffer per context, kept: Tick resolves every frame
	if (!c->resolveBuf) HIPCHK(c, hipMalloc((void**)&c->resolveBuf, (size_t)c->width * c->height * 4));
	if (count) hipLaunchKernelGGL(k_resolve_adaptive, dim3((n + 255) / 256), dim3(256), 0, c->stream, src, count, first, n, c->resolveBuf);
	else hipLaunchKernelGGL(k_resolve, dim3((n + 255) / 256), dim3(256), 0, c->stream, src, first, n, it, c->resolveBuf);
	HIPCHK(c, hipMemcpyAsync(rgb8_out, c->resolveBuf, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return RT_OK;
}

static bool aovs_current(const rt_ctx* c) { return c->aovNrm && c->aovGen == c->sceneGen; }
// 1 / sigma^2 in f32; sigma = +inf gives 0 (the term is dropped), a k that overflows is FLT_MAX (so a zero distance adds 0, not 0 x inf = NaN)
static float denoise_k_clamp(float k) { return std::min(k, FLT_MAX); }
static float denoise_k(float sigma) { return denoise_k_clamp(1.0f / (sigma * sigma)); }
static bool denoise_sigma_ok(float sigma) { return sigma > 0.0f; } // (false for NaN)

// the checks the two parameter records share (s0: sigma_color / sigma_luminance), made before the context: a null one reports them through rt_last_error(NULL)
static int atrous_check(rt_ctx* c, const char* fn, int iterations, float s0, float sNormal, float sPosition, float sAlbedo)
{
	if (iterations < 1 || iterations > 8) return fail(c, RT_E_ARG, "%s: %d iterations (1..8)", fn, iterations);
	if (!denoise_sigma_ok(s0) || !denoise_sigma_ok(sNormal) || !denoise_sigma_ok(sPosition) || !denoise_sigma_ok(sAlbedo))
		return fail(c, RT_E_ARG, "%s: every sigma must be > 0 (+inf drops its term)", fn);
	return RT_OK;
}

// a current G-buffer, the ping-pong pair, and the part of the kernels' arguments that no iteration changes
static int atrous_begin(rt_ctx* c, const char* fn, AtrousArgs& A, float sNormal, float sPosition, float sAlbedo)
{
	if (!aovs_current(c)) return fail(c, RT_E_STATE, "%s: the G-buffer is %s (rt_render_aovs)", fn, c->aovNrm ? "stale" : "missing");
	HIPCHK(c, hipSetDevice(c->device));
	if (!c->denoiseBuf[0]) {
		const size_t n = (size_t)c->width * c->height;
		float4 *b0 = nullptr, *b1 = nullptr;
		hipError_t e = dalloc(c->denoiseAllocs, &b0, n);
		if (e == hipSuccess) e = dalloc(c->denoiseAllocs, &b1, n);
		if (e != hipSuccess) return fail(c, RT_E_HIP, "%s: %s", fn, hipGetErrorString(e));
		c->denoiseBuf[0] = b0, c->denoiseBuf[1] = b1;
	}
	A.nrm = c->aovNrm, A.pos = c->aovPos, A.alb = c->aovAlb;
	A.width = c->width, A.height = c->height;
	A.kn = denoise_k(sNormal), A.kx = denoise_k(sPosition), A.ka = denoise_k(sAlbedo);
	return RT_OK;
}

// iteration i reads what i - 1 wrote (0: first -- the accumulator, or buffer 1 where the variance filter's init wrote) and writes buffer i & 1 at step 2^i
extern "C++" { // (rt_api.hip includes this inside its extern "C")
template <class Launch>
static int atrous_run(rt_ctx* c, AtrousArgs& A, int iterations, const float4* first, Launch launch)
{
	for (int i = 0; i < iterations; i++) {
		A.in = i == 0 ? first : c->denoiseBuf[(i - 1) & 1];
		A.out = c->denoiseBuf[i & 1];
		A.step = 1 << i;
		launch(i, dim3((c->width + RT_DENOISE_TX - 1) / RT_DENOISE_TX, (c->height + RT_DENOISE_TY - 1) / RT_DENOISE_TY), dim3(RT_DENOISE_TX, RT_DENOISE_TY));
	}
	HIPCHK(c, hipGetLastError());
	c->denoised = c->denoiseBuf[(iterations - 1) & 1];
	return RT_OK;
}
}
