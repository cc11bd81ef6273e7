// The camera-sample settings of path mode: the pixel filter, the thin lens, the shutter, autofocus (rt_focus_at) and rt_sample_rays, with the
// checks a call that takes camera samples makes of them (filter_check, lens_check, shutter_check) and set_lens, which puts them into a batch.
// Included by rt_api.hip before rt_api_render.inc.
// dot and cross as include/rt_amd.h defines them (rt_reproject), on the host: this translation unit is compiled with -ffp-contract=off
// (csrc/Makefile), so these are the bits the definition of rt_set_lens names
static float host_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// N = cross(TR - TL, BL - TL) of the camera's screen rectangle
static void screen_normal(const DCamera& C, float* N)
{
	float A[3], B[3];
	for (int i = 0; i < 3; i++) A[i] = C.topRight[i] - C.topLeft[i], B[i] = C.bottomLeft[i] - C.topLeft[i];
	N[0] = A[1] * B[2] - A[2] * B[1], N[1] = A[2] * B[0] - A[0] * B[2], N[2] = A[0] * B[1] - A[1] * B[0];
}
// lam = focus_distance / screen_dist of a pinhole camera, as include/rt_amd.h defines it (rt_set_lens)
static float lens_lam(const DCamera& C, float focusDistance)
{
	float N[3], E[3];
	screen_normal(C, N);
	for (int i = 0; i < 3; i++) E[i] = C.topLeft[i] - C.camPos[i];
	const float screenDist = fabsf(host_dot(E, N)) / sqrtf(host_dot(N, N));
	return focusDistance / screenDist;
}
// rt_set_lens's rules for a call that takes path-mode camera samples (include/rt_amd.h), and the lens's one derived number:
// *lam = focus_distance / screen_dist, or 0 with the lens off
static int lens_check(rt_ctx* c, const char* fn, float* lam)
{
	*lam = 0.0f;
	if (!(c->lens.radius > 0.0f)) return RT_OK;
	if (c->pixelFilter == RT_FILTER_REFERENCE)
		return fail(c, RT_E_UNSUPPORTED, "%s: a lens (rt_set_lens) with RT_FILTER_REFERENCE: the reference's jitter lives on the path's own stream; set a kind with rt_set_pixel_filter first", fn);
	if (c->C.fisheye) return fail(c, RT_E_UNSUPPORTED, "%s: a lens (rt_set_lens) under a fisheye camera", fn);
	const float l = lens_lam(c->C, c->lens.focus_distance);
	if (!(std::isfinite(l) && l > 0.0f)) return fail(c, RT_E_UNSUPPORTED, "%s: a lens (rt_set_lens) over a degenerate screen rectangle (focus_distance / screen_dist = %g)", fn, (double)l);
	*lam = l;
	return RT_OK;
}
// rt_set_shutter's rules for a call that takes path-mode camera samples (include/rt_amd.h), behind a lens_check that passed: with a
// lens, lam is a number of every sample's own camera, which the device computes, and *lam becomes what the device computes it from,
// the focus distance itself (set_lens)
static int shutter_check(rt_ctx* c, const char* fn, float* lam)
{
	if (!c->shutterOn) return RT_OK;
	if (c->pixelFilter == RT_FILTER_REFERENCE)
		return fail(c, RT_E_UNSUPPORTED, "%s: a shutter (rt_set_shutter) with RT_FILTER_REFERENCE: the reference's jitter lives on the path's own stream; set a kind with rt_set_pixel_filter first", fn);
	if (c->C.fisheye) return fail(c, RT_E_UNSUPPORTED, "%s: a shutter (rt_set_shutter) under a fisheye camera", fn);
	if (c->lens.radius > 0.0f) {
		DCamera close = c->C;
		memcpy(close.camPos, c->shutterCam.cam_pos, 12), memcpy(close.topLeft, c->shutterCam.top_left, 12);
		memcpy(close.topRight, c->shutterCam.top_right, 12), memcpy(close.bottomLeft, c->shutterCam.bottom_left, 12);
		const float l = lens_lam(close, c->lens.focus_distance);
		if (!(std::isfinite(l) && l > 0.0f)) return fail(c, RT_E_UNSUPPORTED, "%s: a lens (rt_set_lens) over a degenerate screen rectangle of the shutter's closing camera (rt_set_shutter; focus_distance / screen_dist = %g)", fn, (double)l);
		*lam = c->lens.focus_distance;
	}
	return RT_OK;
}
// rt_set_pixel_filter's, rt_set_lens's and rt_set_shutter's rules for a path-mode render call (include/rt_amd.h); fn: the entry point the caller came through
static int filter_check(rt_ctx* c, const char* fn, float* lam)
{
	int rc = lens_check(c, fn, lam);
	if (rc == RT_OK) rc = shutter_check(c, fn, lam);
	if (rc != RT_OK || c->pixelFilter == RT_FILTER_REFERENCE) return rc;
	if (c->Qt.on) return fail(c, RT_E_UNSUPPORTED, "%s: a pixel filter with the Q-learning sampler on (its learn_mask is defined on the post-jitter state)", fn);
	if (c->C.fisheye && c->pixelFilter != RT_FILTER_POINT) return fail(c, RT_E_UNSUPPORTED, "%s: RT_FILTER_BOX / RT_FILTER_TENT under a fisheye camera", fn);
	return RT_OK;
}
// the lens and the shutter of a batch of camera samples (lam: filter_check's, or lens_check's and shutter_check's; R.mode is set)
static void set_lens(const rt_ctx* c, RenderParams& R, float lam)
{
	if (lam > 0.0f) R.lensRadius = c->lens.radius, R.lensLam = lam;
	if (c->shutterOn && R.mode == RT_MODE_PATH) R.shutter = c->shutterDev;
}

// ---- pixel filter (include/rt_amd.h) ------------------------------------------------------------------
int rt_set_pixel_filter(rt_ctx* c, int kind)
{
	if (!c || kind < RT_FILTER_REFERENCE || kind > RT_FILTER_TENT) return fail(c, RT_E_ARG, "rt_set_pixel_filter: kind %d", kind);
	c->pixelFilter = kind; // neither the accumulator nor the G-buffer depends on it
	return RT_OK;
}
int rt_get_pixel_filter(const rt_ctx* c) { return c ? c->pixelFilter : RT_E_ARG; }

int rt_sample_rays(rt_ctx* c, uint32_t frame, uint32_t seed_base, int y0, int y1, float* O_out, float* D_out)
{
	if (!c || !O_out || !D_out) return fail(c, RT_E_ARG, "rt_sample_rays: null argument");
	if (y0 < 0 || y1 > c->height || y0 >= y1) return fail(c, RT_E_ARG, "rt_sample_rays: rows [%d,%d) outside 0..%d", y0, y1, c->height);
	if (c->C.fisheye && c->pixelFilter > RT_FILTER_POINT) return fail(c, RT_E_UNSUPPORTED, "rt_sample_rays: RT_FILTER_BOX / RT_FILTER_TENT under a fisheye camera");
	float lam = 0.0f;
	{
		int lrc = lens_check(c, "rt_sample_rays", &lam);
		if (lrc == RT_OK) lrc = shutter_check(c, "rt_sample_rays", &lam);
		if (lrc != RT_OK) return lrc;
	}
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * (size_t)(y1 - y0);
	float *dO = nullptr, *dD = nullptr;
	std::vector<void*> tmp;
	struct Guard { rt_ctx* c; std::vector<void*>& v; ~Guard() { (void)hipStreamSynchronize(c->stream); free_pool(v); } } guard{ c, tmp }; // every return path frees
	HIPCHK(c, dalloc(tmp, &dO, 3 * n));
	HIPCHK(c, dalloc(tmp, &dD, 3 * n));
	RenderParams R;
	memset(&R, 0, sizeof(R));
	R.mode = RT_MODE_PATH, R.frame0 = frame, R.nSamples = (uint)n, R.tilePixels = (uint)n, R.seedBase = seed_base, R.rowFirst = y0, R.rowStride = 1;
	R.sceneRt = -1, R.filter = c->pixelFilter;
	set_lens(c, R, lam);
	prof_begin(c, K_QUERY);
	hipLaunchKernelGGL(k_sample_rays, dim3((unsigned)((n + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, c->stream, c->C, R, dO, dD);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(O_out, dO, 12 * n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(D_out, dD, 12 * n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return RT_OK;
}

// ---- thin lens (include/rt_amd.h) ------------------------------------------------------------------
int rt_set_lens(rt_ctx* c, const rt_lens* lens)
{
	if (!c) return fail(c, RT_E_ARG, "rt_set_lens: null context");
	const rt_lens off = { 0.0f, c->lens.focus_distance };
	const rt_lens l = lens ? *lens : off;
	if (!std::isfinite(l.radius) || l.radius < 0.0f) return fail(c, RT_E_ARG, "rt_set_lens: radius %g", (double)l.radius);
	if (l.radius > 0.0f && !(std::isfinite(l.focus_distance) && l.focus_distance > 0.0f)) return fail(c, RT_E_ARG, "rt_set_lens: focus_distance %g", (double)l.focus_distance);
	c->lens = l; // the accumulator, the G-buffer, a captured history, a list and a plan do not depend on it
	return RT_OK;
}
int rt_get_lens(const rt_ctx* c, rt_lens* out)
{
	if (!c || !out) return RT_E_ARG;
	*out = c->lens;
	return RT_OK;
}

// ---- shutter (include/rt_amd.h) --------------------------------------------------------------------
int rt_set_shutter(rt_ctx* c, const rt_camera* cam_close)
{
	if (!c) return fail(c, RT_E_ARG, "rt_set_shutter: null context");
	if (!cam_close) { c->shutterOn = false; return RT_OK; } // (the record stays: nothing reads it with the shutter off)
	if (cam_close->fisheye != 0) return fail(c, RT_E_ARG, "rt_set_shutter: a fisheye closing camera");
	ShutterCam rec;
	memcpy(rec.camPos, cam_close->cam_pos, 12), memcpy(rec.topLeft, cam_close->top_left, 12);
	memcpy(rec.topRight, cam_close->top_right, 12), memcpy(rec.bottomLeft, cam_close->bottom_left, 12);
	const float* f = (const float*)&rec;
	for (int i = 0; i < 12; i++)
		if (!std::isfinite(f[i])) return fail(c, RT_E_ARG, "rt_set_shutter: float %d of the closing camera's twelve is %g", i, (double)f[i]);
	// the device's record, on the context's stream: batches launched before see the record before.  (The copy of a host record this small
	// is staged before the call returns, so 'rec' may leave.)  The accumulator, the G-buffer, a captured history, a list and a plan do
	// not depend on it.
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(c->shutterDev, &rec, sizeof(rec), hipMemcpyHostToDevice, c->stream));
	c->shutterCam = *cam_close, c->shutterOn = true;
	return RT_OK;
}
int rt_get_shutter(const rt_ctx* c, rt_camera* out)
{
	if (!c || !out) return RT_E_ARG;
	if (!c->shutterOn) return 0;
	*out = c->shutterCam;
	return 1;
}

// Autofocus: Camera::GetPrimaryRay(x, y) on the host -- primary_ray_f's operations on whole coordinates, the bits k_primary_aovs gives the
// pixel's ray -- then one ray through rt_intersect_batch (one launch, one query of the profile).
int rt_focus_at(rt_ctx* c, int x, int y, float* distance_out)
{
	if (!c || !distance_out) return fail(c, RT_E_ARG, "rt_focus_at: null argument");
	if (x < 0 || x >= c->width || y < 0 || y >= c->height) return fail(c, RT_E_ARG, "rt_focus_at: pixel (%d, %d) outside %d x %d", x, y, c->width, c->height);
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_focus_at: no scene uploaded");
	if (c->C.fisheye) return fail(c, RT_E_UNSUPPORTED, "rt_focus_at: a fisheye camera");
	const DCamera& C = c->C;
	const float u = (float)x * (1.0f / C.width), v = (float)y * (1.0f / C.height);
	float O[3], D[3], N[3];
	for (int i = 0; i < 3; i++) {
		const float P = C.topLeft[i] + u * (C.topRight[i] - C.topLeft[i]) + v * (C.bottomLeft[i] - C.topLeft[i]);
		O[i] = C.camPos[i], D[i] = P - C.camPos[i];
	}
	const float invLen = 1.0f / sqrtf(host_dot(D, D));
	for (int i = 0; i < 3; i++) D[i] = D[i] * invLen;
	rt_hit hit;
	const int rc = rt_intersect_batch(c, 1, O, D, nullptr, 0.001f, &hit);
	if (rc != RT_OK) return rc;
	screen_normal(C, N);
	*distance_out = hit.obj_idx < 0 ? 0.0f : hit.t * (fabsf(host_dot(D, N)) / sqrtf(host_dot(N, N)));
	return RT_OK;
}
