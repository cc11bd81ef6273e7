// Carrying samples across a camera move, across instance motion and across mesh deformation: rt_history_capture, rt_reproject,
// rt_reproject_motion, rt_reproject_deform, rt_download_aov_positions, rt_download_aov_instances, rt_download_aov_prims.  Included by
// rt_api.hip after rt_api_adaptive.inc.  The kernels are k_reproject, k_reproject_motion and k_reproject_deform (rt_reproject.h); the copy
// on first write that keeps the capture's triangles for the last is history_keep_blas (rt_api_build.inc).
int rt_download_aov_positions(rt_ctx* c, int y0, int y1, float* xyz_out)
{
	if (!xyz_out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_aov_positions: bad argument");
	if (!c->aovNrm || c->aovGen == 0) return fail(c, RT_E_STATE, "rt_download_aov_positions: no G-buffer (rt_render_aovs)");
	const size_t n = (size_t)(y1 - y0) * c->width;
	std::vector<float4> pos(n);
	const int rc = download_rows(c, y0, y1, { { c->aovPos, pos.data(), sizeof(float4) } });
	if (rc != RT_OK) return rc;
	for (size_t i = 0; i < n; i++) xyz_out[3 * i] = pos[i].x, xyz_out[3 * i + 1] = pos[i].y, xyz_out[3 * i + 2] = pos[i].z;
	return RT_OK;
}

int rt_download_aov_instances(rt_ctx* c, int y0, int y1, int32_t* inst_out)
{
	if (!inst_out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_aov_instances: bad argument");
	if (!c->aovNrm || c->aovGen == 0) return fail(c, RT_E_STATE, "rt_download_aov_instances: no G-buffer (rt_render_aovs)");
	return download_rows(c, y0, y1, { { c->aovInst, inst_out, sizeof(int32_t) } });
}

int rt_download_aov_prims(rt_ctx* c, int y0, int y1, int32_t* prim_out)
{
	if (!prim_out || !rows_ok(c, y0, y1)) return fail(c, RT_E_ARG, "rt_download_aov_prims: bad argument");
	if (!c->aovNrm || c->aovGen == 0) return fail(c, RT_E_STATE, "rt_download_aov_prims: no G-buffer (rt_render_aovs)");
	return download_rows(c, y0, y1, { { c->aovPrim, prim_out, sizeof(int32_t) } });
}

// the three levels of a history's validity: rt_reproject's ends with any change of the surfaces, rt_reproject_motion's outlives
// rt_set_instances, rt_reproject_deform's outlives rt_set_triangles and rt_set_time as well
static bool history_valid_deform(const rt_ctx* c) { return c->hist.acc && c->hist.gen != 0 && c->hist.topoGen == c->topoGen; }
static bool history_valid_motion(const rt_ctx* c) { return c->hist.acc && c->hist.gen != 0 && c->hist.shapeGen == c->shapeGen; }
static bool history_valid(const rt_ctx* c) { return c->hist.acc && c->hist.gen != 0 && c->hist.gen == c->geomGen; }

int rt_history_capture(rt_ctx* c)
{
	if (!c) return fail(c, RT_E_ARG, "rt_history_capture: null context");
	if (!c->stats.count) return fail(c, RT_E_STATE, "rt_history_capture: statistics are off (rt_stats_enable)");
	if (!aovs_current(c)) return fail(c, RT_E_STATE, "rt_history_capture: the G-buffer is %s (rt_render_aovs)", c->aovNrm ? "stale" : "missing");
	if (c->camRec.fisheye) return fail(c, RT_E_UNSUPPORTED, "rt_history_capture: the camera is a fisheye (the projection is the pinhole's)");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->width * c->height;
	rt_ctx::History& H = c->hist;
	if (!H.acc) {
		rt_ctx::History B{};
		hipError_t e = dalloc(c->historyAllocs, &B.acc, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.nrm, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.pos, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.alb, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.stats.count, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.stats.sumY, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.stats.sumYY, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.nCarried, (size_t)1);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.inst, n);
		if (e == hipSuccess) e = dalloc(c->historyAllocs, &B.xf, (size_t)RT_TLAS_MAX);
		if (e != hipSuccess) {
			free_pool(c->historyAllocs);
			c->keptBuf.clear(), c->keptCap.clear(), c->keptMark.clear(), c->keptDeltaHost.clear();
			return fail(c, RT_E_HIP, "rt_history_capture: %s", hipGetErrorString(e));
		}
		H = B;
	}
	H.gen = 0; // not a history until every copy is queued
	// the current records are the capture's from here on: no BLAS has a kept copy (the buffers stay for the next one)
	const size_t nBlas = std::max<size_t>(1, c->blasKeep.size());
	if (H.keptDeltaCap < nBlas) {
		HIPCHK(c, dalloc(c->historyAllocs, &H.keptDelta, nBlas));
		H.keptDeltaCap = nBlas;
	}
	c->keptBuf.resize(nBlas, nullptr), c->keptCap.resize(nBlas, 0);
	c->keptMark.assign(nBlas, 0), c->keptDeltaHost.assign(nBlas, 0);
	HIPCHK(c, hipMemsetAsync(H.keptDelta, 0, H.keptDeltaCap * sizeof(long long), c->stream));
	const struct { void* dst; const void* src; size_t elem; } copies[8] = {
		{ H.acc, c->accum, sizeof(float4) }, { H.nrm, c->aovNrm, sizeof(float4) }, { H.pos, c->aovPos, sizeof(float4) }, { H.alb, c->aovAlb, sizeof(float4) },
		{ H.stats.count, c->stats.count, sizeof(uint) }, { H.stats.sumY, c->stats.sumY, sizeof(float) }, { H.stats.sumYY, c->stats.sumYY, sizeof(float) },
		{ H.inst, c->aovInst, sizeof(int) } };
	// the instance records of this moment, for rt_reproject_motion: inst[] as the device holds it, and the host mirror it equals
	const size_t nInst = c->S.useTLAS ? (size_t)c->nInstances : 0;
	prof_begin(c, K_QUERY); // (with rt_set_profiling on: the copies are timed as one entry of rt_profile.query, k_reproject as another)
	hipError_t copied = hipSuccess;
	for (const auto& k : copies)
		if (copied == hipSuccess) copied = hipMemcpyAsync(k.dst, k.src, n * k.elem, hipMemcpyDeviceToDevice, c->stream);
	if (copied == hipSuccess && nInst) copied = hipMemcpyAsync(H.xf, c->S.inst, nInst * sizeof(DInstance), hipMemcpyDeviceToDevice, c->stream);
	prof_end(c);
	HIPCHK(c, copied);
	c->histXfHost.assign(c->instances.inst.begin(), c->instances.inst.begin() + nInst);
	H.cam = c->camRec;
	H.gen = c->geomGen, H.shapeGen = c->shapeGen, H.topoGen = c->topoGen;
	return RT_OK;
}

// rt_reproject, rt_reproject_motion and rt_reproject_deform: the checks, the argument record, the launch and the read-back they share.
// 'mode' (RP_CAMERA, RP_MOTION, RP_DEFORM) chooses the history's level of validity and the kernel.
static int reproject_run(rt_ctx* c, const char* fn, int mode, const rt_reproject_params* params, int* n_carried_out)
{
	const bool motion = mode >= RP_MOTION;
	const rt_reproject_params P = params ? *params : rt_reproject_params RT_REPROJECT_DEFAULTS;
	if (!(P.normal_tolerance >= 0.0f) || !(P.plane_tolerance >= 0.0f)) return fail(c, RT_E_ARG, "%s: the tolerances must be >= 0 (neither NaN)", fn);
	if (P.max_history < 0) return fail(c, RT_E_ARG, "%s: max_history %d (>= 0)", fn, P.max_history);
	if (!c) return fail(c, RT_E_ARG, "%s: null context", fn);
	if (!c->stats.count) return fail(c, RT_E_STATE, "%s: statistics are off (rt_stats_enable)", fn);
	if (!(mode == RP_DEFORM ? history_valid_deform(c) : motion ? history_valid_motion(c) : history_valid(c)))
		return fail(c, RT_E_STATE, "%s: no valid history (rt_history_capture; the scene, the time or the statistics changed since)", fn);
	if (!aovs_current(c)) return fail(c, RT_E_STATE, "%s: the G-buffer is %s (rt_render_aovs)", fn, c->aovNrm ? "stale" : "missing");
	if (c->camRec.fisheye) return fail(c, RT_E_UNSUPPORTED, "%s: the camera is a fisheye (the projection is the pinhole's)", fn);
	HIPCHK(c, hipSetDevice(c->device));
	drop_plan(c); // every pixel's count is rewritten
	const rt_ctx::History& H = c->hist;
	ReprojectDeformArgs D;
	ReprojectMotionArgs& M = D;
	ReprojectArgs& R = D;
	R.nrm = c->aovNrm, R.pos = c->aovPos, R.alb = c->aovAlb;
	R.hNrm = H.nrm, R.hPos = H.pos, R.hAlb = H.alb, R.hAcc = H.acc, R.hSt = H.stats;
	R.acc = c->accum, R.St = c->stats;
	R.mats = c->S.mats, R.nMats = c->S.nMats;
	memcpy(R.cam, H.cam.cam_pos, 12), memcpy(R.TL, H.cam.top_left, 12), memcpy(R.TR, H.cam.top_right, 12), memcpy(R.BL, H.cam.bottom_left, 12);
	R.width = c->width, R.height = c->height;
	R.normalTol2 = P.normal_tolerance * P.normal_tolerance, R.planeTol = P.plane_tolerance;
	R.maxHistory = P.max_history, R.carryViewDependent = P.carry_view_dependent != 0;
	R.nCarried = H.nCarried;
	if (motion) {
		M.inst = c->aovInst, M.hInst = H.inst, M.cur = c->S.inst, M.hXf = H.xf;
		// moved_k: any of the 24 words differs bitwise (the mirrors hold what the device holds: rt_upload_scene and rt_set_instances write both)
		memset(M.moved, 0, sizeof(M.moved));
		const std::vector<DInstance>& now = c->instances.inst;
		for (size_t k = 0; k < c->histXfHost.size() && k < now.size(); k++)
			if (memcmp(now[k].invT, c->histXfHost[k].invT, 48) != 0 || memcmp(now[k].T, c->histXfHost[k].T, 48) != 0) M.moved[k >> 5] |= 1u << (k & 31);
	}
	if (mode == RP_DEFORM) {
		D.prim = c->aovPrim, D.prims = c->S.prims, D.keptDelta = H.keptDelta;
		D.useTLAS = c->S.useTLAS != 0, D.blasOf = c->instances.blasOfDev;
		D.blas0Slots = c->blasKeep.empty() ? 0 : (int)c->blasKeep[0].slotCount;
	}
	HIPCHK(c, hipMemsetAsync(H.nCarried, 0, sizeof(int), c->stream));
	const dim3 grid((c->width + RT_DENOISE_TX - 1) / RT_DENOISE_TX, (c->height + RT_DENOISE_TY - 1) / RT_DENOISE_TY), block(RT_DENOISE_TX, RT_DENOISE_TY);
	prof_begin(c, K_QUERY);
	if (mode == RP_DEFORM) hipLaunchKernelGGL(k_reproject_deform, grid, block, 0, c->stream, D);
	else if (motion) hipLaunchKernelGGL(k_reproject_motion, grid, block, 0, c->stream, M);
	else hipLaunchKernelGGL(k_reproject, grid, block, 0, c->stream, R);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	if (n_carried_out) {
		// the only synchronisation of the call (pinned; the round pipelines use words 0..4, rt_select_active word 8)
		HIPCHK(c, hipMemcpyAsync(c->hostCounts + 9, H.nCarried, sizeof(int), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		*n_carried_out = c->hostCounts[9];
	}
	return RT_OK;
}

int rt_reproject(rt_ctx* c, const rt_reproject_params* params, int* n_carried_out) { return reproject_run(c, "rt_reproject", RP_CAMERA, params, n_carried_out); }
int rt_reproject_motion(rt_ctx* c, const rt_reproject_params* params, int* n_carried_out) { return reproject_run(c, "rt_reproject_motion", RP_MOTION, params, n_carried_out); }
int rt_reproject_deform(rt_ctx* c, const rt_reproject_params* params, int* n_carried_out) { return reproject_run(c, "rt_reproject_deform", RP_DEFORM, params, n_carried_out); }
