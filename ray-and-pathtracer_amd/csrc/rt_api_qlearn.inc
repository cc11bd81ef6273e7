// The Q-learning sampler's host side (rt_qlearn_*; kernels and the scheme in rt_qlearn.h).  Included by rt_api.hip.
int rt_qlearn_enable(rt_ctx* c, const rt_qlearn_params* p)
{
	if (!c) return RT_E_ARG;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	free_pool(c->qAllocs);
	memset(&c->Qt, 0, sizeof(c->Qt));
	if (!p) return RT_OK;
	if (p->grid < 1 || p->grid > 64) return fail(c, RT_E_ARG, "rt_qlearn_enable: grid %d (1..64)", p->grid);
	for (int a = 0; a < 3; a++)
		if (!(p->hi[a] > p->lo[a]) || !std::isfinite(p->lo[a]) || !std::isfinite(p->hi[a])) return fail(c, RT_E_ARG, "rt_qlearn_enable: empty or non-finite box on axis %d", a);
	if (!(p->alpha > 0 && p->alpha <= 1) || !(p->epsilon >= 0 && p->epsilon <= 1) || !(p->q_init > 0) || !std::isfinite(p->q_init)) return fail(c, RT_E_ARG, "rt_qlearn_enable: alpha in (0, 1], epsilon in [0, 1], finite q_init > 0");
	if (c->pathUnsupported) return fail(c, RT_E_UNSUPPORTED, "rt_qlearn_enable: this scene's path mode runs the general kernel (%s)", c->pathUnsupportedWhy.c_str());
	QTable Q;
	memset(&Q, 0, sizeof(Q));
	const size_t cells = (size_t)p->grid * p->grid * p->grid;
	float4* centre = nullptr;
	float* wgt = nullptr;
	HIPCHK(c, dalloc(c->qAllocs, &Q.q, cells * RT_Q_ROW));
	HIPCHK(c, dalloc(c->qAllocs, &Q.v, cells * RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &Q.sum, cells * RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &Q.cnt, cells * RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &Q.acc, cells * RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &centre, (size_t)RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &wgt, (size_t)RT_Q_PATCHES * RT_Q_PATCHES));
	HIPCHK(c, dalloc(c->qAllocs, &Q.ovf, (size_t)4)); // the sampler's own overflow word (flags[2] belongs to the wide occlusion walk's leftover count)
	HIPCHK(c, hipMemsetAsync(Q.ovf, 0, 4 * sizeof(int), c->stream));
	Q.centre = centre, Q.wgt = wgt, Q.grid = p->grid, Q.on = 1;
	for (int a = 0; a < 3; a++) Q.lo[a] = p->lo[a], Q.inv[a] = (float)p->grid / (p->hi[a] - p->lo[a]);
	Q.eps = p->epsilon, Q.alpha = p->alpha, Q.qMin = 1e-4f, Q.learnMask = p->learn_mask;
	hipLaunchKernelGGL(k_q_weights, dim3(RT_Q_PATCHES), dim3(RT_Q_PATCHES), 0, c->stream, centre, wgt);
	hipLaunchKernelGGL(k_q_init, dim3(((int)cells + 63) / 64), dim3(64), 0, c->stream, Q, p->q_init);
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->Qt = Q;
	return RT_OK;
}
int rt_qlearn_apply(rt_ctx* c)
{
	if (!c || !c->Qt.on) return fail(c, RT_E_STATE, "rt_qlearn_apply: the sampler is off");
	HIPCHK(c, hipSetDevice(c->device));
	// stream-ordered, no host wait: the rewards of every batch were folded into the wide sums at the batch's end (run_rounds_stream),
	// where a count field past its limit was reported by the render call itself
	const int cells = c->Qt.grid * c->Qt.grid * c->Qt.grid;
	hipLaunchKernelGGL(k_q_apply, dim3((cells + 63) / 64), dim3(64), 0, c->stream, c->Qt); // a 64 x 64 product per cell: one wave per block spreads the cells over the CUs
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}
int rt_qlearn_get_sums(rt_ctx* c, int64_t* sums, uint32_t* counts)
{
	if (!c || !c->Qt.on || !sums || !counts) return fail(c, RT_E_STATE, "rt_qlearn_get_sums: the sampler is off, or a null argument");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->Qt.grid * c->Qt.grid * c->Qt.grid * RT_Q_PATCHES;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(sums, c->Qt.sum, n * 8, hipMemcpyDeviceToHost));
	HIPCHK(c, hipMemcpy(counts, c->Qt.cnt, n * 4, hipMemcpyDeviceToHost));
	return RT_OK;
}
int rt_qlearn_set_sums(rt_ctx* c, const int64_t* sums, const uint32_t* counts)
{
	if (!c || !c->Qt.on || !sums || !counts) return fail(c, RT_E_STATE, "rt_qlearn_set_sums: the sampler is off, or a null argument");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->Qt.grid * c->Qt.grid * c->Qt.grid * RT_Q_PATCHES;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemset(c->Qt.acc, 0, n * 8)); // the caller's sums replace everything gathered so far
	HIPCHK(c, hipMemcpy(c->Qt.sum, sums, n * 8, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->Qt.cnt, counts, n * 4, hipMemcpyHostToDevice));
	return RT_OK;
}
// The pending reward sums in the CALLER's device memory (several processes: the sums are all-reduced in place between the ranks,
// RCCL on device pointers, instead of four host copies per exchange -- VERDICT r5 item 5).  What was pending moves over.
int rt_qlearn_bind_sums(rt_ctx* c, int64_t* dev_sums, uint32_t* dev_counts)
{
	if (!c || !c->Qt.on || !dev_sums || !dev_counts) return fail(c, RT_E_STATE, "rt_qlearn_bind_sums: the sampler is off, or a null argument");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t n = (size_t)c->Qt.grid * c->Qt.grid * c->Qt.grid * RT_Q_PATCHES;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(dev_sums, c->Qt.sum, n * 8, hipMemcpyDeviceToDevice));
	HIPCHK(c, hipMemcpy(dev_counts, c->Qt.cnt, n * 4, hipMemcpyDeviceToDevice));
	c->Qt.sum = (long long*)dev_sums, c->Qt.cnt = dev_counts; // (the library's own arrays stay in qAllocs until the sampler is switched off)
	return RT_OK;
}
int rt_qlearn_get_table(rt_ctx* c, float* q_out)
{
	if (!c || !c->Qt.on || !q_out) return fail(c, RT_E_STATE, "rt_qlearn_get_table: the sampler is off, or a null argument");
	HIPCHK(c, hipSetDevice(c->device));
	const size_t cells = (size_t)c->Qt.grid * c->Qt.grid * c->Qt.grid;
	std::vector<float> rows(cells * RT_Q_ROW);
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(rows.data(), c->Qt.q, rows.size() * 4, hipMemcpyDeviceToHost));
	for (size_t v = 0; v < cells; v++) memcpy(q_out + v * RT_Q_PATCHES, &rows[v * RT_Q_ROW + 8], RT_Q_PATCHES * 4);
	return RT_OK;
}

