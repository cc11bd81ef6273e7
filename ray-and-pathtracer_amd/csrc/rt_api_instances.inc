// rt_set_instances: bvhInstance::SetTransform + tlas::build into the loaded scene, without a re-upload; rt_set_instance_list: the whole list
// replaced, its length and the instances' BLASes included; rt_download_tlas; rt_scene_array.
// The host side of rt_instances.h, which states why the result is byte-equal to a fresh rt_upload_scene of the updated description.
// Included by rt_api.hip (one translation unit).
static_assert(sizeof(InstReach) == sizeof(Reach) && sizeof(Reach) == 64, "the reach record the host uploads is pack_reach's");

// The tail rt_set_instances, rt_set_instance_list and rt_set_triangles (rt_api_triangles.inc) share: from every instance's new box in I.boundsNew to the TLAS in the
// traversal layout.  tlas::build into scratch and the call's one synchronisation (did it succeed?); then, and only then, the commit: the
// caller's own (commit: its mirrors and copies), the reach records, k_pack_tlas, the scalars.  A build that fails runs undo (whatever the
// caller has queued into the scene so far is taken back), closes the profile entry and returns RT_E_UNSUPPORTED.
//   n       the number of instances after the change (rt_set_instance_list: another than c->nInstances, which its commit sets)
//   reach   instance_reach of every instance after the change; swapped into the context on success
static int tlas_tail(rt_ctx* c, const char* who, uint32_t n, std::vector<Reach>& reach, const std::function<int()>& commit, const std::function<int()>& undo)
{
	rt_ctx::InstanceState& I = c->instances;
	const double originMax = reach_origin_max(reach.data(), reach.size());
	// the scalars that follow from n alone (rt_instances.h, fact 1)
	SceneLayout L;
	L.tlasPairs = n >= 2 ? (int)n : 0, L.nInst = (int)n;
	L.tlasBase = n >= 2 ? c->blasPairs : 0, L.root = n >= 2 ? c->blasPairs : (RT_INST_BIT | 0u);
	L.reachOriginMax = (float)originMax;
	LayoutKnobs knobs;
	knobs.tlasLds = c->knobs.tlasLds;
	split_lds(L, knobs);
	// ---- the TLAS over the new boxes, into scratch ----
	HIPCHK(c, hipMemsetAsync(I.nodesNew, 0, ((size_t)2 * n + 1) * sizeof(TlasNodeDev), c->stream));
	hipLaunchKernelGGL(k_build_tlas, dim3(1), dim3(64), 0, c->stream, I.boundsNew, (int)n, I.nodesNew, I.used);
	// the call's one synchronisation: did the build succeed?
	HIPCHK(c, hipMemcpyAsync(c->hostCounts + 8, I.used, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipGetLastError());
	if (c->hostCounts[8] != (int)(2 * n)) {
		const int rcUndo = undo();
		prof_end(c);
		if (rcUndo != RT_OK) return rcUndo;
		return fail(c, RT_E_UNSUPPORTED, "%s: no finite union area left (degenerate instance bounds); the scene is unchanged", who);
	}
	// ---- commit (whatever an earlier call queued from the mirrors has been consumed: the stream was just drained) ----
	{ const int rc = commit(); if (rc != RT_OK) return rc; }
	I.reach.swap(reach);
	HIPCHK(c, hipMemcpyAsync(I.reachIn, I.reach.data(), (size_t)n * sizeof(Reach), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_pack_tlas, dim3(1), dim3(RT_TLAS_MAX), 0, c->stream, I.nodesNew, (int)n, I.reachIn, originMax, L.tlasBase,
	                   c->pairsMut + 4 * (size_t)L.tlasBase, I.reachMut, I.tlasKeep, I.boundsNew, I.bounds);
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	I.built = true;
	c->S.rootLink = L.root, c->S.tlasBase = L.tlasBase, c->S.tlasPairs = L.tlasPairs, c->S.nInst = L.nInst, c->S.reachOriginMax = L.reachOriginMax;
	c->S.tlasLds = L.tlasLds, c->S.stackRows = L.stackRows;
	int32_t* s = c->layoutScalars; // rootLink, tlasBase, tlasPairs, nInst, reachOriginMax, tlasLds, stackRows: the first seven words
	s[0] = (int32_t)L.root, s[1] = (int32_t)L.tlasBase, s[2] = L.tlasPairs, s[3] = L.nInst, memcpy(&s[4], &L.reachOriginMax, 4), s[5] = L.tlasLds, s[6] = L.stackRows;
	return RT_OK;
}

// What both calls refuse of one instance record (in.blas is a BLAS of the scene): a non-finite matrix entry; box6, the caller's box, beyond
// 1e30; without one, a transform that could take the BLAS's local box there.  'at': the instance's index, for the message.
static int check_instance(rt_ctx* c, const char* who, uint32_t at, const rt_instance& in, const float* box6)
{
	for (int j = 0; j < 16; j++)
		if (!std::isfinite(in.transform[j]) || !std::isfinite(in.inv_transform[j])) return fail(c, RT_E_ARG, "%s: instance %u has a non-finite matrix entry", who, at);
	if (box6) {
		for (int j = 0; j < 6; j++)
			if (!(std::fabs(box6[j]) <= 1e30f)) return fail(c, RT_E_ARG, "%s: instance %u has a non-finite bound or one beyond 1e30", who, at);
		return RT_OK;
	}
	// the box the device will compute stays within the +-1e30 of every stored box: |row . corner| <= sum |c_j| max|corner_j| + |c_3|
	const float* bb = &c->instances.blasBox6[(size_t)6 * in.blas];
	for (int r = 0; r < 3; r++) {
		double reachMax = std::fabs((double)in.transform[4 * r + 3]);
		for (int j = 0; j < 3; j++) reachMax += std::fabs((double)in.transform[4 * r + j]) * std::max(std::fabs((double)bb[j]), std::fabs((double)bb[3 + j]));
		if (!(reachMax <= 1e29) || !(std::fabs(bb[r]) <= 1e30f) || !(std::fabs(bb[3 + r]) <= 1e30f))
			return fail(c, RT_E_ARG, "%s: the transform of instance %u takes its box beyond 1e30", who, at);
	}
	return RT_OK;
}

int rt_set_instances(rt_ctx* c, uint32_t first, uint32_t count, const rt_instance* instances, const float* bounds6)
{
	if (!c || !instances) return fail(c, RT_E_ARG, "rt_set_instances: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_instances: no scene uploaded");
	if (!c->S.useTLAS) return fail(c, RT_E_UNSUPPORTED, "rt_set_instances: the scene has no TLAS");
	rt_ctx::InstanceState& I = c->instances;
	const uint32_t n = (uint32_t)c->nInstances;
	// ---- everything that can be refused is refused here, before anything is queued ----
	if (count == 0 || first >= n || count > n - first) return fail(c, RT_E_ARG, "rt_set_instances: instances [%u, %u + %u) of %u", first, first, count, n);
	for (uint32_t k = 0; k < count; k++) {
		const rt_instance& in = instances[k];
		if (in.blas != I.blasOf[first + k]) return fail(c, RT_E_ARG, "rt_set_instances: instance %u is an instance of blas %d, not %d (an instance cannot be re-pointed)", first + k, I.blasOf[first + k], in.blas);
		const int rc = check_instance(c, "rt_set_instances", first + k, in, bounds6 ? bounds6 + 6 * (size_t)k : nullptr);
		if (rc != RT_OK) return rc;
	}
	for (uint32_t i = 0; i < n; i++)
		if (!I.boundsKnown[i] && (i < first || i >= first + count)) return fail(c, RT_E_ARG, "rt_set_instances: instance %u has no leaf in the uploaded TLAS and no box yet; include it in the update", i);
	// ---- the host's part: the changed instances' records and reach (rt_layout.h instance_reach, f64), originMax over all of them ----
	std::vector<DInstance> inst(I.inst.begin() + first, I.inst.begin() + first + count);
	std::vector<Reach> reach = I.reach;
	std::vector<float> xform((size_t)12 * count);
	for (uint32_t k = 0; k < count; k++) {
		memcpy(inst[k].invT, instances[k].inv_transform, 48), memcpy(inst[k].T, instances[k].transform, 48);
		memcpy(&xform[(size_t)12 * k], instances[k].transform, 48);
		reach[first + k] = instance_reach(I.objBox[instances[k].blas], instances[k].inv_transform);
	}
	HIPCHK(c, hipSetDevice(c->device));
	prof_begin(c, K_QUERY);
	// ---- the new boxes, into scratch ----
	HIPCHK(c, hipMemcpyAsync(I.boundsNew, I.bounds, (size_t)24 * n, hipMemcpyDeviceToDevice, c->stream));
	if (bounds6) HIPCHK(c, hipMemcpyAsync(I.boundsNew + (size_t)6 * first, bounds6, (size_t)24 * count, hipMemcpyHostToDevice, c->stream));
	else {
		HIPCHK(c, hipMemcpyAsync(I.xform, xform.data(), xform.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_instance_bounds, dim3(1), dim3(RT_TLAS_MAX), 0, c->stream, I.xform, I.blasOfDev + first, I.blasBox, (int)count, I.boundsNew + (size_t)6 * first, (const int*)nullptr);
	}
	const int rc = tlas_tail(c, "rt_set_instances", n, reach,
		[&]() -> int {
			std::copy(inst.begin(), inst.end(), I.inst.begin() + first);
			for (uint32_t k = 0; k < count; k++) I.boundsKnown[first + k] = 1;
			HIPCHK(c, hipMemcpyAsync(I.instMut + first, &I.inst[first], (size_t)count * sizeof(DInstance), hipMemcpyHostToDevice, c->stream));
			return RT_OK;
		},
		[]() -> int { return RT_OK; }); // nothing of the scene has been touched yet
	if (rc != RT_OK) return rc;
	c->sceneGen++; // everything rt_set_time invalidates: the G-buffer and the primary-hit table ...
	c->geomGen++;  // ... and a captured history, for rt_reproject; rt_reproject_motion follows the move (shapeGen stays)
	return RT_OK;
}

// The whole list replaced: n records of pack_instances' (the roots per BLAS as the upload kept them), n boxes, tlas::build over them.  The
// device work is rt_set_instances' over all n instances; what differs is on the host: the count and everything that follows from it
// (tlas_tail's scalars), the instances' BLASes, and an upload's invalidation, since an instance index names another object afterwards.
int rt_set_instance_list(rt_ctx* c, uint32_t n, const rt_instance* instances, const float* bounds6)
{
	if (!c || !instances) return fail(c, RT_E_ARG, "rt_set_instance_list: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_instance_list: no scene uploaded");
	if (!c->S.useTLAS) return fail(c, RT_E_UNSUPPORTED, "rt_set_instance_list: the scene has no TLAS");
	rt_ctx::InstanceState& I = c->instances;
	const size_t nBlas = I.objBox.size();
	// ---- everything that can be refused is refused here, before anything is queued ----
	if (n < 1 || n > RT_TLAS_MAX) return fail(c, RT_E_ARG, "rt_set_instance_list: %u instances (a TLAS holds 1..%d)", n, RT_TLAS_MAX);
	for (uint32_t k = 0; k < n; k++) {
		const rt_instance& in = instances[k];
		if (in.blas < 0 || (size_t)in.blas >= nBlas) return fail(c, RT_E_ARG, "rt_set_instance_list: instance %u names blas %d of %zu (a new BLAS needs rt_upload_scene)", k, in.blas, nBlas);
		const int rc = check_instance(c, "rt_set_instance_list", k, in, bounds6 ? bounds6 + 6 * (size_t)k : nullptr);
		if (rc != RT_OK) return rc;
	}
	// ---- the host's part: pack_instances' records, the reach of every instance (rt_layout.h instance_reach, f64) ----
	std::vector<DInstance> inst(n);
	std::vector<int> blasOf(n);
	std::vector<Reach> reach(n);
	std::vector<float> xform((size_t)12 * n);
	for (uint32_t k = 0; k < n; k++) {
		const rt_instance& in = instances[k];
		memset(&inst[k], 0, sizeof(DInstance));
		memcpy(inst[k].invT, in.inv_transform, 48), memcpy(inst[k].T, in.transform, 48);
		inst[k].rootLink = c->blasRoot[(size_t)in.blas], inst[k].rootWide = I.rootWide[(size_t)in.blas];
		inst[k].rootWide8 = I.wide8OK ? I.rootWide8[(size_t)in.blas] : RT_EMPTY;
		blasOf[k] = in.blas;
		memcpy(&xform[(size_t)12 * k], in.transform, 48);
		reach[k] = instance_reach(I.objBox[(size_t)in.blas], in.inv_transform);
	}
	HIPCHK(c, hipSetDevice(c->device));
	prof_begin(c, K_QUERY);
	// ---- the new boxes, into scratch (I.which: the new list's BLASes, where k_instance_bounds reads them before the commit) ----
	if (bounds6) HIPCHK(c, hipMemcpyAsync(I.boundsNew, bounds6, (size_t)24 * n, hipMemcpyHostToDevice, c->stream));
	else {
		HIPCHK(c, hipMemcpyAsync(I.xform, xform.data(), xform.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipMemcpyAsync(I.which, blasOf.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
		hipLaunchKernelGGL(k_instance_bounds, dim3(1), dim3(RT_TLAS_MAX), 0, c->stream, I.xform, (const int*)I.which, I.blasBox, (int)n, I.boundsNew, (const int*)nullptr);
	}
	const int rc = tlas_tail(c, "rt_set_instance_list", n, reach,
		[&]() -> int {
			I.inst.swap(inst), I.blasOf.swap(blasOf);
			I.boundsKnown.assign(n, 1);
			c->nInstances = (int)n;
			HIPCHK(c, hipMemcpyAsync(I.instMut, I.inst.data(), (size_t)n * sizeof(DInstance), hipMemcpyHostToDevice, c->stream));
			HIPCHK(c, hipMemcpyAsync(I.blasOfDev, I.blasOf.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
			return RT_OK;
		},
		[]() -> int { return RT_OK; }); // nothing of the scene has been touched yet
	if (rc != RT_OK) return rc;
	c->sceneGen++;                            // an upload's invalidation: the G-buffer (its instance indices renumber) and the primary-hit table ...
	c->geomGen++, c->shapeGen++, c->topoGen++; // ... and a captured history at every level: an index no longer names the same object, nothing is carried
	return RT_OK;
}

int rt_download_tlas(rt_ctx* c, rt_tlas_node* nodes_out, uint32_t* nodes_used_out)
{
	if (!c || !nodes_out || !nodes_used_out) return fail(c, RT_E_ARG, "rt_download_tlas: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_download_tlas: no scene uploaded");
	if (!c->S.useTLAS) return fail(c, RT_E_UNSUPPORTED, "rt_download_tlas: the scene has no TLAS");
	const rt_ctx::InstanceState& I = c->instances;
	const size_t n = (size_t)c->nInstances;
	static_assert(sizeof(TlasNodeDev) == sizeof(rt_tlas_node), "TLAS node layout");
	if (!I.built) { // the uploaded TLAS, as long as the caller's 2 n + 1 nodes hold it
		if (I.uploaded.size() > 2 * n + 1) return fail(c, RT_E_UNSUPPORTED, "rt_download_tlas: the uploaded TLAS has %zu nodes, more than the 2 n + 1 = %zu of a tlas::build", I.uploaded.size(), 2 * n + 1);
		memcpy(nodes_out, I.uploaded.data(), I.uploaded.size() * sizeof(rt_tlas_node));
		*nodes_used_out = (uint32_t)I.uploaded.size();
		return RT_OK;
	}
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(nodes_out, I.tlasKeep, (2 * n + 1) * sizeof(rt_tlas_node), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	*nodes_used_out = (uint32_t)(2 * n);
	return RT_OK;
}

int rt_scene_array(rt_ctx* c, int which, void* out, size_t cap_bytes, size_t* bytes_out)
{
	if (!c || !bytes_out) return fail(c, RT_E_ARG, "rt_scene_array: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_scene_array: no scene uploaded");
	const void* src = nullptr;
	size_t need = 0;
	bool device = true;
	switch (which) {
	case RT_LAYOUT_PAIRS: src = c->pairsMut, need = ((size_t)c->blasPairs + (size_t)c->S.tlasPairs) * 64; break;
	case RT_LAYOUT_REACH: src = c->instances.reachMut, need = c->S.useTLAS ? ((size_t)c->S.tlasPairs * 12 + 16) * sizeof(float) : 0; break;
	case RT_LAYOUT_INST: src = c->instances.instMut, need = c->S.useTLAS ? (size_t)c->nInstances * sizeof(DInstance) : 0; break;
	case RT_LAYOUT_SCALARS: src = c->layoutScalars, need = sizeof(c->layoutScalars), device = false; break;
	// what rt_set_lights / rt_set_materials (rt_api_materials.inc) rewrite: the two tables (one zeroed record for none) and the brute-force records with their 16 spare words
	case RT_LAYOUT_LIGHTS: src = c->S.lights, need = (size_t)(c->S.nLights > 0 ? c->S.nLights : 1) * sizeof(DLight); break;
	case RT_LAYOUT_MATS: src = c->S.mats, need = (size_t)c->S.nMats * sizeof(DMaterial); break;
	case RT_LAYOUT_BRUTE: src = c->S.brute, need = c->S.useTLAS ? ((size_t)(c->S.nBruteSph + c->S.nBrutePla) * 16 + 16) * sizeof(float) : 0; break;
	default: return fail(c, RT_E_UNSUPPORTED, "rt_scene_array: array %d (PAIRS, REACH, BRUTE, INST, LIGHTS, MATS and SCALARS are kept where they can be read back)", which);
	}
	*bytes_out = need;
	if (!out) return RT_OK; // the size alone
	if (cap_bytes < need) return fail(c, RT_E_ARG, "rt_scene_array: array %d needs %zu bytes, the buffer holds %zu", which, need, cap_bytes);
	if (need == 0) return RT_OK;
	if (!device) { memcpy(out, src, need); return RT_OK; }
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(out, src, need, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return RT_OK;
}
