// rt_set_triangles: the triangles of one BLAS replaced and its tree refitted in the loaded scene, without a re-upload; rt_blas_array.
// The call is a head (the host's loop over the records) and two parts it shares with rt_set_vertices (rt_api_vertices.inc), whose head
// runs on the device: triangles_verdict (the checks and host arithmetic that follow from the boxes) and triangles_tail (what is queued).
// The host side of rt_triangles.h, which states why the result is byte-equal to a fresh rt_upload_scene of the updated description.
// Atomicity: the two record ranges of the BLAS (and its local box) are copied aside on the device before they are rewritten, and copied
// back if the TLAS build over the new boxes fails; a scene without a TLAS has nothing that can fail once the host's checks have passed.
// Included by rt_api.hip (one translation unit).

// What the host decides about a deformation once the new triangles' boxes are known; rt_set_triangles and rt_set_vertices
// (rt_api_vertices.inc) share it.  lo / hi: the local box of ALL new triangles, magnitudes only; objectBox(): blas_object_box of them, asked
// for only under a TLAS and only once the instances have passed.  Nothing is queued here.
struct TriVerdict {
	std::vector<int> which; // the instances of this BLAS
	std::vector<float> xform;
	std::vector<Reach> reach;
	ObjectBox objBox{};
};
static int triangles_verdict(rt_ctx* c, const char* who, uint32_t blas, const float* lo, const float* hi, const std::function<ObjectBox()>& objectBox, TriVerdict& V)
{
	if (!c->S.useTLAS) return RT_OK;
	rt_ctx::InstanceState& I = c->instances;
	const uint32_t n = (uint32_t)c->nInstances;
	for (uint32_t i = 0; i < n; i++) {
		if ((uint32_t)I.blasOf[i] != blas) {
			if (!I.boundsKnown[i]) return fail(c, RT_E_ARG, "%s: instance %u has no leaf in the uploaded TLAS and no box yet; set it with rt_set_instances first", who, i);
			continue;
		}
		// the box the device will compute stays within the +-1e30 of every stored box (rt_set_instances' bounds6 == NULL rule)
		const float* T = I.inst[i].T;
		for (int r = 0; r < 3; r++) {
			double reachMax = std::fabs((double)T[4 * r + 3]);
			for (int j = 0; j < 3; j++) reachMax += std::fabs((double)T[4 * r + j]) * std::max(std::fabs((double)lo[j]), std::fabs((double)hi[j]));
			if (!(reachMax <= 1e29)) return fail(c, RT_E_ARG, "%s: the transform of instance %u takes the new box beyond 1e30", who, i);
		}
		V.which.push_back((int)i);
	}
	// ---- the host's part: the BLAS's object box (blas_object_box's rule), the reach of its instances, originMax over all of them ----
	V.objBox = objectBox();
	V.reach = I.reach;
	V.xform.resize((size_t)12 * V.which.size());
	for (size_t k = 0; k < V.which.size(); k++) {
		const DInstance& in = I.inst[(size_t)V.which[k]];
		memcpy(&V.xform[12 * k], in.T, 48);
		V.reach[(size_t)V.which[k]] = instance_reach(V.objBox, in.invT);
	}
	return RT_OK;
}

// The tail both calls share, after every host check has passed: the scratch growth, the undo copies, history_keep_blas, the records
// (k_set_triangles over the staging array), the refit, the 4-wide boxes, the TLAS half, the generation counters.
//   tris      host records to copy into the staging array, or NULL: the array holds them already (k_assemble_triangles, queued before)
//   profOpen  the caller has opened the call's profile entry already (and closes or cancels it itself if it returns before the tail)
static int triangles_tail(rt_ctx* c, const char* who, uint32_t blas, uint32_t n_tri, const float* lo, const float* hi, TriVerdict& V, const rt_triangle* tris, bool profOpen)
{
	const rt_ctx::BlasKeep& K = c->blasKeep[blas];
	const bool useTLAS = c->S.useTLAS != 0;
	rt_ctx::InstanceState& I = c->instances;
	const uint32_t n = useTLAS ? (uint32_t)c->nInstances : 0;
	const std::vector<int>& which = V.which;
	HIPCHK(c, hipSetDevice(c->device));
	// scratch that only the first call (or a larger BLAS) allocates
	{ const int rc = grow_scene_array(c, &c->triStage, c->triStageCap, (size_t)n_tri * (sizeof(rt_triangle) / sizeof(float))); if (rc != RT_OK) return rc; }
	if (useTLAS) {
		int rc = grow_scene_array(c, &c->undoPairs, c->undoPairCap, (size_t)K.pairCount * 4);
		if (rc == RT_OK) rc = grow_scene_array(c, &c->undoPrims, c->undoPrimCap, (size_t)K.slotCount * 4);
		if (rc != RT_OK) return rc;
	}
	float4* const pairsAt = c->pairsMut + 4 * (size_t)K.pairFirst;
	float4* const primsAt = c->primsMut + 4 * (size_t)K.slotFirst;
	const size_t pairBytes = (size_t)K.pairCount * 64, primBytes = (size_t)K.slotCount * 64;
	float* const boxAt = useTLAS ? I.blasBox + (size_t)6 * blas : nullptr;
	{ const int rc = history_keep_blas(c, blas); if (rc != RT_OK) return rc; } // a live history keeps the capture's records (rt_reproject_deform)

	if (!profOpen) prof_begin(c, K_QUERY);
	if (useTLAS) { // the undo copies
		HIPCHK(c, hipMemcpyAsync(c->undoPairs, pairsAt, pairBytes, hipMemcpyDeviceToDevice, c->stream));
		HIPCHK(c, hipMemcpyAsync(c->undoPrims, primsAt, primBytes, hipMemcpyDeviceToDevice, c->stream));
		HIPCHK(c, hipMemcpyAsync(I.boxUndo, boxAt, 24, hipMemcpyDeviceToDevice, c->stream));
	}
	// ---- the records and the tree ----
	static_assert(sizeof(rt_triangle) == 56, "k_set_triangles reads 14-word records");
	if (tris) HIPCHK(c, hipMemcpyAsync(c->triStage, tris, (size_t)n_tri * sizeof(rt_triangle), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_set_triangles, dim3((n_tri + 255) / 256), dim3(256), 0, c->stream, (const float2*)c->triStage, (int)n_tri, c->slotOf + K.slotFirst, c->primsMut,
	                   c->S.mats, c->S.nMats);
	refit_launch(c, c->refitOrderAll, c->refitLevelAll + K.levelFirst, K.level.data(), (int)K.level.size() - 1);
	// the 4-wide nodes' child boxes follow the pair records (after the build's verdict under a TLAS: nothing reads them before)
	auto wide_sync = [&]() { if (c->S.wide && c->wideNodes > 0) hipLaunchKernelGGL(k_wide_sync, dim3((c->wideNodes * 4 + 255) / 256), dim3(256), 0, c->stream, c->wideMut, c->pairsMut, c->wideNodes); };
	if (!useTLAS) {
		wide_sync();
		// rt_set_time deforms from the new vertices: the kept originals are a fresh upload's
		if (c->primsOrig && blas == 0) HIPCHK(c, hipMemcpyAsync(c->primsOrig, primsAt, primBytes, hipMemcpyDeviceToDevice, c->stream));
		prof_end(c);
		HIPCHK(c, hipGetLastError());
	} else {
		// ---- the TLAS half: the refitted root's box, the boxes of this BLAS's instances, the shared tail ----
		hipLaunchKernelGGL(k_blas_root_box, dim3(1), dim3(64), 0, c->stream, c->pairsMut, c->primsMut, c->blasRoot[blas], boxAt);
		HIPCHK(c, hipMemcpyAsync(I.boundsNew, I.bounds, (size_t)24 * n, hipMemcpyDeviceToDevice, c->stream));
		if (!which.empty()) {
			HIPCHK(c, hipMemcpyAsync(I.xform, V.xform.data(), V.xform.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
			HIPCHK(c, hipMemcpyAsync(I.which, which.data(), which.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
			hipLaunchKernelGGL(k_instance_bounds, dim3(1), dim3(RT_TLAS_MAX), 0, c->stream, I.xform, I.blasOfDev, I.blasBox, (int)which.size(), I.boundsNew, (const int*)I.which);
		}
		const int rc = tlas_tail(c, who, n, V.reach,
			[&]() -> int {
				for (int i : which) I.boundsKnown[(size_t)i] = 1;
				wide_sync();
				return RT_OK;
			},
			[&]() -> int { // the BLAS as it was
				HIPCHK(c, hipMemcpyAsync(pairsAt, c->undoPairs, pairBytes, hipMemcpyDeviceToDevice, c->stream));
				HIPCHK(c, hipMemcpyAsync(primsAt, c->undoPrims, primBytes, hipMemcpyDeviceToDevice, c->stream));
				HIPCHK(c, hipMemcpyAsync(boxAt, I.boxUndo, 24, hipMemcpyDeviceToDevice, c->stream));
				return RT_OK;
			});
		if (rc != RT_OK) return rc;
		I.objBox[blas] = V.objBox;
		for (int a = 0; a < 3; a++) I.blasBox6[(size_t)6 * blas + a] = lo[a], I.blasBox6[(size_t)6 * blas + 3 + a] = hi[a]; // magnitudes: the bits are the device's
	}
	c->S.wide8 = nullptr; // the quantised boxes were rounded around the uploaded geometry: a refitted tree is walked through the exact nodes
	c->sceneGen++;               // everything rt_set_time invalidates: the G-buffer and the primary-hit table ...
	c->geomGen++, c->shapeGen++; // ... and a captured history, for rt_reproject and rt_reproject_motion alike (a deformed surface has no rigid motion to
	                             // take back); rt_reproject_deform follows the deformation through the records kept above (topoGen stays)
	return RT_OK;
}

int rt_set_triangles(rt_ctx* c, uint32_t blas, const rt_triangle* tris, uint32_t n_tri)
{
	if (!c || !tris) return fail(c, RT_E_ARG, "rt_set_triangles: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_triangles: no scene uploaded");
	// ---- everything that can be refused is refused here, before anything is queued ----
	if (blas >= c->blasKeep.size()) return fail(c, RT_E_ARG, "rt_set_triangles: blas %u of %zu", blas, c->blasKeep.size());
	const rt_ctx::BlasKeep& K = c->blasKeep[blas];
	if (n_tri != K.nTri) return fail(c, RT_E_ARG, "rt_set_triangles: %u triangles, blas %u was uploaded with %u (a partial update is not supported)", n_tri, blas, K.nTri);
	if (!K.refittable) return fail(c, RT_E_UNSUPPORTED, "rt_set_triangles: the nodes of blas %u are not a tree", blas);
	if (n_tri == 0) return RT_OK; // nothing to replace
	// the local box of the new triangles, all of them (bvh::Refit folds every primitive of a leaf): magnitudes only, the bits are the device's
	// (the loop's own six floats: the arrays handed on below have their address taken, which would keep the bounds in memory all loop long)
	float l[3] = { 1e30f, 1e30f, 1e30f }, h[3] = { -1e30f, -1e30f, -1e30f };
	for (uint32_t p = 0; p < n_tri; p++) {
		const float* v = tris[p].v0; // v0, v1, v2: nine floats in a row
		for (int j = 0; j < 9; j++) {
			if (!(std::fabs(v[j]) <= 1e29f)) return fail(c, RT_E_ARG, "rt_set_triangles: triangle %u has a non-finite vertex coordinate or one beyond 1e29", p);
			l[j % 3] = std::min(l[j % 3], v[j]), h[j % 3] = std::max(h[j % 3], v[j]);
		}
	}
	const float lo[3] = { l[0], l[1], l[2] }, hi[3] = { h[0], h[1], h[2] };
	TriVerdict V;
	const int rc = triangles_verdict(c, "rt_set_triangles", blas, lo, hi, [&]() {
		rt_blas nb;
		memset(&nb, 0, sizeof(nb));
		nb.tris = tris, nb.n_tri = n_tri, nb.n_prims = n_tri; // an instanced BLAS is triangles only (pack_blas)
		return blas_object_box(nb);
	}, V);
	if (rc != RT_OK) return rc;
	return triangles_tail(c, "rt_set_triangles", blas, n_tri, lo, hi, V, tris, false);
}

int rt_blas_array(rt_ctx* c, uint32_t blas, int which, void* out, size_t cap_bytes, size_t* bytes_out)
{
	if (!c || !bytes_out) return fail(c, RT_E_ARG, "rt_blas_array: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_blas_array: no scene uploaded");
	if (blas >= c->blasKeep.size()) return fail(c, RT_E_ARG, "rt_blas_array: blas %u of %zu", blas, c->blasKeep.size());
	const rt_ctx::BlasKeep& K = c->blasKeep[blas];
	const void* src = nullptr;
	size_t need = 0;
	switch (which) {
	case RT_LAYOUT_PAIRS: src = c->pairsMut + 4 * (size_t)K.pairFirst, need = (size_t)K.pairCount * 64; break;
	case RT_LAYOUT_PRIMS: src = c->primsMut + 4 * (size_t)K.slotFirst, need = (size_t)K.slotCount * 64; break;
	default: return fail(c, RT_E_UNSUPPORTED, "rt_blas_array: array %d (PAIRS and PRIMS are kept per BLAS)", which);
	}
	*bytes_out = need;
	if (!out) return RT_OK; // the size alone
	if (cap_bytes < need) return fail(c, RT_E_ARG, "rt_blas_array: array %d of blas %u needs %zu bytes, the buffer holds %zu", which, blas, need, cap_bytes);
	if (need == 0) return RT_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(out, src, need, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return RT_OK;
}
