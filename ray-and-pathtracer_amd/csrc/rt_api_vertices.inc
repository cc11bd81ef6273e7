// rt_set_mesh_indices, rt_set_vertices, rt_set_vertices_device: an indexed mesh deformed from its vertex array alone.  The host side of
// rt_vertices.h.  The two rt_set_vertices calls are rt_set_triangles (rt_api_triangles.inc) with another head: where that call loops over
// the caller's records on the host, these assemble the records on the device (k_assemble_triangles into the staging array) and read back
// the one small record the host's checks need; triangles_verdict and triangles_tail are then that call's own.
// Included by rt_api.hip (one translation unit).

int rt_set_mesh_indices(rt_ctx* c, uint32_t blas, const uint32_t* idx, uint32_t n_tri, uint32_t n_vertices)
{
	if (!c) return fail(c, RT_E_ARG, "rt_set_mesh_indices: null context");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_mesh_indices: no scene uploaded");
	if (blas >= c->blasKeep.size()) return fail(c, RT_E_ARG, "rt_set_mesh_indices: blas %u of %zu", blas, c->blasKeep.size());
	rt_ctx::BlasKeep& K = c->blasKeep[blas];
	if (!idx) { K.idxBound = false, K.nVertices = 0; return RT_OK; } // unbound (the array stays in the scene pool for the next binding)
	// ---- everything is checked before anything is copied ----
	if (n_tri != K.nTri) return fail(c, RT_E_ARG, "rt_set_mesh_indices: indices of %u triangles, blas %u was uploaded with %u", n_tri, blas, K.nTri);
	if (n_vertices < 1) return fail(c, RT_E_ARG, "rt_set_mesh_indices: no vertices");
	for (uint32_t p = 0; p < n_tri; p++)
		for (int j = 0; j < 3; j++)
			if (idx[3 * (size_t)p + j] >= n_vertices) return fail(c, RT_E_ARG, "rt_set_mesh_indices: triangle %u names vertex %u of %u", p, idx[3 * (size_t)p + j], n_vertices);
	HIPCHK(c, hipSetDevice(c->device));
	if (!K.meshIdx) HIPCHK(c, dalloc(c->sceneAllocs, &K.meshIdx, (size_t)3 * K.nTri));
	if (n_tri > 0) {
		// behind whatever still reads the indices bound before; idx is the caller's again when the call returns
		HIPCHK(c, hipMemcpyAsync(K.meshIdx, idx, (size_t)12 * n_tri, hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
	}
	K.idxBound = true, K.nVertices = n_vertices;
	return RT_OK;
}

// blas_object_box's result from the record: the box of the hittable triangles, or the empty box at the origin
static ObjectBox verdict_object_box(const VertexVerdict& R)
{
	ObjectBox ob;
	double lo[3], hi[3];
	for (int k = 0; k < 3; k++) lo[k] = (double)key_float(R.word[6 + k]), hi[k] = (double)key_float(R.word[9 + k]);
	if (lo[0] > hi[0]) { for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0; } // nothing hittable
	for (int k = 0; k < 3; k++) ob.lo[k] = lo[k], ob.hi[k] = hi[k];
	ob.bounded = R.word[12] == 0;
	return ob;
}

static int set_vertices(rt_ctx* c, const char* who, uint32_t blas, const float* xyz, uint32_t n_vertices, bool onDevice)
{
	if (!c || !xyz) return fail(c, RT_E_ARG, "%s: null argument", who);
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "%s: no scene uploaded", who);
	// ---- what can be refused without the vertices is refused here, before anything is queued ----
	if (blas >= c->blasKeep.size()) return fail(c, RT_E_ARG, "%s: blas %u of %zu", who, blas, c->blasKeep.size());
	const rt_ctx::BlasKeep& K = c->blasKeep[blas];
	if (!K.idxBound) return fail(c, RT_E_STATE, "%s: no indices are bound to blas %u (rt_set_mesh_indices)", who, blas);
	if (n_vertices != K.nVertices) return fail(c, RT_E_ARG, "%s: %u vertices, the indices of blas %u were bound with %u", who, n_vertices, blas, K.nVertices);
	if (!K.refittable) return fail(c, RT_E_UNSUPPORTED, "%s: the nodes of blas %u are not a tree", who, blas);
	const uint32_t n_tri = K.nTri;
	if (n_tri == 0) return RT_OK; // nothing to replace
	HIPCHK(c, hipSetDevice(c->device));
	if (onDevice) {
		// device memory of the context's device, whole floats, and all of the array inside its allocation
		hipPointerAttribute_t at;
		memset(&at, 0, sizeof(at));
		const hipError_t e = hipPointerGetAttributes(&at, xyz);
		if (e != hipSuccess) (void)hipGetLastError(); // (an unregistered host pointer, on runtimes that report it as an error)
		if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->device)
			return fail(c, RT_E_ARG, "%s: dev_xyz is not device memory of device %d", who, c->device);
		if (((uintptr_t)xyz & 3u) != 0) return fail(c, RT_E_ARG, "%s: dev_xyz is not 4-byte aligned", who);
		hipDeviceptr_t base = nullptr;
		size_t size = 0;
		if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)xyz) != hipSuccess) { (void)hipGetLastError(); return fail(c, RT_E_ARG, "%s: dev_xyz is not inside a device allocation", who); }
		const size_t off = (size_t)((const char*)xyz - (const char*)base);
		if (off > size || size - off < (size_t)12 * n_vertices) return fail(c, RT_E_ARG, "%s: %u vertices do not fit the allocation behind dev_xyz", who, n_vertices);
	}
	// scratch that only the first call (or a larger BLAS, or more vertices) allocates
	{ const int rc = grow_scene_array(c, &c->triStage, c->triStageCap, (size_t)n_tri * (sizeof(rt_triangle) / sizeof(float))); if (rc != RT_OK) return rc; }
	if (!onDevice) { const int rc = grow_scene_array(c, &c->vtxStage, c->vtxStageCap, (size_t)3 * n_vertices); if (rc != RT_OK) return rc; }
	if (!c->vtxVerdict) HIPCHK(c, dalloc(c->sceneAllocs, &c->vtxVerdict, 1));

	// ---- the head on the device: nothing of the scene is written here ----
	prof_begin(c, K_QUERY);
	VertexVerdict* const R = (VertexVerdict*)(c->hostCounts + 16);
	static_assert(sizeof(VertexVerdict) <= 64 && sizeof(VertexVerdict) <= 16 * sizeof(int), "the record is read back into hostCounts[16..]");
	for (int k = 0; k < RT_VERDICT_WORDS; k++) R->word[k] = float_key(verdict_takes_min(k) ? 1e30f : -1e30f); // the empty boxes
	R->word[12] = 0, R->word[13] = 0xFFFFFFFFu;
	HIPCHK(c, hipMemcpyAsync(c->vtxVerdict, R, sizeof(VertexVerdict), hipMemcpyHostToDevice, c->stream));
	if (!onDevice) HIPCHK(c, hipMemcpyAsync(c->vtxStage, xyz, (size_t)12 * n_vertices, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_assemble_triangles, dim3((n_tri + 255) / 256), dim3(256), 0, c->stream, (const uint*)K.meshIdx, onDevice ? xyz : (const float*)c->vtxStage, (int)n_tri,
	                   (const uint*)(c->slotOf + K.slotFirst), (const float4*)c->primsMut, (float2*)c->triStage, c->vtxVerdict);
	// the record back: behind the kernel that reads the vertices, before any byte of the scene is rewritten
	HIPCHK(c, hipMemcpyAsync(R, c->vtxVerdict, sizeof(VertexVerdict), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipGetLastError());
	const VertexVerdict rec = *R;

	// ---- the verdict on the host: rt_set_triangles' checks, fed from the record ----
	if (rec.word[13] != 0xFFFFFFFFu) {
		prof_cancel(c);
		return fail(c, RT_E_ARG, "%s: triangle %u has a non-finite vertex coordinate or one beyond 1e29", who, rec.word[13]);
	}
	float lo[3], hi[3];
	for (int a = 0; a < 3; a++) lo[a] = key_float(rec.word[a]), hi[a] = key_float(rec.word[3 + a]);
	TriVerdict V;
	const int rc = triangles_verdict(c, who, blas, lo, hi, [&]() { return verdict_object_box(rec); }, V);
	if (rc != RT_OK) { prof_cancel(c); return rc; }
	return triangles_tail(c, who, blas, n_tri, lo, hi, V, nullptr, true);
}

int rt_set_vertices(rt_ctx* c, uint32_t blas, const float* xyz, uint32_t n_vertices) { return set_vertices(c, "rt_set_vertices", blas, xyz, n_vertices, false); }
int rt_set_vertices_device(rt_ctx* c, uint32_t blas, const float* dev_xyz, uint32_t n_vertices) { return set_vertices(c, "rt_set_vertices_device", blas, dev_xyz, n_vertices, true); }
