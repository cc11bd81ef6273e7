// bvh::Build / tlas::build / Scene::SetTime + bvh::Refit on the device: the host side of rt_build.h (rt_build_bvh[_split], rt_build_tlas, rt_set_time).
// Included by rt_api.hip.
// bvh::Build (splitMethod BINNEDSAH) on the device; see rt_build.h.  Planes never take part in the subdivision
// (separatePlanes, bvh.cpp:202-221: they become the right child of the root), so their node is made here.
int rt_build_bvh(rt_ctx* c, const rt_triangle* tris, uint32_t n_tri, const rt_sphere* spheres, uint32_t n_sph, const rt_plane* planes, uint32_t n_pla,
                 rt_bvh_node* nodes_out, uint32_t* prim_idx_out, uint32_t* nodes_used_out)
{
	return rt_build_bvh_split(c, RT_SPLIT_BINNEDSAH, tris, n_tri, spheres, n_sph, planes, n_pla, nodes_out, prim_idx_out, nodes_used_out);
}

int rt_build_bvh_split(rt_ctx* c, int split_method, const rt_triangle* tris, uint32_t n_tri, const rt_sphere* spheres, uint32_t n_sph, const rt_plane* planes, uint32_t n_pla,
                       rt_bvh_node* nodes_out, uint32_t* prim_idx_out, uint32_t* nodes_used_out)
{
	if (split_method < 0 || split_method > 3) return fail(c, RT_E_ARG, "rt_build_bvh: split method %d (bvh.h:38-43 knows 0..3)", split_method);
	if (!c || !nodes_out || !prim_idx_out || !nodes_used_out) return fail(c, RT_E_ARG, "rt_build_bvh: null argument");
	if ((n_tri && !tris) || (n_sph && !spheres) || (n_pla && !planes)) return fail(c, RT_E_ARG, "rt_build_bvh: null primitive array");
	const uint M = n_tri + n_sph, N = M + n_pla;
	if (M == 0) return fail(c, RT_E_UNSUPPORTED, "rt_build_bvh: no triangle or sphere to subdivide (the reference's paths for an empty or plane-only bvh stay on the host)");
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<void*> tmp;
	struct Guard { std::vector<void*>& v; ~Guard() { free_pool(v); } } guard{ tmp };
	BuildArrays B;
	memset(&B, 0, sizeof(B));
	float *dTri = nullptr, *dSph = nullptr;
	int *openA = nullptr, *openB = nullptr;
	HIPCHK(c, dalloc(tmp, &dTri, (size_t)n_tri * 14 + 4));
	HIPCHK(c, dalloc(tmp, &dSph, (size_t)n_sph * 8 + 4));
	HIPCHK(c, dalloc(tmp, &B.cen, M));
	HIPCHK(c, dalloc(tmp, &B.nlo, M));
	HIPCHK(c, dalloc(tmp, &B.nhi, M));
	HIPCHK(c, dalloc(tmp, &B.blo, M));
	HIPCHK(c, dalloc(tmp, &B.bhi, M));
	HIPCHK(c, dalloc(tmp, &B.idx, M));
	HIPCHK(c, dalloc(tmp, &B.tmp, M));
	HIPCHK(c, dalloc(tmp, &B.hpos, M));
	HIPCHK(c, dalloc(tmp, &B.fpos, M));
	HIPCHK(c, dalloc(tmp, &B.nodes, (size_t)2 * M + 2));
	HIPCHK(c, dalloc(tmp, &B.counters, 8));
	HIPCHK(c, dalloc(tmp, &openA, (size_t)2 * M + 2));
	HIPCHK(c, dalloc(tmp, &openB, (size_t)2 * M + 2));
	static_assert(sizeof(rt_triangle) == 56 && sizeof(rt_sphere) == 32, "primitive layouts of rt_amd.h");
	if (n_tri) HIPCHK(c, hipMemcpyAsync(dTri, tris, (size_t)n_tri * sizeof(rt_triangle), hipMemcpyHostToDevice, c->stream));
	if (n_sph) HIPCHK(c, hipMemcpyAsync(dSph, spheres, (size_t)n_sph * sizeof(rt_sphere), hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipMemsetAsync(B.counters, 0, 8 * sizeof(int), c->stream));
	const int rootList[1] = { 0 }, one = 1;
	HIPCHK(c, hipMemcpyAsync(openA, rootList, sizeof(int), hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_build_prep, dim3((M + 255) / 256), dim3(256), 0, c->stream, dTri, 14, (int)n_tri, dSph, 8, (int)n_sph, B);
	hipLaunchKernelGGL(k_build_root, dim3(1), dim3(RT_BUILD_THREADS), 0, c->stream, B, M);
	HIPCHK(c, hipMemcpyAsync(B.counters + 4, &one, sizeof(int), hipMemcpyHostToDevice, c->stream));
	// Levels are launched in groups without looking at the device: a level's launch covers the most nodes the
	// level can hold (2^level, at most M) and its surplus blocks return at once; the open count is read back
	// after each group.
	int host[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	int *open = openA, *next = openB;
	int level = 0;
	for (bool done = false; !done;) {
		for (int g = 0; g < 16 && (uint)level <= M + 2; g++, level++) { // a tree over M primitives has at most M levels
			const unsigned cap = level < 31 && (1u << level) < M ? (1u << level) : M;
			hipLaunchKernelGGL(k_build_level, dim3(cap), dim3(RT_BUILD_THREADS), 0, c->stream, B, open, next, level, split_method);
			hipLaunchKernelGGL(k_build_advance, dim3(1), dim3(1), 0, c->stream, B, level);
			std::swap(open, next);
		}
		HIPCHK(c, hipMemcpyAsync(host, B.counters, 8 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		if (host[2]) return fail(c, RT_E_UNSUPPORTED, "rt_build_bvh: non-finite vertex, centre or radius (the reference's NaN-order-dependent min / max stay on the host)");
		done = host[4 + (level & 1)] == 0;
		if (!done && (uint)level > M + 2) return fail(c, RT_E_STATE, "rt_build_bvh: more levels than primitives");
	}
	HIPCHK(c, hipGetLastError());
	const int nT = host[0];
	std::vector<TNode> t((size_t)nT);
	HIPCHK(c, hipMemcpy(t.data(), B.nodes, (size_t)nT * sizeof(TNode), hipMemcpyDeviceToHost));
	HIPCHK(c, hipMemcpy(prim_idx_out, B.idx, (size_t)M * sizeof(uint), hipMemcpyDeviceToHost));
	for (uint i = 0; i < n_pla; i++) prim_idx_out[M + i] = M + i;

	// the reference's numbering: Subdivide allocates a node's children (an adjacent pair) when it reaches the
	// node, depth first, left subtree before right (bvh.cpp:317-332)
	memset(nodes_out, 0, (size_t)2 * (N + 1) * sizeof(rt_bvh_node));
	uint nodesUsed = 2;
	uint rootAt = 0;
	if (n_pla > 0) {
		// separatePlanes: root -> { node 2 = what was subdivided above, node 3 = the planes }
		nodesUsed = 4, rootAt = 2;
		rt_bvh_node& pl = nodes_out[3];
		float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f };
		for (uint i = 0; i < n_pla; i++) { // UpdateNodeBounds for planes, Q1 (bvh.cpp:90-111)
			const float* Np = planes[i].N;
			const float invLen = 1.0f / sqrtf(Np[0] * Np[0] + Np[1] * Np[1] + Np[2] * Np[2]);
			const float n[3] = { Np[0] * invLen, Np[1] * invLen, Np[2] * invLen };
			int ax = -1;
			if (n[0] + n[1] + n[2] == 1 && (n[0] == 1 || n[1] == 1 || n[2] == 1)) ax = n[0] == 1 ? 0 : (n[1] == 1 ? 1 : 2);
			if (ax < 0) { for (int k = 0; k < 3; k++) lo[k] = -1e30f, hi[k] = 1e30f; break; }
			for (int k = 0; k < 3; k++) {
				const float sl = k == ax ? 0.0f : -1e30f, sh = k == ax ? 0.0f : 1e30f;
				lo[k] = lo[k] < sl ? lo[k] : sl, hi[k] = hi[k] > sh ? hi[k] : sh;
			}
		}
		memcpy(pl.aabb_min, lo, 12), memcpy(pl.aabb_max, hi, 12);
		pl.left_first = M, pl.prim_count = n_pla;
	}
	std::vector<std::pair<int, uint>> stack; // (TNode, final index)
	stack.push_back({ 0, rootAt });
	while (!stack.empty()) {
		const int id = stack.back().first;
		const uint at = stack.back().second;
		stack.pop_back();
		const TNode& tn = t[(size_t)id];
		rt_bvh_node& o = nodes_out[at];
		memcpy(o.aabb_min, tn.lo, 12), memcpy(o.aabb_max, tn.hi, 12);
		if (tn.left < 0) { o.left_first = tn.first, o.prim_count = tn.count; continue; }
		const uint pair = nodesUsed;
		nodesUsed += 2;
		o.left_first = pair, o.prim_count = 0;
		stack.push_back({ tn.right, pair + 1 }); // popped after the whole left subtree
		stack.push_back({ tn.left, pair });
	}
	// The device's boxes are hardware min / max in reduction order; the reference's are what its closing Refit (bvh.cpp:556-594) leaves:
	// a leaf folds its primitives in primitiveIdx order, an inner node takes its children, both with the ternaries a < b ? a : b and
	// a > b ? a : b.  The two agree in value; where the value is zero and both zeros occur among the candidates, the ternaries keep the
	// sign of the last one and the hardware prefers -0 / +0.  Restore the reference's sign (children have larger numbers than their parent).
	for (uint i = nodesUsed; i-- > rootAt;) {
		if (i == 1 || (n_pla > 0 && i == 3)) continue;
		rt_bvh_node& nd = nodes_out[i];
		for (int k = 0; k < 3; k++) {
			if (nd.aabb_min[k] != 0.0f && nd.aabb_max[k] != 0.0f) continue;
			float lo = 1e30f, hi = -1e30f;
			if (nd.prim_count > 0) {
				for (uint j = 0; j < nd.prim_count; j++) {
					const uint p = prim_idx_out[nd.left_first + j];
					if (p < n_tri) {
						const float v[3] = { tris[p].v0[k], tris[p].v1[k], tris[p].v2[k] };
						for (int q = 0; q < 3; q++) lo = lo < v[q] ? lo : v[q], hi = hi > v[q] ? hi : v[q];
					} else {
						const rt_sphere& s = spheres[p - n_tri];
						const float a = s.pos[k] - s.r, b = s.pos[k] + s.r;
						lo = lo < a ? lo : a, hi = hi > b ? hi : b;
					}
				}
			} else {
				const rt_bvh_node &l = nodes_out[nd.left_first], &r = nodes_out[nd.left_first + 1];
				lo = l.aabb_min[k] < r.aabb_min[k] ? l.aabb_min[k] : r.aabb_min[k], hi = l.aabb_max[k] > r.aabb_max[k] ? l.aabb_max[k] : r.aabb_max[k];
			}
			nd.aabb_min[k] = lo, nd.aabb_max[k] = hi;
		}
	}
	if (n_pla > 0) { // Refit of the root (bvh.cpp:556-594): union of its two children
		rt_bvh_node& r = nodes_out[0];
		const rt_bvh_node &a = nodes_out[2], &b = nodes_out[3];
		for (int k = 0; k < 3; k++) r.aabb_min[k] = a.aabb_min[k] < b.aabb_min[k] ? a.aabb_min[k] : b.aabb_min[k], r.aabb_max[k] = a.aabb_max[k] > b.aabb_max[k] ? a.aabb_max[k] : b.aabb_max[k];
		r.left_first = 2, r.prim_count = 0;
	}
	*nodes_used_out = nodesUsed;
	return RT_OK;
}

// tlas::build on the device (rt_build.h k_build_tlas): bounds6 = per instance the world box bvhInstance::SetTransform
// left in 'bounds' (min.xyz, max.xyz); nodes_out has room for 2 n + 1 nodes.
int rt_build_tlas(rt_ctx* c, const float* bounds6, uint32_t n, rt_tlas_node* nodes_out, uint32_t* nodes_used_out)
{
	if (!c || !bounds6 || !nodes_out || !nodes_used_out) return fail(c, RT_E_ARG, "rt_build_tlas: null argument");
	if (n < 1 || n > RT_TLAS_MAX) return fail(c, RT_E_UNSUPPORTED, "rt_build_tlas: %u instances (the reference's nodeIdx[256] holds 1..256, tlas.cpp:16)", n);
	for (uint32_t i = 0; i < 6 * n; i++)
		if (!(std::fabs(bounds6[i]) <= 1e30f)) return fail(c, RT_E_UNSUPPORTED, "rt_build_tlas: instance %u has a non-finite bound", i / 6);
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<void*> tmp;
	struct Guard { std::vector<void*>& v; ~Guard() { free_pool(v); } } guard{ tmp };
	float* dB = nullptr;
	TlasNodeDev* dN = nullptr;
	int* dU = nullptr;
	static_assert(sizeof(TlasNodeDev) == sizeof(rt_tlas_node), "TLAS node layout");
	HIPCHK(c, dalloc(tmp, &dB, (size_t)6 * n));
	HIPCHK(c, dalloc(tmp, &dN, (size_t)2 * n + 1));
	HIPCHK(c, dalloc(tmp, &dU, 1));
	HIPCHK(c, hipMemsetAsync(dN, 0, ((size_t)2 * n + 1) * sizeof(TlasNodeDev), c->stream));
	HIPCHK(c, hipMemcpyAsync(dB, bounds6, (size_t)24 * n, hipMemcpyHostToDevice, c->stream));
	hipLaunchKernelGGL(k_build_tlas, dim3(1), dim3(64), 0, c->stream, dB, (int)n, dN, dU);
	int used = 0;
	HIPCHK(c, hipMemcpyAsync(&used, dU, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(nodes_out, dN, ((size_t)2 * n + 1) * sizeof(rt_tlas_node), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipGetLastError());
	if (used < 0) return fail(c, RT_E_UNSUPPORTED, "rt_build_tlas: no finite union area left (degenerate instance bounds)");
	*nodes_used_out = (uint32_t)used;
	return RT_OK;
}

// bvh::Refit over one tree, queued on the context's stream: order lists its pair records by level (level l: order[level[l] .. level[l + 1])),
// levelDev is level[] on the device.  Bottom up: a level with more records than one workgroup covers in two passes gets a launch of its
// own across the chip; the narrow levels above the last such level share one workgroup with barriers between them.  rt_set_time and
// rt_set_triangles (rt_api_triangles.inc) refit under this one plan.
static void refit_launch(rt_ctx* c, const uint* order, const int* levelDev, const int* level, int nLevels)
{
	if (nLevels <= 0) return;
	int top = nLevels; // levels [0, top) are left for the single-workgroup kernel
	for (int l = nLevels - 1; l >= 0; l--) {
		const int count = level[l + 1] - level[l];
		if (count < 2048) continue;
		// everything deeper than l must be done first: the narrow levels between two wide ones go with the next wide launch's predecessor
		for (int m = top - 1; m > l; m--) {
			const int cm = level[m + 1] - level[m];
			if (cm > 0) hipLaunchKernelGGL(k_refit_level, dim3((cm + 255) / 256), dim3(256), 0, c->stream, c->pairsMut, c->primsMut, order, level[m], cm);
		}
		hipLaunchKernelGGL(k_refit_level, dim3((count + 255) / 256), dim3(256), 0, c->stream, c->pairsMut, c->primsMut, order, level[l], count);
		top = l;
	}
	if (top > 0) hipLaunchKernelGGL(k_refit, dim3(1), dim3(1024), 0, c->stream, c->pairsMut, c->primsMut, order, levelDev, top);
}

// rt_reproject_deform's copy on first write (rt_ctx.h History): called by whatever is about to rewrite the primitive records of BLAS b,
// before it queues the rewrite.  While a history is valid at the deform level and b has no kept copy yet, the records as they are -- the
// capture's -- are copied aside on the context's stream and the kernel's table entry follows; otherwise nothing is queued.
static int history_keep_blas(rt_ctx* c, uint32_t b)
{
	rt_ctx::History& H = c->hist;
	if (!H.acc || H.gen == 0 || H.topoGen != c->topoGen) return RT_OK;
	if (b >= c->blasKeep.size() || b >= c->keptMark.size() || b >= H.keptDeltaCap || c->keptMark[b]) return RT_OK;
	const rt_ctx::BlasKeep& K = c->blasKeep[b];
	if (K.slotCount == 0) return RT_OK;
	if (c->keptCap[b] < K.slotCount) {
		HIPCHK(c, dalloc(c->historyAllocs, &c->keptBuf[b], (size_t)K.slotCount * 4));
		c->keptCap[b] = K.slotCount;
	}
	const float4* at = c->primsMut + 4 * (size_t)K.slotFirst;
	HIPCHK(c, hipMemcpyAsync(c->keptBuf[b], at, (size_t)K.slotCount * 64, hipMemcpyDeviceToDevice, c->stream));
	c->keptDeltaHost[b] = (long long)((const char*)c->keptBuf[b] - (const char*)at);
	HIPCHK(c, hipMemcpyAsync(H.keptDelta + b, &c->keptDeltaHost[b], sizeof(long long), hipMemcpyHostToDevice, c->stream));
	c->keptMark[b] = 1;
	return RT_OK;
}

int rt_set_time(rt_ctx* c, float t)
{
	if (!c) return RT_E_ARG;
	c->sceneGen++; // the G-buffer (rt_render_aovs) is stale from here on
	c->geomGen++, c->shapeGen++;  // ... and so is a captured history, for rt_reproject and rt_reproject_motion (rt_reproject_deform follows: topoGen stays)
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_time: no scene uploaded");
	if (c->S.useTLAS) return fail(c, RT_E_UNSUPPORTED, "rt_set_time: the reference animates only without the TLAS (animOn, template/scene.h:1389)");
	if (!c->primsOrig) return RT_OK; // nothing to animate
	c->S.wide8 = nullptr; // the quantised boxes were rounded around the uploaded geometry: a refitted tree is walked through the exact nodes
	HIPCHK(c, hipSetDevice(c->device));
	// float r = fmodf(t, 2 * PI); float a = sinf(r) * 0.5f;  (template/scene.h:1229-1230; sinf in f64, rounded once)
	const float r = fmodf(t, 2 * RT_PI);
	const float a = (float)sin((double)r) * 0.5f;
	{ const int rc = history_keep_blas(c, 0); if (rc != RT_OK) return rc; } // k_animate rewrites the scene BVH's records in place
	hipLaunchKernelGGL(k_animate, dim3((c->animSlots + 255) / 256), dim3(256), 0, c->stream, c->primsOrig, c->primsMut, c->animSlots, a);
	refit_launch(c, c->refitOrder, c->refitLevelStart, c->refitLevelHost.data(), c->refitLevels);
	if (c->S.wide && c->wideNodes > 0) hipLaunchKernelGGL(k_wide_sync, dim3((c->wideNodes * 4 + 255) / 256), dim3(256), 0, c->stream, c->wideMut, c->pairsMut, c->wideNodes);
	HIPCHK(c, hipGetLastError());
	return RT_OK;
}

