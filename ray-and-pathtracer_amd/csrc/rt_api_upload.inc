// rt_upload_scene: the reference-shaped arrays of include/rt_amd.h -> the HBM traversal layout of rt_scene_dev.h (pair records, primitive records,
// 4-wide / 8-wide nodes, TLAS pairs + reach boxes, instances, lights, materials, sky).  Host code only.  Included by rt_api.hip (one translation unit).
// ---- scene upload: reference-shaped arrays -> HBM traversal layout ---------------------------------
// matTypes: rt_material::type per material (null: none known); the type of the primitive's material rides in bits 4-5 of the
// record's kind word, so that the kernel that resolves a hit knows what the hit means for the path without a second fetch
static void pack_prim(float* rec, const rt_blas& b, uint p, bool last, const rt_material* mats = nullptr, uint nMats = 0)
{
	memset(rec, 0, 64);
	int kind, obj, mat;
	if (p < b.n_tri) {
		const rt_triangle& t = b.tris[p];
		rec[0] = t.v0[0], rec[1] = t.v0[1], rec[2] = t.v0[2], rec[3] = t.N[0];
		rec[4] = t.v1[0], rec[5] = t.v1[1], rec[6] = t.v1[2], rec[7] = t.N[1];
		rec[8] = t.v2[0], rec[9] = t.v2[1], rec[10] = t.v2[2], rec[11] = t.N[2];
		// float d = -dot(N, v0) (template/scene.h:193), same expression tree as the per-ray evaluation
		volatile float p0 = t.N[0] * t.v0[0], p1 = t.N[1] * t.v0[1], p2 = t.N[2] * t.v0[2];
		volatile float s01 = p0 + p1;
		volatile float s = s01 + p2;
		rec[12] = -s;
		kind = RT_KIND_TRI, obj = t.obj_idx, mat = t.material;
	} else if (p < b.n_tri + b.n_sph) {
		const rt_sphere& s = b.spheres[p - b.n_tri];
		rec[0] = s.pos[0], rec[1] = s.pos[1], rec[2] = s.pos[2], rec[3] = s.r2;
		rec[4] = s.invr, rec[5] = s.r;
		kind = RT_KIND_SPHERE, obj = s.obj_idx, mat = s.material;
	} else {
		const rt_plane& q = b.planes[p - b.n_tri - b.n_sph];
		rec[0] = q.N[0], rec[1] = q.N[1], rec[2] = q.N[2], rec[3] = q.d;
		kind = RT_KIND_PLANE, obj = q.obj_idx, mat = q.material;
	}
	int kl = kind | (last ? RT_LAST_BIT : 0);
	if (mats && mat >= 0 && (uint)mat < nMats) kl |= (mats[mat].type & 3) << RT_TYPE_SHIFT;
	memcpy(rec + 13, &obj, 4), memcpy(rec + 14, &mat, 4), memcpy(rec + 15, &kl, 4);
}

int rt_upload_scene(rt_ctx* c, const rt_scene_desc* d)
{
	if (!c || !d) return fail(c, RT_E_ARG, "rt_upload_scene: null argument");
	c->sceneGen++; // the G-buffer (rt_render_aovs) is stale from here on, whatever the outcome
	c->geomGen++;  // ... and so is a captured history (rt_history_capture)
	HIPCHK(c, hipSetDevice(c->device));
	if (d->n_lights > RT_MAX_LIGHTS) return fail(c, RT_E_UNSUPPORTED, "rt_upload_scene: %u lights (limit %d)", d->n_lights, RT_MAX_LIGHTS);
	if (d->n_blas < 1 || !d->blas) return fail(c, RT_E_ARG, "rt_upload_scene: no bvh");
	if (d->use_tlas && (d->n_instances < 1 || d->n_instances > 256 || !d->tlas_nodes)) return fail(c, RT_E_UNSUPPORTED, "rt_upload_scene: TLAS needs 1..256 instances (nodeIdx[256], tlas.cpp:16)");
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		if (m.type < 1 || m.type > 3) return fail(c, RT_E_ARG, "rt_upload_scene: material %u has type %d", i, m.type);
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->mega.pick = {}; // another scene: the Whitted forms are timed again
	free_pool(c->sceneAllocs);
	c->sceneLoaded = false;
	c->pathUnsupported = false;
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		if (m.type == RT_MAT_DIFFUSE && (m.shinieness != 0 || m.raytracer == 0)) {
			c->pathUnsupported = true;
			c->pathUnsupportedWhy = m.shinieness != 0 ? "a diffuse material has shinieness != 0" : "a diffuse material was built with raytracer == 0";
		}
	}

	// pairs + prims of every BLAS, concatenated
	std::vector<float> pairs, prims;
	std::vector<uint> rootLink(d->n_blas), pairOffOf(d->n_blas);
	for (uint k = 0; k < d->n_blas; k++) {
		const rt_blas& b = d->blas[k];
		if (b.nodes_used < 1 || (b.nodes_used & 1) || !b.nodes) return fail(c, RT_E_ARG, "rt_upload_scene: blas %u has %u nodes (expected an even count >= 2)", k, b.nodes_used);
		if (b.n_prims != b.n_tri + b.n_sph + b.n_pla) return fail(c, RT_E_ARG, "rt_upload_scene: blas %u primitive counts disagree", k);
		// an instanced BLAS is a mesh (bvh(Mesh*), bvh.cpp:5-16): the instance path resolves triangle normals only
		// (bvhInstance.cpp:19), so spheres / planes below an instance are refused rather than shaded wrongly
		if (d->use_tlas && (b.n_sph > 0 || b.n_pla > 0)) return fail(c, RT_E_UNSUPPORTED, "rt_upload_scene: blas %u holds spheres / planes; an instanced BLAS must be triangles only", k);
		// node boxes must be numbers within the reference's +-1e30 sentinels (bvh.cpp:96-109): the hardware min / max
		// slab test of clean rays relies on it
		for (uint i = 0; i < b.nodes_used && b.n_prims > 0; i++) {
			if (i == 1) continue;
			for (int a = 0; a < 3; a++)
				if (!(std::fabs(b.nodes[i].aabb_min[a]) <= 1e30f) || !(std::fabs(b.nodes[i].aabb_max[a]) <= 1e30f))
					return fail(c, RT_E_UNSUPPORTED, "rt_upload_scene: blas %u node %u has a non-finite bound or one beyond 1e30", k, i);
		}
		const uint pairOff = (uint)(pairs.size() / 16), primOff = (uint)(prims.size() / 16);
		pairOffOf[k] = pairOff;
		std::vector<char> last(b.n_prims, 0);
		auto link_of = [&](uint i) -> uint {
			const rt_bvh_node& nd = b.nodes[i];
			if (nd.prim_count > 0) return RT_LEAF_BIT | (primOff + nd.left_first);
			return pairOff + nd.left_first / 2;
		};
		for (uint i = 0; i < b.nodes_used; i++) {
			if (i == 1) continue;
			const rt_bvh_node& nd = b.nodes[i];
			if (nd.prim_count > 0) {
				if (nd.left_first + nd.prim_count > b.n_prims) return fail(c, RT_E_ARG, "rt_upload_scene: blas %u node %u leaf range out of bounds", k, i);
				last[nd.left_first + nd.prim_count - 1] = 1;
			} else if (b.n_prims > 0 && ((nd.left_first & 1) || nd.left_first < 2 || nd.left_first + 1 >= b.nodes_used)) {
				return fail(c, RT_E_ARG, "rt_upload_scene: blas %u node %u child index %u invalid", k, i, nd.left_first);
			}
		}
		rootLink[k] = b.n_prims == 0 ? RT_EMPTY : link_of(0);
		pairs.resize(pairs.size() + (size_t)(b.nodes_used / 2) * 16, 0.0f);
		for (uint i = 2; i + 1 < b.nodes_used + 0u && b.n_prims > 0; i += 2) {
			float* rec = &pairs[(size_t)(pairOff + i / 2) * 16];
			for (int s = 0; s < 2; s++) {
				const rt_bvh_node& nd = b.nodes[i + s];
				uint lk = link_of(i + s);
				memcpy(rec + 8 * s, nd.aabb_min, 12), memcpy(rec + 8 * s + 3, &lk, 4);
				memcpy(rec + 8 * s + 4, nd.aabb_max, 12);
			}
		}
		prims.resize(prims.size() + (size_t)b.n_prims * 16);
		for (uint j = 0; j < b.n_prims; j++) {
			const uint p = b.prim_idx[j];
			if (p >= b.n_prims) return fail(c, RT_E_ARG, "rt_upload_scene: blas %u prim_idx[%u] = %u out of range", k, j, p);
			pack_prim(&prims[(size_t)(primOff + j) * 16], b, p, last[j] != 0, d->materials, d->n_materials);
		}
	}
	// 4-wide nodes (rt_scene_dev.h, wide[]): collapse every BLAS; all or nothing (one flag for the kernels)
	std::vector<float> wide;
	std::vector<uint> rootWide(d->n_blas);
	// Default: on for a scene BVH, off with a TLAS (RT_WIDE=0 / 1 forces).  Exact either way (tests/test_gpu_parity.py::
	// test_wide_walk_*).  Measured (profiles/r02_wide_by_config.txt): one big tree gains (config 4: connect 19.3 -> 16.3 ms
	// per step, config 2: 2.63 -> 2.47), instanced scenes lose or stay level (config 5: 625 -> 660 ms, config 3: 10.1 -> 10.2):
	// there the walk spends its steps on the TLAS level and the first levels of many BLASes, where a 4-wide step
	// replaces fewer binary ones than it costs (four slab tests, a sorting network and up to three pushes).
	bool wideOK = c->knobs.wide >= 0 ? c->knobs.wide != 0 : !d->use_tlas;
	{
		size_t primBase = 0;
		for (uint k = 0; k < d->n_blas && wideOK; k++) {
			const rt_blas& b = d->blas[k];
			const uint primOff = (uint)primBase;
			primBase += b.n_prims;
			rootWide[k] = rootLink[k];
			if (b.n_prims == 0 || b.nodes[0].prim_count > 0) continue; // empty, or the root is a leaf
			// nested?  (parents are unions of their children after bvh::Refit, bvh.cpp:556-594)
			for (uint i = 0; i < b.nodes_used && wideOK; i++) {
				if (i == 1 || b.nodes[i].prim_count > 0) continue;
				for (uint ci = b.nodes[i].left_first; ci < b.nodes[i].left_first + 2; ci++)
					for (int a = 0; a < 3; a++)
						if (!(b.nodes[ci].aabb_min[a] >= b.nodes[i].aabb_min[a]) || !(b.nodes[ci].aabb_max[a] <= b.nodes[i].aabb_max[a])) wideOK = false;
			}
			if (!wideOK) break;
			auto area = [&](uint i) { const rt_bvh_node& n = b.nodes[i]; const double ex = (double)n.aabb_max[0] - n.aabb_min[0], ey = (double)n.aabb_max[1] - n.aabb_min[1], ez = (double)n.aabb_max[2] - n.aabb_min[2]; return ex * ey + ey * ez + ez * ex; };
			// depth-first emission; a record is reserved when its binary node is first reached
			std::vector<std::pair<uint, uint>> todo; // (binary inner node, wide record)
			auto reserve = [&]() { const uint w = (uint)(wide.size() / 32); wide.resize(wide.size() + 32, 0.0f); return w; };
			const uint rootRec = reserve();
			rootWide[k] = rootRec;
			todo.push_back({ 0u, rootRec });
			while (!todo.empty()) {
				const uint node = todo.back().first, rec = todo.back().second;
				todo.pop_back();
				uint ch[4];
				int n = 2;
				ch[0] = b.nodes[node].left_first, ch[1] = ch[0] + 1;
				while (n < 4) {
					int best = -1;
					double bestA = -1;
					for (int j = 0; j < n; j++)
						if (b.nodes[ch[j]].prim_count == 0 && area(ch[j]) > bestA) best = j, bestA = area(ch[j]);
					if (best < 0) break;
					const uint lf = b.nodes[ch[best]].left_first;
					for (int j = n; j > best + 1; j--) ch[j] = ch[j - 1];
					ch[best] = lf, ch[best + 1] = lf + 1;
					n++;
				}
				float* r = &wide[(size_t)rec * 32];
				for (int j = 0; j < 4; j++) {
					uint link = RT_EMPTY, src = 0xFFFFFFFFu;
					float lo[3] = { 1e30f, 1e30f, 1e30f }, hi[3] = { -1e30f, -1e30f, -1e30f }; // inverted: never hit
					if (j < n) {
						const rt_bvh_node& c2 = b.nodes[ch[j]];
						memcpy(lo, c2.aabb_min, 12), memcpy(hi, c2.aabb_max, 12);
						src = pairOffOf[k] * 2 + ch[j]; // global binary node number: pair record (src / 2), side (src & 1)
						if (c2.prim_count > 0) link = RT_LEAF_BIT | (primOff + c2.left_first);
						else { link = reserve(); r = &wide[(size_t)rec * 32]; todo.push_back({ ch[j], link }); }
					}
					for (int a = 0; a < 3; a++) r[4 * a + j] = lo[a], r[12 + 4 * a + j] = hi[a];
					memcpy(&r[24 + j], &link, 4), memcpy(&r[28 + j], &src, 4);
				}
			}
		}
		if (!wideOK) wide.clear();
	}
	// 8-wide nodes with quantised child boxes (rt_scene_dev.h, wide8[] / leafBox[]; SURVEY.md 8f N3): the same collapse, up to eight
	// children, each child's box rounded outwards onto the node's 8-bit grid.  All or nothing.  RT_WIDE8=1 / 0 forces; default: see below.
	std::vector<uint> wide8;     // 32 uints per node
	std::vector<float> leafBox;  // 8 floats per leaf: {min.xyz, first slot}{max.xyz, -}
	std::vector<uint> rootWide8(d->n_blas);
	bool wide8OK = c->knobs.wide8 != 0;
	{
		size_t primBase = 0;
		for (uint k = 0; k < d->n_blas && wide8OK; k++) {
			const rt_blas& b = d->blas[k];
			const uint primOff = (uint)primBase;
			primBase += b.n_prims;
			rootWide8[k] = RT_EMPTY;
			if (b.n_prims == 0) continue;
			// nested and bounded?  (outward rounding needs finite boxes; a plane's +-1e30 slab has no useful grid)
			for (uint i = 0; i < b.nodes_used && wide8OK; i++) {
				if (i == 1) continue;
				for (int a = 0; a < 3; a++)
					if (!(fabsf(b.nodes[i].aabb_min[a]) < 1e29f) || !(fabsf(b.nodes[i].aabb_max[a]) < 1e29f) || !(b.nodes[i].aabb_min[a] <= b.nodes[i].aabb_max[a])) wide8OK = false;
				if (b.nodes[i].prim_count > 0) continue;
				for (uint ci = b.nodes[i].left_first; ci < b.nodes[i].left_first + 2; ci++)
					for (int a = 0; a < 3; a++)
						if (!(b.nodes[ci].aabb_min[a] >= b.nodes[i].aabb_min[a]) || !(b.nodes[ci].aabb_max[a] <= b.nodes[i].aabb_max[a])) wide8OK = false;
			}
			if (!wide8OK) break;
			auto area = [&](uint i) { const rt_bvh_node& n = b.nodes[i]; const double ex = (double)n.aabb_max[0] - n.aabb_min[0], ey = (double)n.aabb_max[1] - n.aabb_min[1], ez = (double)n.aabb_max[2] - n.aabb_min[2]; return ex * ey + ey * ez + ez * ex; };
			auto leaf_link = [&](uint node) {
				const rt_bvh_node& n = b.nodes[node];
				const uint li = (uint)(leafBox.size() / 8);
				const uint slot = primOff + n.left_first;
				float rec[8] = { n.aabb_min[0], n.aabb_min[1], n.aabb_min[2], 0, n.aabb_max[0], n.aabb_max[1], n.aabb_max[2], 0 };
				memcpy(&rec[3], &slot, 4);
				leafBox.insert(leafBox.end(), rec, rec + 8);
				return RT_BOX_BIT | li;
			};
			if (b.nodes[0].prim_count > 0) { rootWide8[k] = leaf_link(0); continue; } // the root is a leaf
			std::vector<std::pair<uint, uint>> todo; // (binary inner node, wide8 record)
			auto reserve = [&]() { const uint w = (uint)(wide8.size() / 32); wide8.resize(wide8.size() + 32, 0u); return w; };
			const uint rootRec = reserve();
			rootWide8[k] = rootRec;
			todo.push_back({ 0u, rootRec });
			while (!todo.empty() && wide8OK) {
				const uint node = todo.back().first, rec = todo.back().second;
				todo.pop_back();
				uint ch[8];
				int n = 2;
				ch[0] = b.nodes[node].left_first, ch[1] = ch[0] + 1;
				while (n < 8) {
					int best = -1;
					double bestA = -1;
					for (int j = 0; j < n; j++)
						if (b.nodes[ch[j]].prim_count == 0 && area(ch[j]) > bestA) best = j, bestA = area(ch[j]);
					if (best < 0) break;
					const uint lf = b.nodes[ch[best]].left_first;
					for (int j = n; j > best + 1; j--) ch[j] = ch[j - 1];
					ch[best] = lf, ch[best + 1] = lf + 1;
					n++;
				}
				uint links[8];
				for (int j = 0; j < 8; j++) {
					links[j] = RT_EMPTY;
					if (j >= n) continue;
					if (b.nodes[ch[j]].prim_count > 0) links[j] = leaf_link(ch[j]);
					else { links[j] = reserve(); todo.push_back({ ch[j], links[j] }); }
				}
				uint* r = &wide8[(size_t)rec * 32];
				unsigned char q[6][8]; // qlo.x qlo.y qlo.z qhi.x qhi.y qhi.z
				uint exps = 0;
				for (int a = 0; a < 3 && wide8OK; a++) {
					float org = b.nodes[ch[0]].aabb_min[a], top = b.nodes[ch[0]].aabb_max[a];
					for (int j = 1; j < n; j++) org = std::min(org, b.nodes[ch[j]].aabb_min[a]), top = std::max(top, b.nodes[ch[j]].aabb_max[a]);
					const double extent = (double)top - (double)org;
					int e = extent > 0 ? (int)std::ceil(std::log2(extent / 255.0)) : -100;
					if (e < -100) e = -100;
					for (bool again = true; again && wide8OK;) {
						again = false;
						if (e > 100) { wide8OK = false; break; }
						const float sc = std::ldexp(1.0f, e);
						for (int j = 0; j < 8 && !again; j++) {
							if (j >= n) { q[a][j] = 255, q[3 + a][j] = 0; continue; } // inverted: never hit (and the link says empty)
							const float lo = b.nodes[ch[j]].aabb_min[a], hi = b.nodes[ch[j]].aabb_max[a];
							int ql = (int)std::floor(((double)lo - (double)org) / (double)sc), qh = (int)std::ceil(((double)hi - (double)org) / (double)sc);
							ql = std::max(0, std::min(255, ql)), qh = std::max(0, std::min(255, qh));
							// the device's own expression must contain the box: fma(q, 2^e, origin)
							while (ql > 0 && std::fmaf((float)ql, sc, org) > lo) ql--;
							while (qh < 255 && std::fmaf((float)qh, sc, org) < hi) qh++;
							if (std::fmaf((float)ql, sc, org) > lo || std::fmaf((float)qh, sc, org) < hi) { e++; again = true; break; } // a coarser grid
							q[a][j] = (unsigned char)ql, q[3 + a][j] = (unsigned char)qh;
						}
					}
					memcpy(&r[a], &org, 4);
					exps |= (uint)(e + 128) << (8 * a);
				}
				r[3] = exps;
				for (int a = 0; a < 6; a++) memcpy(&r[4 + 2 * a], q[a], 8);
				memcpy(&r[16], links, 32);
			}
		}
		if (!wide8OK) wide8.clear(), leafBox.clear();
	}
	// TLAS inner nodes -> pair records appended to the BLAS pairs (children boxes inside the parent's
	// record; child A = leftRight & 0xFFFF, the one tlas::Intersect tests first)
	uint tlasRoot = RT_EMPTY;
	std::vector<uint> tlasSlots; // TLAS node index of every TLAS pair record, in record order
	uint tlasSlotBase = 0;
	if (d->use_tlas) {
		for (uint i = 0; i < d->tlas_nodes_used; i++) {
			const rt_tlas_node& nd = d->tlas_nodes[i];
			if (nd.left_right == 0) { if (nd.blas >= d->n_instances && (i != 0 || d->tlas_nodes_used == 1)) return fail(c, RT_E_ARG, "rt_upload_scene: tlas node %u instance %u out of range", i, nd.blas); }
			else if ((nd.left_right & 0xFFFF) >= d->tlas_nodes_used || (nd.left_right >> 16) >= d->tlas_nodes_used) return fail(c, RT_E_ARG, "rt_upload_scene: tlas node %u child out of range", i);
		}
		for (uint i = 0; i < d->tlas_nodes_used; i++)
			for (int a = 0; a < 3; a++)
				if (!(std::fabs(d->tlas_nodes[i].aabb_min[a]) <= 1e30f) || !(std::fabs(d->tlas_nodes[i].aabb_max[a]) <= 1e30f))
					return fail(c, RT_E_UNSUPPORTED, "rt_upload_scene: tlas node %u has a non-finite bound or one beyond 1e30", i);
		const uint nT = d->tlas_nodes_used;
		std::vector<uint> slotOf(nT, 0);
		uint next = (uint)(pairs.size() / 16);
		tlasSlotBase = next;
		for (uint i = 0; i < nT; i++) if (d->tlas_nodes[i].left_right != 0) slotOf[i] = next++, tlasSlots.push_back(i);
		auto tlink = [&](uint i) -> uint { const rt_tlas_node& nd = d->tlas_nodes[i]; return nd.left_right == 0 ? (RT_INST_BIT | nd.blas) : slotOf[i]; };
		pairs.resize((size_t)next * 16, 0.0f);
		for (uint i = 0; i < nT; i++) {
			const rt_tlas_node& nd = d->tlas_nodes[i];
			if (nd.left_right == 0) continue;
			const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
			float* rec = &pairs[(size_t)slotOf[i] * 16];
			for (int s = 0; s < 2; s++) {
				const rt_tlas_node& cn = d->tlas_nodes[ch[s]];
				const uint lk = tlink(ch[s]);
				memcpy(rec + 8 * s, cn.aabb_min, 12), memcpy(rec + 8 * s + 3, &lk, 4);
				memcpy(rec + 8 * s + 4, cn.aabb_max, 12);
			}
		}
		tlasRoot = tlink(0);
	}
	DScene S;
	memset(&S, 0, sizeof(S));
	float* dp = nullptr;
	HIPCHK(c, dalloc(c->sceneAllocs, &dp, pairs.size() + 16));
	HIPCHK(c, hipMemcpy(dp, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
	S.pairs = (const float4*)dp;

	HIPCHK(c, dalloc(c->sceneAllocs, &dp, prims.size() + 16));
	HIPCHK(c, hipMemcpy(dp, prims.data(), prims.size() * 4, hipMemcpyHostToDevice));
	S.prims = (const float4*)dp;
	S.rootLink = d->use_tlas ? tlasRoot : rootLink[0];
	if (!wide.empty() || wideOK) {
		HIPCHK(c, dalloc(c->sceneAllocs, &dp, wide.size() + 32));
		if (!wide.empty()) HIPCHK(c, hipMemcpy(dp, wide.data(), wide.size() * 4, hipMemcpyHostToDevice));
		S.wide = wideOK ? (const float4*)dp : nullptr;
		S.rootWide = rootWide[0];
		c->wideMut = (float4*)dp, c->wideNodes = (int)(wide.size() / 32);
	} else c->wideMut = nullptr, c->wideNodes = 0;
	S.wide8 = nullptr, S.leafBox = nullptr, S.rootWide8 = RT_EMPTY;
	if (wide8OK && !wide8.empty()) {
		uint* dw = nullptr;
		float* dl = nullptr;
		HIPCHK(c, dalloc(c->sceneAllocs, &dw, wide8.size() + 32));
		HIPCHK(c, hipMemcpy(dw, wide8.data(), wide8.size() * 4, hipMemcpyHostToDevice));
		HIPCHK(c, dalloc(c->sceneAllocs, &dl, leafBox.size() + 8));
		if (!leafBox.empty()) HIPCHK(c, hipMemcpy(dl, leafBox.data(), leafBox.size() * 4, hipMemcpyHostToDevice));
		S.wide8 = (const uint4*)dw, S.leafBox = (const float4*)dl, S.rootWide8 = rootWide8[0];
	}
	c->pairsMut = (float4*)S.pairs, c->primsMut = (float4*)S.prims;
	c->primsOrig = nullptr, c->refitLevels = 0, c->animSlots = 0;
	if (!d->use_tlas && d->blas[0].n_prims > 0) {
		// rt_set_time support: a copy of the uploaded leaf records, and the pair records of the scene
		// BVH grouped by depth (children are deeper than their parents) for the bottom-up refit
		const rt_blas& b = d->blas[0];
		std::vector<uint> order;
		std::vector<int> levelStart(1, 0);
		std::vector<uint> level;
		if (b.nodes[0].prim_count == 0) level.push_back(b.nodes[0].left_first / 2);
		while (!level.empty()) {
			std::vector<uint> next;
			for (uint pr : level) {
				order.push_back(pr);
				for (int sI = 0; sI < 2; sI++) { const rt_bvh_node& nd = b.nodes[2 * pr + sI]; if (nd.prim_count == 0) next.push_back(nd.left_first / 2); }
			}
			levelStart.push_back((int)order.size());
			level.swap(next);
		}
		c->refitLevels = (int)levelStart.size() - 1;
		c->refitLevelHost = levelStart;
		c->animSlots = (int)b.n_prims;
		HIPCHK(c, dalloc(c->sceneAllocs, &c->primsOrig, (size_t)b.n_prims * 4));
		HIPCHK(c, hipMemcpy(c->primsOrig, prims.data(), (size_t)b.n_prims * 64, hipMemcpyHostToDevice));
		HIPCHK(c, dalloc(c->sceneAllocs, &c->refitOrder, order.size() + 1));
		HIPCHK(c, hipMemcpy(c->refitOrder, order.data(), order.size() * 4, hipMemcpyHostToDevice));
		HIPCHK(c, dalloc(c->sceneAllocs, &c->refitLevelStart, levelStart.size()));
		HIPCHK(c, hipMemcpy(c->refitLevelStart, levelStart.data(), levelStart.size() * 4, hipMemcpyHostToDevice));
	}
	S.useTLAS = d->use_tlas ? 1 : 0;
	S.stackRows = RT_STACK_ROWS_MAX;

	if (d->use_tlas) {
		std::vector<DInstance> inst(d->n_instances);
		for (uint i = 0; i < d->n_instances; i++) {
			const rt_instance& in = d->instances[i];
			if (in.blas < 0 || (uint)in.blas >= d->n_blas) return fail(c, RT_E_ARG, "rt_upload_scene: instance %u blas %d out of range", i, in.blas);
			memset(&inst[i], 0, sizeof(DInstance));
			memcpy(inst[i].invT, in.inv_transform, 48), memcpy(inst[i].T, in.transform, 48);
			inst[i].rootLink = rootLink[in.blas];
			inst[i].rootWide = rootWide[in.blas];
			inst[i].rootWide8 = wide8OK ? rootWide8[in.blas] : RT_EMPTY;
		}
		DInstance* di = nullptr;
		HIPCHK(c, dalloc(c->sceneAllocs, &di, inst.size()));
		HIPCHK(c, hipMemcpy(di, inst.data(), inst.size() * sizeof(DInstance), hipMemcpyHostToDevice));
		S.inst = di;
		// brute-force primitives in prim-record form
		rt_blas fake;
		memset(&fake, 0, sizeof(fake));
		fake.spheres = d->brute_spheres, fake.n_sph = d->n_brute_spheres, fake.planes = d->brute_planes, fake.n_pla = d->n_brute_planes;
		const uint nb = fake.n_sph + fake.n_pla;
		std::vector<float> brute((size_t)nb * 16 + 16);
		for (uint j = 0; j < nb; j++) pack_prim(&brute[(size_t)j * 16], fake, j, true, d->materials, d->n_materials);
		HIPCHK(c, dalloc(c->sceneAllocs, &dp, brute.size()));
		HIPCHK(c, hipMemcpy(dp, brute.data(), brute.size() * 4, hipMemcpyHostToDevice));
		S.brute = (const float4*)dp;
		S.nBruteSph = (int)fake.n_sph, S.nBrutePla = (int)fake.n_pla;

		// reach[]: per TLAS pair, the world boxes its children's geometry can occupy (rt_scene_dev.h)
		struct Reach { double lo[3], hi[3], a, b; };
		const double big = 1e30, rel = 1.0 / 32768.0;
		auto unbounded = [&]() { Reach r; for (int k = 0; k < 3; k++) r.lo[k] = -big, r.hi[k] = big; r.a = 0, r.b = 0; return r; };
		std::vector<Reach> instReach(d->n_instances);
		for (uint i = 0; i < d->n_instances; i++) {
			const rt_instance& in = d->instances[i];
			const rt_blas& b = d->blas[in.blas];
			Reach r = unbounded();
			instReach[i] = r;
			// object-space box of everything a ray can hit in this BLAS: triangles and spheres; a plane is
			// unbounded.  Triangle::Intersect rejects a triangle with N == 0 for every ray with finite D
			// (|dot(N, D)| < t_min), and one with a NaN in N for every ray (t is NaN and fails the final
			// range test) -- the two sentinel triangles a .tri mesh ends with (v0 = v1 = v2 = 999) are such.
			if (b.n_prims == 0 || b.n_pla > 0) continue;
			double lo[3] = { big, big, big }, hi[3] = { -big, -big, -big };
			bool finite = true;
			for (uint j = 0; j < b.n_tri; j++) {
				const rt_triangle& t = b.tris[j];
				if ((t.N[0] == 0 && t.N[1] == 0 && t.N[2] == 0) || t.N[0] != t.N[0] || t.N[1] != t.N[1] || t.N[2] != t.N[2]) continue;
				for (int k = 0; k < 3; k++) {
					lo[k] = std::min(lo[k], (double)std::min(t.v0[k], std::min(t.v1[k], t.v2[k])));
					hi[k] = std::max(hi[k], (double)std::max(t.v0[k], std::max(t.v1[k], t.v2[k])));
					if (!(std::fabs(t.v0[k]) < 1e29f && std::fabs(t.v1[k]) < 1e29f && std::fabs(t.v2[k]) < 1e29f)) finite = false;
				}
			}
			for (uint j = 0; j < b.n_sph; j++) {
				const rt_sphere& q = b.spheres[j];
				const double rr = std::max(std::fabs((double)q.r), std::sqrt(std::fabs((double)q.r2))); // r and r2 are separate inputs
				for (int k = 0; k < 3; k++) {
					lo[k] = std::min(lo[k], (double)q.pos[k] - rr), hi[k] = std::max(hi[k], (double)q.pos[k] + rr);
					if (!(std::fabs(q.pos[k]) < 1e29f && rr < 1e29)) finite = false;
				}
			}
			if (lo[0] > hi[0]) { for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0; } // nothing hittable: an empty box at the origin
			if (!finite) continue;
			// exact inverse of the float matrix the device applies (rows 0-2 of invTransform), in double
			const float* m = in.inv_transform;
			const double A[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } }, tv[3] = { m[3], m[7], m[11] };
			const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
			                   A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
			if (!(std::fabs(det) > 1e-30) || !std::isfinite(det)) continue;
			double Ai[3][3];
			for (int rI = 0; rI < 3; rI++)
				for (int cI = 0; cI < 3; cI++) {
					const int r1 = (cI + 1) % 3, r2 = (cI + 2) % 3, c1 = (rI + 1) % 3, c2 = (rI + 2) % 3;
					Ai[rI][cI] = (A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1]) / det;
				}
			double nA = 0, nAi = 0, lmax = 0, wmax = 0;
			for (int rI = 0; rI < 3; rI++) {
				nA = std::max(nA, std::fabs(A[rI][0]) + std::fabs(A[rI][1]) + std::fabs(A[rI][2]));
				nAi = std::max(nAi, std::fabs(Ai[rI][0]) + std::fabs(Ai[rI][1]) + std::fabs(Ai[rI][2]));
			}
			for (int k = 0; k < 3; k++) r.lo[k] = big, r.hi[k] = -big, lmax = std::max(lmax, std::max(std::fabs(lo[k]), std::fabs(hi[k])) + std::fabs(tv[k]));
			for (int corner = 0; corner < 8; corner++) {
				const double l[3] = { (corner & 1 ? hi[0] : lo[0]) - tv[0], (corner & 2 ? hi[1] : lo[1]) - tv[1], (corner & 4 ? hi[2] : lo[2]) - tv[2] };
				for (int k = 0; k < 3; k++) {
					const double w = Ai[k][0] * l[0] + Ai[k][1] * l[1] + Ai[k][2] * l[2];
					r.lo[k] = std::min(r.lo[k], w), r.hi[k] = std::max(r.hi[k], w);
				}
			}
			for (int k = 0; k < 3; k++) wmax = std::max(wmax, std::max(std::fabs(r.lo[k]), std::fabs(r.hi[k])));
			const double cond = std::max(1.0, nA * nAi);
			r.a = rel * (cond * wmax + nAi * lmax) + 1e-20, r.b = rel * cond;
			if (!(wmax < 1e29) || !std::isfinite(r.a) || !std::isfinite(r.b) || r.a > 1e29 || r.b > 1e10) continue;
			instReach[i] = r;
		}
		const uint nT = d->tlas_nodes_used;
		std::vector<Reach> nodeReach(nT);
		std::vector<char> state(nT, 0); // 0 unseen, 1 open, 2 done
		std::vector<uint> walk;
		if (nT > 0 && d->tlas_nodes[0].left_right != 0) walk.push_back(0);
		while (!walk.empty()) {
			const uint i = walk.back();
			const rt_tlas_node& nd = d->tlas_nodes[i];
			if (nd.left_right == 0) { nodeReach[i] = nd.blas < d->n_instances ? instReach[nd.blas] : unbounded(); state[i] = 2; walk.pop_back(); continue; }
			const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
			if (state[i] == 0) {
				state[i] = 1;
				for (int sI = 0; sI < 2; sI++) {
					if (state[ch[sI]] == 1) return fail(c, RT_E_ARG, "rt_upload_scene: tlas node %u is its own ancestor", ch[sI]);
					if (state[ch[sI]] == 0) walk.push_back(ch[sI]);
				}
				continue;
			}
			Reach r = nodeReach[ch[0]];
			const Reach& o = nodeReach[ch[1]];
			for (int k = 0; k < 3; k++) r.lo[k] = std::min(r.lo[k], o.lo[k]), r.hi[k] = std::max(r.hi[k], o.hi[k]);
			r.a = std::max(r.a, o.a), r.b = std::max(r.b, o.b);
			nodeReach[i] = r, state[i] = 2;
			walk.pop_back();
		}
		const uint tlasBase = (uint)tlasSlots.size() ? tlasSlotBase : 0;
		// the boxes are stored inflated for every world origin with |O|_1 <= originMax: 64 x the extent of
		// the instanced geometry (camera and bounce rays start inside that; a ray from further away is
		// simply not culled)
		double extent = 1.0;
		for (uint i = 0; i < d->n_instances; i++)
			if (instReach[i].b > 0) for (int k = 0; k < 3; k++) extent = std::max(extent, std::max(std::fabs(instReach[i].lo[k]), std::fabs(instReach[i].hi[k])));
		const double originMax = 64.0 * 3.0 * extent;
		std::vector<float> reach((size_t)tlasSlots.size() * 12 + 16, 0.0f);
		for (size_t sI = 0; sI < tlasSlots.size(); sI++) {
			const rt_tlas_node& nd = d->tlas_nodes[tlasSlots[sI]];
			const uint ch[2] = { nd.left_right & 0xFFFFu, nd.left_right >> 16 };
			for (int h = 0; h < 2; h++) {
				const Reach& r = state[ch[h]] == 2 ? nodeReach[ch[h]] : unbounded();
				float* rec = &reach[sI * 12 + 6 * h]; // {min.xyz, max.xyz} of child h
				const double m = r.a + r.b * originMax;
				// round outwards: the float box must contain the inflated double one
				for (int k = 0; k < 3; k++) {
					rec[k] = std::nextafterf((float)std::max(r.lo[k] - m, -big), -INFINITY), rec[3 + k] = std::nextafterf((float)std::min(r.hi[k] + m, big), INFINITY);
				}
			}
		}
		HIPCHK(c, dalloc(c->sceneAllocs, &dp, reach.size()));
		HIPCHK(c, hipMemcpy(dp, reach.data(), reach.size() * 4, hipMemcpyHostToDevice));
		S.reach = (const float4*)dp;
		S.tlasBase = tlasBase;
		S.reachOriginMax = (float)originMax;
		S.tlasPairs = (int)tlasSlots.size();
		S.nInst = (int)d->n_instances;
		// the split of a traversal block's LDS (rt_scene_dev.h RT_LDS_WORDS): as many stack rows as the TLAS copy leaves
		{
			const int words = RT_TLAS_COPY_WORDS(S.tlasPairs, S.nInst);
			const int rows = (RT_LDS_WORDS - ((words + 3) & ~3)) / RT_BLOCK - 6;
			S.tlasLds = rows >= RT_STACK_ROWS_MIN ? 1 : 0;
			S.tlasLds = S.tlasLds && c->knobs.tlasLds;
			if (S.tlasLds) S.stackRows = rows < RT_STACK_ROWS_MAX ? rows : RT_STACK_ROWS_MAX;
		}
	}
	std::vector<DLight> lights(d->n_lights ? d->n_lights : 1);
	for (uint i = 0; i < d->n_lights; i++) {
		const rt_light& l = d->lights[i];
		DLight& o = lights[i];
		o.kind = l.kind, o.objIdx = l.obj_idx, o.strength = l.strength, o.radius = l.radius, o.sinAngle = l.sin_angle;
		memcpy(o.pos, l.pos, 12), memcpy(o.col, l.col, 12), memcpy(o.normal, l.normal, 12);
	}
	DLight* dl = nullptr;
	HIPCHK(c, dalloc(c->sceneAllocs, &dl, lights.size()));
	HIPCHK(c, hipMemcpy(dl, lights.data(), lights.size() * sizeof(DLight), hipMemcpyHostToDevice));
	S.lights = dl, S.nLights = (int)d->n_lights;
	std::vector<DMaterial> mats(d->n_materials ? d->n_materials : 1);
	for (uint i = 0; i < d->n_materials; i++) {
		const rt_material& m = d->materials[i];
		DMaterial& o = mats[i];
		o.type = m.type, o.raytracer = m.raytracer, o.specu = m.specu, o.diffu = m.diffu, o.shinieness = m.shinieness, o.N = m.N, o.ir = m.ir;
		memcpy(o.col, m.col, 12), memcpy(o.albedo, m.albedo, 12), memcpy(o.absorption, m.absorption, 12);
	}
	c->matTypes.clear();
	for (size_t i = 0; i < mats.size(); i++) c->matTypes.push_back(mats[i].type);
	DMaterial* dm = nullptr;
	HIPCHK(c, dalloc(c->sceneAllocs, &dm, mats.size()));
	HIPCHK(c, hipMemcpy(dm, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
	S.mats = dm, S.nMats = (int)mats.size();
	S.gammaLut = c->knobs.gammaLut ? c->gammaLut : nullptr;
	if (d->sky_pixels && d->sky_w > 0 && d->sky_h > 0 && d->sky_n >= 3) {
		unsigned char* ds = nullptr;
		const size_t nbytes = (size_t)d->sky_w * d->sky_h * d->sky_n;
		HIPCHK(c, dalloc(c->sceneAllocs, &ds, nbytes));
		HIPCHK(c, hipMemcpy(ds, d->sky_pixels, nbytes, hipMemcpyHostToDevice));
		S.sky = ds, S.skyW = d->sky_w, S.skyH = d->sky_h, S.skyN = d->sky_n;
	}
	c->S = S;
	c->blasRootWide8 = rootWide8;
	c->blasRoot = rootLink, c->blasRootWide = wideOK ? rootWide : rootLink, c->nInstances = d->use_tlas ? (int)d->n_instances : 0;
	c->sceneLoaded = true;
	return RT_OK;
}

