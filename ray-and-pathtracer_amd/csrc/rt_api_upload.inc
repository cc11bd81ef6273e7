// rt_upload_scene: the layout build_layout (rt_layout.h) makes of the reference-shaped arrays of include/rt_amd.h, copied to HBM and named in
// DScene and the context; and the device-free entry points: rt_layout_*, which hand the same layout to the caller, and rt_launch_form (rt_forms.h).  Host code only.
// Included by rt_api.hip (one translation unit).

// scene_array (rt_ctx.h): a vector copied into a new array of the scene pool
#define SCENE_ARRAY(...) do { const int rc_ = scene_array(c, __VA_ARGS__); if (rc_ != RT_OK) return rc_; } while (0)

// RT_LAYOUT_SCALARS (include/rt_amd.h): the 14 words, in their documented order
static void layout_scalars(const SceneLayout& L, int32_t* out)
{
	int32_t originMaxBits;
	memcpy(&originMaxBits, &L.reachOriginMax, 4);
	const int32_t s[14] = { (int32_t)L.root, (int32_t)L.tlasBase, L.tlasPairs, L.nInst, originMaxBits, L.tlasLds, L.stackRows, L.nBruteSph, L.nBrutePla,
	                        L.wideOK, L.wide8OK, L.pathUnsupported, L.animSlots, L.refitLevels };
	memcpy(out, s, sizeof(s));
}

// What rt_set_instances (rt_api_instances.inc) needs of a TLAS scene, kept at upload: see rt_ctx.h InstanceState
static int instances_keep(rt_ctx* c, const rt_scene_desc* d, const SceneLayout& L, DInstance* instDev, float* reachDev)
{
	rt_ctx::InstanceState& I = c->instances;
	I = rt_ctx::InstanceState();
	const uint n = d->n_instances;
	const size_t room = RT_TLAS_MAX - (size_t)n; // rt_set_instance_list replaces the list by one of up to RT_TLAS_MAX instances: every array below has room for it from the start
	I.inst = L.inst, I.instMut = instDev, I.reachMut = reachDev;
	I.rootWide = L.rootWide, I.rootWide8 = L.rootWide8, I.wide8OK = L.wide8OK; // pack_instances' words, per BLAS
	I.blasOf.resize(n), I.reach.resize(n), I.boundsKnown.assign(n, 0);
	I.objBox.resize(d->n_blas), I.blasBox6.resize((size_t)6 * d->n_blas);
	for (uint k = 0; k < d->n_blas; k++) {
		I.objBox[k] = blas_object_box(d->blas[k]);
		// bvh::bounds (bvh.cpp:48-49): an empty box grown by node 0's two corners
		const rt_bvh_node& r = d->blas[k].nodes[0];
		for (int a = 0; a < 3; a++) {
			float lo = 1e30f, hi = -1e30f;
			lo = lo < r.aabb_min[a] ? lo : r.aabb_min[a], hi = hi > r.aabb_min[a] ? hi : r.aabb_min[a];
			lo = lo < r.aabb_max[a] ? lo : r.aabb_max[a], hi = hi > r.aabb_max[a] ? hi : r.aabb_max[a];
			I.blasBox6[6 * k + a] = lo, I.blasBox6[6 * k + 3 + a] = hi;
		}
	}
	for (uint i = 0; i < n; i++) I.blasOf[i] = d->instances[i].blas, I.reach[i] = instance_reach(I.objBox[d->instances[i].blas], d->instances[i].inv_transform);
	// an untouched instance keeps the box of its leaf in the uploaded TLAS (the first one in node order)
	std::vector<float> b6((size_t)6 * n, 0.0f);
	I.uploaded.assign(d->tlas_nodes, d->tlas_nodes + d->tlas_nodes_used);
	for (uint i = d->tlas_nodes_used; i-- > 0;) {
		const rt_tlas_node& nd = d->tlas_nodes[i];
		if (nd.left_right != 0 || nd.blas >= n || (i == 0 && d->tlas_nodes_used > 1)) continue;
		memcpy(&b6[6 * nd.blas], nd.aabb_min, 12), memcpy(&b6[6 * nd.blas + 3], nd.aabb_max, 12);
		I.boundsKnown[nd.blas] = 1;
	}
	SCENE_ARRAY(&I.bounds, b6, 6 * room);
	SCENE_ARRAY(&I.blasBox, I.blasBox6);
	SCENE_ARRAY(&I.blasOfDev, I.blasOf, room);
	HIPCHK(c, dalloc(c->sceneAllocs, &I.tlasKeep, (size_t)2 * RT_TLAS_MAX + 1));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.boundsNew, (size_t)6 * RT_TLAS_MAX));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.nodesNew, (size_t)2 * RT_TLAS_MAX + 1));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.used, 1));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.reachIn, (size_t)RT_TLAS_MAX));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.xform, (size_t)12 * RT_TLAS_MAX));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.which, (size_t)RT_TLAS_MAX));
	HIPCHK(c, dalloc(c->sceneAllocs, &I.boxUndo, 6));
	return RT_OK;
}

// What rt_set_triangles (rt_api_triangles.inc) needs of every BLAS, kept at upload: see rt_ctx.h BlasKeep.  The ranges are pack_blas's
// (nodes_used / 2 pair records and n_prims slots per BLAS, in BLAS order).
static int triangles_keep(rt_ctx* c, const rt_scene_desc* d, const SceneLayout& L)
{
	c->blasKeep.assign(d->n_blas, rt_ctx::BlasKeep());
	c->slotOf = nullptr, c->refitOrderAll = nullptr, c->refitLevelAll = nullptr;
	c->triStage = nullptr, c->triStageCap = 0, c->undoPairs = nullptr, c->undoPrims = nullptr, c->undoPairCap = 0, c->undoPrimCap = 0;
	c->vtxStage = nullptr, c->vtxStageCap = 0, c->vtxVerdict = nullptr; // (rt_api_vertices.inc; the bound indices go with blasKeep)
	std::vector<uint> slotOf, order;
	std::vector<int> levelAll;
	uint pairOff = 0, primOff = 0;
	for (uint k = 0; k < d->n_blas; k++) {
		const rt_blas& b = d->blas[k];
		rt_ctx::BlasKeep& K = c->blasKeep[k];
		K.pairFirst = pairOff, K.pairCount = b.nodes_used / 2, K.slotFirst = primOff, K.slotCount = b.n_prims, K.nTri = b.n_tri;
		slotOf.resize((size_t)primOff + b.n_prims, 0xFFFFFFFFu);
		for (uint j = 0; j < b.n_prims; j++) slotOf[(size_t)primOff + b.prim_idx[j]] = primOff + j; // prim_idx[j] < n_prims: pack_blas checked
		if (k == 0 && !d->use_tlas && L.animSlots > 0) { // the scene BVH's order is pack_refit's own (pairOff 0): not walked a second time
			order = L.refitOrder, K.level = L.refitLevelStart;
			K.refittable = order.size() <= (size_t)K.pairCount;
		} else K.refittable = blas_refit_order(b, pairOff, order, K.level);
		K.levelFirst = levelAll.size();
		levelAll.insert(levelAll.end(), K.level.begin(), K.level.end());
		pairOff += K.pairCount, primOff += K.slotCount;
	}
	SCENE_ARRAY(&c->slotOf, slotOf);
	SCENE_ARRAY(&c->refitOrderAll, order, 1);
	SCENE_ARRAY(&c->refitLevelAll, levelAll);
	return RT_OK;
}

int rt_upload_scene(rt_ctx* c, const rt_scene_desc* d)
{
	if (!c || !d) return fail(c, RT_E_ARG, "rt_upload_scene: null argument");
	c->sceneGen++; // the G-buffer (rt_render_aovs) is stale from here on, whatever the outcome
	c->geomGen++, c->shapeGen++, c->topoGen++;  // ... and so is a captured history (rt_history_capture), at every level
	HIPCHK(c, hipSetDevice(c->device));
	SceneLayout L;
	std::string err;
	int rc = check_desc(d, err); // refused with the old scene still loaded; everything later is refused without one
	if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->mega.pick = {}; // another scene: the Whitted forms are timed again
	free_pool(c->sceneAllocs);
	c->sceneLoaded = false;
	c->instances = rt_ctx::InstanceState();
	LayoutKnobs knobs;
	knobs.wide = c->knobs.wide, knobs.wide8 = c->knobs.wide8, knobs.tlasLds = c->knobs.tlasLds;
	rc = build_layout(d, knobs, L, err);
	c->pathUnsupported = L.pathUnsupported;
	if (L.pathUnsupported) c->pathUnsupportedWhy = L.pathUnsupportedWhy;
	if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());

	DScene S;
	memset(&S, 0, sizeof(S));
	float* dp = nullptr;
	// rt_set_instances rebuilds the TLAS as tlas::build's, n pair records for n instances (rt_instances.h), and rt_set_instance_list
	// replaces the list by one of up to RT_TLAS_MAX: the tail of pairs[] and reach[] have room for that many records from the start
	const size_t tlasRoom = d->use_tlas && RT_TLAS_MAX > L.tlasPairs ? (size_t)(RT_TLAS_MAX - L.tlasPairs) : 0;
	SCENE_ARRAY(&dp, L.pairs, 16 + tlasRoom * 16);
	S.pairs = (const float4*)dp;
	SCENE_ARRAY(&dp, L.prims, 16);
	S.prims = (const float4*)dp;
	S.rootLink = L.root;
	if (!L.wide.empty() || L.wideOK) { // (wideOK without a record, every root a leaf: an array of slack alone)
		SCENE_ARRAY(&dp, L.wide, 32);
		S.wide = L.wideOK ? (const float4*)dp : nullptr;
		S.rootWide = L.rootWide[0];
		c->wideMut = (float4*)dp, c->wideNodes = (int)(L.wide.size() / 32);
	} else c->wideMut = nullptr, c->wideNodes = 0;
	S.wide8 = nullptr, S.leafBox = nullptr, S.rootWide8 = RT_EMPTY;
	if (L.wide8OK && !L.wide8.empty()) {
		uint* dw = nullptr;
		SCENE_ARRAY(&dw, L.wide8, 32);
		SCENE_ARRAY(&dp, L.leafBox, 8);
		S.wide8 = (const uint4*)dw, S.leafBox = (const float4*)dp, S.rootWide8 = L.rootWide8[0];
	}
	c->pairsMut = (float4*)S.pairs, c->primsMut = (float4*)S.prims;
	{ const int rc_ = triangles_keep(c, d, L); if (rc_ != RT_OK) return rc_; }
	c->primsOrig = nullptr, c->refitLevels = L.refitLevels, c->animSlots = L.animSlots;
	if (L.animSlots > 0) {
		// rt_set_time support: a copy of the uploaded leaf records, and the refit order
		c->refitLevelHost = L.refitLevelStart;
		HIPCHK(c, dalloc(c->sceneAllocs, &c->primsOrig, (size_t)L.animSlots * 4));
		HIPCHK(c, hipMemcpy(c->primsOrig, L.prims.data(), (size_t)L.animSlots * 64, hipMemcpyHostToDevice));
		SCENE_ARRAY(&c->refitOrder, L.refitOrder, 1);
		SCENE_ARRAY(&c->refitLevelStart, L.refitLevelStart);
	}
	S.useTLAS = d->use_tlas ? 1 : 0;
	S.stackRows = L.stackRows;
	if (d->use_tlas) {
		DInstance* di = nullptr;
		SCENE_ARRAY(&di, L.inst, RT_TLAS_MAX - L.inst.size()); // (check_desc: at most RT_TLAS_MAX instances)
		S.inst = di;
		SCENE_ARRAY(&dp, L.brute);
		S.brute = (const float4*)dp;
		S.nBruteSph = L.nBruteSph, S.nBrutePla = L.nBrutePla;
		SCENE_ARRAY(&dp, L.reach, tlasRoom * 12);
		S.reach = (const float4*)dp;
		const int rc_ = instances_keep(c, d, L, di, dp);
		if (rc_ != RT_OK) return rc_;
		S.tlasBase = L.tlasBase, S.reachOriginMax = L.reachOriginMax, S.tlasPairs = L.tlasPairs, S.nInst = L.nInst, S.tlasLds = L.tlasLds;
	}
	DLight* dl = nullptr;
	SCENE_ARRAY(&dl, L.lights);
	S.lights = dl, S.nLights = (int)d->n_lights;
	c->matTypes.clear();
	for (size_t i = 0; i < L.mats.size(); i++) c->matTypes.push_back(L.mats[i].type);
	DMaterial* dm = nullptr;
	SCENE_ARRAY(&dm, L.mats);
	S.mats = dm, S.nMats = (int)L.mats.size();
	// what rt_set_lights / rt_set_materials / rt_set_sky (rt_api_materials.inc) start from
	c->matsHost.assign(d->materials, d->materials + d->n_materials), c->nMaterials = d->n_materials;
	c->lightsHost = L.lights, c->lightsCap = 0;
	c->primSlots = (uint32_t)(L.prims.size() / 16);
	c->skyMut = nullptr, c->skyCap = 0;
	S.gammaLut = c->knobs.gammaLut ? c->gammaLut : nullptr;
	if (d->sky_pixels && d->sky_w > 0 && d->sky_h > 0 && d->sky_n >= 3) {
		unsigned char* ds = nullptr;
		const size_t nbytes = (size_t)d->sky_w * d->sky_h * d->sky_n;
		HIPCHK(c, dalloc(c->sceneAllocs, &ds, nbytes));
		HIPCHK(c, hipMemcpy(ds, d->sky_pixels, nbytes, hipMemcpyHostToDevice));
		S.sky = ds, S.skyW = d->sky_w, S.skyH = d->sky_h, S.skyN = d->sky_n;
		c->skyMut = ds, c->skyCap = nbytes;
	}
	c->S = S;
	c->blasPairs = (uint)(L.pairs.size() / 16) - (uint)L.tlasPairs;
	layout_scalars(L, c->layoutScalars);
	c->blasRootWide8 = L.rootWide8;
	c->blasRoot = L.rootLink, c->blasRootWide = L.wideOK ? L.rootWide : L.rootLink, c->nInstances = d->use_tlas ? (int)d->n_instances : 0;
	c->sceneLoaded = true;
	return RT_OK;
}

// ---- the layout without a device (include/rt_amd.h rt_layout_*) ------------------------------------------
struct rt_layout {
	SceneLayout L;
	int32_t scalars[14];
};
rt_layout* rt_layout_build(const rt_scene_desc* d, int wide, int wide8, int tlas_lds)
{
	if (!d) { fail(nullptr, RT_E_ARG, "rt_layout_build: null argument"); return nullptr; }
	rt_layout* o = new rt_layout();
	SceneLayout& L = o->L;
	LayoutKnobs knobs;
	knobs.wide = wide, knobs.wide8 = wide8, knobs.tlasLds = tlas_lds;
	std::string err;
	const int rc = build_layout(d, knobs, L, err);
	if (rc != RT_OK) { fail(nullptr, rc, "%s", err.c_str()); delete o; return nullptr; }
	layout_scalars(L, o->scalars);
	return o;
}
int rt_layout_array(const rt_layout* o, int which, const void** data, size_t* bytes)
{
	if (!o || !data || !bytes) return fail(nullptr, RT_E_ARG, "rt_layout_array: null argument");
	const SceneLayout& L = o->L;
#define ARR(v) { (v).data(), (v).size() * sizeof((v)[0]) }
	const struct { const void* p; size_t n; } arrays[] = { ARR(L.pairs), ARR(L.prims), ARR(L.wide), ARR(L.wide8), ARR(L.leafBox), ARR(L.reach), ARR(L.brute), ARR(L.inst),
		ARR(L.lights), ARR(L.mats), ARR(L.refitOrder), ARR(L.refitLevelStart), ARR(L.rootLink), ARR(L.rootWide), ARR(L.rootWide8), { o->scalars, sizeof(o->scalars) } }; // RT_LAYOUT_* order
#undef ARR
	static_assert(sizeof(arrays) / sizeof(arrays[0]) == RT_LAYOUT_SCALARS + 1, "one entry per RT_LAYOUT_* value");
	if (which >= 0 && which <= RT_LAYOUT_SCALARS) { *data = arrays[which].p, *bytes = arrays[which].n; return RT_OK; }
	return fail(nullptr, RT_E_ARG, "rt_layout_array: array %d", which);
}
void rt_layout_free(rt_layout* o) { delete o; }

// ---- the launch forms without a device (include/rt_amd.h rt_launch_form; csrc/rt_forms.h) ------------------
int rt_launch_form(const int32_t* facts, int round, int32_t* out)
{
	if (!facts || !out) return fail(nullptr, RT_E_ARG, "rt_launch_form: null argument");
	const DenseBatch b{ facts[0] != 0, facts[1] != 0, facts[2], facts[3] != 0, facts[4], facts[5] != 0, facts[6] != 0, facts[7] };
	if (b.chainLevels < 1 || b.chainLevels > 4 || b.rounds < 1 || round < 0 || round >= b.rounds) return fail(nullptr, RT_E_ARG, "rt_launch_form: round %d of %d, %d chain levels", round, b.rounds, b.chainLevels);
	const int f = shade_form(b, round);
	if (!kShadeS[f]) return fail(nullptr, RT_E_STATE, "rt_launch_form: no k_shade_s of form %d (round %d of %d)", f, round, b.rounds);
	out[0] = generate_form(b), out[1] = f, out[2] = light_form(b, round), out[3] = round > 0 ? light_form(b, round - 1) : -1;
	out[4] = shade_bt(f), out[5] = shade_tab(f) ? 1 : 0, out[6] = shade_masked(f) ? 1 : 0, out[7] = round == 0 ? 1 : 0;
	return RT_OK;
}
int rt_any_hit_walk(int counting, int wide, int wide8) { return any_hit_walk(counting != 0, wide != 0, wide8 != 0); }
