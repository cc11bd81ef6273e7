// rt_upload_scene: the layout build_layout (rt_layout.h) makes of the reference-shaped arrays of include/rt_amd.h, copied to HBM and named in
// DScene and the context; and the device-free rt_layout_* entry points, which hand the same layout to the caller.  Host code only.
// Included by rt_api.hip (one translation unit).

// scene_array (rt_ctx.h): a vector copied into a new array of the scene pool
#define SCENE_ARRAY(...) do { const int rc_ = scene_array(c, __VA_ARGS__); if (rc_ != RT_OK) return rc_; } while (0)

int rt_upload_scene(rt_ctx* c, const rt_scene_desc* d)
{
	if (!c || !d) return fail(c, RT_E_ARG, "rt_upload_scene: null argument");
	c->sceneGen++; // the G-buffer (rt_render_aovs) is stale from here on, whatever the outcome
	c->geomGen++;  // ... and so is a captured history (rt_history_capture)
	HIPCHK(c, hipSetDevice(c->device));
	SceneLayout L;
	std::string err;
	int rc = check_desc(d, err); // refused with the old scene still loaded; everything later is refused without one
	if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->mega.pick = {}; // another scene: the Whitted forms are timed again
	free_pool(c->sceneAllocs);
	c->sceneLoaded = false;
	LayoutKnobs knobs;
	knobs.wide = c->knobs.wide, knobs.wide8 = c->knobs.wide8, knobs.tlasLds = c->knobs.tlasLds;
	rc = build_layout(d, knobs, L, err);
	c->pathUnsupported = L.pathUnsupported;
	if (L.pathUnsupported) c->pathUnsupportedWhy = L.pathUnsupportedWhy;
	if (rc != RT_OK) return fail(c, rc, "%s", err.c_str());

	DScene S;
	memset(&S, 0, sizeof(S));
	float* dp = nullptr;
	SCENE_ARRAY(&dp, L.pairs, 16);
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
		SCENE_ARRAY(&di, L.inst);
		S.inst = di;
		SCENE_ARRAY(&dp, L.brute);
		S.brute = (const float4*)dp;
		S.nBruteSph = L.nBruteSph, S.nBrutePla = L.nBrutePla;
		SCENE_ARRAY(&dp, L.reach);
		S.reach = (const float4*)dp;
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
	S.gammaLut = c->knobs.gammaLut ? c->gammaLut : nullptr;
	if (d->sky_pixels && d->sky_w > 0 && d->sky_h > 0 && d->sky_n >= 3) {
		unsigned char* ds = nullptr;
		const size_t nbytes = (size_t)d->sky_w * d->sky_h * d->sky_n;
		HIPCHK(c, dalloc(c->sceneAllocs, &ds, nbytes));
		HIPCHK(c, hipMemcpy(ds, d->sky_pixels, nbytes, hipMemcpyHostToDevice));
		S.sky = ds, S.skyW = d->sky_w, S.skyH = d->sky_h, S.skyN = d->sky_n;
	}
	c->S = S;
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
	int32_t originMaxBits;
	memcpy(&originMaxBits, &L.reachOriginMax, 4);
	const int32_t s[14] = { (int32_t)L.root, (int32_t)L.tlasBase, L.tlasPairs, L.nInst, originMaxBits, L.tlasLds, L.stackRows, L.nBruteSph, L.nBrutePla,
	                        L.wideOK, L.wide8OK, L.pathUnsupported, L.animSlots, L.refitLevels };
	memcpy(o->scalars, s, sizeof(s));
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
