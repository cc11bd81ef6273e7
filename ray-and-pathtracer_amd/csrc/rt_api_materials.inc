// rt_set_lights, rt_set_materials, rt_set_sky: the light table, a range of the material table and the skydome replaced in the loaded scene,
// without a re-upload.  The host side of rt_materials.h, which states why the result is byte-equal to a fresh rt_upload_scene of the updated
// description.  Each call refuses on the host before anything is queued, then queues one table copy (and, for a material that changes its
// type, k_retype_prims over every array of primitive records the context keeps) on the context's stream; none of them synchronises, but
// for a page-locked sky image (see rt_set_sky).
// Included by rt_api.hip (one translation unit).
static_assert(sizeof(rt_light) == sizeof(DLight) && sizeof(DLight) == 56, "a light record is the description's, field for field (rt_layout.h pack_tables)");
static_assert(sizeof(rt_material) == sizeof(DMaterial) && sizeof(DMaterial) == 64, "a material record is the description's, field for field (rt_layout.h pack_tables)");

// What the three calls invalidate: the G-buffer (its albedo and light hits), with it the primary-hit and bounce tables, and a captured
// history at every level, as after rt_upload_scene -- every carried sample holds radiance computed under the old lights, materials or sky.
static void look_changed(rt_ctx* c)
{
	c->sceneGen++;
	c->geomGen++, c->shapeGen++, c->topoGen++;
}

int rt_set_lights(rt_ctx* c, const rt_light* lights, uint32_t n_lights)
{
	if (!c || (!lights && n_lights > 0)) return fail(c, RT_E_ARG, "rt_set_lights: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_lights: no scene uploaded");
	if (n_lights > RT_MAX_LIGHTS) return fail(c, RT_E_UNSUPPORTED, "rt_set_lights: %u lights (limit %d)", n_lights, RT_MAX_LIGHTS);
	HIPCHK(c, hipSetDevice(c->device));
	DLight* table = (DLight*)c->S.lights;
	if (c->lightsCap < RT_MAX_LIGHTS) { // the first call: room for every table the call accepts
		HIPCHK(c, dalloc(c->sceneAllocs, &table, (size_t)RT_MAX_LIGHTS));
		c->lightsCap = RT_MAX_LIGHTS;
	}
	// pack_tables' table: n records, or one zeroed record for none.  The host copy is what the device copy is made from: the caller's
	// array has been read here
	DLight none;
	memset(&none, 0, sizeof(none));
	c->lightsHost.assign(n_lights ? n_lights : 1, none);
	if (n_lights) memcpy(c->lightsHost.data(), lights, (size_t)n_lights * sizeof(DLight));
	prof_begin(c, K_QUERY);
	HIPCHK(c, hipMemcpyAsync(table, c->lightsHost.data(), c->lightsHost.size() * sizeof(DLight), hipMemcpyHostToDevice, c->stream));
	prof_end(c);
	c->S.lights = table, c->S.nLights = (int)n_lights; // (the path state's per-light planes follow nLights: ensure_state, ensure_stream_state)
	look_changed(c);
	return RT_OK;
}

int rt_set_materials(rt_ctx* c, uint32_t first, uint32_t count, const rt_material* materials)
{
	if (!c || !materials) return fail(c, RT_E_ARG, "rt_set_materials: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_materials: no scene uploaded");
	// ---- everything that can be refused is refused here, before anything is queued ----
	const uint32_t n = c->nMaterials;
	if (count == 0 || first >= n || count > n - first) return fail(c, RT_E_ARG, "rt_set_materials: materials [%u, %u + %u) of %u (the number of materials cannot change)", first, first, count, n);
	for (uint32_t k = 0; k < count; k++)
		if (materials[k].type < 1 || materials[k].type > 3) return fail(c, RT_E_ARG, "rt_set_materials: material %u has type %d", first + k, materials[k].type);
	// check_path_support's rule over ALL materials of the updated description
	std::vector<rt_material> all = c->matsHost;
	std::copy(materials, materials + count, all.begin() + first);
	SceneLayout L;
	rt_scene_desc d;
	memset(&d, 0, sizeof(d));
	d.materials = all.data(), d.n_materials = n;
	check_path_support(&d, L);
	if (L.pathUnsupported && c->Qt.on)
		return fail(c, RT_E_UNSUPPORTED, "rt_set_materials: with this edit the scene's path mode runs the general kernel (%s), which the Q-learning sampler does not guide; the scene is unchanged", L.pathUnsupportedWhy.c_str());
	bool retype = false;
	for (uint32_t k = 0; k < count; k++) retype = retype || c->matTypes[first + k] != materials[k].type;
	HIPCHK(c, hipSetDevice(c->device));
	// ---- commit: the host's table first (the caller's array has been read here), the device's range from it ----
	c->matsHost.swap(all);
	DMaterial* const table = (DMaterial*)c->S.mats;
	prof_begin(c, K_QUERY);
	HIPCHK(c, hipMemcpyAsync(table + first, &c->matsHost[first], (size_t)count * sizeof(DMaterial), hipMemcpyHostToDevice, c->stream));
	if (retype) {
		// every array of primitive records the context keeps: prims[] of all BLASes, the brute-force records, rt_set_time's originals
		auto over = [&](float4* recs, uint32_t nRecs) { if (recs && nRecs > 0) hipLaunchKernelGGL(k_retype_prims, dim3((nRecs + 255) / 256), dim3(256), 0, c->stream, recs, nRecs, (const DMaterial*)table, c->S.nMats); };
		over(c->primsMut, c->primSlots);
		if (c->S.useTLAS) over((float4*)c->S.brute, (uint32_t)(c->S.nBruteSph + c->S.nBrutePla));
		over(c->primsOrig, (uint32_t)c->animSlots);
	}
	prof_end(c);
	HIPCHK(c, hipGetLastError());
	for (uint32_t k = 0; k < count; k++) c->matTypes[first + k] = materials[k].type;
	c->pathUnsupported = L.pathUnsupported;
	if (L.pathUnsupported) c->pathUnsupportedWhy = L.pathUnsupportedWhy;
	c->layoutScalars[11] = L.pathUnsupported ? 1 : 0;
	look_changed(c);
	return RT_OK;
}

int rt_set_sky(rt_ctx* c, const uint8_t* pixels, int32_t w, int32_t h, int32_t n)
{
	if (!c) return fail(c, RT_E_ARG, "rt_set_sky: null argument");
	if (!c->sceneLoaded) return fail(c, RT_E_STATE, "rt_set_sky: no scene uploaded");
	if (pixels && (w < 1 || h < 1 || n < 3)) return fail(c, RT_E_ARG, "rt_set_sky: a skydome of %d x %d pixels with %d channels (at least 1 x 1 with 3)", w, h, n);
	if (!pixels) { // off: misses return black (the array stays, for the next image that fits it)
		prof_begin(c, K_QUERY), prof_end(c); // (one entry, like every call: nothing is queued between its events)
		c->S.sky = nullptr, c->S.skyW = 0, c->S.skyH = 0, c->S.skyN = 0;
		look_changed(c);
		return RT_OK;
	}
	HIPCHK(c, hipSetDevice(c->device));
	const size_t nbytes = (size_t)w * (size_t)h * (size_t)n;
	if (c->skyCap < nbytes) {
		unsigned char* ds = nullptr;
		HIPCHK(c, dalloc(c->sceneAllocs, &ds, nbytes));
		c->skyMut = ds, c->skyCap = nbytes;
	}
	// ordinary memory has been read when hipMemcpyAsync returns; page-locked memory is read when the stream gets there, so for such an
	// image -- and only for one -- the call waits for its copy
	hipPointerAttribute_t at;
	const bool pinned = hipPointerGetAttributes(&at, pixels) == hipSuccess && at.type == hipMemoryTypeHost;
	(void)hipGetLastError(); // (an unregistered pointer is an error to the runtime, not to this call)
	prof_begin(c, K_QUERY);
	HIPCHK(c, hipMemcpyAsync(c->skyMut, pixels, nbytes, hipMemcpyHostToDevice, c->stream));
	prof_end(c);
	if (pinned) HIPCHK(c, hipStreamSynchronize(c->stream));
	c->S.sky = c->skyMut, c->S.skyW = w, c->S.skyH = h, c->S.skyN = n;
	look_changed(c);
	return RT_OK;
}
