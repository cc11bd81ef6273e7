// ORACLE (test infrastructure, NOT product code) -- parity unpinned, see oracle/README.md.
//
// C entry points over the CPU restatement so that tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg can drive it through ctypes.  Nothing in the product path links or loads this.
#include "orc_render.h"
#include <omp.h>

using namespace orc;

struct OrcScene {
	Scene sc;
	std::string err;
};
struct OrcRenderer {
	Renderer r;
};

static float3 f3(const float* p) { return float3(p[0], p[1], p[2]); }

extern "C" {

void* orc_scene_new() { return new OrcScene(); }
void orc_scene_free(void* h)
{
	OrcScene* s = (OrcScene*)h;
	if (!s) return;
	delete s->sc.b;
	delete s->sc.tl;
	for (auto* p : s->sc.instances) delete p;
	for (auto* p : s->sc.blasList) delete p;
	delete s;
}
const char* orc_last_error(void* h) { return ((OrcScene*)h)->err.c_str(); }

// diffuse(a, c, ks, kd, n, rt, e, s) -- template/scene.h:595-601
int orc_add_diffuse(void* h, const float* albedo, const float* col, float ks, float kd, int n, float emission, float shininess, int rt)
{
	Scene& sc = ((OrcScene*)h)->sc;
	Material m;
	m.type = DIFFUSE, m.albedo = f3(albedo), m.col = f3(col), m.specu = ks, m.diffu = kd, m.N = n;
	m.emission = float3(emission), m.shinieness = shininess, m.raytracer = rt != 0;
	sc.materials.push_back(m);
	return (int)sc.materials.size() - 1;
}
// metal(f, c, rt) -- template/scene.h:629
int orc_add_metal(void* h, float fuzzy, const float* col, int rt)
{
	Scene& sc = ((OrcScene*)h)->sc;
	Material m;
	m.type = METAL, m.col = f3(col), m.fuzzy = fuzzy < 1 ? fuzzy : 1, m.raytracer = rt != 0;
	sc.materials.push_back(m);
	return (int)sc.materials.size() - 1;
}
// glass(refIndex, c, a, r, n, rt) -- template/scene.h:643-646
int orc_add_glass(void* h, float ir, const float* col, const float* absorption, int rt)
{
	Scene& sc = ((OrcScene*)h)->sc;
	Material m;
	m.type = GLASS, m.col = f3(col), m.ir = ir, m.invIr = 1 / ir, m.absorption = f3(absorption), m.raytracer = rt != 0;
	sc.materials.push_back(m);
	return (int)sc.materials.size() - 1;
}
// AreaLight(idx, p, str, c, r, n, s, rt) -- template/scene.h:97-103
int orc_add_area_light(void* h, int idx, const float* pos, float strength, const float* col, float radius, const float* normal)
{
	Scene& sc = ((OrcScene*)h)->sc;
	Light l;
	l.kind = 0, l.objIdx = idx, l.pos = f3(pos), l.strength = strength, l.col = f3(col), l.normal = f3(normal);
	l.radius = radius, l.radius2 = radius * radius, l.area = 2 * l.radius2 * PI, l.raytracer = sc.raytracer;
	sc.lights.push_back(l);
	return (int)sc.lights.size() - 1;
}
// DirectionalLight(idx, p, str, c, n, r, rt) -- template/scene.h:146-148
int orc_add_dir_light(void* h, int idx, const float* pos, float strength, const float* col, const float* normal, float r)
{
	Scene& sc = ((OrcScene*)h)->sc;
	Light l;
	l.kind = 1, l.objIdx = idx, l.pos = f3(pos), l.strength = strength, l.col = f3(col), l.normal = f3(normal);
	l.sinAngle = x_sinf(r * PI / 2), l.raytracer = sc.raytracer;
	sc.lights.push_back(l);
	return (int)sc.lights.size() - 1;
}
int orc_add_sphere(void* h, int idx, int mat, const float* pos, float r)
{
	Scene& sc = ((OrcScene*)h)->sc;
	sc.spheres.push_back(Sphere(idx, mat, f3(pos), r));
	return (int)sc.spheres.size() - 1;
}
int orc_add_plane(void* h, int idx, int mat, const float* N, float d)
{
	Scene& sc = ((OrcScene*)h)->sc;
	sc.planes.push_back(Plane(idx, mat, f3(N), d));
	return (int)sc.planes.size() - 1;
}
int orc_add_mesh_raw(void* h, int group, int mat, const float* v9, int n)
{
	Scene& sc = ((OrcScene*)h)->sc;
	sc.meshes.push_back(Mesh(group, mat, v9, n));
	return (int)sc.meshes.size() - 1;
}
int orc_add_mesh_obj(void* h, int group, const char* path, int mat, const float* pos, float scale)
{
	OrcScene* s = (OrcScene*)h;
	Mesh m;
	if (!Mesh::LoadObj(m, group, path, mat, f3(pos), scale)) { s->err = std::string("cannot load obj ") + path; return -1; }
	s->sc.meshes.push_back(m);
	return (int)s->sc.meshes.size() - 1;
}
int orc_add_mesh_tri(void* h, int group, const char* path, int mat)
{
	OrcScene* s = (OrcScene*)h;
	Mesh m;
	if (!Mesh::LoadTri(m, group, path, mat)) { s->err = std::string("cannot load tri ") + path; return -1; }
	s->sc.meshes.push_back(m);
	return (int)s->sc.meshes.size() - 1;
}
int orc_mesh_count(void* h, int mesh) { return (int)((OrcScene*)h)->sc.meshes[mesh].tri.size(); }
// per triangle: v0 v1 v2 N centroid (15 floats) and objIdx
void orc_mesh_get(void* h, int mesh, float* out15, int* outIdx)
{
	const Mesh& m = ((OrcScene*)h)->sc.meshes[mesh];
	for (size_t i = 0; i < m.tri.size(); i++) {
		const Triangle& t = m.tri[i];
		const float3* src[5] = { &t.v0, &t.v1, &t.v2, &t.N, &t.centroid };
		for (int k = 0; k < 5; k++) { out15[15 * i + 3 * k] = src[k]->x; out15[15 * i + 3 * k + 1] = src[k]->y; out15[15 * i + 3 * k + 2] = src[k]->z; }
		outIdx[i] = t.objIdx;
	}
}
int orc_set_sky(void* h, int w, int hgt, int n, const unsigned char* px)
{
	Scene& sc = ((OrcScene*)h)->sc;
	sc.skydomeX = w, sc.skydomeY = hgt, sc.skydomeN = n;
	sc.skydome.assign(px, px + (size_t)w * hgt * n);
	return 0;
}
// Scene::toogleRaytracer semantics: lights follow the scene flag, materials keep theirs
void orc_set_raytracer(void* h, int rt)
{
	Scene& sc = ((OrcScene*)h)->sc;
	if (sc.raytracer != (rt != 0)) sc.toogleRaytracer();
}

void orc_set_time(void* h, float t) { ((OrcScene*)h)->sc.SetTime(t); }

// non-TLAS scene: new bvh(this); Build(false) -- template/scene.h:700-702
int orc_build(void* h, int splitMethod)
{
	Scene& sc = ((OrcScene*)h)->sc;
	delete sc.b;
	sc.useTLAS = false;
	sc.b = new bvh(&sc);
	sc.b->splitMethod = splitMethod;
	sc.b->Build();
	return 0;
}
// TLAS scene in the style of TLASSceneTest2 (template/scene.h:941-972): one bvh per referenced
// mesh, one bvhInstance per (mesh, transform), then tlas::build
int orc_build_tlas(void* h, int splitMethod, int nInst, const int* meshIdx, const float* transforms)
{
	OrcScene* s = (OrcScene*)h;
	Scene& sc = s->sc;
	sc.useTLAS = true;
	std::vector<int> blasOfMesh(sc.meshes.size(), -1);
	for (int i = 0; i < nInst; i++) {
		int mi = meshIdx[i];
		if (mi < 0 || mi >= (int)sc.meshes.size()) { s->err = "bad mesh index"; return -1; }
		if (blasOfMesh[mi] < 0) {
			bvh* b = new bvh(&sc.meshes[mi]);
			b->splitMethod = splitMethod;
			b->Build();
			blasOfMesh[mi] = (int)sc.blasList.size();
			sc.blasList.push_back(b);
		}
		bvhInstance* inst = new bvhInstance(sc.blasList[blasOfMesh[mi]]);
		inst->blasIdx = blasOfMesh[mi];
		mat4 T;
		memcpy(T.cell, transforms + 16 * i, 64);
		inst->SetTransform(T);
		sc.instances.push_back(inst);
	}
	sc.tl = new tlas(sc.instances);
	if (!sc.tl->build()) { s->err = "tlas build failed (1..256 instances)"; return -1; }
	return 0;
}

static const bvh* pick_bvh(const Scene& sc, int blas) { return blas < 0 ? sc.b : sc.blasList[blas]; }
int orc_blas_count(void* h) { return (int)((OrcScene*)h)->sc.blasList.size(); }
// info[0..6] = nodesUsed, N, NTri, NSph, NPla, maxDepth, allocated nodes
void orc_bvh_info(void* h, int blas, int* info)
{
	const bvh* b = pick_bvh(((OrcScene*)h)->sc, blas);
	info[0] = b->nodesUsed, info[1] = b->N, info[2] = b->NTri, info[3] = b->NSph, info[4] = b->NPla, info[5] = b->maxDepth, info[6] = (int)b->bvhNode.size();
}
// nodes: nodesUsed records of 32 bytes (reference BVHNode layout); primIdx: N uints
void orc_bvh_get(void* h, int blas, void* nodes, unsigned* primIdx)
{
	const bvh* b = pick_bvh(((OrcScene*)h)->sc, blas);
	memcpy(nodes, b->bvhNode.data(), (size_t)b->nodesUsed * sizeof(BVHNode));
	memcpy(primIdx, b->primitiveIdx.data(), (size_t)b->N * 4);
}
int orc_tlas_nodes_used(void* h) { return (int)((OrcScene*)h)->sc.tl->nodesUsed; }
void orc_tlas_get(void* h, void* nodes) { const tlas* t = ((OrcScene*)h)->sc.tl; memcpy(nodes, t->tlasNode.data(), (size_t)t->nodesUsed * sizeof(TLASNode)); }
// per instance: blas index, transform[16], invTransform[16], bounds min/max [6]
void orc_instance_get(void* h, int i, int* blas, float* T, float* invT, float* bounds)
{
	const bvhInstance* in = ((OrcScene*)h)->sc.instances[i];
	*blas = in->blasIdx;
	memcpy(T, in->matTransform.cell, 64);
	memcpy(invT, in->invTransform.cell, 64);
	bounds[0] = in->bounds.bmin.x, bounds[1] = in->bounds.bmin.y, bounds[2] = in->bounds.bmin.z;
	bounds[3] = in->bounds.bmax.x, bounds[4] = in->bounds.bmax.y, bounds[5] = in->bounds.bmax.z;
}

static void counters_out(const Counters& c, unsigned long long* out)
{
	if (!out) return;
	out[0] = c.inner_visits, out[1] = c.prim_tests, out[2] = c.tlas_inner, out[3] = c.instance_visits;
	out[4] = c.rays_nearest, out[5] = c.rays_occluded, out[6] = c.brute_tests, out[7] = c.light_tests;
	out[8] = c.tri_intersect_calls;
}

// Scene::FindNearest on n rays (O, D: n*3 floats; tmax: n floats or NULL for 1e34f).
// Outputs: t, objIdx, material index, hit normal.
int orc_find_nearest_batch(void* h, int n, const float* O, const float* D, const float* tmax, float t_min,
                           float* outT, int* outObj, int* outMat, float* outN, unsigned long long* counters)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		sc.FindNearest(r, t_min, cnt);
		outT[i] = r.t, outObj[i] = r.objIdx;
		if (outMat) outMat[i] = r.objIdx == -1 ? -1 : r.mat;
		if (outN) { outN[3 * i] = r.hitNormal.x, outN[3 * i + 1] = r.hitNormal.y, outN[3 * i + 2] = r.hitNormal.z; }
	}
	counters_out(cnt, counters);
	return 0;
}
// The queries below Scene level: scope 1 = the scene's accelerator alone (bvh::Intersect of the scene bvh / tlas::Intersect:
// no lights, no brute-force primitives), 2 = bvh::Intersect of BLAS 'index' in its own object space, 3 =
// bvhInstance::BIntersect of instance 'index' (bvh.cpp:596-604, tlas.cpp:65-122, bvhInstance.cpp:3-35).
int orc_scope_nearest(void* h, int scope, int index, int n, const float* O, const float* D, const float* tmax,
                      float* outT, int* outObj, int* outMat, float* outN)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		r.objIdx = -1;
		if (scope == 1) { if (sc.useTLAS) sc.tl->Intersect(r, cnt); else sc.b->Intersect(r, cnt); }
		else if (scope == 2) (sc.useTLAS ? sc.blasList[index] : sc.b)->Intersect(r, cnt);
		else sc.instances[index]->BIntersect(r, cnt);
		outT[i] = r.t, outObj[i] = r.objIdx, outMat[i] = r.objIdx == -1 ? -1 : r.mat;
		outN[3 * i] = r.hitNormal.x, outN[3 * i + 1] = r.hitNormal.y, outN[3 * i + 2] = r.hitNormal.z;
	}
	return 0;
}
int orc_scope_occluded(void* h, int scope, int index, int n, const float* O, const float* D, const float* tmax, unsigned char* out)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		bool o;
		if (scope == 1) o = sc.useTLAS ? sc.tl->IsOccluded(r, cnt) : sc.b->IsOccluded(r, cnt);
		else if (scope == 2) o = (sc.useTLAS ? sc.blasList[index] : sc.b)->IsOccluded(r, cnt);
		else o = sc.instances[index]->IsOccluded(r, cnt);
		out[i] = o ? 1 : 0;
	}
	return 0;
}
// The peak stack pointers of each ray's walk (Counters::sp_blas, sp_tlas, sp_stacked: peaks[3 * i ..]), for the query orc_find_nearest_batch
// (scope 0, with t_min) or orc_scope_nearest (scope 1 .. 3) makes of it.  A tally: the walks are the ones above, their results are not returned.
static void peaks_out(const Counters& c, unsigned* p) { p[0] = c.sp_blas, p[1] = c.sp_tlas, p[2] = c.sp_stacked; }
int orc_peaks_nearest(void* h, int scope, int index, int n, const float* O, const float* D, const float* tmax, float t_min, unsigned* peaks)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		r.objIdx = -1;
		cnt.clear_peaks();
		if (scope == 0) sc.FindNearest(r, t_min, cnt);
		else if (scope == 1) { if (sc.useTLAS) sc.tl->Intersect(r, cnt); else sc.b->Intersect(r, cnt); }
		else if (scope == 2) (sc.useTLAS ? sc.blasList[index] : sc.b)->Intersect(r, cnt);
		else sc.instances[index]->BIntersect(r, cnt);
		peaks_out(cnt, peaks + 3 * i);
	}
	return 0;
}
// ... of orc_is_occluded_batch (scope 0) or orc_scope_occluded (scope 1 .. 3)
int orc_peaks_occluded(void* h, int scope, int index, int n, const float* O, const float* D, const float* tmax, unsigned* peaks)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		cnt.clear_peaks();
		if (scope == 0) sc.IsOccluded(r, cnt);
		else if (scope == 1) { if (sc.useTLAS) sc.tl->IsOccluded(r, cnt); else sc.b->IsOccluded(r, cnt); }
		else if (scope == 2) (sc.useTLAS ? sc.blasList[index] : sc.b)->IsOccluded(r, cnt);
		else sc.instances[index]->IsOccluded(r, cnt);
		peaks_out(cnt, peaks + 3 * i);
	}
	return 0;
}
// Scene::GetSkyColor (template/scene.h:1312-1327) for n directions
void orc_sky_color(void* h, int n, const float* D, float* rgb)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	for (int i = 0; i < n; i++) {
		Ray r(float3(0), f3(D + 3 * i));
		const float3 c = sc.GetSkyColor(r);
		rgb[3 * i] = c.x, rgb[3 * i + 1] = c.y, rgb[3 * i + 2] = c.z;
	}
}
int orc_is_occluded_batch(void* h, int n, const float* O, const float* D, const float* tmax, unsigned char* out, unsigned long long* counters)
{
	const Scene& sc = ((OrcScene*)h)->sc;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax ? tmax[i] : 1e34f);
		out[i] = sc.IsOccluded(r, cnt) ? 1 : 0;
	}
	counters_out(cnt, counters);
	return 0;
}

// ---- renderer ---------------------------------------------------------------------------------
void* orc_renderer_new(void* scene, int w, int hgt)
{
	OrcRenderer* r = new OrcRenderer();
	r->r.scene = &((OrcScene*)scene)->sc;
	r->r.Init(w, hgt);
	return r;
}
void orc_renderer_free(void* h) { delete (OrcRenderer*)h; }
void orc_renderer_set_camera(void* h, const float* camPos, const float* TL, const float* TR, const float* BL, int fisheye, float viewAngle, float yAngle)
{
	Camera& c = ((OrcRenderer*)h)->r.camera;
	c.camPos = f3(camPos), c.topLeft = f3(TL), c.topRight = f3(TR), c.bottomLeft = f3(BL);
	c.fishEye = fisheye != 0, c.viewAngle = viewAngle, c.yAngle = yAngle;
}
void orc_renderer_get_camera(void* h, float* out12)
{
	const Camera& c = ((OrcRenderer*)h)->r.camera;
	const float3* v[4] = { &c.camPos, &c.topLeft, &c.topRight, &c.bottomLeft };
	for (int k = 0; k < 4; k++) out12[3 * k] = v[k]->x, out12[3 * k + 1] = v[k]->y, out12[3 * k + 2] = v[k]->z;
}
void orc_renderer_clear(void* h)
{
	Renderer& r = ((OrcRenderer*)h)->r;
	std::fill(r.accumulator.begin(), r.accumulator.end(), float4{ 0, 0, 0, 0 });
	r.iterationNumber = 1;
}
// The pixel loop of Renderer::Tick for frames [frame0, frame0+nframes), rows [y0, y1).
// Mode follows the scene's raytracer flag.  nthreads <= 0: OpenMP default.
int orc_render(void* h, unsigned frame0, int nframes, unsigned seedBase, int y0, int y1, int nthreads, int maxDepthTrace, unsigned long long* counters)
{
	Renderer& r = ((OrcRenderer*)h)->r;
	r.max_depth_trace = maxDepthTrace;
	const int W = r.camera.width;
	Counters total;
	if (nthreads > 0) omp_set_num_threads(nthreads);
	for (int f = 0; f < nframes; f++) {
#pragma omp parallel
		{
			Counters local;
#pragma omp for schedule(dynamic)
			for (int y = y0; y < y1; ++y)
				for (int x = 0; x < W; ++x) r.Pixel(x, y, frame0 + f, seedBase, local);
#pragma omp critical
			total.add(local);
		}
		if (!r.scene->raytracer) r.iterationNumber++; // renderer.cpp:293-294
	}
	counters_out(total, counters);
	return 0;
}
// Q-learning guided sampler (orc_qlearn.h): grid == 0 switches it off
void orc_qlearn_enable(void* h, int grid, const float* lo, const float* hi, float alpha, float eps, float qInit, unsigned learnMask)
{
	QLearn& q = ((OrcRenderer*)h)->r.ql;
	if (grid <= 0) { q = QLearn(); return; }
	q.enable(grid, lo, hi, alpha, eps, qInit, learnMask);
}
void orc_qlearn_apply(void* h) { ((OrcRenderer*)h)->r.ql.apply(); }
void orc_qlearn_get(void* h, long long* sums, unsigned* counts, float* table)
{
	const QLearn& q = ((OrcRenderer*)h)->r.ql;
	const size_t cells = (size_t)q.grid * q.grid * q.grid;
	if (sums) memcpy(sums, q.sum.data(), cells * 64 * 8);
	if (counts) memcpy(counts, q.cnt.data(), cells * 64 * 4);
	if (table) for (size_t c = 0; c < cells; c++) memcpy(table + c * 64, &q.q[c * 72 + 8], 64 * 4);
}
void orc_qlearn_set_table(void* h, const float* table) { ((OrcRenderer*)h)->r.ql.set_table(table); }
int orc_qlearn_patch_of(const float* n) { return QLearn::patch_of(float3(n[0], n[1], n[2])); }
// the cell of n points (x: n*3 floats) and one guided pick per (cell, stream state): patch, P, direction and the state after the four draws
void orc_qlearn_cell(void* h, int n, const float* x, int* out)
{
	const QLearn& q = ((OrcRenderer*)h)->r.ql;
	for (int i = 0; i < n; i++) out[i] = q.cell(f3(x + 3 * i));
}
void orc_qlearn_sample(void* h, int n, const int* cell, const unsigned* seedIn, int* patch, float* P, float* dir, unsigned* seedOut)
{
	const QLearn& q = ((OrcRenderer*)h)->r.ql;
	for (int i = 0; i < n; i++) {
		uint seed = seedIn[i];
		const float3 d = q.sample(cell[i], seed, P[i], patch[i]);
		dir[3 * i] = d.x, dir[3 * i + 1] = d.y, dir[3 * i + 2] = d.z, seedOut[i] = seed;
	}
}
// QLearn::direction of n (band, sector, u1, u2) and the fixed-point word QLearn::reward adds for n rewards
void orc_qlearn_direction(int n, const int* ij, const float* u, float* dir)
{
	for (int i = 0; i < n; i++) {
		const float3 d = QLearn::direction(ij[2 * i], ij[2 * i + 1], u[2 * i], u[2 * i + 1]);
		dir[3 * i] = d.x, dir[3 * i + 1] = d.y, dir[3 * i + 2] = d.z;
	}
}
void orc_qlearn_reward_fixed(int n, const float* R, long long* out)
{
	for (int i = 0; i < n; i++) out[i] = QLearn::reward_fixed(R[i]);
}
void orc_qlearn_get_wgt(void* h, float* wgt) { memcpy(wgt, ((OrcRenderer*)h)->r.ql.wgt, 64 * 64 * 4); }
void orc_qlearn_get_v(void* h, float* v, float* centres)
{
	const QLearn& q = ((OrcRenderer*)h)->r.ql;
	memcpy(v, q.v.data(), q.v.size() * 4);
	for (int p = 0; p < 64; p++) centres[3 * p] = q.centre[p].x, centres[3 * p + 1] = q.centre[p].y, centres[3 * p + 2] = q.centre[p].z;
}
void orc_qlearn_set(void* h, const long long* sums, const unsigned* counts)
{
	QLearn& q = ((OrcRenderer*)h)->r.ql;
	const size_t cells = (size_t)q.grid * q.grid * q.grid;
	memcpy(q.sum.data(), sums, cells * 64 * 8);
	memcpy(q.cnt.data(), counts, cells * 64 * 4);
}
// Renderer::Tick: one frame with the reference's iteration bookkeeping; *camChanged in/out
int orc_tick(void* h, int* camChanged, unsigned frame, unsigned seedBase, int nthreads, unsigned* pixels)
{
	Renderer& r = ((OrcRenderer*)h)->r;
	if (nthreads > 0) omp_set_num_threads(nthreads);
	bool ch = *camChanged != 0;
	r.max_depth_trace = 4;
	r.Tick(ch, frame, seedBase, pixels);
	*camChanged = ch ? 1 : 0;
	return r.iterationNumber;
}
// Renderer::Trace (mode 0) / Renderer::Sample (mode 1) on caller rays with a caller energy; ray i draws from the
// stream StreamSeed(seedBase + i), as rt_trace_batch does
static void trace_rays(void* h, int mode, int n, const float* O, const float* D, int depth, const float* energy, unsigned seedBase, float* rgb, unsigned* peaks)
{
	Renderer& r = ((OrcRenderer*)h)->r;
	Counters cnt;
	for (int i = 0; i < n; i++) {
		uint seed = StreamSeed(seedBase + (uint)i);
		Ray ray(f3(O + 3 * i), f3(D + 3 * i));
		cnt.clear_peaks();
		const float3 c = mode == 0 ? r.Trace(ray, depth, f3(energy), seed, cnt) : r.Sample(ray, depth, f3(energy), seed, cnt, 0, r.ql.on && (seed & r.ql.learnMask) == 0);
		rgb[3 * i] = c.x, rgb[3 * i + 1] = c.y, rgb[3 * i + 2] = c.z;
		if (peaks) peaks_out(cnt, peaks + 3 * i);
	}
}
void orc_trace_rays(void* h, int mode, int n, const float* O, const float* D, int depth, const float* energy, unsigned seedBase, float* rgb)
{
	trace_rays(h, mode, n, O, D, depth, energy, seedBase, rgb, nullptr);
}
// ... and per ray the peak stack pointers over every walk of its tree or path (nearest-hit and shadow rays alike): peaks[3 * i ..]
void orc_trace_rays_peaks(void* h, int mode, int n, const float* O, const float* D, int depth, const float* energy, unsigned seedBase, float* rgb, unsigned* peaks)
{
	trace_rays(h, mode, n, O, D, depth, energy, seedBase, rgb, peaks);
}
void orc_get_accumulator(void* h, float* out) { const Renderer& r = ((OrcRenderer*)h)->r; memcpy(out, r.accumulator.data(), r.accumulator.size() * 16); }
// screen->pixels for iteration count 'it' (renderer.cpp:287-290)
void orc_resolve(void* h, int it, unsigned* out)
{
	const Renderer& r = ((OrcRenderer*)h)->r;
	for (size_t i = 0; i < r.accumulator.size(); i++) out[i] = r.ResolvePixel(i, it);
}
// ResolvePixel of n caller-given float4 values (rgba: 4 floats each) for iteration count 'it', without a renderer
void orc_resolve_values(const float* rgba, size_t n, int it, unsigned* out)
{
	for (size_t i = 0; i < n; i++) out[i] = Renderer::ResolveValue(float4{ rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3] }, it);
}
// primary rays only: GetPrimaryRay + FindNearest(t_min) per pixel
void orc_primary_hits(void* h, float t_min, int* outObj, float* outT, unsigned long long* counters)
{
	const Renderer& r = ((OrcRenderer*)h)->r;
	Counters cnt;
	const int W = r.camera.width, H = r.camera.height;
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
		Ray pr = r.camera.GetPrimaryRay(x, y);
		r.scene->FindNearest(pr, t_min, cnt);
		outObj[x + y * W] = pr.objIdx, outT[x + y * W] = pr.t;
	}
	counters_out(cnt, counters);
}
void orc_primary_rays(void* h, float* O, float* D)
{
	const Renderer& r = ((OrcRenderer*)h)->r;
	const int W = r.camera.width, H = r.camera.height;
	for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
		Ray pr = r.camera.GetPrimaryRay(x, y);
		size_t i = (size_t)x + (size_t)y * W;
		O[3 * i] = pr.O.x, O[3 * i + 1] = pr.O.y, O[3 * i + 2] = pr.O.z;
		D[3 * i] = pr.D.x, D[3 * i + 1] = pr.D.y, D[3 * i + 2] = pr.D.z;
	}
}

// ---- unit-level entry points (per-function parity vectors) -----------------------------------
void orc_rng_stream(unsigned seedBase, int n, unsigned* outU, float* outF)
{
	uint s = StreamSeed(seedBase);
	for (int i = 0; i < n; i++) { uint before = s; (void)before; float f = RandomFloat(s); outU[i] = s; outF[i] = f; }
}
void orc_hemisphere(unsigned seedBase, int n, const float* normals, float* out)
{
	uint s = StreamSeed(seedBase);
	for (int i = 0; i < n; i++) { float3 v = RandomInHemisphere(s, f3(normals + 3 * i)); out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z; }
}
float orc_intersect_aabb(const float* O, const float* D, float t, const float* bmin, const float* bmax)
{
	Ray r(f3(O), f3(D), t);
	return IntersectAABB(r, f3(bmin), f3(bmax));
}
void orc_fresnel(int n, const float* I, const float* N, float ior, float* kr)
{
	for (int i = 0; i < n; i++) glass_fresnel(f3(I + 3 * i), f3(N + 3 * i), ior, kr[i]);
}
void orc_refract(int n, const float* I, const float* N, float ratio, float* out)
{
	for (int i = 0; i < n; i++) { float3 v = glass_refract(f3(I + 3 * i), f3(N + 3 * i), ratio); out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z; }
}
void orc_mat4_inverse(const float* m, float* out) { mat4 a; memcpy(a.cell, m, 64); mat4 r = a.Inverted(); memcpy(out, r.cell, 64); }
// Translate * Scale * RotateX * RotateY * RotateZ, the product every TLAS scene uses (template/scene.h:927)
void orc_mat4_trs(const float* t, float s, float rx, float ry, float rz, float* out)
{
	mat4 M = mat4::Translate(f3(t)) * mat4::Scale(s) * mat4::RotateX(rx) * mat4::RotateY(ry) * mat4::RotateZ(rz);
	memcpy(out, M.cell, 64);
}

// ---- leaf entry points: the oracle's own functions, one call per case ---------------------------
// The same signatures as oracle/ref/ref_leaf.cpp exports for the reference's compiled code (ref_*), so
// tests/test_ref_leaf_cpu.py drives both with one caller and compares the answers bit for bit.
static void put3(float* p, const float3& v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }
static Triangle leaf_tri(const float* v) { return Triangle(7, 0, f3(v), f3(v + 3), f3(v + 6)); }
static void leaf_hit(const Ray& r, int i, int* hit, float* t, float* nrm) { hit[i] = r.objIdx, t[i] = r.t, put3(nrm + 3 * i, r.hitNormal); }
// light[12]: pos(3) strength col(3) radius normal(3) raytracer -- AreaLight's constructor, template/scene.h:97-103
static Light leaf_area(const float* L)
{
	Light a;
	a.kind = 0, a.objIdx = 7, a.pos = f3(L), a.strength = L[3], a.col = f3(L + 4), a.radius = L[7], a.radius2 = L[7] * L[7];
	a.area = 2 * a.radius2 * PI, a.normal = f3(L + 8), a.raytracer = L[11] != 0;
	return a;
}
// light[8]: pos(3) strength normal(3) r -- DirectionalLight's constructor, template/scene.h:146-148
static Light leaf_dir(const float* L)
{
	Light d;
	d.kind = 1, d.objIdx = 7, d.pos = f3(L), d.strength = L[3], d.col = float3(1), d.normal = f3(L + 4);
	d.sinAngle = x_sinf(L[7] * PI / 2);
	return d;
}
void orc_leaf_tri_ctor(int n, const float* v9, float* N, float* centroid)
{
	for (int i = 0; i < n; i++) { Triangle t = leaf_tri(v9 + 9 * i); put3(N + 3 * i, t.N), put3(centroid + 3 * i, t.centroid); }
}
void orc_leaf_tri_intersect(int n, const float* v9, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); leaf_tri(v9 + 9 * i).Intersect(r, tmin[i]); leaf_hit(r, i, hit, t, nrm); }
}
void orc_leaf_tri_occluding(int n, const float* v9, const float* O, const float* D, const float* tmax, const float* tmin, int* occ)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); occ[i] = leaf_tri(v9 + 9 * i).IsOccluding(r, tmin[i]); }
}
void orc_leaf_sphere_intersect(int n, const float* pos, const float* rad, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); Sphere(7, 0, f3(pos + 3 * i), rad[i]).Intersect(r, tmin[i]); leaf_hit(r, i, hit, t, nrm); }
}
void orc_leaf_sphere_occluding(int n, const float* pos, const float* rad, const float* O, const float* D, const float* tmax, const float* tmin, int* occ)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); occ[i] = Sphere(7, 0, f3(pos + 3 * i), rad[i]).IsOccluding(r, tmin[i]); }
}
void orc_leaf_sphere_normal(int n, const float* pos, const float* rad, const float* I, float* nrm)
{
	// Sphere::GetNormal (template/scene.h:382-385), as Sphere::Intersect applies it to the hit point
	for (int i = 0; i < n; i++) { Sphere s(7, 0, f3(pos + 3 * i), rad[i]); put3(nrm + 3 * i, (f3(I + 3 * i) - s.pos) * s.invr); }
}
void orc_leaf_plane_intersect(int n, const float* N, const float* d, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); Plane(7, 0, f3(N + 3 * i), d[i]).Intersect(r, tmin[i]); leaf_hit(r, i, hit, t, nrm); }
}
void orc_leaf_plane_occluding(int n, const float* N, const float* d, const float* O, const float* D, const float* tmax, const float* tmin, int* occ)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); occ[i] = Plane(7, 0, f3(N + 3 * i), d[i]).IsOccluding(r, tmin[i]); }
}
void orc_leaf_area_intersect(int n, const float* L, const float* O, const float* D, const float* tmax, const float* tmin, int* hit, float* t, float* nrm)
{
	for (int i = 0; i < n; i++) { Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]); leaf_area(L + 12 * i).Intersect(r, tmin[i]); leaf_hit(r, i, hit, t, nrm); }
}
void orc_leaf_area_intensity(int n, const float* L, const float* p, const float* nrm, const float* from, float* rgb)
{
	for (int i = 0; i < n; i++) put3(rgb + 3 * i, leaf_area(L + 12 * i).GetLightIntensityAt(f3(p + 3 * i), f3(nrm + 3 * i), f3(from + 3 * i)));
}
void orc_leaf_area_position(int n, const float* L, const unsigned* seedIn, float* pos, unsigned* seedOut)
{
	for (int i = 0; i < n; i++) { uint s = seedIn[i]; put3(pos + 3 * i, leaf_area(L + 12 * i).GetLightPosition(s)); seedOut[i] = s; }
}
void orc_leaf_dir_ctor(int n, const float* L, float* sinAngle)
{
	for (int i = 0; i < n; i++) sinAngle[i] = leaf_dir(L + 8 * i).sinAngle;
}
void orc_leaf_dir_intensity(int n, const float* L, const float* p, float* rgb)
{
	for (int i = 0; i < n; i++) put3(rgb + 3 * i, leaf_dir(L + 8 * i).GetLightIntensityAt(f3(p + 3 * i), float3(0, 1, 0), float3(0)));
}
void orc_leaf_glass_fresnel(int n, const float* I, const float* N, const float* ior, float* kr)
{
	for (int i = 0; i < n; i++) { float k = 0; glass_fresnel(f3(I + 3 * i), f3(N + 3 * i), ior[i], k); kr[i] = k; }
}
void orc_leaf_glass_refract(int n, const float* D, const float* N, const float* ratio, float* out)
{
	for (int i = 0; i < n; i++) put3(out + 3 * i, glass_refract(f3(D + 3 * i), f3(N + 3 * i), ratio[i]));
}
// m[6]: albedo(3) ks kd n; a material built with raytracer == true (no draw)
void orc_leaf_diffuse_scatter(int n, const float* m, const float* O, const float* D, const float* t, const float* lightDir, const float* lightInt,
                              const float* nrm, const float* energyIn, float* att, float* energyOut, float* scatO)
{
	for (int i = 0; i < n; i++) {
		const float* M = m + 6 * i;
		Material d;
		d.type = DIFFUSE, d.albedo = f3(M), d.col = float3(1), d.specu = M[3], d.diffu = M[4], d.N = (int)M[5], d.raytracer = true;
		Ray r(f3(O + 3 * i), f3(D + 3 * i), t[i]);
		float3 a(0), dir(0), e = f3(energyIn + 3 * i);
		uint seed = 1;
		diffuse_scatter(d, r, a, dir, f3(lightDir + 3 * i), f3(lightInt + 3 * i), f3(nrm + 3 * i), e, seed);
		put3(att + 3 * i, a), put3(energyOut + 3 * i, e), put3(scatO + 3 * i, r.IntersectionPoint()); // :615: the scattered ray starts at the hit point
	}
}
void orc_leaf_metal_scatter(int n, const float* O, const float* D, const float* t, const float* nrm, float* outO, float* outD, int* ret)
{
	for (int i = 0; i < n; i++) {
		Ray r(f3(O + 3 * i), f3(D + 3 * i), t[i]);
		float3 nn = f3(nrm + 3 * i);
		Ray s = metal_scatter(r, nn);
		ret[i] = dot(s.D, nn) > 0; // :634
		put3(outO + 3 * i, s.O), put3(outD + 3 * i, s.D);
	}
}
// cam[15]: camPos(3) topLeft(3) topRight(3) bottomLeft(3) fishEye viewAngle yAngle; the reference's fixed 600 x 400
void orc_leaf_camera_rays(const float* cam, int n, const int* xs, const int* ys, float* O, float* D)
{
	Camera c;
	c.camPos = f3(cam), c.topLeft = f3(cam + 3), c.topRight = f3(cam + 6), c.bottomLeft = f3(cam + 9);
	c.fishEye = cam[12] != 0, c.viewAngle = cam[13], c.yAngle = cam[14];
	for (int i = 0; i < n; i++) { Ray r = c.GetPrimaryRay(xs[i], ys[i]); put3(O + 3 * i, r.O), put3(D + 3 * i, r.D); }
}
void orc_leaf_sky_color(int w, int h, int nch, const unsigned char* px, int n, const float* D, float* rgb)
{
	Scene s;
	s.skydome.assign(px, px + (size_t)w * h * nch), s.skydomeX = w, s.skydomeY = h, s.skydomeN = nch;
	for (int i = 0; i < n; i++) put3(rgb + 3 * i, s.GetSkyColor(Ray(f3(D + 3 * i), f3(D + 3 * i))));
}

// ---- scan: every primitive against every ray, no tree, no stack, no order -------------------------
// The second statement of FindNearest / IsOccluded that tests/scan_ref.py words (rules A, B and the two occlusion rules): the pinned leaf
// bodies above over arrays of primitives, and the one box fact a tree may use, IntersectAABB of a primitive's OWN box.  Nothing of bvh,
// bvhInstance or tlas is named here but IntersectAABB.
// Primitives: triangles v9 (+ optional stored normals triN, else Triangle's own), spheres pos + r, planes N + d; ids: (obj, mat) per
// primitive in that order.  flags bit 0: spheres and planes carry no box (the brute-force primitives of a TLAS scene).
struct ScanPrims {
	std::vector<Triangle> tri; std::vector<Sphere> sph; std::vector<Plane> pla;
	std::vector<float3> bmin, bmax; // own boxes: triangle min / max of its vertices, sphere pos -/+ r, plane as bvh::UpdateNodeBounds (Q1)
	bool nobox = false;
	size_t size() const { return tri.size() + sph.size() + pla.size(); }
};
static ScanPrims scan_prims(int nTri, const float* v9, const float* triN, int nSph, const float* sph4, int nPla, const float* pla4, const int* ids, int flags)
{
	ScanPrims P;
	P.nobox = (flags & 1) != 0;
	for (int i = 0; i < nTri; i++, ids += 2) {
		Triangle t(ids[0], ids[1], f3(v9 + 9 * i), f3(v9 + 9 * i + 3), f3(v9 + 9 * i + 6));
		if (triN) t.N = f3(triN + 3 * i);
		P.tri.push_back(t);
		P.bmin.push_back(t_fminf(t_fminf(t.v0, t.v1), t.v2)), P.bmax.push_back(t_fmaxf(t_fmaxf(t.v0, t.v1), t.v2));
	}
	for (int i = 0; i < nSph; i++, ids += 2) {
		Sphere s(ids[0], ids[1], f3(sph4 + 4 * i), sph4[4 * i + 3]);
		P.sph.push_back(s);
		P.bmin.push_back(s.pos - float3(s.r)), P.bmax.push_back(s.pos + float3(s.r));
	}
	for (int i = 0; i < nPla; i++, ids += 2) {
		Plane q(ids[0], ids[1], f3(pla4 + 4 * i), pla4[4 * i + 3]);
		P.pla.push_back(q);
		float3 n = normalize(q.N), lo(-1e30f), hi(1e30f);
		if (n.x + n.y + n.z == 1 && (n.x == 1 || n.y == 1 || n.z == 1)) { // Q1: a slab at coordinate 0
			if (n.x == 1) lo.x = hi.x = 0; else if (n.y == 1) lo.y = hi.y = 0; else lo.z = hi.z = 0;
		}
		P.bmin.push_back(lo), P.bmax.push_back(hi);
	}
	return P;
}
static inline void scan_leaf(const ScanPrims& P, size_t p, Ray& r, float t_min)
{
	if (p < P.tri.size()) P.tri[p].Intersect(r, t_min);
	else if (p < P.tri.size() + P.sph.size()) P.sph[p - P.tri.size()].Intersect(r, t_min);
	else P.pla[p - P.tri.size() - P.sph.size()].Intersect(r, t_min);
}
static inline bool scan_leaf_occ(const ScanPrims& P, size_t p, const Ray& r, float t_min)
{
	if (p < P.tri.size()) return P.tri[p].IsOccluding(r, t_min);
	else if (p < P.tri.size() + P.sph.size()) return P.sph[p - P.tri.size()].IsOccluding(r, t_min);
	else return P.pla[p - P.tri.size() - P.sph.size()].IsOccluding(r, t_min);
}
static inline bool scan_box(const ScanPrims& P, size_t p, const Ray& r, float rayT)
{
	if (P.nobox && p >= P.tri.size()) return true;
	Ray b = r;
	b.t = rayT;
	return IntersectAABB(b, P.bmin[p], P.bmax[p]) != 1e30f;
}
static inline unsigned fbits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
// the scan's own thread count: orc_render / orc_tick leave omp_set_num_threads at what their caller asked for (often 1), and a scan is
// rays x primitives.  OMP_NUM_THREADS where it is set, else the processors, 16 at most.
static int scan_threads()
{
	const char* e = getenv("OMP_NUM_THREADS");
	int n = e ? atoi(e) : omp_get_num_procs();
	return n < 1 ? 1 : n > 16 ? 16 : n;
}
// Per ray i, each primitive's leaf Intersect on a fresh Ray(O, D, tmax[i]) at t_min:
//   tAll[i]  the nearest leaf t over all primitives (1e30f: none hit); tNext[i] the nearest one that is farther than tAll[i] (1e30f: none)
//   tFlt[i]  the nearest leaf t over those whose own box passes IntersectAABB with ray.t = T[i], and gate[i] != 0 (gate NULL: all open)
//   witT[i]  the first primitive whose leaf t has T[i]'s bits (-1: none)
//   witFull[i]  the first such primitive whose obj, mat and normal bits are gotObj / gotMat / gotN's too (-1: none; gotMat, gotN NULL: not
//            compared, for a query that reports neither); nrmM (16 floats or
//            NULL): the normal is normalize(TransformVector(hitNormal, nrmM)) as bvhInstance::BIntersect leaves it
void orc_scan_nearest(int nTri, const float* v9, const float* triN, int nSph, const float* sph4, int nPla, const float* pla4, const int* ids, int flags,
                      int n, const float* O, const float* D, const float* tmax, float t_min, const float* T, const unsigned char* gate,
                      const int* gotObj, const int* gotMat, const float* gotN, const float* nrmM,
                      float* tAll, float* tNext, float* tFlt, int* witT, int* witFull)
{
	const ScanPrims P = scan_prims(nTri, v9, triN, nSph, sph4, nPla, pla4, ids, flags);
	mat4 M;
	if (nrmM) memcpy(M.cell, nrmM, 64);
	const size_t N = P.size();
	const int nt = scan_threads();
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
	for (int i = 0; i < n; i++) {
		float best = 1e30f, next = 1e30f, bestF = 1e30f;
		int wT = -1, wF = -1;
		const Ray base(f3(O + 3 * i), f3(D + 3 * i), tmax[i]);
		for (size_t p = 0; p < N; p++) {
			Ray r = base;
			scan_leaf(P, p, r, t_min);
			if (!(r.t < base.t)) continue; // every leaf body accepts only t < ray.t
			if (r.t < best) next = best, best = r.t;
			else if (r.t > best && r.t < next) next = r.t;
			if ((!gate || gate[i]) && r.t < bestF && scan_box(P, p, base, T[i])) bestF = r.t;
			if (fbits(r.t) == fbits(T[i])) {
				if (wT < 0) wT = (int)p;
				if (wF < 0 && gotObj) {
					float3 nn = nrmM ? normalize(TransformVector(r.hitNormal, M)) : r.hitNormal;
					if (r.objIdx == gotObj[i] && (!gotMat || r.mat == gotMat[i]) &&
					    (!gotN || (fbits(nn.x) == fbits(gotN[3 * i]) && fbits(nn.y) == fbits(gotN[3 * i + 1]) && fbits(nn.z) == fbits(gotN[3 * i + 2])))) wF = (int)p;
				}
			}
		}
		tAll[i] = best, tNext[i] = next, tFlt[i] = bestF, witT[i] = wT, witFull[i] = wF;
	}
}
// Per ray i, each primitive's leaf IsOccluding on Ray(O, D, tmax[i]) at t_min: occAll[i] some primitive occludes; occFlt[i] some primitive
// occludes while its own box passes IntersectAABB with ray.t = tmax[i], and gate[i] != 0
void orc_scan_occluded(int nTri, const float* v9, const float* triN, int nSph, const float* sph4, int nPla, const float* pla4, const int* ids, int flags,
                       int n, const float* O, const float* D, const float* tmax, float t_min, const unsigned char* gate,
                       unsigned char* occAll, unsigned char* occFlt)
{
	const ScanPrims P = scan_prims(nTri, v9, triN, nSph, sph4, nPla, pla4, ids, flags);
	const size_t N = P.size();
	const int nt = scan_threads();
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
	for (int i = 0; i < n; i++) {
		const Ray r(f3(O + 3 * i), f3(D + 3 * i), tmax[i]);
		bool any = false, anyF = false;
		for (size_t p = 0; p < N && !anyF; p++) {
			if (!scan_leaf_occ(P, p, r, t_min)) continue;
			any = true;
			if ((!gate || gate[i]) && scan_box(P, p, r, r.t)) anyF = true;
		}
		occAll[i] = any, occFlt[i] = anyF;
	}
}
// IntersectAABB of ray i with ray.t = t[i] against box6[i] (perRay) or box6[0]: min then max
void orc_slab_batch(int n, const float* O, const float* D, const float* t, int perRay, const float* box6, float* out)
{
	for (int i = 0; i < n; i++) {
		const float* b = box6 + (perRay ? 6 * i : 0);
		out[i] = IntersectAABB(Ray(f3(O + 3 * i), f3(D + 3 * i), t[i]), f3(b), f3(b + 3));
	}
}
// world ray -> instance ray, as bvhInstance::BIntersect / IsOccluded do it (bvhInstance.cpp:6-7, 26-27): no normalisation, t keeps its meaning
void orc_leaf_instance_ray(int n, const float* O, const float* D, const float* invT, float* outO, float* outD)
{
	mat4 M;
	memcpy(M.cell, invT, 64);
	for (int i = 0; i < n; i++) put3(outO + 3 * i, TransformPosition(f3(O + 3 * i), M)), put3(outD + 3 * i, TransformVector(f3(D + 3 * i), M));
}

} // extern "C"
