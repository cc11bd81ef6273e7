// rapt.h -- C++ host mirror of the reference's interface for the trace-loop path.
//
// Same class names, member names, constructor argument orders and call shapes as the reference
// (template/scene.h, bvh.h, bvhInstance.h, tlas.h, camera.h, renderer.h) so that host code written
// against it -- scene factories, the OBJ/.tri loaders' callers, the frame loop -- ports by changing
// the namespace.  What differs: the queries and the pixel loop execute on the GPU through the C ABI
// of include/rt_amd.h; host objects hold parameters and the builders' output only.
//
//   reference                                   here
//   Scene::FindNearest(Ray&, float) const       Scene::FindNearest (1 ray) / FindNearestBatch
//   Scene::IsOccluded(Ray&) const               Scene::IsOccluded  (1 ray) / IsOccludedBatch
//   Renderer::Init / Tick / Trace / Sample      same names, same arguments
//   bvh::Build, Refit, bvhInstance::SetTransform, tlas::build   host-side, same outputs
//
// After the last scene edit call Scene::Commit(): it builds nothing, it only flattens the objects
// into an rt_scene_desc and uploads it (the reference needs no such step because its queries chase
// host pointers).
#pragma once
#include "rapt_math.h"
#include "../../include/rt_amd.h"
#include <map>
#include <string>
#include <vector>

namespace rapt {

enum MAT_TYPE { DIFFUSE = 1, METAL = 2, GLASS = 3 }; // template/scene.h:33-37

// template/scene.h:582-676 (parameters only; scatter / fresnel / RefractRay run on the device)
class material {
public:
	material(float3 c, bool rt) : col(c), raytracer(rt) {}
	virtual ~material() {}
	void SetColor(float3 c) { col = c; }
	float3 col, albedo = float3(0), emission = float3(0);
	int type = DIFFUSE;
	bool raytracer;
};
class diffuse : public material {
public:
	diffuse(float3 a = float3(0), float3 c = float3(0), float ks = 0.2f, float kd = 0.8f, int n = 2, bool rt = true, float e = 0, float s = 0)
		: material(c, rt), specu(ks), diffu(kd), shinieness(s), N(n) { type = DIFFUSE; albedo = a; emission = float3(e); }
	float specu, diffu, shinieness;
	int N;
};
class metal : public material {
public:
	metal(float f, float3 c, bool rt) : material(c, rt), fuzzy(f < 1 ? f : 1) { type = METAL; }
	float fuzzy;
};
class glass : public material {
public:
	glass(float refIndex, float3 c, float3 a, float r, float n, bool rt)
		: material(c, rt), ir(refIndex), specu(r), N(n), absorption(a) { type = GLASS; invIr = 1 / ir; }
	float ir, specu, N, invIr;
	float3 absorption;
};

// template/scene.h:38-73
class Ray {
public:
	Ray() = default;
	Ray(float3 origin, float3 direction, float3 color, float distance = 1e34f)
	{
		O = origin, D = direction, t = distance;
		rD = float3(1 / D.x, 1 / D.y, 1 / D.z);
		this->color = color;
		exists = true;
	}
	float3 IntersectionPoint() const { return O + t * D; }
	void SetMaterial(material* mat) { m = mat; }
	material* GetMaterial() { return m; }
	void SetNormal(float3 normal) { hitNormal = normal; }
	float3 O, D, rD;
	float t = 1e34f;
	int objIdx = -1;
	bool inside = false, exists = false;
	float3 color = float3(0);
	float3 hitNormal;
	material* m = nullptr;
};

// template/scene.h:75-168 (parameters; Intersect / GetLightIntensityAt / GetLightPosition on device)
class Light {
public:
	Light() = default;
	Light(int idx, float3 p, float str, float3 c, float3 n, bool rt) : pos(p), raytracer(rt), col(c), strength(str), objIdx(idx), normal(n) {}
	virtual ~Light() {}
	virtual int kind() const { return RT_LIGHT_BASE; }
	virtual void updateTracing(bool rt) { raytracer = rt; }
	float3 pos;
	bool raytracer = true;
	float3 col;
	float strength = 1;
	int objIdx = 0;
	float3 normal;
};
class AreaLight : public Light {
public:
	AreaLight(int idx, float3 p, float str, float3 c, float r, float3 n, int s, bool rt) : Light(idx, p, str, c, n, rt)
	{
		radius = r, radius2 = r * r, samples = s, area = 2 * radius2 * 3.14159265358979323846264f;
	}
	int kind() const override { return RT_LIGHT_AREA; }
	int samples;
	float radius, radius2, area;
};
class DirectionalLight : public Light {
public:
	DirectionalLight(int idx, float3 p, float str, float3 c, float3 n, float r, bool rt) : Light(idx, p, str, c, n, rt)
	{
		sinAngle = sinf_r(r * 3.14159265358979323846264f / 2);
	}
	int kind() const override { return RT_LIGHT_DIRECTIONAL; }
	float sinAngle;
};

// template/scene.h:175-251
class Triangle {
public:
	Triangle() = default;
	Triangle(int idx, material* m, float3 ver0, float3 ver1, float3 ver2) : v0(ver0), v1(ver1), v2(ver2), objIdx(idx), mat(m) { derive(); }
	Triangle(int idx, material* m, int3 facesIdx, const std::vector<float3>& vertices)
		: v0(vertices[facesIdx.x]), v1(vertices[facesIdx.y]), v2(vertices[facesIdx.z]), objIdx(idx), mat(m) { derive(); }
	void update(int3 faces, const std::vector<float3>& vertices) { v0 = vertices[faces.x], v1 = vertices[faces.y], v2 = vertices[faces.z]; derive(); }
	float3 GetNormal(const float3) const { return N; }
	float3 v0, v1, v2, e1, e2, centroid, N;
	int objIdx = -1;
	material* mat = nullptr;
private:
	void derive()
	{
		e1 = v1 - v0;
		e2 = v2 - v0;
		N = normalize(cross(e1, e2));
		centroid = (v0 + v1 + v2) * 0.333f;
	}
};

// template/scene.h:258-340.  The file constructors keep the reference's argument orders; failures
// throw std::runtime_error (the reference exits or crashes).
class Mesh {
public:
	Mesh() = default;
	Mesh(int idGroup, const char* path, material* m);                             // .tri
	Mesh(int idGroup, std::string path, material* m, float3 pos, float scale);    // .obj
	Mesh(int idGroup, material* m, const float* v9, int n);                       // in-memory triangles
	uint getSize() const { return (uint)tri.size(); }
	void update() { for (size_t i = 0; i < faces.size(); i++) { int3 f = faces[i]; f.x--, f.y--, f.z--; tri[i].update(f, vertices); } }
	std::vector<float3> vertices;
	std::vector<int3> faces;
	std::vector<Triangle> tri;
	std::vector<float3> originalVerts;
	material* mat = nullptr;
	int groupIdx = -1;
};

// template/scene.h:347-394
class Sphere {
public:
	Sphere() = default;
	Sphere(int idx, material* m, float3 p, float r) : pos(p), r2(r * r), invr(1 / r), r(r), objIdx(idx), mat(m) {}
	float3 pos = float3(0);
	float r2 = 0, invr = 0, r = 0;
	int objIdx = -1;
	material* mat = nullptr;
};
// template/scene.h:401-448
class Plane {
public:
	Plane() = default;
	Plane(int idx, material* m, float3 normal, float dist) : N(normal), d(dist), objIdx(idx), mat(m) {}
	float3 N;
	float d = 0;
	int objIdx = -1;
	material* mat = nullptr;
};

class Scene;

struct BVHNode { // bvh.h:10-24
	float3 aabbMin; uint leftFirst;
	float3 aabbMax; uint primCount;
	bool isLeaf() const { return primCount > 0; }
};
static_assert(sizeof(BVHNode) == 32, "BVHNode must match rt_bvh_node");

enum SplitMethod { BINNEDSAH = 0, SAMESIZE = 1, LONGESTAXIS = 2, SAH = 3 }; // bvh.h:38-43

// bvh.h:45-86.  Build() and Refit() run on the host and reproduce the reference's node array
// and primitiveIdx order (builder quirks included: they decide hit ids).  QBVH is not built
// (disabled in the reference, template/scene.h:704-707).
class bvh {
public:
	bvh(Scene* s);
	bvh(Mesh* m);
	~bvh();
	void Build(bool isQ = false);
	// Build() through rt_build_bvh (include/rt_amd.h): the same tree, made on the device.  BINNEDSAH only;
	// throws for what the device builder refuses (no triangle or sphere, non-finite geometry)
	void BuildOnDevice(rt_ctx* ctx);
	void Refit();
	// bvh.h:57, :65 -- on the device, in this bvh's own space (rt_intersect_scope RT_SCOPE_BLAS); valid after Scene::Commit
	void Intersect(Ray& ray);
	bool IsOccluded(Ray& ray);
	Scene* owner = nullptr; int blasIndex = -1; // set by Scene::Commit
	uint rootNodeIdx = 0, nodesUsed = 2, NTri = 0, NSph = 0, NPla = 0, N = 0;
	uint* primitiveIdx = nullptr;
	Scene* scene = nullptr;
	BVHNode* bvhNode = nullptr;
	Mesh* mesh = nullptr;
	aabb bounds;
	int splitMethod = BINNEDSAH;
	int treeDepth = 0; // DataCollector::maxTreeDepth analogue
private:
	struct Builder;
};

// bvhInstance.h
class bvhInstance {
public:
	bvhInstance() = default;
	bvhInstance(bvh* blas);
	void SetTransform(mat4& transform);
	// bvhInstance.h:11-12 -- on the device (RT_SCOPE_INSTANCE); valid after Scene::Commit
	void BIntersect(Ray& ray);
	bool IsOccluded(Ray& ray);
	Scene* owner = nullptr; int index = -1; // set by Scene::Commit
	mat4 invTransform, matTransform;
	bvh* blas = nullptr; // the reference names this member 'bvh'
	aabb bounds;
};

struct TLASNode { // tlas.h:4-11
	float3 aabbMin; uint leftRight;
	float3 aabbMax; uint BLAS;
	bool isLeaf() const { return leftRight == 0; }
};
static_assert(sizeof(TLASNode) == 32, "TLASNode must match rt_tlas_node");

// tlas.h:13-29
class tlas {
public:
	tlas(bvhInstance* bvhList, int N);
	~tlas();
	void build();
	void BuildOnDevice(rt_ctx* ctx); // tlas::build through rt_build_tlas
	// tlas.h:20-21 -- on the device (RT_SCOPE_ACCEL); valid after Scene::Commit
	void Intersect(Ray& ray);
	bool IsOccluded(Ray& ray);
	Scene* owner = nullptr; // set by Scene::Commit
	int FindBestMatch(int* list, int N, int A);
	TLASNode* tlasNode = nullptr;
	uint nodesUsed = 0;
	bvhInstance* blas = nullptr;
	uint blasCount = 0;
};

// camera.h (state read by GetPrimaryRay; the interactive move/rotate helpers are UI, out of scope)
class Camera {
public:
	Camera() { Reset(600, 400); }
	void Reset(int w, int h)
	{
		aspect = (float)w / (float)h;
		camPos = float3(0, 1, -2);
		topLeft = float3(-aspect, 2, 0);
		topRight = float3(aspect, 2, 0);
		bottomLeft = float3(-aspect, 0, 0);
		changed = false; // camera.h:52: the constructor does not mark a change; the mutators do
	}
	void ToogleFisheye() { changed = true; fishEye = !fishEye; }
	void SetChange(bool s) { changed = s; }
	bool GetChange() const { return changed; }
	float aspect = 1.5f;
	float viewAngle = 0.25f;
	float3 camPos, topLeft, topRight, bottomLeft;
	float yAngle = 0;
	bool paused = false, fishEye = false, changed = false;
};

// template/scene.h:685-1397: container + the three queries.  Owns what is added to it.
class Scene {
public:
	Scene();
	~Scene();
	// the default construction path of the reference (template/scene.h:688-716): after filling the
	// containers call BuildBVH() (new bvh(this); Build) or BuildTLAS() (tlas(bvhList, bvhCount); build)
	// deviceBuild != nullptr: BuildBVH / BuildTLAS make their trees (any split method) and the TLAS on that context's GPU
	// (bvh::BuildOnDevice -> rt_build_bvh_split, tlas::BuildOnDevice -> rt_build_tlas)
	rt_ctx* deviceBuild = nullptr;
	void BuildBVH(int splitMethod = BINNEDSAH);
	// instances reference meshes by index; one bvh per distinct mesh (TLASSceneTest2 shares one)
	void BuildTLAS(const std::vector<int>& meshOfInstance, const std::vector<mat4>& transforms, int splitMethod = BINNEDSAH);
	// Scene description file (host/scene_file.cpp): the data a reference scene factory hard-codes
	// (template/scene.h:791-1209) as a text file; builds the BVH / TLAS it names.  Throws on errors.
	void LoadFile(const std::string& path);
	// skydome = stbi_load(path, &x, &y, &n, 3) for a Radiance .hdr file (template/scene.h:792)
	bool LoadSkyHDR(const char* path, std::string* why = nullptr);
	// flatten + upload to the device context (must be called before queries / rendering)
	void Commit(rt_ctx* ctx);
	void CommitAlso(rt_ctx* other); // the same flattened scene to one more context (multi-GPU: every GPU holds a copy); SetTime reaches it too

	// template/scene.h:1210: mesh wobble + bvh::Refit, executed on the device (rt_set_time); the
	// reference runs it only when animOn (raytracer && defaultAnim && !useTLAS)
	void SetTime(float t);
	// Moving instances without a re-upload (rt_set_instances; the reference leaves tl->Build() commented out, template/scene.h:1245): call
	// bvhList[i].SetTransform(M) for every instance that moved, then this.  It sends ALL instances' matrices and their 'bounds' -- which
	// SetTransform grows and never resets, as the reference's -- to ctx and every context of CommitAlso, and refreshes tl->tlasNode /
	// nodesUsed from rt_download_tlas, so that tl is the tree the device walks.  Throws without useTLAS (RT_E_UNSUPPORTED) and for what
	// rt_set_instances refuses.  The accumulator is the caller's to clear (Renderer: camera.SetChange(true) before the next Tick).
	void CommitInstances();
	// Adding, removing and re-pointing instances without a re-upload (rt_set_instance_list).  CommitInstanceList: call it after REPLACING
	// the instance array and the TLAS object -- bvhList / bvhCount / Transforms and tl = new tlas(bvhList, bvhCount), 1..256 instances,
	// every one over a bvh the committed scene holds (a new mesh needs Commit).  It sends the whole list with each bvhInstance's own
	// 'bounds' to ctx and every context of CommitAlso and refreshes tl from rt_download_tlas, as CommitInstances does.  Throws without
	// useTLAS and for what rt_set_instance_list refuses.  A bvh left without an instance stays on the device and can be named again.
	// SetInstanceList does the replacing: fresh bvhInstances (meshOfInstance[i] names the mesh as BuildTLAS does; the mesh must have been
	// given a bvh by BuildTLAS), their transforms, a new tlas built on the host.  It sends nothing.
	// (Describe() numbers the BLASes by first use in bvhList and leaves out one without an instance: after a list edit it describes what a
	// new Commit would upload, which holds the committed contexts' BLASes in the committed order only while the list's first uses keep it.)
	void SetInstanceList(const std::vector<int>& meshOfInstance, const std::vector<mat4>& transforms);
	void CommitInstanceList();
	// Deforming a mesh without a re-upload (rt_set_triangles): call it after rewriting the triangles of the mesh(es) under 'bv' (same
	// count; Triangle::update or new Triangles).  It runs the host bvh::Refit() and refreshes bv->bounds, sends all of bv's triangles to
	// ctx and every context of CommitAlso, and -- the library's choice, stated as in CommitInstances' counterpart rt_set_instances with
	// bounds6 == NULL -- RESETS the 'bounds' of bv's instances to the box of a fresh instance under their current transform (they do not
	// accumulate across a deformation); then tl is refreshed from rt_download_tlas.  Throws for what rt_set_triangles refuses.
	void CommitTriangles(bvh* bv);
	// The same for an indexed mesh, from its vertices alone (rt_set_mesh_indices, rt_set_vertices): call it after rewriting
	// bv->mesh->vertices (same count).  bv must be a BLAS over ONE Mesh that has faces (1-based there, as in the reference; the C ABI's are
	// 0-based).  It runs Mesh::update() (the triangles follow the vertices), then what CommitTriangles runs, but sends the vertex array
	// in place of the triangle records; the first call after a Commit binds the faces to every committed context.  The device derives the
	// normals Mesh::update derives here.  Throws for a bvh without such a mesh and for what rt_set_vertices refuses.
	void CommitVertices(bvh* bv);
	// Relighting without a re-upload (rt_set_lights, rt_set_materials, rt_set_sky), to ctx and every context of CommitAlso.
	// CommitLights: after changing, adding or removing entries of 'lights' (at most 32): the whole table is sent.
	// CommitMaterials: after changing the fields of the materials (col, albedo, shinieness, ir, ...), or after ReplaceMaterial: every
	//   material of the committed scene is sent, index for index; their number cannot change.
	// ReplaceMaterial(index, m): materials[index] becomes m (owned from here on; the old object is deleted) and every mesh, triangle,
	//   sphere and plane that named the old one names m: how a material changes its class -- diffuse to metal -- on the host.
	// CommitSky: after rewriting skydome / skydomeX / skydomeY / skydomeN (an empty skydome: no sky, misses are black).
	// Each throws for what its rt_set_* refuses.  The accumulator is the caller's to clear (Renderer: the calls of the same names).
	void CommitLights();
	void CommitMaterials();
	void ReplaceMaterial(int index, material* m);
	void CommitSky();
	void FindNearest(Ray& ray, float t_min) const;   // template/scene.h:1248
	bool IsOccluded(Ray& ray) const;                 // template/scene.h:1286
	float3 GetSkyColor(Ray& ray) const;              // template/scene.h:1312, evaluated on the device (rt_sky_color_batch)
	// the queries below Scene level (bvh / tlas / bvhInstance members call these)
	void ScopeNearest(int scope, int index, Ray& ray) const;
	bool ScopeOccluded(int scope, int index, Ray& ray) const;
	void FindNearestBatch(int n, const float* O, const float* D, const float* tmax, float t_min, rt_hit* out) const;
	void IsOccludedBatch(int n, const float* O, const float* D, const float* tmax, uint8_t* out) const;

	uint getTriangleNb() const;                      // :1329
	const Triangle& getTriangle(uint idx) const;     // :1337
	void toogleRaytracer();                          // :1352
	void SetIterationNumber(int i) { iterationNumber = i; }
	int GetIterationNumber() const { return iterationNumber; }

	// flattening (also used by tests to inspect what is uploaded)
	const rt_scene_desc& Describe();
	int materialIndex(const material* m) const;

	int skydomeX = 0, skydomeY = 0, skydomeN = 3;
	std::vector<unsigned char> skydome;
	bvh* b = nullptr; tlas* tl = nullptr; bvhInstance* bvhList = nullptr;
	uint bvhCount = 0;
	mat4* Transforms = nullptr;
	std::vector<Light*> lights;
	std::vector<Sphere> spheres;
	std::vector<Mesh> meshes;
	std::vector<Plane> planes;
	std::vector<material*> materials; // owned; the reference leaks them
	int aaSamples = 1;
	int iterationNumber = 1;
	int totIterationNumber = 0;
	bool raytracer = true;
	bool useTLAS = false;
	rt_ctx* ctx = nullptr;
	std::vector<rt_ctx*> alsoCtx; // the further contexts the scene was committed to (CommitAlso): SetTime animates every copy
	std::map<const bvh*, std::vector<rt_ctx*>> facesBound; // CommitVertices: the contexts that hold bv's faces (a binding ends with the upload)
private:
	struct Flat;
	Flat* flat = nullptr;
	std::vector<bvh*> blasOwned;
};

// renderer.h / renderer.cpp
// One GPU: exactly the reference's shape.  Several GPUs: UseDevices() before Init() makes Init create
// one rt_ctx per device; Commit() uploads the scene to each; Tick() renders the interleaved rows k, k + n, ... on
// context k from one host thread per context, gathers the rows into context 0's accumulator device to device
// (rt_gather_rows) and resolves there.  Pixels are independent (per-pixel RNG streams), so the frame is the
// one-GPU frame bit for bit.
class Renderer {
public:
	Renderer(int width, int height, int device = 0);
	~Renderer();
	void UseDevices(const std::vector<int>& devs);         // before Init(); a device may be named twice (two contexts on it)
	void UseAllDevices();                                  // every device rt_device_count() reports
	void Init();                                           // renderer.cpp:5-11
	void Commit();                                         // scene.Commit() on every context
	float3 Trace(Ray& ray, int depth, float3 energy);      // renderer.cpp:21   } with scene.raytracer as the Scene holds it: every combination of function
	float3 Sample(Ray& ray, int depth, float3 energy);     // renderer.cpp:128  } and flag the reference's bodies contain (:33-43, :107-121, :143-153 included)
	void Tick(float deltaTime);                            // renderer.cpp:240
	void Shutdown();
	// Q-learning guided sampling of the indirect bounce in path mode (README.md:36-42 of the reference names Dahm & Keller 2017;
	// the snapshot holds no code for it, so this is the library's own statement: rt_qlearn_*, PARITY UNPINNED).  Tick folds the
	// frame's rewards into the table after every path frame; with several contexts their integer reward sums are added first, so
	// every GPU learns the same table and the frame does not depend on how its rows were sharded.
	void EnableQLearning(int grid, float3 lo, float3 hi, float alpha = 0.3f, float epsilon = 0.2f, float qInit = 1.0f);
	void DisableQLearning();
	bool qlearning = false;
	int qgrid = 0;
	uint32_t qlearnMask = 0;          // rt_qlearn_params::learn_mask for the next EnableQLearning (0: every sample pays rewards)
	// Pixel filter of the path-mode camera samples (rt_set_pixel_filter: RT_FILTER_REFERENCE, the default, is the reference's truncated
	// jitter; POINT / BOX / TENT are sub-pixel samples centred on the G-buffer's ray).  Tick sends it to every context with the camera.  A
	// change of kind between two path Ticks is treated like a camera change without a reprojection carry: the Tick clears (the accumulator
	// would mix two estimators), and under 'adaptive' min_samples whole frames follow.  With BOX / TENT under a fisheye camera, or a kind
	// other than REFERENCE with the Q-learning sampler, the path Tick throws (RT_E_UNSUPPORTED).
	int pixelFilter = RT_FILTER_REFERENCE;
	void SyncPixelFilter();           // pixelFilter -> every context, now (Tick does it anyway)
	// Thin lens of the path-mode camera samples (rt_set_lens): lensRadius 0, the default, is the pinhole; with lensRadius > 0 the camera is
	// focused on the plane focusDistance from it (FocusAt gives the distance of what a pixel sees).  Tick sends the lens with the camera and
	// the filter, and treats a change of lens between two path Ticks as it treats a change of filter kind: it clears, with no reprojection
	// carry.  A lens needs a pixelFilter other than REFERENCE and a pinhole camera: otherwise the path Tick throws (RT_E_UNSUPPORTED).
	// (The G-buffer, the denoisers and the carries keep seeing the pinhole ray through the pixel: include/rt_amd.h rt_set_lens, "Limits".)
	float lensRadius = 0.0f;
	float focusDistance = 1.0f;
	void SyncLens();                  // the lens -> every context, now (Tick does it anyway)
	float FocusAt(int x, int y);      // rt_focus_at of context 0 under 'camera' (sent first) and the committed scene: 0 where the pixel sees the sky; sets nothing
	// Shutter of the path-mode camera samples (rt_set_shutter): with 'shutter' set, 'camera' is the camera at shutter open and the four
	// points of shutterCamera the camera at shutter close; every sample looks through the camera interpolated to a time of its own.
	// (shutterCamera's fisheye members are not sent; its change flag is not looked at.)  Tick sends the shutter with the camera, the filter
	// and the lens, and treats a change of it between two path Ticks as it treats a change of lens: it clears, with no reprojection carry.
	// A shutter needs a pixelFilter other than REFERENCE and a pinhole camera: otherwise the path Tick throws (RT_E_UNSUPPORTED).
	// (The G-buffer, the denoisers, the carries and FocusAt see the camera at shutter open: include/rt_amd.h rt_set_shutter, "Limits".)
	bool shutter = false;
	Camera shutterCamera;
	void SyncShutter();               // the shutter -> every context, now (Tick does it anyway)
	// Denoised preview (path mode only): Tick refreshes the G-buffer when something changed (rt_render_aovs, 0.001f as Sample), filters the
	// mean with rt_denoise and shows rt_resolve_denoised in screenPixels; 'accumulator' stays the raw download.  Off: Tick is unchanged.
	// (The G-buffer's ray of a pixel is GetPrimaryRay(x, y): in reference mode one of the up to four integer-pixel rays its samples take,
	// with a pixelFilter the centre of their footprint.)
	bool denoise = false;
	rt_denoise_params denoiseParams = RT_DENOISE_DEFAULTS;
	// Adaptive sampling (path mode only): Tick keeps per-pixel statistics (rt_stats_enable), renders whole frames until every
	// pixel has adaptiveParams.min_samples samples, and from then on one frame of the pixels rt_select_active still finds noisy
	// (rt_render_active); screenPixels is rt_resolve_adaptive (every pixel divided by its own count), 'accumulator' stays the raw download,
	// activePixels is the number of pixels the last Tick sampled.  Switching it on clears the accumulator (the counts start with it); a
	// camera change clears as ever.  Together with denoise (rt_denoise divides by ONE iteration count) or with the Q-learning sampler, Tick
	// throws.  Off: Tick is unchanged.
	// With several contexts every context keeps statistics and does all of this for its own interleaved rows: rt_render_rows and
	// rt_gather_stats_rows in the whole-frame phase, then rt_select_active_rows / rt_select_budget_rows, the pass, and rt_gather_active
	// (the listed pixels alone; rt_gather_stats_rows where the devices are no peers) into context 0, which holds the gathered frame WITH its
	// statistics and resolves, denoises and reprojects it; after a reprojection carry rt_gather_stats_rows pushes each context's rows back
	// to it.  activePixels and passSamples are the sums over the contexts.  The frame, the statistics and both numbers equal the
	// one-context run's bit for bit, with one proviso: adaptiveMaxPassSamples is each CONTEXT's own limit (the fit rule of
	// rt_select_budget_rows sees its shard's total), so the equality holds whenever no fit rule lowered a cap, in either run.
	bool adaptive = false;
	rt_adaptive_params adaptiveParams = RT_ADAPTIVE_DEFAULTS;
	int activePixels = 0;
	// Budgeted adaptive Ticks (adaptivePassCap > 0): every adaptive Tick is one rt_select_budget + rt_render_budget -- each active pixel
	// gets its own number of samples, at most adaptivePassCap of them (and the pass at most adaptiveMaxPassSamples; 0: the context's own
	// limit), in one batch.  There is no whole-frame phase: after a clear every pixel is below min_samples and gets min(min_samples, cap).
	// The passes' frame_base is the value of 'frame' at the last clear or the last reprojection carry, so a pixel's sample k is frame
	// frame_base + k (counted from the carried count after a carry); 'frame' still advances by one per Tick.  passSamples is the number of
	// samples the last Tick took.  0: TickAdaptive is unchanged.  Set it at a clear (before the first adaptive Tick, or together with a
	// camera change that clears): "count n = n frames from frame_base" and the independence of a pixel's samples hold only when every
	// sample since the last clear or carry came from budgeted passes.  Switched on mid-run after frame-by-frame Ticks that followed a carry,
	// a pixel may already hold frame numbers above frame_base + count, and a pass would draw one of them again.
	int adaptivePassCap = 0;
	uint32_t adaptiveMaxPassSamples = 0;
	int passSamples = 0;
	// Dilated selection (adaptiveDilate > 0, at most RT_DILATE_MAX_RADIUS): the adaptive Ticks' selections also list the pixels within that
	// many pixels of an active one (rt_select_active_dilated; rt_select_budget_dilated when adaptivePassCap > 0), so a pixel that missed a
	// rare bright path goes on sampling while its neighbours do.  0: TickAdaptive is unchanged.  With adaptivePassCap == 0 a pixel that is
	// listed again after a pause takes the Tick's frame like every listed pixel: its frames are distinct, not consecutive.  With several
	// contexts (UseDevices) Tick throws: a context that holds one row shard has no statistics for its neighbours' rows.
	int adaptiveDilate = 0;
	// Variance-guided denoised preview of the adaptive frame (needs 'adaptive': the filter reads its statistics; 'denoise' clear): every
	// adaptive Tick ends with rt_render_aovs (0.001f, a no-op on a current G-buffer), rt_denoise_variance and rt_resolve_denoised into
	// screenPixels; 'accumulator' stays the raw download.  Without 'adaptive', Tick throws.  Off: Tick is unchanged.
	bool denoiseVariance = false;
	rt_denoise_var_params denoiseVarParams = RT_DENOISE_VAR_DEFAULTS;
	// Samples carried across a camera move (needs 'adaptive': rt_reproject rewrites the per-pixel statistics).  An adaptive Tick that finds
	// the camera changed, straight after another adaptive Tick (a Whitted Tick in between overwrites the accumulator), with statistics already on and
	// neither the old nor the new camera a fisheye, does not clear: it runs
	// rt_render_aovs under the camera of the last Tick (a no-op on a current G-buffer), rt_history_capture, SyncCamera, rt_render_aovs, rt_reproject, and goes
	// straight on to rt_select_active / rt_render_active (a pixel below min_samples is active by definition).  Otherwise the Tick clears
	// as ever.  Without 'adaptive', Tick throws.  Never set: Tick is unchanged.
	bool reproject = false;
	rt_reproject_params reprojectParams = RT_REPROJECT_DEFAULTS;
	int carriedPixels = 0;            // the pixels the last reprojecting Tick carried
	// Scene::CommitInstances (after bvhInstance::SetTransform on scene.bvhList[...]) for a renderer that may keep its samples.  With
	// 'reproject' and 'adaptive' set, in path mode, straight after an adaptive Tick and with pinhole cameras, it runs rt_render_aovs (a
	// no-op on a current G-buffer) and rt_history_capture under the camera of the last Tick, then scene.CommitInstances(), and the next
	// adaptive Tick carries the samples with rt_reproject_motion instead of clearing -- along the path of the camera carry above (the
	// push-back to the other contexts of UseDevices included), whether the camera moved as well or not.  Otherwise it is
	// scene.CommitInstances() followed by camera.SetChange(true): the next Tick clears, as callers of Scene::CommitInstances do by hand.
	// A Commit() before that Tick (a new upload ends the captured history) makes it clear as well.  If scene.CommitInstances() throws, no
	// carry is pending; context 0 then holds the camera of the last Tick until the next Tick syncs the renderer's camera, as every Tick does.
	void CommitInstances();
	// Scene::CommitTriangles(bv) (after the triangles of bv's mesh were rewritten) for such a renderer, the sibling of CommitInstances: under
	// the same conditions it captures the history the same way, then calls scene.CommitTriangles(bv), and the next adaptive Tick carries
	// the samples with rt_reproject_deform -- which subsumes the motion and the camera carry, so any sequence of CommitInstances and
	// CommitTriangles before that Tick is one capture and one carry.  Otherwise it commits and the next Tick clears.  If
	// scene.CommitTriangles throws, this call leaves no carry pending.
	void CommitTriangles(bvh* bv);
	// Scene::CommitVertices(bv) under the same rules (the carry is rt_reproject_deform's as well)
	void CommitVertices(bvh* bv);
	// Scene::CommitLights / CommitMaterials / CommitSky for a renderer: they commit and the next Tick clears (the clearPending path).  There
	// is no carry, deliberately: every sample holds radiance computed under the old lights, materials or sky, and the device ends a
	// captured history at every level.  A carry that CommitInstances / CommitTriangles left pending becomes that clear.
	void CommitLights();
	void CommitMaterials();
	void CommitSky();
	// Scene::CommitInstanceList along the same path: it commits and the next Tick clears.  No carry either: an instance index names
	// another object afterwards, and the device ends a captured history at every level.
	void CommitInstanceList();
	float4* accumulator = nullptr; // host copy, refreshed by Tick
	uint32_t* screenPixels = nullptr; // Surface::pixels analogue (template/precomp.h:134)
	Scene scene;
	Camera camera;
	int width, height, device;
	rt_ctx* ctx = nullptr;            // context 0: holds the gathered accumulator, resolves the pixels
	std::vector<rt_ctx*> ctxs;        // all contexts, ctxs[0] == ctx
	std::vector<int> devices;
	uint32_t seedBase = 0x12345678; // template/template.cpp:671
	uint32_t frame = 0;
	bool downloadEachTick = true;
	void SyncCamera();
private:
	struct Workers;                   // one parked host thread per context (several contexts only)
	Workers* workers = nullptr;
	void TickAdaptive();              // Tick's path-mode body with 'adaptive' set
	bool adaptiveOn = false;          // the context's statistics were enabled by TickAdaptive
	int wholeFrames = 0;              // whole frames rendered since the accumulator was last cleared
	uint32_t frameBase = 0;           // 'frame' at the last clear or reprojection carry: rt_render_budget's frame_base
	int sampledFilter = RT_FILTER_REFERENCE; // pixelFilter of the last path Tick: the kind the accumulator's samples were taken with
	rt_lens sampledLens{ 0.0f, 1.0f }; // ... and the lens of the last path Tick
	bool LensChanged() const { return lensRadius != sampledLens.radius || (lensRadius > 0.0f && focusDistance != sampledLens.focus_distance); }
	bool sampledShutter = false;      // ... and its shutter: on or off, and the closing record while on
	rt_camera sampledShutterCam{};
	rt_camera ShutterRecord() const;  // shutterCamera's four points as the record rt_set_shutter takes
	bool ShutterChanged() const;
	void ShutterSampled();            // the shutter of this path Tick becomes the sampled one
	rt_camera syncedCam{};            // the record of the last SyncCamera
	bool lastTickAdaptive = false;    // the last Tick was TickAdaptive: the accumulator holds its samples, taken under sampledCam
	rt_camera sampledCam{};           // ... and of the last adaptive Tick: the camera the accumulator's samples were taken with
	bool CaptureForCarry();           // CommitInstances' and CommitTriangles' common head
	void CommitDeformation(bvh* bv, bool fromVertices); // CommitTriangles and CommitVertices
	void CommitLook(void (Scene::*commit)());           // CommitLights, CommitMaterials, CommitSky and CommitInstanceList
	bool motionPending = false;       // CommitInstances / CommitTriangles captured a history and changed the scene: the next adaptive Tick carries across it
	bool deformPending = false;       // ... and one of the changes was a deformation: the carry is rt_reproject_deform
	bool clearPending = false;        // CommitInstances moved instances without a capture, or Commit() followed one: the next Tick clears, with no carry
};

} // namespace rapt
