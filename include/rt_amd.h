/* rt_amd.h -- C ABI of the MI355X trace-loop library (librt_amd.so).
 *
 * This is the drop-in boundary for ONE hot path of Fannollost/Ray-and-pathtracer: the per-pixel
 * trace loop.  The reference has no device boundary (everything is one address space); this
 * library inserts one at the `#pragma omp parallel for` line of Renderer::Tick
 * (renderer.cpp:259): one rt_render() call replaces the whole parallel region, and the batch
 * queries replace Scene::FindNearest / Scene::IsOccluded.  Citations are file:line in the
 * reference repository.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every call returns 0 on success or a
 * negative rt_status; rt_last_error() gives the text.  The caller owns every host buffer.  A
 * context is bound to one GPU and is NOT thread-safe (one host thread per context, one context per
 * GPU).  The library never falls back to a CPU path: without a usable gfx950 device rt_create()
 * fails.
 */
#ifndef RT_AMD_H
#define RT_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

typedef enum {
	RT_OK = 0,
	RT_E_NODEVICE = -1,    /* no HIP device / not gfx950 */
	RT_E_ARG = -2,         /* bad argument */
	RT_E_HIP = -3,         /* HIP runtime error */
	RT_E_UNSUPPORTED = -4, /* scene feature outside the device path (see rt_upload_scene) */
	RT_E_STATE = -5,       /* call order (e.g. render before upload) */
	RT_E_OVERFLOW = -6     /* traversal stack deeper than 130 = tlas.cpp:67 stack[64] + instance sentinel + bvh.cpp:608 stack[64], too many pending Whitted branches, a full call-frame stack in the general Trace / Sample kernels (see rt_set_scene_raytracer), or (Q-learning sampler) more than 2^19 rewards for one (cell, direction) within one batch of frames of a render call (reported by that call) */
} rt_status;

/* ---- scene records -------------------------------------------------------------------------
 * Shapes follow the reference's own structures so a binding can fill them with a few loops.
 * 'material' fields are indices into rt_scene_desc.materials (the reference stores material*). */

/* BVHNode (bvh.h:10-24), 32 bytes, identical layout. leaf: prim_count > 0, left_first = first
 * entry in prim_idx; inner: prim_count == 0, children at left_first and left_first + 1. */
typedef struct { float aabb_min[3]; uint32_t left_first; float aabb_max[3]; uint32_t prim_count; } rt_bvh_node;

/* TLASNode (tlas.h:4-11), 32 bytes, identical layout. leaf: left_right == 0, blas = instance
 * index; inner: children = left_right & 0xFFFF and left_right >> 16. Node 0 is the root. */
typedef struct { float aabb_min[3]; uint32_t left_right; float aabb_max[3]; uint32_t blas; } rt_tlas_node;

/* Triangle (template/scene.h:175-251): v0, v1, v2, N, objIdx, mat (e1, e2, centroid are derived) */
typedef struct { float v0[3], v1[3], v2[3], N[3]; int32_t obj_idx; int32_t material; } rt_triangle;
/* Sphere (template/scene.h:347-394) */
typedef struct { float pos[3]; float r2, invr, r; int32_t obj_idx; int32_t material; } rt_sphere;
/* Plane (template/scene.h:401-448) */
typedef struct { float N[3]; float d; int32_t obj_idx; int32_t material; } rt_plane;

/* Light / AreaLight / DirectionalLight (template/scene.h:75-168) */
enum { RT_LIGHT_AREA = 0, RT_LIGHT_DIRECTIONAL = 1, RT_LIGHT_BASE = 2 };
typedef struct {
	int32_t kind; int32_t obj_idx;
	float pos[3]; float strength; float col[3]; float normal[3];
	float radius;    /* AreaLight */
	float sin_angle; /* DirectionalLight */
} rt_light;

/* material / diffuse / metal / glass (template/scene.h:582-676) */
enum { RT_MAT_DIFFUSE = 1, RT_MAT_METAL = 2, RT_MAT_GLASS = 3 };
typedef struct {
	int32_t type;
	int32_t raytracer; /* material::raytracer as captured at construction */
	float col[3], albedo[3];
	float specu, diffu, shinieness; int32_t N; /* diffuse */
	float ir; float absorption[3];           /* glass */
} rt_material;

/* One bvh object (bvh.h:45-86): node array, primitiveIdx, and the primitive arrays it indexes.
 * prim_idx values < n_tri address triangles, then spheres, then planes (bvh.cpp:618-627).
 * A mesh BVH (bvh(Mesh*)) has n_sph = n_pla = 0. */
typedef struct {
	const rt_bvh_node* nodes; uint32_t nodes_used;
	const uint32_t* prim_idx; uint32_t n_prims;
	const rt_triangle* tris; uint32_t n_tri;
	const rt_sphere* spheres; uint32_t n_sph;
	const rt_plane* planes; uint32_t n_pla;
} rt_blas;

/* bvhInstance (bvhInstance.h): BLAS index + matTransform + invTransform (row-major mat4) */
typedef struct { int32_t blas; float transform[16]; float inv_transform[16]; } rt_instance;

typedef struct {
	/* use_tlas == 0 (template/scene.h:1388): blas[0] is the scene BVH, nothing else is used.
	 * use_tlas != 0: tlas_nodes/instances/blas[] are traversed, brute_spheres/brute_planes are
	 * tested by brute force in FindNearest and ignored by IsOccluded (template/scene.h:1259-1263,
	 * 1288). */
	int32_t use_tlas;
	const rt_blas* blas; uint32_t n_blas;
	const rt_instance* instances; uint32_t n_instances;
	const rt_tlas_node* tlas_nodes; uint32_t tlas_nodes_used;
	const rt_sphere* brute_spheres; uint32_t n_brute_spheres;
	const rt_plane* brute_planes; uint32_t n_brute_planes;
	const rt_light* lights; uint32_t n_lights;
	const rt_material* materials; uint32_t n_materials;
	/* skydome as loaded by stbi_load(..., 3): 8-bit, sky_n channels (template/scene.h:1312-1327).
	 * sky_pixels == NULL: misses return black. */
	const uint8_t* sky_pixels; int32_t sky_w, sky_h, sky_n;
} rt_scene_desc;

/* Camera state read by Camera::GetPrimaryRay (camera.h:24-52) */
typedef struct {
	float cam_pos[3], top_left[3], top_right[3], bottom_left[3];
	int32_t fisheye; float view_angle; float y_angle;
} rt_camera;

/* result of one nearest-hit query: the fields Scene::FindNearest leaves in the Ray
 * (template/scene.h:66-72): t, objIdx (-1 = miss), material index, hitNormal */
typedef struct { float t; int32_t obj_idx; int32_t material; float normal[3]; } rt_hit;

/* work counters = the reference's DataCollector tallies (bvh.cpp:610-631) plus ray counts */
typedef struct {
	uint64_t inner_visits, prim_tests, tlas_inner, instance_visits;
	uint64_t rays_nearest, rays_occluded, brute_tests, light_tests;
} rt_counters;

/* per-kernel device time, measured with HIP events on the context's stream */
typedef struct { uint64_t launches; double ms; } rt_kernel_time;
typedef struct { rt_kernel_time generate, extend, shade, connect, query; } rt_profile;

enum { RT_MODE_WHITTED = 0, RT_MODE_PATH = 1 };

/* ---- lifetime ------------------------------------------------------------------------------ */
int rt_device_count(void);
/* Replaces Renderer::Init (renderer.cpp:5-11): allocates the float4 accumulator [width*height] in
 * HBM (zeroed) plus the path-state arrays.  Returns NULL on failure (rt_last_error(NULL)). */
rt_ctx* rt_create(int device, int width, int height);
void rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);

/* ---- scene / camera -------------------------------------------------------------------------- */
/* Copies the scene into HBM in the traversal layout.  Replaces the pointers Scene keeps to
 * bvh / tlas / bvhInstance / primitive vectors (template/scene.h:1371-1378).
 * RT_E_UNSUPPORTED: more than 32 lights, or a TLAS with more than 256 instances. */
int rt_upload_scene(rt_ctx* ctx, const rt_scene_desc* desc);
int rt_set_camera(rt_ctx* ctx, const rt_camera* cam);
/* Scene::SetTime(t) with animation on (template/scene.h:1228-1244): every triangle of the scene BVH
 * is deformed from its ORIGINAL (uploaded) vertices -- rotation about z by a*y*0.2, a = sin(fmod(t,
 * 2*pi))/2 -- its normal re-derived (Triangle::update, template/scene.h:238-246) and the BVH refitted
 * bottom-up (bvh::Refit, bvh.cpp:556-594), all on the GPU.  Non-TLAS scenes only (the reference's
 * animOn is false under useTLAS, template/scene.h:1389).  t = 0 restores the uploaded geometry. */
int rt_set_time(rt_ctx* ctx, float t);
/* The traversal layout rt_upload_scene copies to the device, built on the host and handed to the caller: no device, no context.  For tests
 * and tools that want to look at what upload makes of a description (csrc/rt_layout.h describes the records).
 * rt_layout_build: wide (-1 / 0 / 1), wide8 and tlas_lds are the values of RT_WIDE, RT_WIDE8 and RT_TLAS_LDS a context would have read.
 *   NULL on failure: rt_last_error(NULL) then holds the message, and the status is the one rt_upload_scene returns for that description.
 * rt_layout_array: *data / *bytes of array 'which' (owned by the layout, valid until rt_layout_free; an array that was not built has 0 bytes):
 *   PAIRS, PRIMS, WIDE, LEAFBOX, REACH, BRUTE f32; WIDE8, REFIT_ORDER, ROOT_LINK, ROOT_WIDE, ROOT_WIDE8 (the last three per BLAS) u32;
 *   REFIT_LEVEL_START i32; INST 128-byte, LIGHTS 56-byte and MATS 64-byte device records; REACH and BRUTE end with 16 spare words.
 *   SCALARS: 14 32-bit words in this order: rootLink, tlasBase, tlasPairs, nInst, reachOriginMax (the f32's bits), tlasLds, stackRows,
 *   nBruteSph, nBrutePla, wideOK, wide8OK, pathUnsupported, animSlots, refitLevels.  RT_E_ARG: a null pointer, an unknown array. */
typedef struct rt_layout rt_layout;
enum { RT_LAYOUT_PAIRS = 0, RT_LAYOUT_PRIMS, RT_LAYOUT_WIDE, RT_LAYOUT_WIDE8, RT_LAYOUT_LEAFBOX, RT_LAYOUT_REACH, RT_LAYOUT_BRUTE, RT_LAYOUT_INST,
       RT_LAYOUT_LIGHTS, RT_LAYOUT_MATS, RT_LAYOUT_REFIT_ORDER, RT_LAYOUT_REFIT_LEVEL_START, RT_LAYOUT_ROOT_LINK, RT_LAYOUT_ROOT_WIDE,
       RT_LAYOUT_ROOT_WIDE8, RT_LAYOUT_SCALARS };
rt_layout* rt_layout_build(const rt_scene_desc* desc, int wide, int wide8, int tlas_lds);
int rt_layout_array(const rt_layout* layout, int which, const void** data, size_t* bytes);
void rt_layout_free(rt_layout* layout);
/* Which kernel instantiations the dense path-mode pipeline launches for a batch, and which any-hit walk a queue of shadow rays takes: the
 * host's decisions (csrc/rt_forms.h) without a device or a context, for tests/test_forms_cpu.py.
 * rt_launch_form: facts = { primary table current, bounce table current, chain levels the batch may read (1-4), RT_BOUNCE_TABLE != 0,
 *   RT_ROUND0_ENTRIES, sampler on, fisheye camera, rounds }; round in [0, rounds).  out = { generate kernel (0 k_generate_c, 1 k_generate_t,
 *   2 k_generate_s), k_shade_s's template bits (1 QL, 2 BOUNCE, 4 TABLE0, 8 CHAIN), k_light_s's TABLE0 over this round's shadow records,
 *   the same over the round before's (the launch of a mixed round; -1 at round 0), shade's BounceTable argument (0 empty, 1 the bounce
 *   table, 2 chain level round + 1), its PrimaryTable argument (0 empty, 1 the table), whether it is handed the RT_BOUNCE_TABLE mask,
 *   fresh }.  RT_E_ARG: a null pointer, a round or a level count out of range; RT_E_STATE: a combination no kernel was built for.
 * rt_any_hit_walk: 0 binary, 1 counting, 2 4-wide, 4 8-wide (3 is the walk over the list a wide walk hands back: never chosen). */
int rt_launch_form(const int32_t* facts, int round, int32_t* out);
int rt_any_hit_walk(int counting, int wide, int wide8);

/* ---- the pixel loop ---------------------------------------------------------------------------- */
/* Replaces the pixel loop of Renderer::Tick (renderer.cpp:259-285) for frames
 * [frame0, frame0 + nframes) and rows [y0, y1): per pixel, Camera::GetPrimaryRay then
 * Renderer::Trace (mode RT_MODE_WHITTED, renderer.cpp:21-126; nframes must be 1) or
 * Renderer::Sample (RT_MODE_PATH, renderer.cpp:128-236), accumulated into the accumulator exactly
 * as :270 / :279-282 do.  The random stream of pixel p in frame f starts at
 * InitSeed(seed_base + p + f*width*height) (template/template.cpp:680-683; the single index whose
 * hash is 0 starts at 0x9E3779B9 instead, because xorshift32 cannot leave state 0).
 * max_depth is the depth argument of Trace (4 at renderer.cpp:269); Sample always starts at 4.
 * In RT_MODE_PATH a scene with a diffuse material that has shinieness != 0 or raytracer == 0 (random
 * draws then interleave with shadow queries in depth-first order) is rendered by a slower
 * one-lane-per-sample kernel instead of the wavefront kernels; results follow the same definition. */
int rt_render(rt_ctx* ctx, int mode, uint32_t frame0, int nframes, uint32_t seed_base, int y0, int y1, int max_depth);
/* Same for the rows row_first + k*row_stride, k < row_count: the row-interleaved pixel shard used
 * when the frame is split over several GPUs (rank r of n renders row_first = r, row_stride = n). */
int rt_render_rows(rt_ctx* ctx, int mode, uint32_t frame0, int nframes, uint32_t seed_base, int row_first, int row_stride, int row_count, int max_depth);
/* ---- pixel filter: sub-pixel camera samples in path mode ------------------------------------------------------------------
 * The reference's Tick draws a jitter and GetPrimaryRay(const int, const int) truncates it: every path sample of pixel (x, y) looks through
 * the corner of one of the integer pixels [x - 1, x] x [y - 1, y], and a converged frame is a 2 x 2 box blur of a point-sampled image.
 * RT_FILTER_REFERENCE (the default of a context) is that, bit for bit.  The other kinds apply to RT_MODE_PATH camera samples -- rt_render,
 * rt_render_rows, rt_render_active, rt_render_budget -- and change nothing else: Whitted mode and rt_trace_batch* ignore the filter.
 * Definition for sample (pixel p = y * width + x, frame f, seed_base); all arithmetic f32, IEEE divide and square root, no contraction:
 *   s  = seed_base + p + f * width * height                       (uint32, wrapping)
 *   the path's random stream starts at StreamSeed(s) = InitSeed(s), or 0x9E3779B9 where that is 0, with NO draw consumed: the stream
 *   rt_trace_batch gives ray s - seed_base (reference mode starts the path two draws in: they were its jitter);
 *   js = StreamSeed(~s); u1 = RandomFloat(js); u2 = RandomFloat(js)  (a stream of its own: the offset is not tied to the first bounce)
 *   dx = o(u1), dy = o(u2) with  POINT: o(u) = 0 (no draw is made)
 *                                BOX:   o(u) = u - 0.5f
 *                                TENT:  o(u) = u < 0.5f ? sqrtf(2 * u) - 1 : 1 - sqrtf(2 - 2 * u)       (radius 1 pixel)
 *   (RandomFloat can return 1.0f: the offsets lie in the closed intervals [-0.5, 0.5] and [-1, 1])
 *   fx = (float)x + dx; fy = (float)y + dy
 *   the ray is Camera::GetPrimaryRay's on u = fx * (1.0f / width), v = fy * (1.0f / height): P = topLeft + u * (topRight - topLeft) +
 *   v * (bottomLeft - topLeft), D = normalize(P - camPos); integral fx, fy give GetPrimaryRay(x, y)'s bits.
 * The filter is centred on the ray rt_render_aovs traces for the pixel, not on x + 0.5.  A sample is accumulated into its own pixel (filter
 * importance sampling, no splatting), so it stays a function of (seed_base, pixel, frame, kind): lists, budget plans, row shards, the
 * statistics, rt_reproject and both denoisers compose with it as they do with the reference's samples.
 * A fisheye camera: POINT is GetPrimaryRay(x, y) itself; BOX / TENT make the render calls return RT_E_UNSUPPORTED (nothing pins them).
 * With the Q-learning sampler on and a kind other than REFERENCE set, the render calls return RT_E_UNSUPPORTED (its learn_mask is defined
 * on the post-jitter state).  rt_set_pixel_filter does not clear the accumulator and does not make the G-buffer stale; the primary-hit table
 * (RT_PRIMARY_TABLE) serves reference-mode batches only: with a filter kind every camera ray is traced.  RT_E_ARG: an unknown kind.
 * rt_sample_rays: the camera rays of one frame's path samples under the context's kind (REFERENCE included), rows [y0, y1): O_out, D_out
 *   3 floats per pixel, row-major; one launch, a lane per pixel, counted as a query in rt_get_profile.  Synchronous.  RT_E_UNSUPPORTED:
 *   BOX / TENT under a fisheye camera. */
enum { RT_FILTER_REFERENCE = 0, RT_FILTER_POINT = 1, RT_FILTER_BOX = 2, RT_FILTER_TENT = 3 };
int rt_set_pixel_filter(rt_ctx* ctx, int kind);
int rt_get_pixel_filter(const rt_ctx* ctx);
int rt_sample_rays(rt_ctx* ctx, uint32_t frame, uint32_t seed_base, int y0, int y1, float* O_out, float* D_out);
/* ---- thin lens: depth of field for path-mode camera samples ------------------------------------------------------------------
 * The reference's camera is a pinhole: every sample of a pixel leaves from cam_pos.  rt_set_lens gives the camera a circular aperture of
 * 'radius' (world units) focused on the plane parallel to the screen rectangle, focus_distance from cam_pos along its normal.  The
 * reference has no lens: this is the library's own definition, restated in numpy by tests/lens_ref.py.  radius 0 (a context's default,
 * and what a NULL lens sets) is off: no lens draw is made and every bit is the pixel filter's.
 * Definition of camera sample (pixel (x, y), frame f, seed_base) with radius > 0; all arithmetic f32, IEEE divide and square root, no
 * contraction; s, StreamSeed, RandomFloat, o(), u, v are rt_set_pixel_filter's above; dot, cross and normalize are rt_reproject's and
 * rt_reproject_motion's below; TL, TR, BL, cam are the camera's top_left, top_right, bottom_left, cam_pos:
 *   the path's random stream: StreamSeed(s), nothing drawn (unchanged)
 *   js = StreamSeed(~s)
 *   BOX / TENT: u1 = RandomFloat(js); u2 = RandomFloat(js); dx = o(u1); dy = o(u2)        (POINT: no draw, dx = dy = 0)
 *   the lens point, by rejection, on the SAME stream js, behind the filter's draws:
 *     a = b = 0
 *     for k in 0 .. RT_LENS_TRIES - 1:
 *         ca = RandomFloat(js) * 2 - 1;  cb = RandomFloat(js) * 2 - 1
 *         if ca * ca + cb * cb <= 1.0f: a = ca; b = cb; stop       (a sample refused RT_LENS_TRIES times looks through the lens centre)
 *   A = TR - TL;  B = BL - TL;  N = cross(A, B);  E = TL - cam
 *   screen_dist = fabsf(dot(E, N)) / sqrtf(dot(N, N))
 *   lam = focus_distance / screen_dist                              (one number per camera and lens; the library computes it on the host)
 *   P = (TL + u * A) + v * B   with u = (x + dx) * (1.0f / width), v = (y + dy) * (1.0f / height)          (GetPrimaryRay's P)
 *   F = cam + lam * (P - cam)                                       (the point of the focal plane the pinhole ray looks at)
 *   O = (cam + (a * radius) * normalize(A)) + (b * radius) * normalize(B)
 *   D = normalize(F - O)
 * The lens applies to the RT_MODE_PATH camera samples of rt_render, rt_render_rows, rt_render_active and rt_render_budget and to
 * rt_sample_rays; Whitted mode, rt_trace_batch*, rt_render_aovs and rt_primary_hits ignore it.  A sample stays a function of (seed_base,
 * pixel, frame, kind, lens) and is accumulated into its own pixel: lists, budget plans, row shards, the statistics and the split of frames
 * into calls compose with it as with the filter.  From those calls, with radius > 0, RT_E_UNSUPPORTED (never a silent pinhole):
 *   - kind RT_FILTER_REFERENCE (its jitter lives on the path's own stream, and the primary-hit and bounce tables serve that mode: set a
 *     kind with rt_set_pixel_filter first);
 *   - a fisheye camera;
 *   - lam not finite and > 0 (a degenerate screen rectangle);
 *   - (the Q-learning sampler is refused with any filter kind already).
 * rt_set_lens does not clear the accumulator, does not make the G-buffer stale, does not end a captured history and drops no list or
 * plan.  RT_E_ARG, checked before the context is touched: a radius that is negative or not finite; with radius > 0 a focus_distance
 * that is not finite and > 0.
 * Limits: the G-buffer, both denoisers and the three reprojections keep seeing the pinhole ray through the pixel.  A pixel far out of focus
 * mixes surfaces its G-buffer record does not describe: the denoisers' edge stops are too sharp there, and a carry moves its samples as if
 * the point were in focus (rt_reproject_params::max_history is the remedy at hand).  A circular aperture only: no blades, no anamorphic lens.
 * rt_focus_at (autofocus): the focus distance that puts what pixel (x, y) sees in focus -- Camera::GetPrimaryRay(x, y) and
 *   Scene::FindNearest(0.001f): *distance_out = t * (fabsf(dot(D, N)) / sqrtf(dot(N, N))), N as above; a miss writes 0.0f and returns
 *   RT_OK.  It does NOT set the lens.  Synchronous; one query in rt_get_profile.  RT_E_ARG: a pixel outside the frame, a null pointer;
 *   RT_E_STATE: no scene; RT_E_UNSUPPORTED: a fisheye camera. */
typedef struct { float radius; float focus_distance; } rt_lens;   /* radius 0: off (a context's default) */
#define RT_LENS_TRIES 16
int rt_set_lens(rt_ctx* ctx, const rt_lens* lens);     /* NULL: off */
int rt_get_lens(const rt_ctx* ctx, rt_lens* out);
int rt_focus_at(rt_ctx* ctx, int x, int y, float* distance_out);
/* ---- shutter: camera motion blur for path-mode camera samples ------------------------------------------------------------------
 * Every path sample of a batch is otherwise taken at one instant, through the context's one rt_camera record.  rt_set_shutter makes that
 * record the camera at shutter OPEN and gives the context a second record, the camera at shutter CLOSE: every path-mode camera sample
 * draws a time tau of its own in [0, 1] and looks through the camera interpolated to that time.  The reference has no shutter: this is
 * the library's own definition, restated in numpy by tests/shutter_ref.py.  A NULL record switches the shutter off (a context's
 * default): no time is drawn and every bit is the pixel filter's and the lens's.
 * Definition of camera sample (pixel (x, y), frame f, seed_base) with the shutter on; all arithmetic f32, IEEE divide and square root, no
 * contraction; s, StreamSeed, RandomFloat, o(), dot, cross, normalize and RT_LENS_TRIES are rt_set_pixel_filter's and rt_set_lens's above;
 * X0 is any of the twelve floats cam_pos, top_left, top_right, bottom_left of the context's camera, X1 the same float of cam_close:
 *   the path's random stream: StreamSeed(s), nothing drawn (unchanged)
 *   js = StreamSeed(~s)
 *   BOX / TENT: u1 = RandomFloat(js); u2 = RandomFloat(js); dx = o(u1); dy = o(u2)        (POINT: no draw, dx = dy = 0)
 *   tau = RandomFloat(js)                    (behind the filter's draws, in front of the lens's; the CLOSED interval [0, 1])
 *   X(tau) = X0 + tau * (X1 - X0)            per float, for all twelve
 *   without a lens: the pixel filter's ray -- GetPrimaryRay's P and D on u = (x + dx) * (1.0f / width), v = (y + dy) * (1.0f / height) --
 *     computed on the camera X(tau): O = cam(tau), D = normalize(P - cam(tau));
 *   with a lens (radius > 0): rt_set_lens's ray on the camera X(tau).  The rejection pairs continue on js behind tau, and lam is
 *     evaluated per sample on the device, lam = focus_distance / (fabsf(dot(E, N)) / sqrtf(dot(N, N))) with A, B, N, E of X(tau).
 *     (With the shutter off lam stays the host's number, and every bit is what rt_set_lens alone gives.)
 * tau = 1.0f does not give X1's bits in general (X0 + (X1 - X0) rounds twice).  A closing record that equals the open camera gives
 * X(tau) = X0 exactly (X1 - X0 = 0); it still consumes the tau draw, so without a lens its rays are the pixel filter's bit for bit, but
 * with a lens the lens point comes from later draws and it is NOT bit-equal to the shutter switched off.
 * The shutter applies to the RT_MODE_PATH camera samples of rt_render, rt_render_rows, rt_render_active and rt_render_budget and to
 * rt_sample_rays; Whitted mode, rt_trace_batch*, rt_render_aovs, rt_primary_hits and rt_focus_at ignore it.  A sample stays a function of
 * (seed_base, pixel, frame, kind, lens, shutter) and is accumulated into its own pixel: split calls, row shards, lists, budget plans, the
 * statistics and rt_gather_* compose with it as with the lens.  From those calls, with the shutter on, RT_E_UNSUPPORTED (never a silent
 * still camera):
 *   - kind RT_FILTER_REFERENCE (the lens's rule: its jitter lives on the path's own stream and the hit tables serve that mode);
 *   - a fisheye open camera;
 *   - with a lens: lam at the open or at the closing camera not finite and > 0;
 *   - (the Q-learning sampler is refused with any filter kind already).
 * rt_set_shutter: RT_E_ARG, checked before the context is touched, for a float among cam_close's twelve that is not finite and for
 * cam_close->fisheye != 0; view_angle and y_angle are not looked at.  It does not clear the accumulator, does not make the G-buffer
 * stale, does not end a captured history and drops no list or plan.  rt_set_camera keeps the shutter: the closing record is the
 * caller's to update when the open camera moves.  The record is copied to the device on the context's stream.
 * rt_get_shutter returns 1 (on; *out = the record as it was set), 0 (off; *out untouched) or a negative rt_status.
 * Limits: camera motion only -- objects do not blur (moving instances and deforming meshes would need a time in the traversal state).
 * The G-buffer, both denoisers, the three reprojections and rt_focus_at see the camera at shutter open.  A pixel that the motion sweeps
 * over several surfaces mixes surfaces its G-buffer record does not describe: the denoisers' edge stops are too sharp there, and a carry
 * moves its samples as if the camera stood still at shutter open.  The time is uniform and unstratified: no shutter efficiency curve,
 * no rolling shutter. */
int rt_set_shutter(rt_ctx* ctx, const rt_camera* cam_close);   /* NULL: off (a context's default) */
int rt_get_shutter(const rt_ctx* ctx, rt_camera* out);         /* 1: on, *out = the record; 0: off, *out untouched; < 0: an rt_status */
/* memset of the accumulator (renderer.cpp:9, :274) */
int rt_clear(rt_ctx* ctx);
/* rows [y0, y1) of the float4 accumulator -> host (Renderer::accumulator, renderer.h:98) */
int rt_download_accumulator(rt_ctx* ctx, int y0, int y1, float* out);
/* screen->pixels for rows [y0, y1): RGBF32_to_RGB8(accumulator / iteration) (renderer.cpp:287-290,
 * template/precomp.h:445-448) */
int rt_resolve(rt_ctx* ctx, int iteration, int y0, int y1, uint32_t* rgb8_out);
/* Device address of the accumulator (width*height float4), and rebinding it to caller-owned device
 * memory (e.g. a torch tensor handed to an RCCL gather).  The caller keeps that memory alive. */
void* rt_accumulator_device_ptr(rt_ctx* ctx);
int rt_bind_accumulator(rt_ctx* ctx, void* device_ptr);
/* Multi-GPU from one process (one host thread + one rt_ctx per GPU): copy the accumulator rows
 * row_first + k*row_stride, k < row_count, that context src rendered into the same rows of context dst's
 * accumulator -- device to device over xGMI (peer access is enabled on first use; without it the rows are
 * copied one by one through hipMemcpyPeerAsync).  Asynchronous: the copy is a push queued on src's stream behind
 * the rendering already queued there (several sources push over their own links at the same time) AND behind
 * whatever was queued on dst's stream when the call was made (rt_clear's memset, dst's own resolve of the frame
 * before: src's stream waits for an event recorded on dst's stream first), and dst's stream is made to wait for
 * it, so whatever is queued on dst afterwards (rt_resolve, rt_download_accumulator, the next frame) sees the
 * rows; the host does not wait.  src's accumulator must not be re-bound or freed before dst has synchronised.
 * May be called from src's host thread while another thread drives dst (only stream operations touch dst; EVERY
 * error of the call, the argument checks included, is reported on src: rt_last_error(src)).  Both contexts
 * must have the same width and height.  rt_device_of: the HIP device a context lives on.
 * rt_gather_begin(dst): called by dst's owner ONCE PER FRAME, after whatever must precede the frame's rows on dst (rt_clear, the
 * resolve of the frame before) and BEFORE dst's own share of the frame is queued: it marks "dst's rows are free" on dst's stream,
 * and every rt_gather_rows into dst until the next rt_gather_begin waits for that mark only -- not for dst's own rendering of
 * the frame, and not for the pushes of the sources that called earlier: the pushes then run side by side, each over its own
 * xGMI link.  Without it (never called on dst) every gather orders itself behind all that dst's stream held when it was
 * called, which is correct and serialises the pushes behind dst's rendering.
 * rt_gather_stats_rows: rt_gather_rows for the accumulator AND the three statistics arrays (count, sum_y, sum_yy: 28 B per pixel) of
 *   those rows -- what dst needs to run rt_resolve_adaptive, rt_denoise_variance or rt_reproject on a gathered frame.  The same ordering
 *   (the rt_gather_begin mark, or "behind all dst holds now"), errors on src, RT_OK without work when dst == src.  RT_E_STATE: statistics
 *   off on either context.  Either direction: a push from the context that holds the frame to the one that renders those rows is how
 *   rows rewritten there (rt_reproject) get back to their owner.
 * rt_gather_active: pushes accumulator, count, sum_y and sum_yy of the pixels on src's installed active-pixel list (rt_select_active,
 *   rt_select_budget, their _rows forms, rt_set_active_pixels), and nothing else, into the same pixels of dst: after a pass over the list
 *   only they have changed on src.  One kernel on src's stream, a lane per entry, stores through dst's pointers (the same device, or a
 *   peer: access is enabled on first use); ordering as above.  Every pixel of dst that is not on the list is not written.  The caller's
 *   part: the listed pixels must not be written by dst's own queued work in the meantime (disjoint row shards give this for free).
 *   dst's own list and plan are not touched.  src's list outlives rt_render_budget, which consumes only the plan, so the call serves after
 *   either kind of pass.  An empty list: RT_OK without a launch.  RT_E_STATE: no list on src, statistics off on either context.
 *   RT_E_ARG: the sizes differ.  RT_E_UNSUPPORTED (never a silent fallback): dst lives on another device that src's device cannot access
 *   as a peer -- the caller then pushes the rows with rt_gather_stats_rows. */
int rt_gather_begin(rt_ctx* dst);
int rt_gather_rows(rt_ctx* dst, rt_ctx* src, int row_first, int row_stride, int row_count);
int rt_gather_stats_rows(rt_ctx* dst, rt_ctx* src, int row_first, int row_stride, int row_count);
int rt_gather_active(rt_ctx* dst, rt_ctx* src);
int rt_device_of(const rt_ctx* ctx);
/* PCI address ("0000:c1:00.0") of HIP device 'device' into out[cap >= 16]: the ranks of a multi-process run exchange these to
 * prove that no two of them render on the same GPU (bench.py ranks_devices). */
int rt_device_pci_bus_id(int device, char* out, int cap);

/* ---- batch queries ---------------------------------------------------------------------------- */
/* Scene::FindNearest(ray, t_min) (template/scene.h:1248-1267) for n rays. O, D: n*3 floats;
 * tmax: n floats or NULL (1e34f, the Ray constructor default, template/scene.h:42). */
int rt_intersect_batch(rt_ctx* ctx, int n, const float* O, const float* D, const float* tmax, float t_min, rt_hit* out);
/* Scene::IsOccluded(ray) (template/scene.h:1286-1291) for n rays; out[i] = 0 / 1 */
int rt_occluded_batch(rt_ctx* ctx, int n, const float* O, const float* D, const float* tmax, uint8_t* out);
/* The queries BELOW Scene level, with the reference's own names: scope
 *   RT_SCOPE_SCENE     Scene::FindNearest / Scene::IsOccluded (what the two calls above do)
 *   RT_SCOPE_ACCEL     the scene's accelerator alone: bvh::Intersect / IsOccluded of the scene bvh (bvh.cpp:596-604) or
 *                      tlas::Intersect / IsOccluded (tlas.cpp:65-122): no lights, no brute-force primitives
 *   RT_SCOPE_BLAS      bvh::Intersect / IsOccluded of BLAS 'index' in its own object space
 *   RT_SCOPE_INSTANCE  bvhInstance::BIntersect / IsOccluded of instance 'index' (bvhInstance.cpp:3-35): ray to object
 *                      space, normal back to world
 * t_min matters for RT_SCOPE_SCENE only (the BVH uses 0.0001, bvh.cpp:607). */
enum { RT_SCOPE_SCENE = 0, RT_SCOPE_ACCEL = 1, RT_SCOPE_BLAS = 2, RT_SCOPE_INSTANCE = 3 };
int rt_intersect_scope(rt_ctx* ctx, int scope, int index, int n, const float* O, const float* D, const float* tmax, float t_min, rt_hit* out);
int rt_occluded_scope(rt_ctx* ctx, int scope, int index, int n, const float* O, const float* D, const float* tmax, uint8_t* out);
/* Scene::GetSkyColor (template/scene.h:1312-1327) for n directions (D: n*3 floats, rgb_out: n*3 floats) */
int rt_sky_color_batch(rt_ctx* ctx, int n, const float* D, float* rgb_out);
/* Camera::GetPrimaryRay(x, y) + Scene::FindNearest(t_min) for every pixel ("primary rays only") */
int rt_primary_hits(rt_ctx* ctx, float t_min, int32_t* obj_idx_out, float* t_out);
/* Renderer::Trace / Renderer::Sample on caller-supplied rays: rgb_out[n*3].  Stream i starts at
 * InitSeed(seed_base + i).  Any depth is accepted; the one-lane-per-call-tree kernels hold at most 12 (Trace) / 6 (Sample) nested call
 * frames and answer a deeper nesting with RT_E_OVERFLOW: see rt_set_scene_raytracer. */
int rt_trace_batch(rt_ctx* ctx, int mode, int n, const float* O, const float* D, int depth, uint32_t seed_base, float* rgb_out);
/* scene.raytracer as the caller's Scene holds it, for rt_trace_batch*: -1 (default) the flag follows the function called -- Trace with the
 * flag set, Sample with it clear, as Renderer::Tick calls them (renderer.cpp:268-283); 0 / 1: the flag's value.  Trace with the flag clear
 * (Russian roulette, sampled light positions, an indirect child: renderer.cpp:33-43, 107-121) and Sample with it set (:143-153) are what the
 * reference's Renderer::Trace / Sample compute when called that way; the device evaluates them one lane per call tree (slow path,
 * correctness only; not with the Q-learning sampler on: RT_E_UNSUPPORTED).  rt_render ignores the flag (it is Tick's loop).
 * Both general kernels (k_trace_general, k_sample_general) run one lane per call tree: ray i's whole recursion is one lane's loop, so a wave
 * holds 64 unrelated trees and lasts as long as its longest, and the cost of a call grows with n and the depth, not with a frame's size.
 * Frame limits of that slow path (it also serves Sample on a scene with a shiny diffuse material or one built with raytracer == false): a
 * call tree may hold at most 12 nested call frames in Trace and 6 in Sample.  A frame is a shiny diffuse hit waiting for its mirror child
 * (in Trace also a glass hit's reflection child waiting for the refraction child).  The limits bound the frames nested at one moment, not
 * the depth argument as such: two facing shiny surfaces reach them at depth 12 (Trace) and 5 (Sample), a scene without such hits never
 * does.  Past them the call returns RT_E_OVERFLOW, rt_last_error names the call-frame stack and the limit, rgb_out is left unwritten and
 * the context stays usable: start at a lower depth. */
int rt_set_scene_raytracer(rt_ctx* ctx, int flag);
/* The same with Trace / Sample's third argument: energy[3] instead of float3(1) */
int rt_trace_batch_energy(rt_ctx* ctx, int mode, int n, const float* O, const float* D, int depth, uint32_t seed_base, const float* energy, float* rgb_out);

/* ---- G-buffer and denoised preview ------------------------------------------------------------------
 * rt_render_aovs: the G-buffer of the frame -- per pixel, Camera::GetPrimaryRay(x, y) + Scene::FindNearest(t_min) (in reference mode ONE of
 *   the up to four integer-pixel rays the pixel's path samples take: Tick's jitter, truncated by GetPrimaryRay's int parameters, lands on
 *   pixels [x - 1, x] x [y - 1, y]; with a pixel filter set, rt_set_pixel_filter, the ray the pixel's samples are centred on) as the rt_hit record rt_intersect_batch gives,
 *   an albedo (diffuse: col * albedo, metal / glass: col, a light: the light's col, a miss: 0) and the world position O + D * t (f32).
 *   t_min: 0.001f is what Sample uses (renderer.cpp:133), 1e-6f what Trace uses.  The buffers belong to the context (allocated on first
 *   use); the launch counts as a query in rt_get_profile.  The G-buffer goes stale with rt_upload_scene, rt_set_time and an rt_set_camera
 *   whose record differs byte-wise from the current one (an unchanged camera sent every Tick keeps it); on a current G-buffer with the same
 *   t_min the call returns at once without a launch.  Synchronous.
 * rt_download_aovs: rows [y0, y1) of the G-buffer: hits_out (rt_hit per pixel) and / or albedo_rgb_out (3 floats per pixel); either NULL.
 * rt_denoise: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of the mean colour accumulator / iteration (whatever
 *   accumulator is bound), on the whole frame, on the context's stream, without synchronising.  Definition (tests/denoise_ref.py restates it):
 *     c_p = acc_p.xyz / iteration (f32, as rt_resolve); a pixel with a non-finite component is passed through and is no tap of any neighbour;
 *     for i = 0 .. iterations - 1, step s = 2^i: taps at s * (dx, dy), dx, dy in [-2, 2], B3-spline h = (1/16, 1/4, 3/8, 1/4, 1/16),
 *     taps outside the image or non-finite skipped, w = h[dx] h[dy] exp(-(|c_p - c_q|^2 kc_i + |n_p - n_q|^2 kn + |x_p - x_q|^2 / t_p^2 kx
 *     + |a_p - a_q|^2 ka)), kc_i = 4^i / sigma_color^2, kn = 1 / sigma_normal^2, kx = 1 / sigma_position^2, ka = 1 / sigma_albedo^2 (f32;
 *     sigma = +inf drops its term).  Every k is clamped to FLT_MAX where it overflows: kc_i as the f32 product (1 / sigma_color^2) 4^i,
 *     kn, kx, ka, and kx / t_p^2 per pixel.  A zero distance then weighs exp(0) = 1 and a nonzero one under a tiny sigma about 0, so a
 *     tiny sigma mixes only neighbours identical in that feature and never produces NaN; two misses compare colour only, a hit and a miss do not mix (w = 0); out = sum w c_q / sum w, w channel 0.
 *   params NULL: RT_DENOISE_DEFAULTS.  RT_E_ARG: iteration < 1, iterations outside 1..8, a sigma <= 0 or NaN.  RT_E_STATE: the G-buffer is
 *   missing or stale (rt_render_aovs first).  The accumulator is not written.
 * rt_download_denoised: rows [y0, y1) of the last rt_denoise result (float4 per pixel).
 * rt_resolve_denoised: RGBF32_to_RGB8 of those rows (rt_resolve of the denoised mean, iteration 1). */
typedef struct { int32_t iterations; float sigma_color, sigma_normal, sigma_position, sigma_albedo; } rt_denoise_params;
#define RT_DENOISE_DEFAULTS { 5, 0.5f, 0.25f, 0.1f, 0.1f }
int rt_render_aovs(rt_ctx* ctx, float t_min);
int rt_download_aovs(rt_ctx* ctx, int y0, int y1, rt_hit* hits_out, float* albedo_rgb_out);
int rt_denoise(rt_ctx* ctx, int iteration, const rt_denoise_params* params);
int rt_download_denoised(rt_ctx* ctx, int y0, int y1, float* out);
int rt_resolve_denoised(rt_ctx* ctx, int y0, int y1, uint32_t* rgb8_out);

/* ---- adaptive sampling: per-pixel statistics and active-pixel batches --------------------------------------
 * Path mode (RT_MODE_PATH).  A list belongs to one context; several contexts that shard the frame by rows each select over their own
 * rows (rt_select_active_rows) and push what they sampled to the context that holds the frame (rt_gather_stats_rows, rt_gather_active,
 * below).  Unused, nothing else changes.  (This library's own addition: the reference samples every pixel alike.)
 * rt_stats_enable(on != 0): allocates and zeroes three per-pixel buffers (12 B per pixel); while they exist every path-mode accumulation
 *   (rt_render, rt_render_rows, rt_render_active) also keeps, per pixel, count (uint32: samples added), sum_y and sum_yy (f32): with
 *   y = (0.2126f * r + 0.7152f * g) + 0.0722f * b of the sample exactly as it is added to the accumulator (after the gamma), f32 in that order
 *   without contraction, y and y * y are added one at a time in frame order like the accumulator, so the values do not depend on how
 *   frames are split into batches or calls.  rt_clear zeroes them with the accumulator; on == 0 frees them.  Whitted frames do not touch
 *   them.  The accumulator's bits do not depend on whether they are on.
 * rt_download_stats: rows [y0, y1) of the three buffers; any pointer may be NULL.  RT_E_STATE when statistics are off.
 * rt_select_active: builds the context's active-pixel list on the device from the statistics.  Per pixel, all arithmetic f32 with IEEE
 *   division and square root, ternaries as written (tests/adaptive_ref.py restates it and is compared exactly):
 *     n = (float)count
 *     m = sum_y / n
 *     v = (sum_yy - sum_y * m) / (n - 1)
 *     v = v > 0 ? v : 0
 *     e = sqrtf(v / n)
 *     d = m > floor ? m : floor
 *     active = count < min_samples
 *           || (count < max_samples && isfinite(sum_y) && isfinite(sum_yy) && e / d > threshold)
 *   e is the standard error of the pixel's mean luminance, e / d its size relative to the mean (floor keeps dark pixels from asking for
 *   samples for ever).  A pixel that views a light directly sums to +inf: once it has min_samples samples it is never active.  The list
 *   holds pixel indices y * width + x in strictly ascending order; *n_active_out is its length, and reading those 4 bytes back is the
 *   only synchronisation of the call.  params NULL: RT_ADAPTIVE_DEFAULTS (a starting point, NOT tuned).  RT_E_STATE: statistics off.
 *   RT_E_ARG: min_samples < 2, max_samples < min_samples, a NaN or negative threshold, floor <= 0 or NaN.
 * rt_select_active_rows: rt_select_active over the pixels of rows row_first + k*row_stride, k < row_count, only (the rows
 *   rt_render_rows renders with the same three numbers): the same predicate, storage and order, and the list holds exactly the pixels
 *   of rt_select_active's list that lie in those rows.  No pixel of another row is read: a context that renders one share of the rows has
 *   count 0 elsewhere, which the whole-frame call would list.  On the device, lane i < row_count * width of the compaction owns pixel
 *     p = (row_first + (i / width) * row_stride) * width + i % width
 *   which ascends with i.  RT_E_ARG also for a row set outside the frame, by rt_gather_rows' rule: row_first < 0, row_stride < 1,
 *   row_count < 1 or row_first + (row_count - 1) * row_stride >= height.  rt_select_active is the case (0, 1, height) of the same code.
 * rt_set_active_pixels: installs a caller's list instead: n indices, strictly ascending, every one < width * height, else RT_E_ARG
 *   (checked before anything is uploaded); n = 0 is allowed.  A list is only indices: it survives rt_clear, rt_set_camera and
 *   rt_upload_scene.
 * rt_download_active: the first min(cap, n) entries of the list to out; *n_out = n, the list's true length.  RT_E_STATE: no list.
 * rt_render_active: adds frames [frame0, frame0 + nframes) of Renderer::Sample to the accumulator for the listed pixels only.  On every
 *   listed pixel the accumulator and the statistics end bit-equal to what rt_render(ctx, RT_MODE_PATH, frame0, nframes, seed_base, 0,
 *   height, max_depth) would have left there from the same starting state; every other pixel is not written at all.  An empty list:
 *   RT_OK without a launch.  No list installed: RT_E_STATE.  With the Q-learning sampler on: RT_E_UNSUPPORTED (the rewards of a subset
 *   are a different table).  Works with statistics off: it is also the region-of-interest render.
 * rt_resolve_adaptive: rt_resolve with the pixel's own count as the divisor; count == 0 gives black.  RT_E_STATE: statistics off. */
typedef struct { int32_t min_samples, max_samples; float threshold, floor; } rt_adaptive_params;
#define RT_ADAPTIVE_DEFAULTS { 16, 1024, 0.05f, 1e-3f }
int rt_stats_enable(rt_ctx* ctx, int on);
int rt_download_stats(rt_ctx* ctx, int y0, int y1, uint32_t* count, float* sum_y, float* sum_yy);
int rt_select_active(rt_ctx* ctx, const rt_adaptive_params* params, int* n_active_out);
int rt_select_active_rows(rt_ctx* ctx, const rt_adaptive_params* params, int row_first, int row_stride, int row_count, int* n_active_out);
int rt_set_active_pixels(rt_ctx* ctx, const uint32_t* pixels, int n);
int rt_download_active(rt_ctx* ctx, uint32_t* out, int cap, int* n_out);
int rt_render_active(rt_ctx* ctx, uint32_t frame0, int nframes, uint32_t seed_base, int max_depth);
int rt_resolve_adaptive(rt_ctx* ctx, int y0, int y1, uint32_t* rgb8_out);

/* ---- budgeted adaptive passes: per-pixel sample counts in one batch -------------------------------------------
 * rt_render_active gives every listed pixel the same number of frames; these calls give each active pixel ITS OWN number of samples,
 * predicted from its variance, and run them all as one batch -- the fixed costs of a pass are paid once however uneven the need is.
 * Sample k of a pixel is always frame frame_base + k, so a pixel's value depends only on how many samples it has (see rt_render_budget).
 * rt_select_budget: builds the active-pixel list exactly as rt_select_active(ctx, &params->select, ...) would (same storage, same
 *   ascending order: rt_download_active and rt_render_active serve it afterwards) and the PLAN: a budget b per list entry.  All arithmetic
 *   f32 with IEEE division and no contraction, ternaries as written (a NaN falls to the last branch); n, m, v, d are rt_select_active's
 *   (v after its clamp to >= 0), cap the effective cap of the fit rule below (tests/budget_ref.py restates it and is compared exactly):
 *     count < min_samples:  b = min_samples - count
 *     otherwise (the pixel is active because it is noisy):
 *         g    = threshold * d
 *         t    = v / (g * g)           the sample count at which sqrtf(v / n) / d == threshold, were v and m to stay
 *         need = t - n
 *         b    = need >= (float)cap ? cap : (need >= 1.0f ? (int)ceilf(need) : 1)
 *     then, both branches:  b = min(b, cap);  b = min(b, max_samples - count)
 *   b >= 1 on every listed pixel (an active pixel has count < max_samples).  The plan also records each entry's count at selection time
 *   (the pixel's first frame) and the exclusive prefix sums of the budgets.  *n_samples_out is the sum of the budgets, formed in 64 bits
 *   on the device.
 *   The fit rule: the limit is max_pass_samples, or, when that is 0, the capacity of the finished-sample buffer (RT_SAMPLE_GIB GiB / 16 B);
 *   either way at most 2^31 - 1 (sample ids are ints).  cap = pass_cap >> k for the smallest k >= 0 whose total fits the limit; each
 *   attempt is one more count pass and one more small read-back (the normal case is one); *cap_used_out reports cap.  If even cap = 1
 *   does not fit (n_active > limit): RT_E_UNSUPPORTED, *n_active_out is set, no plan is installed, and the list stays installed
 *   (rt_render_active can still serve it).  The read-backs of n_active and the total are the call's only synchronisation.
 *   params NULL: RT_BUDGET_DEFAULTS.  RT_E_ARG (checked before the context): everything rt_select_active refuses, pass_cap outside
 *   1..1024, a null output pointer.  RT_E_STATE: statistics off.
 * rt_select_budget_rows: rt_select_budget over the pixels of rows row_first + k*row_stride, k < row_count, only, as
 *   rt_select_active_rows is rt_select_active over them: the same predicate, budgets, storage, order and plan (a record names the frame's
 *   pixel index, so rt_download_active, rt_download_budgets, rt_render_active and rt_render_budget serve the result unchanged).  The fit
 *   rule sees the total of THESE rows: a shard's budgets equal the whole-frame call's at its pixels whenever neither call lowered its cap.
 *   RT_E_ARG also for a row set outside the frame (rt_select_active_rows' rule).  rt_select_budget is the case (0, 1, height).
 * rt_download_budgets: the first min(cap, n) budgets in list order; *n_out = n.  RT_E_STATE without a plan.
 * rt_render_budget: for list entry i (pixel p, first frame c, budget b) adds frames frame_base + c ... frame_base + c + b - 1 of
 *   Renderer::Sample to the accumulator and the statistics of p, in frame order, with the seeds rt_render uses for (p, that frame);
 *   frame numbers wrap as rt_render's do.  Unlisted pixels are not written.  The guarantee: start from rt_clear; run any sequence of
 *   whole-frame renders that begins at frame_base with every frame numbered consecutively in the order it is added, and of budgeted
 *   passes with the same frame_base and seed_base; then a pixel with count n holds accumulator and statistics bit-equal to
 *   rt_render(ctx, RT_MODE_PATH, frame_base, n, seed_base, 0, height, max_depth) at that pixel.  The pass is ONE batch, on whichever
 *   pipeline serves that many samples, by the rules of every path batch (the primary-hit table included).
 *   The plan is consumed: a second call without a new selection is RT_E_STATE.  It is also dropped by anything that changes counts or
 *   the list: rt_render / rt_render_rows / rt_render_active in path mode, rt_clear, rt_stats_enable, rt_reproject, rt_select_active,
 *   rt_select_active_dilated, rt_set_active_pixels.  An empty list: RT_OK without a launch.  With the Q-learning sampler on: RT_E_UNSUPPORTED (rt_render_active's
 *   rule).  Statistics off: RT_E_STATE. */
typedef struct {
    rt_adaptive_params select;   /* which pixels: exactly rt_select_active's predicate */
    int32_t  pass_cap;           /* most samples one pixel may get in one pass, 1..1024 */
    uint32_t max_pass_samples;   /* most samples of the whole pass; 0: the context's own limit */
} rt_budget_params;
#define RT_BUDGET_DEFAULTS { RT_ADAPTIVE_DEFAULTS, 64, 0 }   /* a starting point, NOT tuned */
int rt_select_budget(rt_ctx* ctx, const rt_budget_params* params, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out);
int rt_select_budget_rows(rt_ctx* ctx, const rt_budget_params* params, int row_first, int row_stride, int row_count, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out);
int rt_download_budgets(rt_ctx* ctx, uint32_t* out, int cap, int* n_out);
int rt_render_budget(rt_ctx* ctx, uint32_t frame_base, uint32_t seed_base, int max_depth);

/* ---- dilated adaptive selection: also sample the neighbours of noisy pixels -----------------------------------
 * rt_select_active decides per pixel, from that pixel's own statistics: a pixel that has not yet seen a rare bright path looks
 * converged, is dropped, and can never come back because its statistics no longer change.  These calls also list the pixels around
 * an active one, as production renderers grow their active mask by a few pixels.  Whole frame only: a context that holds one row shard
 * has no statistics for its neighbours' rows, so there are no _rows forms.
 * rt_select_active_dilated: with raw_q the unchanged predicate of rt_select_active on pixel q (same params), radius r and p = (x, y)
 *   (tests/dilate_ref.py restates it and is compared exactly):
 *     win(p)     = { (x + dx, y + dy) : |dx| <= r, |dy| <= r, 0 <= x + dx < width, 0 <= y + dy < height }
 *     eligible_p = count_p < max_samples && isfinite(sum_y_p) && isfinite(sum_yy_p)
 *     active_p   = raw_p || (eligible_p && OR over q in win(p) of raw_q)
 *   The window is clipped to the frame per axis: a source at the end of one row never lights the start of the next.  A pixel that views
 *   a light (sums +inf) or sits at max_samples is never listed by dilation alone.  r = 0 gives rt_select_active's list entry for entry.
 *   The list is empty exactly when rt_select_active's is, so a loop that stops on *n_active_out == 0 stops under the same condition as
 *   before, and after at most max_samples passes (every listed pixel is below max_samples and gains a sample per pass).  Same list
 *   storage, ascending order and single read-back as rt_select_active: rt_download_active, rt_render_active and rt_gather_active serve
 *   the result unchanged.  An existing plan is dropped.  On the device the predicate is evaluated once per pixel and kept as a bit;
 *   the dilation works on bitmasks (width * height / 8 bytes each, allocated with the list) and reads no neighbour's statistics.
 *   RT_E_ARG (checked before the context): everything rt_select_active refuses, radius outside 0..RT_DILATE_MAX_RADIUS, a null output
 *   pointer.  RT_E_STATE: statistics off.
 * rt_select_budget_dilated: rt_select_active_dilated(ctx, &params->select, radius, ...)'s list with rt_select_budget's plan: an entry
 *   that is raw-active gets exactly rt_select_budget's budget b at the effective cap; an entry listed by dilation alone gets b = 1; either
 *   way the entry's first frame is its count.  The fit rule (on the total of THESE budgets), RT_E_UNSUPPORTED when even cap = 1 does not
 *   fit (the list stays installed, no plan), *cap_used_out and the 64-bit total are rt_select_budget's; rt_download_budgets and
 *   rt_render_budget (with its guarantee: a pixel's value depends only on its count) serve the plan unchanged.
 *   RT_E_ARG (checked before the context): everything rt_select_budget refuses and a radius outside 0..RT_DILATE_MAX_RADIUS.
 *   RT_E_STATE: statistics off. */
#define RT_DILATE_MAX_RADIUS 16
int rt_select_active_dilated(rt_ctx* ctx, const rt_adaptive_params* params, int radius, int* n_active_out);
int rt_select_budget_dilated(rt_ctx* ctx, const rt_budget_params* params, int radius, int* n_active_out, uint32_t* n_samples_out, int* cap_used_out);

/* ---- variance-guided denoiser for an adaptively sampled frame ------------------------------------------------
 * rt_denoise_variance: rt_denoise's a-trous filter for a frame whose pixels have different sample counts (the spatial half of SVGF,
 *   Schied et al. 2017): every pixel's mean is accumulator / its own count, the colour edge-stopping term is a luminance difference scaled
 *   by the local standard deviation of the mean, taken from the statistics (rt_stats_enable), and the variance is filtered along with the
 *   colour.  On the whole frame, on the context's stream, without synchronising; neither the accumulator nor the statistics are written.
 *   The result lies where rt_denoise leaves its own: rt_download_denoised and rt_resolve_denoised serve whichever of the two ran last.
 *   (This library's own addition.)  All arithmetic f32 with IEEE division and square root, no contraction (tests/denoise_var_ref.py
 *   restates it).  Inputs per pixel p, n = count_p:
 *     n == 0 (empty): the output colour is (0, 0, 0), as rt_resolve_adaptive's black; p is no tap of any neighbour.
 *     c_p = acc_p.xyz / (float)n.  If a component of c_p, sum_y or sum_yy is non-finite, p is passed through (c_p as it is) and is no tap
 *       of any neighbour (rt_denoise's rule for a directly viewed light).
 *     y_p = (0.2126f * r + 0.7152f * g) + 0.0722f * b of c_p (the statistics' luminance).
 *     v_p, the variance of the mean:
 *       n >= 2:  m = sum_y / n;  s = (sum_yy - sum_y * m) / (n - 1);  s = s > 0 ? s : 0;  v_p = s / n   (rt_select_active's e, squared)
 *       n == 1:  v_p = y_p * y_p   (one sample says nothing about its spread; its own square lets the pixel be smoothed freely)
 *       v_p = fminf(v_p, FLT_MAX)   (an overflowing variance is clamped like every k of rt_denoise: a tap of weight 0 adds 0, never 0 x inf)
 *   Which pixels are filtered and may be taps is decided by these inputs once, for every iteration.
 *   Iteration i = 0 .. iterations - 1, step s = 2^i, on the current (c, v), y_p the luminance of the current c_p:
 *     g_p = the 3 x 3 prefilter of v: taps at ONE pixel's distance (not s), weights k3[dx] k3[dy], k3 = (1/4, 1/2, 1/4), over the taps inside
 *       the image that are neither empty nor passed through and have p's hit class (hit or miss); normalised by the sum of the weights used.
 *     kl_p = fminf(1 / (sigma_luminance * sqrtf(g_p) + epsilon), FLT_MAX) (a tiny epsilon on a zero variance: the centre tap's zero
 *       difference weighs exp(0), never 0 x inf); sigma_luminance = +inf drops the term (kl_p = 0).
 *     25 taps at s * (dx, dy), dx, dy in [-2, 2], h as rt_denoise; skipped: taps outside the image, empty, passed through, hit against miss.
 *     w = h[dx] h[dy] exp(-(|y_p - y_q| * kl_p + |n_p - n_q|^2 kn + |x_p - x_q|^2 / t_p^2 kx + |a_p - a_q|^2 ka)), the last three terms
 *       exactly rt_denoise's: k = 1 / sigma^2, clamped to FLT_MAX (kx / t_p^2 per pixel), sigma = +inf drops its term, two misses compare
 *       colour only.  There is no 4^i on the colour term: the falling variance does that job.
 *     c_out = sum w c_q / sum w,  v_out = fminf(sum w^2 v_q / (sum w)^2, FLT_MAX).
 *   Result: float4 per pixel, xyz the filtered colour, w the filtered variance of a filtered pixel and 0 of an empty or passed-through one.
 *   params NULL: RT_DENOISE_VAR_DEFAULTS (sigma_luminance 4 is SVGF's; a starting point, NOT tuned).  RT_E_ARG (checked before the context):
 *   iterations outside 1..8, a sigma <= 0 or NaN, epsilon <= 0 or NaN.  RT_E_STATE: statistics off; the G-buffer missing or stale
 *   (rt_render_aovs first, rt_denoise's rule). */
typedef struct { int32_t iterations; float sigma_luminance, sigma_normal, sigma_position, sigma_albedo, epsilon; } rt_denoise_var_params;
#define RT_DENOISE_VAR_DEFAULTS { 5, 4.0f, 0.25f, 0.1f, 0.1f, 1e-4f }
int rt_denoise_variance(rt_ctx* ctx, const rt_denoise_var_params* params);

/* ---- reprojection: carrying samples and statistics across a camera move and across instance motion ---------------
 * A camera move need not throw every sample away: the radiance a diffuse surface point sends does not depend on the view, so the pixel
 * that sees the point after the move may keep the samples of the pixel that saw it before.  Pinhole cameras only; nearest history pixel,
 * no interpolation; statistics (rt_stats_enable) required.  (This library's own addition.)  The caller's sequence:
 *   rt_render_aovs (old camera) - rt_history_capture - rt_set_camera - rt_render_aovs - rt_reproject - rt_select_active / rt_render_active
 * rt_download_aov_positions: rows [y0, y1) of the G-buffer's world positions, 3 floats per pixel: O + D * t as k_primary_aovs stored it
 *   (a restatement of rt_reproject must start from these bits, not from a product recomputed on the host).  Errors as rt_download_aovs.
 * rt_download_aov_instances: rows [y0, y1) of the G-buffer's instance indices, one int32 per pixel: the TLAS instance whose BLAS holds the
 *   primitive the pixel's ray hit; -1 for a miss, a light, a brute-force sphere or plane, and every hit of a scene without a TLAS.  The
 *   array is made by rt_render_aovs with the other three and goes stale with them.  Errors as rt_download_aov_positions.
 * rt_download_aov_prims: rows [y0, y1) of the G-buffer's primitive indices, one int32 per pixel: the index of the record the pixel's ray hit
 *   in the context's RT_LAYOUT_PRIMS array (the per-BLAS slices rt_blas_array(..., RT_LAYOUT_PRIMS) returns, in BLAS order); -1 for a
 *   miss, a light and a brute-force sphere or plane.  Made by rt_render_aovs in the same launch, stale with the others.  Errors as
 *   rt_download_aov_instances.
 * rt_history_capture: copies the bound accumulator, the three statistics arrays, the G-buffer arrays (the instance indices included), the
 *   current camera record and, of a scene with a TLAS, every instance's transform and inv_transform (rows 0..2: 12 + 12 floats, as they
 *   are at this moment) into history buffers of the context (allocated on first use, freed by rt_destroy): device to device on the context's stream, without
 *   synchronising.  RT_E_STATE: statistics off; the G-buffer missing or stale (rt_render_aovs first).  RT_E_UNSUPPORTED: the current
 *   camera is a fisheye.  A history stays valid until rt_upload_scene, rt_set_time, rt_set_instances or rt_stats_enable(ctx, 0); rt_clear and rt_set_camera
 *   do not touch it.  Validity has two levels: rt_set_instances ends it for rt_reproject only -- for rt_reproject_motion the history stays
 *   valid across any number of rt_set_instances calls (a failed one changes nothing for either).  A third level is rt_reproject_deform's:
 *   for it the history also outlives rt_set_triangles and rt_set_time, and ends with rt_upload_scene and rt_stats_enable(ctx, 0) alone
 *   (which also frees the history's buffers).
 * rt_reproject: rewrites the accumulator and the statistics of EVERY pixel: carried from the history, or zeroed (a zero float4, count 0,
 *   sums 0).  On the context's stream; *n_carried_out (may be NULL) receives the number of carried pixels, and reading those 4 bytes back
 *   is the only synchronisation of the call.  The history is not modified (a second call gives the same result), the active-pixel list
 *   and the G-buffer are not touched.  All arithmetic f32 with IEEE division, no contraction (tests/reproject_ref.py restates it):
 *     dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z
 *     cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)
 *     dist2(a, b) = dot(a - b, a - b)
 *   Primed values are the history's; W, H the frame's size.  For the current pixel p, (n_p, t_p) the G-buffer's normal and distance,
 *   x_p its position, obj_p its object (-1: a miss), mat_p its material index:
 *     eligible = obj_p != -1 && (carry_view_dependent
 *                || (0 <= mat_p < n_materials && material[mat_p].type == RT_MAT_DIFFUSE && material[mat_p].shinieness == 0))
 *     A = TR' - TL';  B = BL' - TL';  N = cross(A, B);  E = TL' - cam';  d = x_p - cam'
 *     lam = dot(E, N) / dot(d, N)                        needs isfinite(lam) && lam > 0 (the point lies in front of the history camera)
 *     Q = lam * d - E  (per component)                   the point's image on the history's screen plane, from its top left corner
 *     nn = dot(N, N);  u = dot(cross(Q, B), N) / nn;  v = dot(cross(A, Q), N) / nn
 *     rx = floorf(u * (float)W + 0.5f);  ry = floorf(v * (float)H + 0.5f)     needs 0 <= rx < W, 0 <= ry < H, compared as floats (NaN fails)
 *     q = (int)ry * W + (int)rx                          (pixel x's ray passes through u = x / W: the nearest pixel, not a truncation)
 *     carried = eligible && the above
 *            && count'_q > 0 && obj'_q == obj_p && mat'_q == mat_p
 *            && dist2(n_p, n'_q) <= normal_tolerance * normal_tolerance
 *            && fabsf(dot(n'_q, x_p - x'_q)) <= plane_tolerance * t_p
 *   The last test is the distance of x_p from the history pixel's TANGENT PLANE, not from its point: snapping to the nearest pixel moves
 *   the history point by up to half a pixel's footprint along the surface, which a point distance would reject at small frames.
 *   A carried pixel takes acc'_q, count'_q, sum_y'_q, sum_yy'_q unchanged, unless max_history > 0 && count'_q > max_history: then
 *   f = (float)max_history / (float)count'_q multiplies the four accumulator channels and both sums, and the count becomes max_history
 *   (the mean stays, the old samples weigh less against new ones).
 *   View dependence: a diffuse material with shinieness == 0 is what Renderer::Sample shades independently of the view; everything else
 *   (metal, glass, shiny diffuse, a light seen directly) starts empty unless carry_view_dependent is set; a miss is never carried.
 *   params NULL: RT_REPROJECT_DEFAULTS.  RT_E_ARG (checked before the context): a tolerance that is negative or NaN, max_history < 0.
 *   RT_E_STATE: statistics off; no valid history; the current G-buffer missing or stale.  RT_E_UNSUPPORTED: the current camera is a
 *   fisheye.  With rt_set_profiling on, rt_history_capture's copies and k_reproject are each one launch of rt_profile.query.
 *   Object motion is not reprojected by this call: rt_set_instances (like rt_set_time and rt_upload_scene) invalidates the history for it,
 *   and its carry is across a camera move only.  rt_reproject_motion is the call that follows instances.
 * rt_reproject_motion: rt_reproject with the other half of a motion vector: a surface point of an instance that has moved since the capture
 *   (rt_set_instances, any number of times) is taken back through the instance's own motion before it is projected into the history camera.
 *   The caller's sequence:
 *     rt_render_aovs - rt_history_capture - rt_set_instances [- rt_set_camera] - rt_render_aovs - rt_reproject_motion - rt_select_active / ...
 *   Same parameters, defaults, outputs, stream ordering, single read-back, profiling entry (k_reproject_motion: one launch of
 *   rt_profile.query), dropped budget plan and errors as rt_reproject, except that an instance move since the capture is no error:
 *   RT_E_STATE only after rt_upload_scene, rt_set_time or rt_stats_enable(ctx, 0).  The definition is rt_reproject's with these changes (all
 *   f32, no contraction; tests/reproject_motion_ref.py restates it).  For the current pixel p let k = inst_p, the G-buffer's instance index:
 *     moved_k = k >= 0 && any of instance k's 24 words (transform rows 0..2, inv_transform rows 0..2) differs BITWISE from the capture's
 *     !moved_k:  x_h = x_p;  n_h = n_p                     (no arithmetic: an unmoved point keeps its bits)
 *      moved_k:  x_h = xform_pos(T'_k, xform_pos(invT_k, x_p))         invT_k: the CURRENT inv_transform, T'_k: the capture's transform
 *                n_h = normalize(xform_vec(T'_k, xform_vec(invT_k, n_p)))
 *     xform_pos(c, a) = (((c[0] * a.x + c[1] * a.y) + c[2] * a.z) + c[3] * 1.0f,
 *                        ((c[4] * a.x + c[5] * a.y) + c[6] * a.z) + c[7] * 1.0f,
 *                        ((c[8] * a.x + c[9] * a.y) + c[10] * a.z) + c[11] * 1.0f)          c: rows 0..2 of a row-major 4 x 4 matrix
 *     xform_vec(c, a) = the same with c[3] * 0.0f, c[7] * 0.0f, c[11] * 0.0f as the last terms (a non-finite c[3] makes a NaN)
 *     normalize(v)    = v * (1.0f / sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z))              (per component; IEEE sqrt and division)
 *   Normals go through transform, not its inverse transpose: that is how a world normal is made from an instance's local one, so n_h is
 *   the normal the capture would have stored.  Then, in rt_reproject's definition:
 *     d = x_h - cam'                                      the projection starts from the point taken back
 *     carried = eligible && the projection's conditions
 *            && count'_q > 0 && obj'_q == obj_p && mat'_q == mat_p && inst'_q == inst_p
 *            && dist2(n_h, n'_q) <= normal_tolerance * normal_tolerance
 *            && fabsf(dot(n'_q, x_h - x'_q)) <= plane_tolerance * t_p         (t_p stays the scale: the unmoved case is rt_reproject's)
 *   A NaN anywhere (a singular inverse) fails a comparison and the pixel starts empty.  Eligibility, the max_history rescale and the
 *   zeroing of pixels that are not carried are unchanged.  Two consequences: with no instance moved since the capture (or every moved one
 *   moved back to the same bits), and on any scene without a TLAS, the call leaves accumulator, statistics and *n_carried_out bit-equal
 *   to rt_reproject's; and a second call gives the same result (the history is not modified).
 *   What it does not do: it moves SAMPLES, not light.  Radiance on and around a moved object changes -- its shadow, what it reflects onto
 *   its neighbours, its own lighting as it turns towards or away from the lights -- and the carried samples there are biased until new
 *   ones outweigh them: max_history is the remedy (a small value lets new samples take over quickly).  Deforming meshes (rt_set_time,
 *   rt_set_triangles) still invalidate the history for this call, and so does rt_upload_scene; rt_reproject_deform follows deformations.
 * rt_reproject_deform: rt_reproject_motion with a third way back: a surface point of a triangle that has been rewritten since the capture
 *   (rt_set_triangles, rt_set_time; a refit keeps the tree's shape and the leaf order, so a leaf slot names the same triangle before and
 *   after) takes its barycentric coordinates in the current triangle to the triangle the capture saw.  The caller's sequence:
 *     rt_render_aovs - rt_history_capture - rt_set_triangles / rt_set_time / rt_set_instances ... [- rt_set_camera] - rt_render_aovs -
 *     rt_reproject_deform - rt_select_active / ...
 *   Same parameters, defaults, outputs, stream ordering, single read-back, profiling entry (k_reproject_deform: one launch of
 *   rt_profile.query), dropped budget plan and errors as rt_reproject_motion, except that RT_E_STATE follows the third level of validity:
 *   any number of rt_set_triangles, rt_set_time and rt_set_instances calls since the capture is no error.
 *   The capture's triangles are kept on first write: while a history is valid at this level, the first rt_set_triangles of BLAS b (and the
 *   first rt_set_time, for BLAS 0 of a scene without a TLAS) after a capture first queues a device-to-device copy of that BLAS's
 *   primitive records (64 B per leaf slot) into a buffer of the history, on the context's stream ahead of the rewrite; later rewrites
 *   of b leave the copy alone, rt_history_capture makes the current records the capture's again, and the buffers grow only until
 *   rt_destroy or rt_stats_enable(ctx, 0) frees them.  COST: with a valid history, one more copy of the BLAS's records in time and in
 *   memory (537 MB for an 8.4 M-triangle mesh); without one, nothing is queued and nothing allocated.  The results of rt_set_triangles and
 *   rt_set_time do not depend on a history.  A failed rt_set_triangles restores the records: the kept copy then equals them and the
 *   bitwise rule below makes it harmless.
 *   The definition is rt_reproject_motion's with these changes (all f32, IEEE division, no contraction; tests/reproject_deform_ref.py
 *   restates it).  For pixel p let k = inst_p and s = prim_p (rt_download_aov_prims); R_s the current record at slot s, R'_s the
 *   capture's: the kept copy if the BLAS of s (under a TLAS the BLAS of instance k, otherwise BLAS 0) has one, else the current record:
 *     deformed_p = s >= 0 && the BLAS of s has a kept copy && R_s is a triangle record
 *                  && any of the 12 words v0, v1, v2, N of R_s differs BITWISE from R'_s
 *     !deformed_p:  x_h, n_h exactly as rt_reproject_motion defines them (an untouched triangle of a deformed mesh keeps its bits)
 *      deformed_p:  x_o  = k >= 0 ? xform_pos(invT_k, x_p) : x_p          invT_k: the CURRENT inv_transform
 *                   e1 = v1 - v0;  e2 = v2 - v0;  w = x_o - v0            (current vertices)
 *                   d11 = dot(e1,e1); d12 = dot(e1,e2); d22 = dot(e2,e2); w1 = dot(w,e1); w2 = dot(w,e2)
 *                   den = d11 * d22 - d12 * d12
 *                   bu  = (d22 * w1 - d12 * w2) / den;   bv = (d11 * w2 - d12 * w1) / den
 *                   e1' = v1' - v0';  e2' = v2' - v0'                     (the capture's vertices)
 *                   x_o' = (v0' + bu * e1') + bv * e2'                    (per component)
 *                   x_h  = k >= 0 ? xform_pos(T'_k, x_o') : x_o'          T'_k: the capture's transform
 *                   n_h  = k >= 0 ? normalize(xform_vec(T'_k, N')) : N'   N': the capture's record's normal
 *   n_h is the normal the capture stored for any pixel that saw the triangle.  The projection starts from d = x_h - cam'; the acceptance
 *   is rt_reproject_motion's, unchanged (q need not have seen the same triangle: nearest-pixel snapping crosses edges on a smooth
 *   mesh).  A degenerate current triangle (den == 0) or a singular inverse makes a NaN, which fails a comparison: the pixel starts empty.
 *   Consequences: with no deformation since the capture, or every deformed triangle rewritten back to the same bits, the result is
 *   bit-equal to rt_reproject_motion's (and with no instance moved either, to rt_reproject's); a second call gives the same result; the
 *   history, the active-pixel list and the G-buffer are not touched.
 *   What it does not do: like the motion carry it moves samples, not light -- carried samples on and around a deformed surface are biased
 *   until new ones outweigh them (max_history) -- and it does not follow a change of topology: rt_upload_scene ends the history. */
typedef struct { float normal_tolerance, plane_tolerance; int32_t max_history; int32_t carry_view_dependent; } rt_reproject_params;
#define RT_REPROJECT_DEFAULTS { 0.25f, 0.01f, 0, 0 }   /* a starting point, NOT tuned */
int rt_history_capture(rt_ctx* ctx);
int rt_reproject(rt_ctx* ctx, const rt_reproject_params* params, int* n_carried_out);
int rt_reproject_motion(rt_ctx* ctx, const rt_reproject_params* params, int* n_carried_out);
int rt_download_aov_positions(rt_ctx* ctx, int y0, int y1, float* xyz_out);
int rt_download_aov_instances(rt_ctx* ctx, int y0, int y1, int32_t* inst_out);
int rt_reproject_deform(rt_ctx* ctx, const rt_reproject_params* params, int* n_carried_out);
int rt_download_aov_prims(rt_ctx* ctx, int y0, int y1, int32_t* prim_out);

/* ---- Q-learning guided sampling ("next" row N4) ------------------------------------------------------
 * The reference snapshot has no code for it: README.md:36-42 names Dahm & Keller 2017, "Learning Light Transport
 * the Reinforced Way", and lists "initialize sampling positions; pick sampling direction according to the QValue of neighboring
 * points; store and update directions with a corresponding probability per sampling point".  These calls are this library's
 * statement of that scheme (csrc/rt_qlearn.h; PARITY UNPINNED: there is nothing in the reference to compare with).
 * rt_qlearn_enable: path-mode batches draw the indirect bounce of every diffuse hit from a table of grid^3 cells over the box
 *   [lo, hi] x 64 direction patches, P(patch) = (1 - epsilon) Q / sum Q + epsilon / 64, and collect rewards (integer sums);
 *   the table starts at q_init everywhere.  params == NULL switches the sampler off and frees the table.  Batches larger than
 *   the slot budget, and scenes that need the general path kernel, return RT_E_UNSUPPORTED while it is on.
 *   Refused with RT_E_ARG: grid outside 1..64, a box that is empty or not finite on an axis, alpha outside (0, 1], epsilon outside
 *   [0, 1], q_init that is not a finite number above 0 (an infinite one would make every P NaN).  The previous table is freed before
 *   the arguments are looked at: after ANY refused rt_qlearn_enable the sampler is off, as after rt_qlearn_enable(NULL), and path
 *   frames have the bits they had before it was ever on.
 * rt_trace_batch* in path mode with the sampler on is a batch like any other: ray i is guided at every diffuse hit, it pays rewards
 *   iff (the state its stream starts Sample with, InitSeed(seed_base + i)) & learn_mask == 0 -- there is no pixel jitter to draw
 *   first -- and its rewards are added to the pending sums.  A batch that cannot have an entry per sample (n above the slot
 *   budget, RT_COUNT_REFERENCE) returns RT_E_UNSUPPORTED as rt_render does: rgb_out, the pending sums and the accumulator stay as
 *   they were.
 * rt_qlearn_apply: Q <- (1 - alpha) Q + alpha * mean reward, for every (cell, patch) that received one; call it BETWEEN
 *   batches (within a batch the table is read-only, so a frame does not depend on scheduling or sharding).
 * rt_qlearn_get_sums / rt_qlearn_set_sums: the pending rewards (int64 sums in 48.16 fixed point, uint32 counts, grid^3 * 64
 *   each) -- with several ranks the sums are all-reduced between the ranks before every rank applies them.
 * rt_qlearn_get_table: Q as grid^3 * 64 floats (cell-major, patch = 8 * band + sector). */
typedef struct {
	int32_t grid; float lo[3], hi[3]; float alpha, epsilon, q_init;
	/* learn_mask: a sample pays rewards iff (the state of its random stream after the pixel jitter) & learn_mask == 0 -- 0: every
	 * sample learns; 3: every fourth one (a surface hit's reward reads 64 table values: the picks stay guided for all samples,
	 * the table is taught by a fixed, scheduling-independent quarter of them) */
	uint32_t learn_mask;
} rt_qlearn_params;
int rt_qlearn_enable(rt_ctx* ctx, const rt_qlearn_params* params);
int rt_qlearn_apply(rt_ctx* ctx);
int rt_qlearn_get_sums(rt_ctx* ctx, int64_t* sums_out, uint32_t* counts_out);
int rt_qlearn_set_sums(rt_ctx* ctx, const int64_t* sums, const uint32_t* counts);
int rt_qlearn_get_table(rt_ctx* ctx, float* q_out);
/* The pending sums live in the caller's DEVICE arrays from here on (grid^3 * 64 int64 / uint32; what was pending is copied over;
 * the caller keeps them alive until the sampler is switched off): one process per GPU all-reduces them in place between the
 * ranks (RCCL on device memory) before every rank's rt_qlearn_apply -- no host copy in the exchange. */
int rt_qlearn_bind_sums(rt_ctx* ctx, int64_t* dev_sums, uint32_t* dev_counts);

/* ---- acceleration structure build ("next" row N1) ------------------------------------------------ */
/* bvh::Build() with splitMethod BINNEDSAH (bvh.cpp:18-56; FindBestSplitPlane :116-193, Subdivide :223-333,
 * separatePlanes :202-221, Refit :556-594) on the device.  The result is the reference's tree bit for bit: node
 * numbering, boxes and primitiveIdx order.  nodes_out: 2 * (n_tri + n_sph + n_pla + 1) entries (bvh.cpp:33),
 * prim_idx_out: n_tri + n_sph + n_pla entries.  RT_E_UNSUPPORTED (never a silent fallback) for an input with
 * no triangle or sphere, or with a non-finite vertex / centre / radius. */
int rt_build_bvh(rt_ctx* ctx, const rt_triangle* tris, uint32_t n_tri, const rt_sphere* spheres, uint32_t n_sph, const rt_plane* planes, uint32_t n_pla,
                 rt_bvh_node* nodes_out, uint32_t* prim_idx_out, uint32_t* nodes_used_out);
/* The same with bvh.h:38-43's splitMethod: 0 BINNEDSAH (what rt_build_bvh builds), 1 SAMESIZE (median of the longest
 * axis, bvh.cpp:233-252), 2 LONGESTAXIS (spatial middle, :226-232), 3 SAH (every centroid tried as the plane, :275-293
 * with EvaluateSAH :514-554 -- quadratic in the node size like the reference). */
int rt_build_bvh_split(rt_ctx* ctx, int split_method, const rt_triangle* tris, uint32_t n_tri, const rt_sphere* spheres, uint32_t n_sph,
                       const rt_plane* planes, uint32_t n_pla, rt_bvh_node* nodes_out, uint32_t* prim_idx_out, uint32_t* nodes_used_out);
/* tlas::build (tlas.cpp:13-48: agglomerative clustering by smallest union surface area, FindBestMatch :50-63) on the
 * device.  bounds6: per instance the world box its bvhInstance holds (min.xyz, max.xyz, template bvhInstance.cpp:37-44);
 * 1 <= n <= 256; nodes_out has room for 2 n + 1 nodes.  Same node order and boxes as the host builder. */
int rt_build_tlas(rt_ctx* ctx, const float* bounds6, uint32_t n, rt_tlas_node* nodes_out, uint32_t* nodes_used_out);

/* ---- moving instances without a re-upload -------------------------------------------------------------------
 * A TLAS exists so that objects can move without rebuilding their trees.  rt_set_instances is bvhInstance::SetTransform
 * (bvhInstance.cpp:37-44) for instances [first, first + count) followed by tlas::build (tlas.cpp:13-48) over ALL instances, on the device,
 * into the loaded scene: no BLAS is laid out or copied again.  Afterwards the context holds, byte for byte, what rt_upload_scene would hold
 * of the updated description (same BLASes, the new instance records, tlas_nodes = the rebuilt TLAS): the inst[] records, the TLAS pair
 * records, the reach[] records and the scalars rootLink, tlasBase, tlasPairs, reachOriginMax, tlasLds, stackRows (rt_scene_array reads
 * them back).  (The reference leaves tl->Build() commented out, template/scene.h:1245: moving instances is this library's own addition.)
 *   Transforms: instances[k].transform / .inv_transform replace those of instance first + k.  instances[k].blas must equal the uploaded
 *     instance's BLAS (RT_E_ARG otherwise): an instance cannot be re-pointed at another BLAS.
 *   bounds6 != NULL: count * 6 floats (min.xyz, max.xyz), the world box the caller's bvhInstance holds after its SetTransform.  The
 *     reference never resets 'bounds' (bvhInstance.h:15-30), so a caller that mirrors it sends a box that grows with every move: that is
 *     the reference's behaviour, the host mirror's, and what rt_build_tlas takes.
 *   bounds6 == NULL: the device computes the box of a FRESH instance -- bvhInstance(blas) followed by one SetTransform: the BLAS's local
 *     box (bvh::bounds = node 0's box, bvh.cpp:48-49; kept per BLAS at upload) grown by the 8 corners TransformPosition(corner(i),
 *     transform), i = 0..7, corner(i) taking max.x / max.y / max.z where bits 0 / 1 / 2 of i are set and min otherwise; f32 in
 *     TransformPosition's operation order ((c0 * x + c1 * y) + c2 * z) + c3 * 1.0f, no contraction.  This box does NOT accumulate over
 *     successive calls: it is what an animation wants, and the library's own choice.
 *   The TLAS afterwards is tlas::build's over the boxes of all n instances.  An untouched instance keeps the box it last had; one never
 *     set, the box of its leaf in the uploaded tlas_nodes (the first such leaf in node order; an instance without one must be part of the
 *     first update).  Node numbering and boxes are exactly rt_build_tlas's on those boxes.  An uploaded TLAS of another shape (a hand-made
 *     tree, another pair count) is replaced by it; the split of a traversal block's LDS is re-evaluated for the new pair count.
 *   Ordering: queued on the context's stream behind what is there.  The nodes are built into scratch first; reading 4 bytes (nodes used)
 *     back is the call's only synchronisation.  If the build finds no finite union area left (rt_build_tlas's failure: e.g. boxes whose
 *     union areas all reach 1e30), the call returns RT_E_UNSUPPORTED and the scene is exactly as before; only after that check do the
 *     copies and the kernel that rewrite the scene run.
 *   Invalidation: everything rt_set_time invalidates -- the G-buffer is stale (rt_render_aovs), the primary-hit table is rebuilt by the
 *     next dense batch, a captured history is invalid for rt_reproject (RT_E_STATE until a new rt_history_capture).  The accumulator, the
 *     statistics and the active-pixel list are not touched: the caller clears, or carries the samples with rt_reproject_motion, which
 *     follows the instances (rt_reproject itself does not follow object motion).  A call that fails invalidates nothing.
 *   Errors.  RT_E_STATE: no scene loaded.  RT_E_UNSUPPORTED: the scene has no TLAS (rt_set_time stays RT_E_UNSUPPORTED under one).
 *     RT_E_ARG, checked on the host before anything is queued, the scene unchanged: a null ctx or instances; count == 0; a range outside
 *     the instances; a blas mismatch; a non-finite matrix entry; a bound that is non-finite or beyond 1e30 in magnitude (with bounds6 ==
 *     NULL: a transform that could take the BLAS's box there); an untouched instance that has no box yet.
 *   Q-learning, the wide walks (per BLAS: a transform does not change them), counters and profiling work as before; with rt_set_profiling
 *     on, the call is one entry of rt_profile.query (its copies, kernels and the read-back).
 * rt_download_tlas: the TLAS the context walks now, as rt_build_tlas returns it: nodes_out has room for 2 n + 1 nodes, *nodes_used_out
 *   = 2 n after an rt_set_instances; before the first one, the uploaded tlas_nodes and their count (RT_E_UNSUPPORTED if they are more than
 *   2 n + 1).  Synchronous.  RT_E_STATE: no scene; RT_E_UNSUPPORTED: no TLAS.
 * rt_scene_array: what the context holds of the layout rt_layout_build describes, read back from the device: which in { RT_LAYOUT_PAIRS,
 *   RT_LAYOUT_REACH, RT_LAYOUT_BRUTE, RT_LAYOUT_INST, RT_LAYOUT_LIGHTS, RT_LAYOUT_MATS, RT_LAYOUT_SCALARS }, the element formats, sizes
 *   and the 14 scalars of rt_layout_array; any other array: RT_E_UNSUPPORTED (RT_LAYOUT_PRIMS is read per BLAS: rt_blas_array).  *bytes_out receives the array's size; out == NULL asks for the size alone;
 *   cap_bytes below it: RT_E_ARG.  Synchronous; for tests and tools.  RT_E_STATE: no scene. */
int rt_set_instances(rt_ctx* ctx, uint32_t first, uint32_t count, const rt_instance* instances, const float* bounds6);
int rt_download_tlas(rt_ctx* ctx, rt_tlas_node* nodes_out, uint32_t* nodes_used_out);
int rt_scene_array(rt_ctx* ctx, int which, void* out, size_t cap_bytes, size_t* bytes_out);

/* ---- adding, removing and re-pointing instances without a re-upload -----------------------------------------------
 * rt_set_instances moves the objects of a scene; rt_set_instance_list changes WHICH objects there are.  It replaces the whole instance list
 * of the loaded TLAS scene by 'instances': n records, 1 <= n <= 256, n free to differ from the current count, instances[i].blas any BLAS
 * of the upload (several instances may share one, a BLAS may end up with none -- it stays loaded and can be named again; a BLAS needs no
 * instance at upload either, so a library of meshes can be uploaded once and the scene populated from it).  No BLAS is laid out or copied
 * again.  The yardstick is rt_set_instances': afterwards the context holds, byte for byte, what rt_upload_scene would hold of the updated
 * description -- the uploaded one as the earlier rt_set_* calls have left it, with instances / n_instances replaced and tlas_nodes =
 * tlas::build over the n boxes: inst[], the TLAS pair records at the tail of pairs[], reach[], scalars 0-6 of RT_LAYOUT_SCALARS (nInst
 * included; rt_scene_array), and rt_download_tlas returns the 2 n nodes rt_build_tlas makes of the boxes.  Queries, frames and counters
 * equal a freshly uploaded context's bit for bit.
 *   Records: transform / inv_transform are the caller's; the root words are the ones the upload made per BLAS (the 8-wide root RT_EMPTY
 *     where the upload had no 8-wide walk).  The wide arrays and scalars 9-10 keep their upload-time shape, as under rt_set_triangles.
 *   Boxes: bounds6 != NULL: n * 6 floats, used as given (the caller's bvhInstance::bounds, accumulating or not); bounds6 == NULL: the box
 *     of a FRESH instance for every entry (rt_set_instances' NULL rule).  Every instance has a box afterwards.
 *   What follows n: n == 1 has no TLAS pair record (root = the instance, tlasBase 0); the split of a traversal block's LDS is re-evaluated
 *     (the TLAS copy in LDS switches off from 38 instances on under the default build, and comes back below that).  Later
 *     rt_set_instances / rt_set_triangles calls work against the new list: its range, its BLASes, the instances of a deformed BLAS.
 *   Room: under a TLAS rt_upload_scene reserves room for 256 instances in every per-instance array (under 100 KB); this call never
 *     allocates or copies a large array.  rt_scene_array's sizes follow the current count.
 *   Ordering and failure: rt_set_instances' -- boxes and nodes go to scratch, the 4-byte read-back of the build is the only
 *     synchronisation, the scene is written only after it.  If the build finds no finite union area the call returns RT_E_UNSUPPORTED,
 *     the scene is byte-equal to what it was and nothing is invalidated.
 *   Invalidation: an upload's, for everything that names an instance -- the G-buffer is stale (its instance indices renumber), the
 *     primary-hit and bounce tables are rebuilt by the next dense batch, and a captured history ends at EVERY level: rt_reproject,
 *     rt_reproject_motion and rt_reproject_deform return RT_E_STATE until a new rt_history_capture.  There is deliberately no carry: an
 *     instance index no longer names the same object.  Not touched: accumulator, statistics, active list, budget plan, Q table, bound
 *     mesh indices (they are per BLAS), lens, filter, lights, materials, sky.  With rt_set_profiling on, one rt_profile.query entry.
 *   Errors, all checked on the host before anything is queued.  RT_E_STATE: no scene.  RT_E_UNSUPPORTED: the scene has no TLAS.  RT_E_ARG:
 *     a null ctx or instances; n outside 1..256; a blas outside the uploaded BLASes; a non-finite matrix entry; a bound that is non-finite
 *     or beyond 1e30 (with bounds6 == NULL: a transform that could take the BLAS's box there).
 *   Limits: 256 instances (the reference's nodeIdx[256]); no new BLAS (it would shift tlasBase and the wide arrays and grow pairs[] /
 *     prims[]: rt_upload_scene); the brute-force spheres and planes of a TLAS scene are not edited; no carry across a list edit. */
int rt_set_instance_list(rt_ctx* ctx, uint32_t n, const rt_instance* instances, const float* bounds6);

/* ---- deforming a mesh without a re-upload ----------------------------------------------------------------------
 * A skinned character, cloth or a morph target changes its vertices and keeps its topology.  rt_set_triangles replaces ALL triangles of BLAS
 * 'blas' of the loaded scene and runs bvh::Refit (bvh.cpp:556-594) over that BLAS's tree on the device: the tree keeps its shape and its
 * prim_idx order, no other BLAS is touched, nothing is laid out again.  It works with and without a TLAS (without one, blas 0 is the scene
 * BVH; its spheres and planes keep their records).  Afterwards the context holds, byte for byte, what rt_upload_scene would hold of the
 * updated description: the uploaded one with blas[blas].tris replaced, blas[blas].nodes after bvh::Refit over the new primitives and,
 * under a TLAS, every instance of that BLAS under the box of a fresh instance with its current transform (rt_set_instances' bounds6 ==
 * NULL rule, applied to the refitted node 0's box; every other instance keeps the box it last had) and tlas_nodes = tlas::build over all
 * the boxes.  That covers the BLAS's primitive and pair records (rt_blas_array), inst[], the TLAS pair records, reach[] and scalars 0-8 and
 * 11-13 (rt_scene_array).  wideOK / wide8OK and the wide arrays keep their upload-time shape: the 4-wide child boxes are brought up to date,
 * the 8-wide quantised walk is switched off for the scene, as rt_set_time does.
 *   tris[p] replaces primitive p as a whole record: v0, v1, v2, N, obj_idx, material.  N is the caller's own Triangle::update and is not
 *     checked, as at upload.  n_tri must equal the uploaded n_tri: a partial update is not supported (the object box the reach[] records
 *     rest on needs every triangle).  A later rt_set_time deforms from the new vertices.
 *   Ordering: queued on the context's stream behind what is there.  Under a TLAS the 4-byte read-back of the TLAS build is the call's only
 *     synchronisation; without one there is none.  (The first call on a scene, or one for a larger BLAS than any before, also allocates
 *     its staging and undo arrays.)  tris is copied with one hipMemcpyAsync: ordinary (pageable) memory has been read when the call
 *     returns; page-locked memory is read when the stream gets there, so without a TLAS it stays the caller's to keep unchanged until
 *     rt_synchronize or any later call that synchronises.
 *   Failure is atomic.  RT_E_ARG, checked on the host before anything is queued: a null pointer; blas >= n_blas; n_tri different from the
 *     uploaded count; a vertex coordinate that is non-finite or beyond 1e29 in magnitude; a transform of an instance of the BLAS that could
 *     take the new box beyond 1e30; an instance of another BLAS that has no box yet (rt_set_instances' rule).  RT_E_STATE: no scene.
 *     RT_E_UNSUPPORTED: the TLAS build finds no finite union area (rt_build_tlas's failure); the call returns this after its read-back, and
 *     the records it had rewritten are copied back on the device: the scene is byte-equal to what it was.  (Also RT_E_UNSUPPORTED: the
 *     uploaded nodes of the BLAS were not a tree.)
 *   Invalidation is rt_set_time's: the G-buffer goes stale, the primary-hit table is rebuilt by the next dense batch, a captured history
 *     becomes invalid for rt_reproject AND rt_reproject_motion (a deformed surface has no rigid motion to take back; rt_reproject_deform follows it).  Accumulator,
 *     statistics and lists are untouched; a failed call invalidates nothing.  With rt_set_profiling on, the call is one entry of
 *     rt_profile.query.
 * rt_blas_array: the context's records of one BLAS, read back from the device: which in { RT_LAYOUT_PAIRS, RT_LAYOUT_PRIMS }, in
 *   rt_layout_array's formats, so that the result equals the BLAS's slice of rt_layout_build's arrays (nodes_used / 2 pair records and
 *   n_prims primitive records per BLAS, in BLAS order).  out == NULL asks for the size alone.  RT_E_ARG: a short buffer, a bad BLAS;
 *   RT_E_UNSUPPORTED: any other array; RT_E_STATE: no scene.  Synchronous; for tests and tools. */
int rt_set_triangles(rt_ctx* ctx, uint32_t blas, const rt_triangle* tris, uint32_t n_tri);
int rt_blas_array(rt_ctx* ctx, uint32_t blas, int which, void* out, size_t cap_bytes, size_t* bytes_out);

/* ---- deforming an indexed mesh from its vertices alone -----------------------------------------------------------
 * A triangle record is 56 bytes, repeats every shared vertex and carries a normal the caller derived on the host.  An indexed mesh is
 * deformed by sending its vertex array alone, from host memory or straight from device memory (a skinning, cloth or morph step that already
 * runs on the GPU): the records are assembled, the normals derived and the call's checks reduced on the device.
 * rt_set_mesh_indices binds an index buffer to BLAS 'blas' of the loaded scene: triangle p has the corners idx[3p], idx[3p + 1],
 *   idx[3p + 2], 0-based.  idx is host memory; it is checked, then copied to the device and kept per BLAS (12 bytes per triangle); it has
 *   been read when the call returns.  RT_E_ARG, before anything is copied: n_tri different from the uploaded n_tri, n_vertices < 1, an
 *   index >= n_vertices (the message names the first such triangle), blas >= n_blas.  idx == NULL unbinds (n_tri and n_vertices are not
 *   looked at).  The binding survives rt_set_triangles, rt_set_instances, rt_set_time and the two calls below and ends with
 *   rt_upload_scene and rt_destroy.  It touches nothing of the scene and invalidates nothing.  RT_E_STATE: no scene.
 * rt_set_vertices: xyz is n_vertices points of three floats in host memory.  The context ends byte for byte as after
 *   rt_set_triangles(ctx, blas, T, n_tri) with, for every primitive p,
 *     T[p].v0 = V[idx[3p]], T[p].v1 = V[idx[3p + 1]], T[p].v2 = V[idx[3p + 2]],
 *     T[p].N = Triangle::update's (template/scene.h:238-246): normalize(cross(v1 - v0, v2 - v0)), cross as a.y * b.z - a.z * b.y ..., dot
 *       as (xx + yy) + zz, N = c * (1 / sqrtf(dot)), every operation rounded to f32 on its own (IEEE divide and square root, no contraction),
 *     T[p].obj_idx, T[p].material = what primitive p's record holds now (from the upload or the last rt_set_triangles; a primitive prim_idx
 *       never names has no record and gets none).
 *   A degenerate triangle gets the NaN normal the reference gives it; which NaN (sign, payload) is the device's, in N.x, N.y, N.z and d of
 *   that one record.  Everything else is rt_set_triangles' own: with and without a TLAS, atomic failure, the same invalidation, the kept
 *   records for rt_reproject_deform, the 8-wide walk switched off, the originals of a later rt_set_time refreshed, one rt_profile.query
 *   entry.  The refusals are that call's on the assembled triangles -- RT_E_ARG: a coordinate of a REFERENCED vertex that is non-finite or
 *   beyond 1e29 (the message names a triangle that has one; a vertex no triangle names is never looked at and may hold anything), a
 *   transform that takes the new box beyond 1e30, an instance of another BLAS without a box; RT_E_UNSUPPORTED: a BLAS that is not a tree,
 *   a TLAS build without a finite union area (the records restored) -- and three of its own: RT_E_STATE: no indices are bound to the
 *   BLAS; RT_E_ARG: n_vertices differs from the bound count; RT_E_ARG: a null pointer.
 * rt_set_vertices_device: the same call with dev_xyz in device memory of the context's device.  The pointer is looked up with
 *   hipPointerGetAttributes before anything is queued: RT_E_ARG if it is not device memory of that device, not 4-byte aligned, or if
 *   n_vertices points do not fit the allocation behind it.  The library reads the array on its OWN stream: the caller orders the work that
 *   produces the array before the call (synchronise the producing stream, or make the context's stream wait for it).
 *   Synchronisation: both calls read one 56-byte record (boxes and flags) back before any byte of the scene is rewritten; with the TLAS
 *     build's 4-byte read-back these are their only synchronisations.  That read-back follows the kernel that reads the vertices: when
 *     either call returns, successful or refused, xyz / dev_xyz has been read in full and is the caller's again (page-locked memory
 *     included).  This differs from rt_set_triangles, which without a TLAS does not synchronise at all: here the read-back is the one
 *     synchronisation such a scene's call has. */
int rt_set_mesh_indices(rt_ctx* ctx, uint32_t blas, const uint32_t* idx, uint32_t n_tri, uint32_t n_vertices);
int rt_set_vertices(rt_ctx* ctx, uint32_t blas, const float* xyz, uint32_t n_vertices);            /* host memory   */
int rt_set_vertices_device(rt_ctx* ctx, uint32_t blas, const float* dev_xyz, uint32_t n_vertices); /* device memory */

/* ---- relighting without a re-upload: lights, materials, skydome ------------------------------------------------------
 * The lights, the materials and the skydome are the smallest parts of a scene (56 bytes per light, 64 per material) and the ones an
 * interactive renderer changes most: a lamp dimmed, a wall turned from diffuse to metal, another sky.  The three calls below replace them
 * in the loaded scene; no BLAS is laid out or copied again.  The yardstick is rt_set_instances': afterwards the context holds, byte for
 * byte, what rt_upload_scene would hold of the updated description -- the uploaded one, as rt_set_instances / rt_set_triangles /
 * rt_set_time have left it, with lights / n_lights, materials[first .. first + count) or sky_* replaced -- and every query, frame and
 * executed-walk counter equals a freshly uploaded context's bit for bit.  rt_scene_array reads the tables back.
 * rt_set_lights replaces the WHOLE light table: n_lights may differ from the uploaded count, 0 .. 32 (lights may be NULL only with
 *   n_lights == 0).  The fields are not validated, as at upload.  The first call gives the device table room for 32 records (scene
 *   pool); later calls allocate nothing.  The per-light planes of the path state re-size themselves at the next batch that needs them.
 *   RT_E_UNSUPPORTED: more than 32 lights (rt_upload_scene's rule).
 * rt_set_materials replaces materials [first, first + count).  The NUMBER of materials cannot change: primitive records hold indices.
 *   A primitive record carries the type of its material in its kind word (csrc/rt_layout.h pack_prim), so a material that changes its
 *   'type' has that word rewritten, on the device (csrc/rt_materials.h k_retype_prims), in every primitive record the context keeps:
 *   all BLASes, the brute-force spheres and planes, the originals rt_set_time deforms from.  A call that changes no type queues the
 *   table copy alone: its cost does not depend on the size of the scene.  What path mode runs follows the new table (a diffuse material
 *   with shinieness != 0 or raytracer == 0 anywhere in it: the general kernel; RT_LAYOUT_SCALARS word 11), and so does the bounce table.
 *   RT_E_ARG: first + count beyond the uploaded count, count == 0, a null pointer, a type outside 1..3.  RT_E_UNSUPPORTED, with the
 *   Q-learning sampler on: an edit after which path mode would need the general kernel (rt_qlearn_enable's refusal, mirrored).
 * rt_set_sky replaces the skydome: pixels in rt_scene_desc's format (8-bit, n channels, w x h).  pixels == NULL switches the sky off --
 *   misses return black -- and w, h, n are not looked at.  The device array is reused when the new image fits it (also after a NULL),
 *   otherwise a new one comes from the scene pool.  RT_E_ARG: w or h below 1, or n below 3, with non-null pixels.
 *   Common to the three.  RT_E_STATE: no scene loaded.  Everything refusable is refused on the host before anything is queued: after a
 *     refusal the scene, the generations and the G-buffer are as they were.  Ordering: queued on the context's stream behind what is
 *     there.  The caller's array has been read when the call returns (the tables are copied to the host mirror first; a sky image in
 *     page-locked memory, which a copy reads only when the stream gets there, makes rt_set_sky wait for its copy); there is no other
 *     synchronisation.  With rt_set_profiling on, each call is one entry of rt_profile.query.
 *   Invalidation: the G-buffer goes stale (its albedo and light hits changed; rt_denoise is RT_E_STATE until rt_render_aovs), the next
 *     dense batch rebuilds the primary-hit and bounce tables, and a captured history ends at EVERY level, as after rt_upload_scene: every
 *     carried sample holds radiance computed under the old lights, materials or sky, so rt_reproject, rt_reproject_motion and
 *     rt_reproject_deform return RT_E_STATE until a new rt_history_capture.  Not touched: the accumulator, the statistics, the active
 *     list, a budget plan, the Q table, bound mesh indices, the lens, the filter.  The caller clears. */
int rt_set_lights(rt_ctx* ctx, const rt_light* lights, uint32_t n_lights);
int rt_set_materials(rt_ctx* ctx, uint32_t first, uint32_t count, const rt_material* materials);
int rt_set_sky(rt_ctx* ctx, const uint8_t* pixels, int32_t w, int32_t h, int32_t n);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Kernels tally rt_counters (slower; keep off when timing).
 *   RT_COUNT_REFERENCE  the walk bvh::BIntersect / tlas::Intersect make: the DataCollector tallies
 *                       (bvh.cpp:610-631), identical to the oracle's
 *   RT_COUNT_EXECUTED   the walk the timed kernels make: they skip TLAS children whose geometry the ray
 *                       cannot reach, so fewer instance / node visits; same results.  The camera rays of a dense
 *                       path batch are answered from the context's primary-hit table when the timed launch
 *                       would do so (RT_PRIMARY_TABLE, default on): every sample is still one rays_nearest
 *                       query with its light_tests / brute_tests, but its walk is not repeated.  The table's own
 *                       walk (inner_visits, prim_tests, tlas_inner, instance_visits of one ray per pixel of
 *                       [-1, width] x [-1, height]) is tallied when the counting launch is the one that builds
 *                       it; a table that was already current contributes none of these walk tallies.  The same
 *                       holds one round further for the bounce table (RT_BOUNCE_TABLE, default on): the ray a glass
 *                       or metal primary hit scatters is answered from it, still one rays_nearest query with its
 *                       light_tests / brute_tests; the walk of its at most two rays per table record is tallied
 *                       by the counting launch that builds it, and a current table adds none.  And for the chain
 *                       tables (RT_BOUNCE_DEPTH 2-4): while every hit of a path so far was glass or metal, the ray of
 *                       rounds 2 .. depth is answered the same way, from levels built behind the bounce table */
#define RT_COUNT_OFF 0
#define RT_COUNT_REFERENCE 1
#define RT_COUNT_EXECUTED 2
int rt_set_counting(rt_ctx* ctx, int counting);
int rt_get_counters(rt_ctx* ctx, rt_counters* out, int reset);
/* the same tallies kept apart: nearest-hit queries (extend kernel) / occlusion queries (connect) */
int rt_get_counters_split(rt_ctx* ctx, rt_counters* nearest, rt_counters* occluded, int reset);
/* profiling != 0: HIP events bracket every kernel launch on the context's stream (rt_profile.query also takes one entry per
 * rt_select_active / rt_select_active_rows -- its three launches --, one per rt_select_active_dilated (its five launches) and per
 * rt_select_budget_dilated (the whole call, its read-backs included) and, on the SOURCE context, one per rt_gather_rows,
 * rt_gather_stats_rows or rt_gather_active: the push's copies or kernel, behind its wait) */
int rt_set_profiling(rt_ctx* ctx, int profiling);
int rt_get_profile(rt_ctx* ctx, rt_profile* out, int reset);
int rt_synchronize(rt_ctx* ctx);
/* What the library was built with (the -D flags given to the build and the compile-time tuning macros), and the tuning a
 * context resolved from its environment at rt_create (RT_* variables): measurement files are stamped with both, so that
 * counters taken on one build / tuning are not priced against timings of another.  Static / context-owned strings. */
const char* rt_build_info(void);
const char* rt_tuning_info(rt_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
