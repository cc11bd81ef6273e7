// Renderer (renderer.h, renderer.cpp of the reference): Init / Tick / Trace / Sample with the
// reference's signatures.  The pixel loop of Tick (renderer.cpp:259-291) is one rt_render() +
// rt_resolve() pair on the device; Trace and Sample evaluate a caller-supplied ray there too.
#include "rapt.h"
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

namespace rapt {

// One host thread per context, started once and parked on a condition variable between Ticks (a context is not thread safe,
// and each thread binds its context's device once): the scanline loop of renderer.cpp:259 with one interleaved share of the rows
// per GPU.  Round 3 spawned and joined N std::threads in every Tick.
struct Renderer::Workers {
	struct Slot { std::thread th; std::function<void()> job; bool busy = false; std::exception_ptr err; };
	std::vector<Slot> slots;
	std::mutex m;
	std::condition_variable wake, done;
	bool quit = false;
	explicit Workers(int n) : slots((size_t)n)
	{
		for (int k = 0; k < n; k++)
			slots[(size_t)k].th = std::thread([this, k]() {
				Slot& s = slots[(size_t)k];
				std::unique_lock<std::mutex> lk(m);
				for (;;) {
					wake.wait(lk, [&]() { return quit || s.busy; });
					if (quit) return;
					std::function<void()> job = s.job;
					lk.unlock();
					std::exception_ptr e;
					try { job(); } catch (...) { e = std::current_exception(); }
					lk.lock();
					s.err = e, s.busy = false;
					done.notify_all();
				}
			});
	}
	~Workers()
	{
		{ std::lock_guard<std::mutex> lk(m); quit = true; }
		wake.notify_all();
		for (Slot& s : slots) s.th.join();
	}
	// run job(k) on worker k for every k, wait for all, rethrow the first failure
	void run(const std::function<void(int)>& job)
	{
		{
			std::lock_guard<std::mutex> lk(m);
			for (size_t k = 0; k < slots.size(); k++) slots[k].job = [&job, k]() { job((int)k); }, slots[k].busy = true, slots[k].err = nullptr;
		}
		wake.notify_all();
		std::unique_lock<std::mutex> lk(m);
		done.wait(lk, [&]() { for (const Slot& s : slots) if (s.busy) return false; return true; });
		for (Slot& s : slots) if (s.err) std::rethrow_exception(s.err);
	}
};

static void check(rt_ctx* ctx, int rc)
{
	if (rc != RT_OK) throw std::runtime_error(std::string("rt_amd: ") + rt_last_error(ctx));
}

Renderer::Renderer(int w, int h, int dev) : width(w), height(h), device(dev) { camera.Reset(w, h); devices.assign(1, dev); }

void Renderer::UseDevices(const std::vector<int>& devs)
{
	if (ctx) throw std::runtime_error("Renderer::UseDevices: call before Init()");
	if (devs.empty()) throw std::runtime_error("Renderer::UseDevices: no device");
	devices = devs;
	device = devs[0];
}
void Renderer::UseAllDevices()
{
	std::vector<int> d;
	for (int i = 0; i < rt_device_count(); i++) d.push_back(i);
	if (d.empty()) throw std::runtime_error("rt_amd: no HIP device");
	UseDevices(d);
}
Renderer::~Renderer() { Shutdown(); }

void Renderer::Init() // renderer.cpp:5-11: allocate and zero the float4 accumulator
{
	if (ctx) return;
	for (int d : devices) {
		rt_ctx* c = rt_create(d, width, height);
		if (!c) { const std::string why = rt_last_error(nullptr); for (rt_ctx* o : ctxs) rt_destroy(o); ctxs.clear(); throw std::runtime_error("rt_amd: " + why); }
		ctxs.push_back(c);
	}
	ctx = ctxs[0];
	if (ctxs.size() > 1) workers = new Workers((int)ctxs.size());
	accumulator = new float4[(size_t)width * height]();
	screenPixels = new uint32_t[(size_t)width * height];
	memset(screenPixels, 0, 4 * (size_t)width * height);
	frame = 0;
}

void Renderer::Shutdown()
{
	delete workers;
	workers = nullptr;
	for (rt_ctx* c : ctxs) rt_destroy(c);
	ctxs.clear();
	ctx = nullptr;
	scene.ctx = nullptr, scene.alsoCtx.clear(); // the scene's contexts are gone with ours
	delete[] accumulator;
	delete[] screenPixels;
	accumulator = nullptr, screenPixels = nullptr;
}

void Renderer::Commit()
{
	if (!ctx) Init();
	scene.Commit(ctx);
	for (size_t k = 1; k < ctxs.size(); k++) scene.CommitAlso(ctxs[k]);
	if (motionPending) motionPending = deformPending = false, clearPending = true, camera.SetChange(true); // the upload ended the history CommitInstances / CommitTriangles captured: the next Tick clears
}

// what CommitInstances and CommitTriangles do before the scene's own commit: may the next adaptive Tick carry?  If so, and no capture is
// pending yet, the history is captured under the camera of the samples
bool Renderer::CaptureForCarry()
{
	const bool carry = reproject && adaptive && !scene.raytracer && adaptiveOn && lastTickAdaptive && !sampledCam.fisheye && !camera.fishEye;
	if (carry && !motionPending) { // (a second change before the Tick: the history of the first capture still holds the samples' moment)
		check(ctx, rt_set_camera(ctx, &sampledCam)); // the camera of the samples: already the context's unless a caller synced the new one early
		check(ctx, rt_render_aovs(ctx, 0.001f));     // a no-op when the G-buffer is current
		check(ctx, rt_history_capture(ctx));
	}
	return carry;
}

// Scene::CommitInstances for a renderer that may keep its samples: see rapt.h
void Renderer::CommitInstances()
{
	if (!ctx) Init();
	const bool carry = CaptureForCarry();
	// (if this throws after the capture, context 0 keeps the camera of the samples until the next Tick syncs the renderer's, as every Tick
	// does; nothing is pending, so that Tick treats the frame as it would have without this call)
	scene.CommitInstances();
	if (carry) motionPending = true;
	else clearPending = true, camera.SetChange(true); // the accumulator holds the scene before the move: the next Tick clears (no camera carry either)
}

// Scene::CommitTriangles and Scene::CommitVertices likewise: see rapt.h
void Renderer::CommitDeformation(bvh* bv, bool fromVertices)
{
	if (!ctx) Init();
	const bool carry = CaptureForCarry();
	// (a throw leaves no carry pending: with several contexts the update may have reached some of them only, so a carry that an earlier
	// call left pending becomes a clear)
	try { if (fromVertices) scene.CommitVertices(bv); else scene.CommitTriangles(bv); }
	catch (...) {
		if (motionPending) motionPending = deformPending = false, clearPending = true, camera.SetChange(true);
		throw;
	}
	if (carry) motionPending = deformPending = true;
	else clearPending = true, camera.SetChange(true);
}
void Renderer::CommitTriangles(bvh* bv) { CommitDeformation(bv, false); }
void Renderer::CommitVertices(bvh* bv) { CommitDeformation(bv, true); }

// Scene::CommitLights / CommitMaterials / CommitSky: the next Tick clears, whatever was pending (see rapt.h)
void Renderer::CommitLook(void (Scene::*commit)())
{
	if (!ctx) Init();
	try { (scene.*commit)(); }
	catch (...) { // (with several contexts the edit may have reached some of them only)
		motionPending = deformPending = false, clearPending = true, camera.SetChange(true);
		throw;
	}
	motionPending = deformPending = false, clearPending = true, camera.SetChange(true);
}
void Renderer::CommitLights() { CommitLook(&Scene::CommitLights); }
void Renderer::CommitMaterials() { CommitLook(&Scene::CommitMaterials); }
void Renderer::CommitSky() { CommitLook(&Scene::CommitSky); }
void Renderer::CommitInstanceList() { CommitLook(&Scene::CommitInstanceList); }

void Renderer::SyncCamera()
{
	rt_camera c;
	memset(&c, 0, sizeof(c));
	c.cam_pos[0] = camera.camPos.x, c.cam_pos[1] = camera.camPos.y, c.cam_pos[2] = camera.camPos.z;
	c.top_left[0] = camera.topLeft.x, c.top_left[1] = camera.topLeft.y, c.top_left[2] = camera.topLeft.z;
	c.top_right[0] = camera.topRight.x, c.top_right[1] = camera.topRight.y, c.top_right[2] = camera.topRight.z;
	c.bottom_left[0] = camera.bottomLeft.x, c.bottom_left[1] = camera.bottomLeft.y, c.bottom_left[2] = camera.bottomLeft.z;
	c.fisheye = camera.fishEye ? 1 : 0, c.view_angle = camera.viewAngle, c.y_angle = camera.yAngle;
	for (rt_ctx* k : ctxs) check(k, rt_set_camera(k, &c));
	syncedCam = c;
}

void Renderer::SyncPixelFilter()
{
	for (rt_ctx* k : ctxs) check(k, rt_set_pixel_filter(k, pixelFilter));
}

void Renderer::SyncLens()
{
	const rt_lens l = { lensRadius, focusDistance };
	for (rt_ctx* k : ctxs) check(k, rt_set_lens(k, &l));
}

rt_camera Renderer::ShutterRecord() const
{
	rt_camera c;
	memset(&c, 0, sizeof(c));
	const Camera& k = shutterCamera;
	c.cam_pos[0] = k.camPos.x, c.cam_pos[1] = k.camPos.y, c.cam_pos[2] = k.camPos.z;
	c.top_left[0] = k.topLeft.x, c.top_left[1] = k.topLeft.y, c.top_left[2] = k.topLeft.z;
	c.top_right[0] = k.topRight.x, c.top_right[1] = k.topRight.y, c.top_right[2] = k.topRight.z;
	c.bottom_left[0] = k.bottomLeft.x, c.bottom_left[1] = k.bottomLeft.y, c.bottom_left[2] = k.bottomLeft.z;
	return c;
}

void Renderer::SyncShutter()
{
	const rt_camera c = ShutterRecord();
	for (rt_ctx* k : ctxs) check(k, rt_set_shutter(k, shutter ? &c : nullptr));
}

bool Renderer::ShutterChanged() const
{
	if (shutter != sampledShutter) return true;
	if (!shutter) return false;
	const rt_camera c = ShutterRecord();
	return memcmp(&c, &sampledShutterCam, sizeof(c)) != 0;
}

void Renderer::ShutterSampled()
{
	sampledShutter = shutter;
	if (shutter) sampledShutterCam = ShutterRecord();
}

float Renderer::FocusAt(int x, int y)
{
	if (!ctx) Init();
	float d = 0.0f;
	SyncCamera(); // (an unchanged camera keeps the G-buffer current)
	check(ctx, rt_focus_at(ctx, x, y, &d));
	return d;
}

// renderer.cpp:240-305 without the animation, input and printf parts.  As in the reference, 'it' is read before a
// camera change resets the iteration number (:247 vs :253-255): the frame on which the camera changed is resolved
// with the stale count and does not advance it (:293-294).
void Renderer::Tick(float /*deltaTime*/)
{
	if (!ctx) Init();
	if (adaptive) {
		if (denoise) throw std::runtime_error("Renderer::Tick: adaptive with denoise: rt_denoise divides the whole frame by one iteration count");
		if (qlearning) throw std::runtime_error("Renderer::Tick: adaptive with the Q-learning sampler: the rewards of a pixel subset are not defined");
		if (adaptiveDilate > 0 && ctxs.size() > 1) throw std::runtime_error("Renderer::Tick: adaptiveDilate with several contexts: a context that holds one row shard has no statistics for its neighbours' rows");
		if (!scene.raytracer) { TickAdaptive(); return; }
	} else {
		if (denoiseVariance) throw std::runtime_error("Renderer::Tick: denoiseVariance without adaptive: rt_denoise_variance needs the per-pixel statistics adaptive sampling keeps");
		if (reproject) throw std::runtime_error("Renderer::Tick: reproject without adaptive: rt_reproject rewrites the per-pixel statistics adaptive sampling keeps");
		if (adaptiveOn) {
			for (rt_ctx* k : ctxs) check(k, rt_stats_enable(k, 0));
			adaptiveOn = false;
		}
	}
	lastTickAdaptive = false;
	if (motionPending) motionPending = deformPending = false, camera.SetChange(true); // the carry was for an adaptive Tick: this one clears (path) or redraws
	clearPending = false; // (this Tick clears on the camera change that was set with it)
	scene.totIterationNumber++;
	const int it = scene.GetIterationNumber();
	SyncPixelFilter();
	SyncLens();
	SyncShutter();
	// (a path Tick under another filter kind, lens or shutter than the last one's: like a camera change)
	const bool camChanged = camera.GetChange() || (!scene.raytracer && (pixelFilter != sampledFilter || LensChanged() || ShutterChanged()));
	if (!scene.raytracer) sampledFilter = pixelFilter, sampledLens = { lensRadius, focusDistance }, ShutterSampled();
	if (camChanged && !scene.raytracer) {
		scene.SetIterationNumber(1);
		for (rt_ctx* k : ctxs) check(k, rt_clear(k)); // accumulator[...] = float3(0) for every pixel (:273-275)
	}
	SyncCamera();
	const int mode = scene.raytracer ? RT_MODE_WHITTED : RT_MODE_PATH;
	const int n = (int)ctxs.size();
	if (n == 1) check(ctx, rt_render(ctx, mode, frame, 1, seedBase, 0, height, 4));
	else {
		// the scanline loop of renderer.cpp:259, one interleaved share of the rows per GPU, each on its context's own (parked)
		// host thread; a share's rows are pushed to context 0 from that thread as soon as they are queued -- every gather is
		// issued before anything waits (rt_gather_rows is asynchronous: context 0's stream waits for the rows, not the host)
		check(ctx, rt_gather_begin(ctx)); // context 0's rows are free from here on (after the clear above and the resolve of the frame before): the pushes wait for this mark alone
		workers->run([&](int k) {
			const int count = (height - k + n - 1) / n;
			if (count <= 0) return;
			check(ctxs[k], rt_render_rows(ctxs[k], mode, frame, 1, seedBase, k, n, count, 4));
			if (k > 0) check(ctxs[k], rt_gather_rows(ctx, ctxs[k], k, n, count)); // (its errors are reported on the source context)
		});
	}
	if (!scene.raytracer && qlearning) {
		// learning happens between frames: add the contexts' pending (integer) reward sums, give every context the total, apply
		if (n > 1) {
			std::vector<int64_t> sum, s1;
			std::vector<uint32_t> cnt, c1;
			const size_t cells = (size_t)qgrid * qgrid * qgrid * 64;
			sum.assign(cells, 0), cnt.assign(cells, 0), s1.resize(cells), c1.resize(cells);
			for (rt_ctx* k : ctxs) {
				check(k, rt_qlearn_get_sums(k, s1.data(), c1.data()));
				for (size_t i = 0; i < cells; i++) sum[i] += s1[i], cnt[i] += c1[i];
			}
			for (rt_ctx* k : ctxs) check(k, rt_qlearn_set_sums(k, sum.data(), cnt.data()));
		}
		for (rt_ctx* k : ctxs) check(k, rt_qlearn_apply(k));
	}
	if (!scene.raytracer) frame++;
	if (!scene.raytracer && denoise) {
		// context 0 holds the gathered accumulator (its stream already waits for every gather) and the synced camera
		check(ctx, rt_render_aovs(ctx, 0.001f)); // a no-op unless the camera, the scene or the time changed
		check(ctx, rt_denoise(ctx, it, &denoiseParams));
		check(ctx, rt_resolve_denoised(ctx, 0, height, screenPixels));
	} else
		check(ctx, rt_resolve(ctx, it, 0, height, screenPixels));
	if (downloadEachTick) check(ctx, rt_download_accumulator(ctx, 0, height, &accumulator[0].x));
	if (!scene.raytracer && !camChanged) scene.SetIterationNumber(it + 1);
	camera.SetChange(false);
}

// Tick in path mode with 'adaptive' set: the iteration bookkeeping of Tick, whole frames until every pixel has min_samples samples, then
// one frame of the pixels that are still noisy; every pixel is shown divided by its own count.  With adaptivePassCap > 0 every Tick is a
// budgeted pass instead (rt_select_budget + rt_render_budget).  With adaptiveDilate > 0 (one context only) the selections are the dilated ones.
// Several contexts: context k renders, selects and samples the rows k, k + n, ... only (rt_render_rows, rt_select_active_rows /
// rt_select_budget_rows: the predicate is per pixel and a sample a function of (seed, pixel, frame), so the shards' lists are the
// one-context list cut by rows and the frame is the one-context frame bit for bit) and pushes what it wrote to context 0: whole rows with
// their statistics after a whole frame (rt_gather_stats_rows), the listed pixels alone after a pass (rt_gather_active).  Context 0 holds
// the gathered frame and its statistics: the carry, the resolve and the denoiser run there.
void Renderer::TickAdaptive()
{
	scene.totIterationNumber++;
	const int it = scene.GetIterationNumber();
	const int n = (int)ctxs.size();
	const bool filterChanged = pixelFilter != sampledFilter || LensChanged() || ShutterChanged(); // like a camera change, without a carry: the carried samples would be the old kind's, the old lens's or the old shutter's
	SyncPixelFilter();
	SyncLens();
	SyncShutter();
	sampledFilter = pixelFilter, sampledLens = { lensRadius, focusDistance }, ShutterSampled();
	const bool motion = motionPending; // CommitInstances captured the history and moved the instances: carry with rt_reproject_motion
	const bool deform = deformPending; // ... CommitTriangles deformed a mesh as well: rt_reproject_deform, which subsumes the other two carries
	motionPending = deformPending = false;
	const bool mustClear = clearPending; // the instances moved without a capture (or the scene was committed again): nothing to carry from
	clearPending = false;
	bool reset = camera.GetChange() || filterChanged || motion || mustClear;
	// a camera move with 'reproject' set (statistics already on, pinhole before and after): the samples follow their surface points
	// (only straight after an adaptive Tick: a Whitted Tick in between has overwritten the accumulator under cameras of its own);
	// an instance move through Renderer::CommitInstances takes the same path, the camera moved as well or not
	const bool carry = reset && !filterChanged && !mustClear && reproject && adaptiveOn && lastTickAdaptive && !sampledCam.fisheye && !camera.fishEye;
	if (!adaptiveOn) {
		for (rt_ctx* k : ctxs) check(k, rt_stats_enable(k, 1));
		adaptiveOn = true, reset = true; // the counts start now, so the accumulator does too
	}
	if (carry) {
		scene.SetIterationNumber(1);
		if (!motion) {
			check(ctx, rt_set_camera(ctx, &sampledCam)); // the camera of the samples: already the context's unless a caller synced the new one early
			check(ctx, rt_render_aovs(ctx, 0.001f));     // a no-op when the G-buffer is current
			check(ctx, rt_history_capture(ctx));
		}
		SyncCamera();
		check(ctx, rt_render_aovs(ctx, 0.001f));
		if (motion && deform) check(ctx, rt_reproject_deform(ctx, &reprojectParams, &carriedPixels));
		else if (motion) check(ctx, rt_reproject_motion(ctx, &reprojectParams, &carriedPixels));
		else check(ctx, rt_reproject(ctx, &reprojectParams, &carriedPixels));
		// every pixel of context 0 is rewritten: each context gets its own rows back before it selects over them
		for (int k = 1; k < n; k++) {
			const int count = (height - k + n - 1) / n;
			if (count > 0) check(ctx, rt_gather_stats_rows(ctxs[k], ctx, k, n, count)); // (context 0 is the source: its errors are reported there)
		}
		wholeFrames = adaptiveParams.min_samples; // straight to the selection: a pixel below min_samples is active by definition
		frameBase = frame;
	} else if (reset) {
		scene.SetIterationNumber(1);
		for (rt_ctx* k : ctxs) check(k, rt_clear(k)); // the statistics with the accumulator
		wholeFrames = 0;
		frameBase = frame;
	}
	if (!carry) SyncCamera();
	sampledCam = syncedCam, lastTickAdaptive = true;
	rt_budget_params bp;
	bp.select = adaptiveParams, bp.pass_cap = adaptivePassCap, bp.max_pass_samples = adaptiveMaxPassSamples;
	const bool budgeted = adaptivePassCap > 0, whole = !budgeted && wholeFrames < adaptiveParams.min_samples;
	if (n > 1) {
		// context 0's pixels are free from here on: after the clear or the carry above (its pushes to the other contexts included) and the
		// resolve of the Tick before; the pushes of this Tick wait for this mark alone
		check(ctx, rt_gather_begin(ctx));
		std::vector<int> active((size_t)n, 0);
		std::vector<uint32_t> taken((size_t)n, 0);
		workers->run([&](int k) {
			rt_ctx* c = ctxs[(size_t)k];
			const int count = (height - k + n - 1) / n;
			if (count <= 0) return;
			if (whole) {
				check(c, rt_render_rows(c, RT_MODE_PATH, frame, 1, seedBase, k, n, count, 4));
				active[(size_t)k] = count * width, taken[(size_t)k] = (uint32_t)(count * width);
				if (k > 0) check(c, rt_gather_stats_rows(ctx, c, k, n, count));
				return;
			}
			if (budgeted) {
				int capUsed = 0;
				check(c, rt_select_budget_rows(c, &bp, k, n, count, &active[(size_t)k], &taken[(size_t)k], &capUsed));
				check(c, rt_render_budget(c, frameBase, seedBase, 4));
			} else {
				check(c, rt_select_active_rows(c, &adaptiveParams, k, n, count, &active[(size_t)k]));
				check(c, rt_render_active(c, frame, 1, seedBase, 4));
				taken[(size_t)k] = (uint32_t)active[(size_t)k];
			}
			if (k > 0) {
				int rc = rt_gather_active(ctx, c); // the list outlives the pass
				if (rc == RT_E_UNSUPPORTED) rc = rt_gather_stats_rows(ctx, c, k, n, count); // no peer access from this context's device: its rows whole
				check(c, rc);
			}
		});
		activePixels = passSamples = 0;
		for (int k = 0; k < n; k++) activePixels += active[(size_t)k], passSamples += (int)taken[(size_t)k];
		if (whole) wholeFrames++;
		else wholeFrames = adaptiveParams.min_samples;
	} else if (budgeted) {
		// a budgeted pass: every active pixel's own number of samples as one batch (no whole-frame phase: a pixel below min_samples is active)
		uint32_t taken = 0;
		int capUsed = 0;
		if (adaptiveDilate > 0) check(ctx, rt_select_budget_dilated(ctx, &bp, adaptiveDilate, &activePixels, &taken, &capUsed));
		else check(ctx, rt_select_budget(ctx, &bp, &activePixels, &taken, &capUsed));
		check(ctx, rt_render_budget(ctx, frameBase, seedBase, 4));
		passSamples = (int)taken;
		wholeFrames = adaptiveParams.min_samples; // (switching the cap off mid-run goes on with selections: the counts are uneven)
	} else if (whole) {
		check(ctx, rt_render(ctx, RT_MODE_PATH, frame, 1, seedBase, 0, height, 4));
		wholeFrames++, activePixels = width * height, passSamples = activePixels;
	} else {
		if (adaptiveDilate > 0) check(ctx, rt_select_active_dilated(ctx, &adaptiveParams, adaptiveDilate, &activePixels));
		else check(ctx, rt_select_active(ctx, &adaptiveParams, &activePixels));
		check(ctx, rt_render_active(ctx, frame, 1, seedBase, 4));
		passSamples = activePixels;
	}
	frame++;
	if (denoiseVariance) {
		check(ctx, rt_render_aovs(ctx, 0.001f)); // a no-op unless the camera, the scene or the time changed
		check(ctx, rt_denoise_variance(ctx, &denoiseVarParams));
		check(ctx, rt_resolve_denoised(ctx, 0, height, screenPixels));
	} else
		check(ctx, rt_resolve_adaptive(ctx, 0, height, screenPixels));
	if (downloadEachTick) check(ctx, rt_download_accumulator(ctx, 0, height, &accumulator[0].x));
	if (!reset) scene.SetIterationNumber(it + 1);
	camera.SetChange(false);
}

void Renderer::EnableQLearning(int grid, float3 lo, float3 hi, float alpha, float epsilon, float qInit)
{
	if (!ctx) Init();
	rt_qlearn_params p;
	p.grid = grid, p.alpha = alpha, p.epsilon = epsilon, p.q_init = qInit, p.learn_mask = qlearnMask;
	p.lo[0] = lo.x, p.lo[1] = lo.y, p.lo[2] = lo.z, p.hi[0] = hi.x, p.hi[1] = hi.y, p.hi[2] = hi.z;
	for (rt_ctx* k : ctxs) check(k, rt_qlearn_enable(k, &p));
	qlearning = true, qgrid = grid;
}
void Renderer::DisableQLearning()
{
	for (rt_ctx* k : ctxs) check(k, rt_qlearn_enable(k, nullptr));
	qlearning = false;
}

static float3 eval(rt_ctx* ctx, int mode, const Ray& ray, int depth, const float3& energy, uint32_t seed)
{
	float rgb[3];
	check(ctx, rt_trace_batch_energy(ctx, mode, 1, &ray.O.x, &ray.D.x, depth, seed, &energy.x, rgb));
	return float3(rgb[0], rgb[1], rgb[2]);
}
// Trace / Sample on a caller's ray, with scene.raytracer as the Scene holds it: the combinations Tick makes (Trace with the flag set, Sample
// with it clear) run the wavefront kernels, the other two (renderer.cpp:33-43, 107-121, 143-153) the general kernels (rt_set_scene_raytracer).
// (the flag is the context's only for the duration of the call: direct users of the C ABI keep their own setting's default)
struct ScopedSceneFlag {
	rt_ctx* ctx;
	ScopedSceneFlag(rt_ctx* c, bool raytracer) : ctx(c) { check(c, rt_set_scene_raytracer(c, raytracer ? 1 : 0)); }
	~ScopedSceneFlag() { (void)rt_set_scene_raytracer(ctx, -1); }
};
float3 Renderer::Trace(Ray& ray, int depth, float3 energy)
{
	ScopedSceneFlag flag(ctx, scene.raytracer);
	return eval(ctx, RT_MODE_WHITTED, ray, depth, energy, seedBase);
}
float3 Renderer::Sample(Ray& ray, int depth, float3 energy)
{
	ScopedSceneFlag flag(ctx, scene.raytracer);
	return eval(ctx, RT_MODE_PATH, ray, depth, energy, seedBase);
}

} // namespace rapt
