// Headless C++ host over the rapt:: mirror of the reference's interface: load a scene description,
// run Renderer::Tick like the reference's main loop does (template/template.cpp:266-270), write the
// resolved frame as a binary PPM.  Everything below Renderer / Scene goes through the C ABI of
// include/rt_amd.h.
//
//   g++ -std=c++17 -O2 examples/render_scene.cpp -Iray-and-pathtracer_amd/host \
//       -Lray-and-pathtracer_amd/host -lrapt_host -Lray-and-pathtracer_amd/csrc -lrt_amd \
//       -Wl,-rpath,$PWD/ray-and-pathtracer_amd/host -Wl,-rpath,$PWD/ray-and-pathtracer_amd/csrc -o render_scene
//   ./render_scene scene.rapt out.ppm 640 360 path 16 [all | d0,d1,...] [--filter reference|point|box|tent] [--aperture R --focus D | --focus-pixel X,Y] [--shutter DX,DY,DZ] [--spin DEG [--carry]]
// The optional last argument spreads every Tick over several GPUs (one rt_ctx and one host thread per device,
// rows interleaved, rt_gather_rows into device d0): "all" = every visible device.  --filter (anywhere after the frame count) sets
// Renderer::pixelFilter: the sub-pixel camera samples of path mode (rt_set_pixel_filter; default: the reference's truncated jitter).
// --aperture R (path mode, with a --filter other than reference) gives the camera a thin lens of radius R (Renderer::lensRadius, rt_set_lens)
// focused at --focus D, or on what pixel X,Y sees with --focus-pixel X,Y (Renderer::FocusAt, rt_focus_at), which also prints that distance.
// --shutter DX,DY,DZ (path mode, with a --filter other than reference): camera motion blur.  The camera translates by that vector over the
// exposure, all four points (Renderer::shutter / shutterCamera, rt_set_shutter): every sample is taken at a time of its own.
// --spin DEG (a TLAS scene): before the last frame instance 0 is turned by DEG degrees about y (bvhInstance::SetTransform) and sent on with
// Scene::CommitInstances (rt_set_instances: no re-upload); that Tick clears, so the image is the moved scene's.
// --carry (path mode with --spin only; refused otherwise): the Ticks are adaptive with Renderer::reproject set and the move goes through Renderer::CommitInstances,
// so the last Tick keeps the samples of the frames before it where their surface points are still in view (rt_reproject_motion).
#include "rapt.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <vector>

using namespace rapt;

int main(int argc, char** argv)
{
	if (argc < 7) { fprintf(stderr, "usage: %s scene.rapt out.ppm width height whitted|path frames [all | d0,d1,...] [--filter reference|point|box|tent] [--aperture R --focus D | --focus-pixel X,Y] [--shutter DX,DY,DZ] [--spin DEG [--carry]]\n", argv[0]); return 2; }
	int filter = RT_FILTER_REFERENCE;
	float spin = 0;
	bool carry = false;
	for (int a = 7; a < argc; a++) {
		if (strcmp(argv[a], "--carry") != 0) continue;
		carry = true;
		for (int b = a; b + 1 < argc; b++) argv[b] = argv[b + 1];
		argc -= 1, a--;
	}
	for (int a = 7; a + 1 < argc; a++) {
		if (strcmp(argv[a], "--spin") != 0) continue;
		spin = (float)atof(argv[a + 1]);
		for (int b = a; b + 2 < argc; b++) argv[b] = argv[b + 2];
		argc -= 2, a--;
	}
	float aperture = 0, focus = 1;
	int focusX = -1, focusY = -1;
	for (int a = 7; a + 1 < argc; a++) {
		const bool ap = strcmp(argv[a], "--aperture") == 0, fo = strcmp(argv[a], "--focus") == 0, fp = strcmp(argv[a], "--focus-pixel") == 0;
		if (!ap && !fo && !fp) continue;
		if (ap) aperture = (float)atof(argv[a + 1]);
		if (fo) focus = (float)atof(argv[a + 1]);
		if (fp && sscanf(argv[a + 1], "%d,%d", &focusX, &focusY) != 2) { fprintf(stderr, "--focus-pixel X,Y\n"); return 2; }
		for (int b = a; b + 2 < argc; b++) argv[b] = argv[b + 2];
		argc -= 2, a--;
	}
	float shutterMove[3] = { 0, 0, 0 };
	bool shutter = false;
	for (int a = 7; a + 1 < argc; a++) {
		if (strcmp(argv[a], "--shutter") != 0) continue;
		if (sscanf(argv[a + 1], "%f,%f,%f", &shutterMove[0], &shutterMove[1], &shutterMove[2]) != 3) { fprintf(stderr, "--shutter DX,DY,DZ\n"); return 2; }
		shutter = true;
		for (int b = a; b + 2 < argc; b++) argv[b] = argv[b + 2];
		argc -= 2, a--;
	}
	for (int a = 7; a < argc; a++) {
		if (strcmp(argv[a], "--filter") != 0) continue;
		static const char* const names[4] = { "reference", "point", "box", "tent" };
		int k = -1;
		for (int i = 0; i < 4 && a + 1 < argc; i++) if (strcmp(argv[a + 1], names[i]) == 0) k = i;
		if (k < 0) { fprintf(stderr, "--filter reference|point|box|tent\n"); return 2; }
		filter = k;
		for (int b = a; b + 2 < argc; b++) argv[b] = argv[b + 2]; // the positional arguments close up
		argc -= 2, a--;
	}
	const int w = atoi(argv[3]), h = atoi(argv[4]), frames = atoi(argv[6]);
	const bool path = strcmp(argv[5], "path") == 0;
	if (carry && (spin == 0 || !path)) { fprintf(stderr, "--carry needs --spin DEG and path mode (it keeps the path samples across the spin)\n"); return 2; }
	try {
		Renderer app(w, h, 0);
		if (argc > 7) {
			if (strcmp(argv[7], "all") == 0) app.UseAllDevices();
			else {
				std::vector<int> devs;
				for (const char* p = argv[7]; *p;) { devs.push_back(atoi(p)); while (*p && *p != ',') p++; if (*p) p++; }
				app.UseDevices(devs);
			}
		}
		app.pixelFilter = filter;
		if (carry) app.adaptive = app.reproject = true;
		app.Init();                          // allocates the accumulator on the GPU(s)
		app.scene.LoadFile(argv[1]);         // meshes, materials, lights, BVH / TLAS (host builders)
		if (path) app.scene.toogleRaytracer(); // key 'P' in the reference: path tracing, lights sampled
		app.Commit();                        // flatten + rt_upload_scene on every context
		if (focusX >= 0) {
			focus = app.FocusAt(focusX, focusY);
			printf("focus distance at pixel %d,%d: %g%s\n", focusX, focusY, focus, focus > 0 ? "" : " (the sky: the lens stays off)");
			if (!(focus > 0)) aperture = 0;
		}
		app.lensRadius = aperture, app.focusDistance = focus;
		if (shutter) {
			const float3 move(shutterMove[0], shutterMove[1], shutterMove[2]);
			app.shutterCamera = app.camera; // the camera at shutter close: the open camera, translated
			app.shutterCamera.camPos = app.camera.camPos + move, app.shutterCamera.topLeft = app.camera.topLeft + move;
			app.shutterCamera.topRight = app.camera.topRight + move, app.shutterCamera.bottomLeft = app.camera.bottomLeft + move;
			app.shutter = true;
		}
		const int ticks = path ? frames : 1;
		for (int f = 0; f < ticks; f++) {
			if (spin != 0 && f == ticks - 1) {
				if (!app.scene.useTLAS) throw std::runtime_error("--spin needs a scene with a TLAS");
				mat4 M = app.scene.bvhList[0].matTransform * mat4::RotateY(spin * 3.14159265358979f / 180.0f);
				app.scene.bvhList[0].SetTransform(M);
				if (carry) app.CommitInstances(); // adaptive path Ticks: this Tick carries the samples across the move; otherwise it clears
				else {
					app.scene.CommitInstances();
					app.camera.SetChange(true); // the accumulator holds the scene before the move: this Tick clears
				}
			}
			app.Tick(0.0f);
		}
		FILE* out = fopen(argv[2], "wb");
		if (!out) { perror(argv[2]); return 1; }
		fprintf(out, "P6\n%d %d\n255\n", w, h);
		for (int i = 0; i < w * h; i++) {
			const uint32_t p = app.screenPixels[i]; // 0x00RRGGBB, as Surface::pixels
			const unsigned char rgb[3] = { (unsigned char)(p >> 16), (unsigned char)(p >> 8), (unsigned char)p };
			fwrite(rgb, 1, 3, out);
		}
		fclose(out);
		app.Shutdown();
	} catch (const std::exception& e) {
		fprintf(stderr, "error: %s\n", e.what());
		return 1;
	}
	return 0;
}
