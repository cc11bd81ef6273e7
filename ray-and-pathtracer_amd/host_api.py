"""ctypes bindings of the product: the C ABI of librt_amd.so (include/rt_amd.h) and the C++ host
mirror librapt_host.so (host/rapt.h).  No CPU fallback exists: loading fails loudly when a library
is missing, and every device call raises when there is no gfx950 GPU.

HostScene implements the scene-builder protocol used by scenes.py (the same protocol the oracle
implements in oracle/oracle_api.py, which this module never imports).
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
RT_SO = os.path.join(_HERE, "csrc", "librt_amd.so")
HOST_SO = os.path.join(_HERE, "host", "librapt_host.so")

RT_MODE_WHITTED, RT_MODE_PATH = 0, 1
RT_COUNT_OFF, RT_COUNT_REFERENCE, RT_COUNT_EXECUTED = 0, 1, 2
COUNTER_NAMES = ["inner_visits", "prim_tests", "tlas_inner", "instance_visits",
                 "rays_nearest", "rays_occluded", "brute_tests", "light_tests"]

# every symbol include/rt_amd.h declares
RT_SYMBOLS = ["rt_device_count", "rt_create", "rt_destroy", "rt_last_error", "rt_upload_scene", "rt_set_camera", "rt_set_time",
              "rt_render", "rt_render_rows", "rt_clear", "rt_download_accumulator", "rt_resolve", "rt_accumulator_device_ptr",
              "rt_bind_accumulator", "rt_intersect_batch", "rt_occluded_batch", "rt_primary_hits", "rt_trace_batch",
              "rt_set_counting", "rt_get_counters", "rt_get_counters_split", "rt_set_profiling", "rt_get_profile", "rt_synchronize",
              "rt_build_bvh", "rt_build_bvh_split", "rt_build_tlas", "rt_gather_rows", "rt_gather_begin", "rt_device_of",
              "rt_intersect_scope", "rt_occluded_scope", "rt_sky_color_batch", "rt_trace_batch_energy", "rt_build_info", "rt_tuning_info",
              "rt_qlearn_enable", "rt_qlearn_apply", "rt_qlearn_get_sums", "rt_qlearn_set_sums", "rt_qlearn_get_table", "rt_qlearn_bind_sums",
              "rt_device_pci_bus_id", "rt_set_scene_raytracer",
              "rt_render_aovs", "rt_download_aovs", "rt_denoise", "rt_download_denoised", "rt_resolve_denoised",
              "rt_stats_enable", "rt_download_stats", "rt_select_active", "rt_set_active_pixels", "rt_download_active",
              "rt_render_active", "rt_resolve_adaptive", "rt_denoise_variance",
              "rt_select_budget", "rt_download_budgets", "rt_render_budget",
              "rt_history_capture", "rt_reproject", "rt_download_aov_positions", "rt_reproject_motion", "rt_download_aov_instances",
              "rt_reproject_deform", "rt_download_aov_prims",
              "rt_select_active_rows", "rt_select_budget_rows", "rt_gather_stats_rows", "rt_gather_active",
              "rt_select_active_dilated", "rt_select_budget_dilated",
              "rt_set_pixel_filter", "rt_get_pixel_filter", "rt_sample_rays",
              "rt_set_lens", "rt_get_lens", "rt_focus_at",
              "rt_set_shutter", "rt_get_shutter",
              "rt_layout_build", "rt_layout_array", "rt_layout_free", "rt_launch_form", "rt_any_hit_walk",
              "rt_set_instances", "rt_set_instance_list", "rt_download_tlas", "rt_scene_array",
              "rt_set_triangles", "rt_blas_array",
              "rt_set_mesh_indices", "rt_set_vertices", "rt_set_vertices_device",
              "rt_set_lights", "rt_set_materials", "rt_set_sky"]

RT_E_ARG, RT_E_STATE = -2, -5
# include/rt_amd.h rt_set_pixel_filter
RT_FILTER_REFERENCE, RT_FILTER_POINT, RT_FILTER_BOX, RT_FILTER_TENT = 0, 1, 2, 3
RT_E_UNSUPPORTED = -4
# include/rt_amd.h rt_set_lens
RT_LENS_TRIES = 16
# include/rt_amd.h RT_ADAPTIVE_DEFAULTS (a starting point, not tuned)
ADAPTIVE_DEFAULTS = dict(min_samples=16, max_samples=1024, threshold=0.05, floor=1e-3)
# include/rt_amd.h RT_DENOISE_DEFAULTS
DENOISE_DEFAULTS = dict(iterations=5, sigma_color=0.5, sigma_normal=0.25, sigma_position=0.1, sigma_albedo=0.1)


class RtQlearnParams(C.Structure):
    _fields_ = [("grid", C.c_int32), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("alpha", C.c_float), ("epsilon", C.c_float), ("q_init", C.c_float), ("learn_mask", C.c_uint32)]


class RtLens(C.Structure):
    _fields_ = [("radius", C.c_float), ("focus_distance", C.c_float)]


class RtCamera(C.Structure):
    """include/rt_amd.h rt_camera"""
    _fields_ = [("cam_pos", C.c_float * 3), ("top_left", C.c_float * 3), ("top_right", C.c_float * 3), ("bottom_left", C.c_float * 3),
                ("fisheye", C.c_int32), ("view_angle", C.c_float), ("y_angle", C.c_float)]


class RtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float), ("sigma_albedo", C.c_float)]


def denoise_params(params=None):
    """rt_denoise_params from a dict of DENOISE_DEFAULTS' keys (missing keys: the defaults); None -> None (the library's defaults)"""
    if params is None:
        return None
    p = dict(DENOISE_DEFAULTS, **params)
    return RtDenoiseParams(int(p["iterations"]), p["sigma_color"], p["sigma_normal"], p["sigma_position"], p["sigma_albedo"])


# include/rt_amd.h RT_DENOISE_VAR_DEFAULTS (a starting point, not tuned)
DENOISE_VAR_DEFAULTS = dict(iterations=5, sigma_luminance=4.0, sigma_normal=0.25, sigma_position=0.1, sigma_albedo=0.1, epsilon=1e-4)


class RtDenoiseVarParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("sigma_albedo", C.c_float), ("epsilon", C.c_float)]


def denoise_var_params(params=None):
    """rt_denoise_var_params from a dict of DENOISE_VAR_DEFAULTS' keys (missing keys: the defaults); None -> None (the library's defaults)"""
    if params is None:
        return None
    p = dict(DENOISE_VAR_DEFAULTS, **params)
    return RtDenoiseVarParams(int(p["iterations"]), p["sigma_luminance"], p["sigma_normal"], p["sigma_position"], p["sigma_albedo"], p["epsilon"])


class RtAdaptiveParams(C.Structure):
    _fields_ = [("min_samples", C.c_int32), ("max_samples", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float)]


def adaptive_params(params=None):
    """rt_adaptive_params from a dict of ADAPTIVE_DEFAULTS' keys (missing keys: the defaults); None -> None (the library's defaults)"""
    if params is None:
        return None
    p = dict(ADAPTIVE_DEFAULTS, **params)
    return RtAdaptiveParams(int(p["min_samples"]), int(p["max_samples"]), p["threshold"], p["floor"])


# include/rt_amd.h RT_BUDGET_DEFAULTS (a starting point, not tuned); 'select' is a dict of ADAPTIVE_DEFAULTS' keys
BUDGET_DEFAULTS = dict(select=None, pass_cap=64, max_pass_samples=0)


class RtBudgetParams(C.Structure):
    _fields_ = [("select", RtAdaptiveParams), ("pass_cap", C.c_int32), ("max_pass_samples", C.c_uint32)]


def budget_params(params=None):
    """rt_budget_params from a dict of BUDGET_DEFAULTS' keys (missing keys: the defaults; 'select': see adaptive_params); None -> None"""
    if params is None:
        return None
    p = dict(BUDGET_DEFAULTS, **params)
    return RtBudgetParams(adaptive_params(p["select"] or {}), int(p["pass_cap"]), int(p["max_pass_samples"]))


# include/rt_amd.h RT_REPROJECT_DEFAULTS (a starting point, not tuned)
REPROJECT_DEFAULTS = dict(normal_tolerance=0.25, plane_tolerance=0.01, max_history=0, carry_view_dependent=0)


class RtReprojectParams(C.Structure):
    _fields_ = [("normal_tolerance", C.c_float), ("plane_tolerance", C.c_float), ("max_history", C.c_int32), ("carry_view_dependent", C.c_int32)]


def reproject_params(params=None):
    """rt_reproject_params from a dict of REPROJECT_DEFAULTS' keys (missing keys: the defaults); None -> None (the library's defaults)"""
    if params is None:
        return None
    p = dict(REPROJECT_DEFAULTS, **params)
    return RtReprojectParams(p["normal_tolerance"], p["plane_tolerance"], int(p["max_history"]), int(p["carry_view_dependent"]))


class RtCamera(C.Structure):
    _fields_ = [("cam_pos", C.c_float * 3), ("top_left", C.c_float * 3), ("top_right", C.c_float * 3),
                ("bottom_left", C.c_float * 3), ("fisheye", C.c_int32), ("view_angle", C.c_float), ("y_angle", C.c_float)]


class RtKernelTime(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("ms", C.c_double)]


class RtProfile(C.Structure):
    _fields_ = [("generate", RtKernelTime), ("extend", RtKernelTime), ("shade", RtKernelTime),
                ("connect", RtKernelTime), ("query", RtKernelTime)]


RT_TRIANGLE_DTYPE = np.dtype([("v0", np.float32, 3), ("v1", np.float32, 3), ("v2", np.float32, 3), ("N", np.float32, 3), ("obj_idx", np.int32), ("material", np.int32)])
RT_SPHERE_DTYPE = np.dtype([("pos", np.float32, 3), ("r2", np.float32), ("invr", np.float32), ("r", np.float32), ("obj_idx", np.int32), ("material", np.int32)])
RT_PLANE_DTYPE = np.dtype([("N", np.float32, 3), ("d", np.float32), ("obj_idx", np.int32), ("material", np.int32)])
RT_BVH_NODE_DTYPE = np.dtype([("aabb_min", np.float32, 3), ("left_first", np.uint32), ("aabb_max", np.float32, 3), ("prim_count", np.uint32)])
RT_INSTANCE_DTYPE = np.dtype([("blas", np.int32), ("transform", np.float32, 16), ("inv_transform", np.float32, 16)])
RT_TLAS_NODE_DTYPE = np.dtype([("aabb_min", np.float32, 3), ("left_right", np.uint32), ("aabb_max", np.float32, 3), ("blas", np.uint32)])
RT_LIGHT_DTYPE = np.dtype([("kind", np.int32), ("obj_idx", np.int32), ("pos", np.float32, 3), ("strength", np.float32), ("col", np.float32, 3), ("normal", np.float32, 3),
                           ("radius", np.float32), ("sin_angle", np.float32)])
RT_MATERIAL_DTYPE = np.dtype([("type", np.int32), ("raytracer", np.int32), ("col", np.float32, 3), ("albedo", np.float32, 3), ("specu", np.float32), ("diffu", np.float32),
                              ("shinieness", np.float32), ("N", np.int32), ("ir", np.float32), ("absorption", np.float32, 3)])
RT_HIT_DTYPE = np.dtype([("t", np.float32), ("obj_idx", np.int32), ("material", np.int32), ("normal", np.float32, 3)])


def build(force=False):
    """Compile both product libraries in-tree (hipcc cross-compiles gfx950 without a GPU)."""
    def stale(so, d):
        srcs = [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".h", ".cpp", ".hip", ".inc")) or f == "Makefile"]
        srcs.append(os.path.join(_HERE, "..", "include", "rt_amd.h"))
        return force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)
    if stale(RT_SO, os.path.join(_HERE, "csrc")):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s"])
    if stale(HOST_SO, os.path.join(_HERE, "host")) or os.path.getmtime(RT_SO) > os.path.getmtime(HOST_SO):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "host"), "-s"])


_rt = None
_host = None


def rt_lib():
    global _rt
    if _rt is None:
        if not os.path.exists(RT_SO):
            raise RuntimeError("librt_amd.so is not built (run __graft_entry__.build()); there is no fallback path")
        L = C.CDLL(RT_SO, mode=C.RTLD_GLOBAL)
        L.rt_create.restype = C.c_void_p
        L.rt_create.argtypes = [C.c_int, C.c_int, C.c_int]
        L.rt_last_error.restype = C.c_char_p
        L.rt_last_error.argtypes = [C.c_void_p]
        L.rt_qlearn_enable.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_qlearn_apply.argtypes = [C.c_void_p]
        L.rt_qlearn_get_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_qlearn_set_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_qlearn_get_table.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_qlearn_bind_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_int]
        L.rt_gather_begin.argtypes = [C.c_void_p]
        L.rt_set_scene_raytracer.argtypes = [C.c_void_p, C.c_int]
        L.rt_build_info.restype = C.c_char_p
        L.rt_build_info.argtypes = []
        L.rt_tuning_info.restype = C.c_char_p
        L.rt_tuning_info.argtypes = [C.c_void_p]
        L.rt_accumulator_device_ptr.restype = C.c_void_p
        L.rt_accumulator_device_ptr.argtypes = [C.c_void_p]
        for name in ["rt_destroy", "rt_upload_scene", "rt_set_camera", "rt_set_time", "rt_clear", "rt_synchronize"]:
            getattr(L, name).argtypes = [C.c_void_p] + ([C.c_void_p] if name in ("rt_upload_scene", "rt_set_camera") else [])
        L.rt_set_time.argtypes = [C.c_void_p, C.c_float]
        L.rt_render.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int]
        L.rt_render_rows.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.rt_get_counters_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.rt_download_accumulator.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_resolve.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.rt_bind_accumulator.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_intersect_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.rt_occluded_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_primary_hits.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.rt_trace_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        L.rt_trace_batch_energy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_intersect_scope.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.rt_occluded_scope.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_sky_color_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_set_counting.argtypes = [C.c_void_p, C.c_int]
        L.rt_build_bvh.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_build_bvh_split.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_build_tlas.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_get_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rt_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.rt_get_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rt_render_aovs.argtypes = [C.c_void_p, C.c_float]
        L.rt_download_aovs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_denoise.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rt_download_denoised.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_resolve_denoised.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_stats_enable.argtypes = [C.c_void_p, C.c_int]
        L.rt_download_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_select_active.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_set_active_pixels.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.rt_download_active.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rt_render_active.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_int]
        L.rt_resolve_adaptive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_denoise_variance.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_select_budget.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_download_budgets.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rt_render_budget.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
        L.rt_history_capture.argtypes = [C.c_void_p]
        L.rt_reproject.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_download_aov_positions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_reproject_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_download_aov_instances.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_reproject_deform.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_download_aov_prims.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_select_active_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.rt_select_budget_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_gather_stats_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.rt_gather_active.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_select_active_dilated.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.rt_select_budget_dilated.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_set_pixel_filter.argtypes = [C.c_void_p, C.c_int]
        L.rt_get_pixel_filter.argtypes = [C.c_void_p]
        L.rt_sample_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_set_lens.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_get_lens.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_focus_at.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.rt_set_shutter.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_get_shutter.argtypes = [C.c_void_p, C.c_void_p]
        L.rt_layout_build.restype = C.c_void_p
        L.rt_layout_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.rt_layout_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.rt_layout_free.argtypes = [C.c_void_p]
        L.rt_launch_form.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.rt_any_hit_walk.argtypes = [C.c_int, C.c_int, C.c_int]
        L.rt_set_instances.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_set_instance_list.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rt_download_tlas.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.rt_scene_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rt_set_triangles.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rt_blas_array.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rt_set_mesh_indices.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rt_set_vertices.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rt_set_vertices_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.rt_set_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rt_set_materials.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rt_set_sky.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        _rt = L
    return _rt


def host_lib():
    global _host
    if _host is None:
        rt_lib()
        if not os.path.exists(HOST_SO):
            raise RuntimeError("librapt_host.so is not built (run __graft_entry__.build())")
        L = C.CDLL(HOST_SO)
        for name in ["rth_scene_new", "rth_renderer_new", "rth_renderer_new_multi", "rth_renderer_scene", "rth_renderer_ctx", "rth_renderer_ctx_at", "rth_describe",
                     "rth_renderer_accumulator", "rth_renderer_pixels", "rth_get_sky"]:
            getattr(L, name).restype = C.c_void_p
        L.rth_last_error.restype = C.c_char_p
        L.rth_renderer_error.restype = C.c_char_p
        _host = L
    return _host


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class HostScene:
    """rapt::Scene through the rth_* C entry points.  Standalone (CPU only: loaders and builders) or
    the scene member of a HostRenderer."""

    def __init__(self, handle=None):
        self.L = host_lib()
        self.owned = handle is None
        self.h = C.c_void_p(self.L.rth_scene_new()) if handle is None else C.c_void_p(handle)

    def close(self):
        if self.h and self.owned:
            self.L.rth_scene_free(self.h)
        self.h = None

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.rth_last_error(self.h).decode())
        return rc

    # ---- builder protocol (see scenes.py) ----
    def diffuse(self, albedo, col, ks=0.2, kd=0.8, n=2, emission=0.0, shininess=0.0, rt=True):
        a = albedo if hasattr(albedo, "__len__") else (albedo,) * 3
        return self.L.rth_add_diffuse(self.h, _f3(a), _f3(col), C.c_float(ks), C.c_float(kd), int(n),
                                      C.c_float(emission), C.c_float(shininess), int(rt))

    def metal(self, fuzzy, col, rt=True):
        return self.L.rth_add_metal(self.h, C.c_float(fuzzy), _f3(col), int(rt))

    def glass(self, ir, col, absorption=(0, 0, 0), rt=True):
        return self.L.rth_add_glass(self.h, C.c_float(ir), _f3(col), _f3(absorption), int(rt))

    def area_light(self, idx, pos, strength, col, radius, normal):
        return self.L.rth_add_area_light(self.h, idx, _f3(pos), C.c_float(strength), _f3(col), C.c_float(radius), _f3(normal))

    def dir_light(self, idx, pos, strength, col, normal, r):
        return self.L.rth_add_dir_light(self.h, idx, _f3(pos), C.c_float(strength), _f3(col), _f3(normal), C.c_float(r))

    def sphere(self, idx, mat, pos, r):
        return self.L.rth_add_sphere(self.h, idx, mat, _f3(pos), C.c_float(r))

    def plane(self, idx, mat, N, d):
        return self.L.rth_add_plane(self.h, idx, mat, _f3(N), C.c_float(d))

    def mesh_raw(self, group, mat, v9):
        v9 = np.ascontiguousarray(v9, dtype=np.float32).reshape(-1, 9)
        return self.L.rth_add_mesh_raw(self.h, group, mat, _p(v9), len(v9))

    def mesh_obj(self, group, path, mat, pos, scale):
        return self._chk(self.L.rth_add_mesh_obj(self.h, group, path.encode(), mat, _f3(pos), C.c_float(scale)))

    def mesh_tri(self, group, path, mat):
        return self._chk(self.L.rth_add_mesh_tri(self.h, group, path.encode(), mat))

    def sky(self, pixels):
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        hgt, w, n = px.shape
        self.L.rth_set_sky(self.h, w, hgt, n, _p(px))

    def load_file(self, path):
        """Scene::LoadFile: build the scene a 'rapt-scene 1' description file names."""
        self._chk(self.L.rth_scene_load_file(self.h, path.encode()))

    def sky_hdr(self, path):
        """Scene's stbi_load(path, ..., 3) of a Radiance .hdr file; returns the 8-bit texels [H, W, 3]."""
        self._chk(self.L.rth_load_sky_hdr(self.h, path.encode()))
        dims = (C.c_int * 3)()
        p = self.L.rth_get_sky(self.h, dims)
        buf = C.cast(p, C.POINTER(C.c_ubyte))
        return np.ctypeslib.as_array(buf, shape=(dims[1], dims[0], dims[2])).copy()

    def trs(self, t, s, rx, ry, rz):
        out = np.zeros(16, dtype=np.float32)
        self.L.rth_mat4_trs(_f3(t), C.c_float(s), C.c_float(rx), C.c_float(ry), C.c_float(rz), _p(out))
        return out

    def device_build(self, ctx):
        """Build BINNEDSAH trees with rt_build_bvh on the device of 'ctx' (None: on the host again)."""
        self.L.rth_scene_device_build(self.h, ctx)

    def build(self, split=0):
        self._chk(self.L.rth_build(self.h, split))

    def build_tlas(self, split, instances):
        idx = np.array([i for i, _ in instances], dtype=np.int32)
        T = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float32).reshape(16) for _, t in instances]))
        self._chk(self.L.rth_build_tlas(self.h, split, len(idx), _p(idx), _p(T)))

    def set_raytracer(self, rt):
        self.L.rth_set_raytracer(self.h, int(rt))

    def raytracer(self):
        return bool(self.L.rth_get_raytracer(self.h))

    def set_time(self, t):
        """Scene::SetTime (animation + refit on the device); needs a committed scene."""
        self._chk(self.L.rth_scene_set_time(self.h, C.c_float(t)))

    def set_transforms(self, first, transforms):
        """bvhInstance::SetTransform for instances first, first + 1, ... (row-major mat4 each); commit_instances() sends them to the device"""
        T = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float32).reshape(16) for t in transforms]))
        self._chk(self.L.rth_scene_set_transforms(self.h, int(first), len(T), _p(T)))

    def commit_instances(self):
        """Scene::CommitInstances: every instance's matrices and (accumulating) bounds through rt_set_instances, to every committed context;
        the scene's tlas is then the tree the device walks.  Needs a committed scene."""
        self._chk(self.L.rth_scene_commit_instances(self.h))

    def set_instance_list(self, instances):
        """Scene::SetInstanceList: the instance array and the tlas replaced by fresh instances, (mesh index, row-major mat4) each as
        build_tlas takes them; every mesh named must have been part of build_tlas.  commit_instance_list() sends the list to the device"""
        idx = np.array([i for i, _ in instances], dtype=np.int32)
        T = np.ascontiguousarray(np.stack([np.asarray(t, dtype=np.float32).reshape(16) for _, t in instances]))
        self._chk(self.L.rth_scene_set_instance_list(self.h, len(idx), _p(idx), _p(T)))

    def commit_instance_list(self):
        """Scene::CommitInstanceList: the whole (replaced) instance list with the instances' own bounds through rt_set_instance_list, to
        every committed context; the scene's tlas is then the tree the device walks.  Needs a committed scene."""
        self._chk(self.L.rth_scene_commit_instance_list(self.h))

    def set_mesh_vertices(self, mesh, v9):
        """the triangles of mesh 'mesh' rewritten from (n, 9) vertices (n: its triangle count), as mesh_raw makes them; objIdx and material
        stay.  commit_triangles() sends them to the device"""
        v9 = np.ascontiguousarray(v9, dtype=np.float32).reshape(-1, 9)
        self._chk(self.L.rth_mesh_set_vertices(self.h, int(mesh), _p(v9), len(v9)))

    def refit(self, blas=-1):
        """bvh::Refit of BLAS 'blas' (-1: the scene BVH) on the host alone: bvh_dump() then shows the refitted boxes"""
        self._chk(self.L.rth_bvh_refit(self.h, int(blas)))

    def commit_triangles(self, blas=-1):
        """Scene::CommitTriangles of BLAS 'blas' (describe()'s order; -1: the scene BVH of a scene without a TLAS): the host bvh::Refit,
        rt_set_triangles to every committed context, the BLAS's instances under the box of a fresh instance, the scene's tlas refreshed
        from the device.  Needs a committed scene."""
        self._chk(self.L.rth_scene_commit_triangles(self.h, int(blas)))

    def mesh_indexed(self, mesh):
        """Mesh::vertices as (n_vertices, 3) float32 and Mesh::faces as (n_tri, 3) int32, 1-based as the reference keeps them"""
        nv = self.L.rth_mesh_vertex_count(self.h, int(mesh))
        if nv < 0:
            raise IndexError("mesh %d of %d" % (mesh, self.n_meshes()))
        xyz = np.zeros((nv, 3), dtype=np.float32)
        faces = np.zeros((self.L.rth_mesh_indexed(self.h, int(mesh), None, None), 3), dtype=np.int32)
        self._chk(self.L.rth_mesh_indexed(self.h, int(mesh), _p(xyz), _p(faces)))
        return xyz, faces

    def set_mesh_vertex_array(self, mesh, xyz):
        """Mesh::vertices of mesh 'mesh' replaced by (n_vertices, 3) floats (the same count); the faces stay.  commit_vertices() runs
        Mesh::update (the triangles follow) and sends the array to the device; mesh_update() runs Mesh::update alone"""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self._chk(self.L.rth_mesh_set_vertex_array(self.h, int(mesh), _p(xyz), len(xyz)))

    def mesh_update(self, mesh):
        """Mesh::update on the host alone: mesh_tris() then shows the triangles re-derived from vertices and faces"""
        self._chk(self.L.rth_mesh_update(self.h, int(mesh)))

    def commit_vertices(self, blas):
        """Scene::CommitVertices of BLAS 'blas' (describe()'s order), a BLAS over one mesh with faces: Mesh::update, the host bvh::Refit,
        the faces bound on the first call (rt_set_mesh_indices), rt_set_vertices with Mesh::vertices to every committed context, the
        instances and the scene's tlas refreshed as commit_triangles does.  Needs a committed scene."""
        self._chk(self.L.rth_scene_commit_vertices(self.h, int(blas)))

    # ---- relighting: the host half (Scene::ReplaceMaterial, the lights, the skydome) and Scene::CommitLights / CommitMaterials / CommitSky ----
    def replace_diffuse(self, index, albedo, col, ks=0.2, kd=0.8, n=2, emission=0.0, shininess=0.0, rt=True):
        """Scene::ReplaceMaterial(index, a new diffuse): diffuse()'s arguments; every primitive that named the old material names the new one"""
        a = albedo if hasattr(albedo, "__len__") else (albedo,) * 3
        self._chk(self.L.rth_replace_diffuse(self.h, int(index), _f3(a), _f3(col), C.c_float(ks), C.c_float(kd), int(n),
                                             C.c_float(emission), C.c_float(shininess), int(rt)))

    def replace_metal(self, index, fuzzy, col, rt=True):
        """Scene::ReplaceMaterial(index, a new metal): metal()'s arguments"""
        self._chk(self.L.rth_replace_metal(self.h, int(index), C.c_float(fuzzy), _f3(col), int(rt)))

    def replace_glass(self, index, ir, col, absorption=(0, 0, 0), rt=True):
        """Scene::ReplaceMaterial(index, a new glass): glass()'s arguments"""
        self._chk(self.L.rth_replace_glass(self.h, int(index), C.c_float(ir), _f3(col), _f3(absorption), int(rt)))

    def clear_lights(self):
        """every light removed; area_light() / dir_light() then make the new table, commit_lights() sends it"""
        self.L.rth_clear_lights(self.h)

    def clear_sky(self):
        """no skydome (misses are black); commit_sky() sends that on"""
        self.L.rth_clear_sky(self.h)

    def commit_lights(self):
        """Scene::CommitLights: the whole light table through rt_set_lights, to every committed context.  Needs a committed scene."""
        self._chk(self.L.rth_scene_commit_look(self.h, 0))

    def commit_materials(self):
        """Scene::CommitMaterials: every material of the committed scene, re-derived from its object, through rt_set_materials"""
        self._chk(self.L.rth_scene_commit_look(self.h, 1))

    def commit_sky(self):
        """Scene::CommitSky: the skydome (sky() / clear_sky()) through rt_set_sky"""
        self._chk(self.L.rth_scene_commit_look(self.h, 2))

    def rebuild_tlas(self):
        """tlas::build on the host over the instances' current bounds"""
        self._chk(self.L.rth_scene_rebuild_tlas(self.h))

    # ---- dumps ----
    def n_meshes(self):
        return int(self.L.rth_meshes(self.h))

    def mesh_tris(self, mesh):
        n = self.L.rth_mesh_count(self.h, mesh)
        if n < 0:
            raise IndexError("mesh %d of %d" % (mesh, self.n_meshes()))
        out = np.zeros((n, 15), dtype=np.float32)
        ids = np.zeros(n, dtype=np.int32)
        self.L.rth_mesh_get(self.h, mesh, _p(out), _p(ids))
        return out, ids

    def bvh_dump_info(self, blas=-1):
        """sizes of a tree without copying it: nodes_used, N (primitives), NTri, NSph, NPla, max_depth"""
        info = (C.c_int * 7)()
        self.L.rth_bvh_info(self.h, blas, info)
        return dict(nodes_used=info[0], N=info[1], NTri=info[2], NSph=info[3], NPla=info[4], max_depth=info[5])

    def bvh_dump(self, blas=-1):
        info = (C.c_int * 7)()
        self.L.rth_bvh_info(self.h, blas, info)
        nodes = np.zeros((info[0], 8), dtype=np.uint32)
        prim = np.zeros(info[1], dtype=np.uint32)
        self.L.rth_bvh_get(self.h, blas, _p(nodes), _p(prim))
        return dict(nodes=nodes, prim_idx=prim, nodes_used=info[0], N=info[1], NTri=info[2], NSph=info[3],
                    NPla=info[4], max_depth=info[5])

    def blas_count(self):
        return self.L.rth_blas_count(self.h)

    def tlas_dump(self):
        n = self.L.rth_tlas_nodes_used(self.h)
        nodes = np.zeros((n, 8), dtype=np.uint32)
        self.L.rth_tlas_get(self.h, _p(nodes))
        return nodes

    def instance_dump(self, i):
        blas = C.c_int()
        T = np.zeros(16, dtype=np.float32)
        iT = np.zeros(16, dtype=np.float32)
        b = np.zeros(6, dtype=np.float32)
        self.L.rth_instance_get(self.h, i, C.byref(blas), _p(T), _p(iT), _p(b))
        return dict(blas=blas.value, T=T, invT=iT, bounds=b)

    def describe(self):
        """Pointer to the rt_scene_desc this scene flattens to (valid until the scene changes)."""
        p = self.L.rth_describe(self.h)
        if not p:
            raise RuntimeError(self.L.rth_last_error(self.h).decode())
        return C.c_void_p(p)

    # single-ray forms with the reference's call shape (one device round trip each)
    def find_nearest_one(self, O, D, tmax=1e34, t_min=1e-6):
        t, obj = C.c_float(), C.c_int()
        n = (C.c_float * 3)()
        self._chk(self.L.rth_scene_find_nearest(self.h, _f3(O), _f3(D), C.c_float(tmax), C.c_float(t_min), C.byref(t), C.byref(obj), n))
        return t.value, obj.value, np.array(list(n), dtype=np.float32)

    def member_intersect(self, which, index, O, D, tmax=1e34):
        """bvh::Intersect (which 0), tlas::Intersect (1), bvhInstance::BIntersect (2) on one ray: (t, objIdx, normal)"""
        t, obj = C.c_float(), C.c_int()
        n = (C.c_float * 3)()
        self._chk(self.L.rth_member_intersect(self.h, which, index, _f3(O), _f3(D), C.c_float(tmax), C.byref(t), C.byref(obj), n))
        return t.value, obj.value, np.array(list(n), dtype=np.float32)

    def member_occluded(self, which, index, O, D, tmax=1e34):
        return bool(self._chk(self.L.rth_member_occluded(self.h, which, index, _f3(O), _f3(D), C.c_float(tmax))))

    def sky_color_one(self, D):
        rgb = (C.c_float * 3)()
        self._chk(self.L.rth_scene_sky_color(self.h, _f3(D), rgb))
        return np.array(list(rgb), dtype=np.float32)

    def is_occluded_one(self, O, D, tmax=1e34):
        return bool(self._chk(self.L.rth_scene_is_occluded(self.h, _f3(O), _f3(D), C.c_float(tmax))))


class HostRenderer:
    """rapt::Renderer (Init / Tick / Trace / Sample) plus direct access to its device context through
    the C ABI of include/rt_amd.h."""

    def __init__(self, width, height, device=0, devices=None):
        """devices: list of HIP devices for rapt::Renderer::UseDevices (one context each; Tick shards the rows over
        them and gathers into context 0).  A device may repeat: [0, 0] runs the multi-context path on one GPU."""
        self.L = host_lib()
        self.rt = rt_lib()
        self.w, self.hgt = width, height
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            self.h = C.c_void_p(self.L.rth_renderer_new_multi(width, height, len(devices), arr))
        else:
            self.h = C.c_void_p(self.L.rth_renderer_new(width, height, device))
        self.scene = HostScene(self.L.rth_renderer_scene(self.h))
        self._chk(self.L.rth_renderer_init(self.h))
        self.ctx = C.c_void_p(self.L.rth_renderer_ctx(self.h))

    def close(self):
        if self.h:
            self.L.rth_renderer_free(self.h)
            self.h = None

    def _chk(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.rth_renderer_error(self.h).decode())
        return rc

    def _rt(self, rc):
        if rc != 0:
            raise RuntimeError("rt_amd error %d: %s" % (rc, self.rt.rt_last_error(self.ctx).decode()))

    def commit(self):
        """Scene::Commit: flatten + rt_upload_scene."""
        self._chk(self.L.rth_renderer_commit(self.h))

    def set_camera(self, cam_pos, top_left, top_right, bottom_left, fisheye=False, view_angle=0.25, y_angle=0.0):
        self.L.rth_renderer_set_camera(self.h, _f3(cam_pos), _f3(top_left), _f3(top_right), _f3(bottom_left),
                                       int(fisheye), C.c_float(view_angle), C.c_float(y_angle))
        self._chk(self.L.rth_renderer_sync_camera(self.h))

    def camera(self):
        out = np.zeros(12, dtype=np.float32)
        self.L.rth_renderer_get_camera(self.h, _p(out))
        return out.reshape(4, 3)

    # ---- Renderer surface ----
    def tick(self):
        self._chk(self.L.rth_renderer_tick(self.h))

    def tick_qlearning(self, grid, lo=(0, 0, 0), hi=(1, 1, 1), alpha=0.3, epsilon=0.2, q_init=1.0):
        """rapt::Renderer::EnableQLearning (grid > 0) / DisableQLearning: Tick then learns between path frames, on every context"""
        self._qgrid = grid
        self._chk(self.L.rth_renderer_qlearning(self.h, grid, _f3(lo), _f3(hi), C.c_float(alpha), C.c_float(epsilon), C.c_float(q_init)))

    def iteration(self):
        """Scene::GetIterationNumber()"""
        return int(self.L.rth_renderer_iteration(self.h))

    def tick_accumulator(self):
        p = C.cast(self.L.rth_renderer_accumulator(self.h), C.POINTER(C.c_float))
        return np.ctypeslib.as_array(p, shape=(self.hgt, self.w, 4)).copy()

    def tick_pixels(self):
        p = C.cast(self.L.rth_renderer_pixels(self.h), C.POINTER(C.c_uint32))
        return np.ctypeslib.as_array(p, shape=(self.hgt, self.w)).copy()

    def set_pixel_filter(self, kind):
        """rapt::Renderer::pixelFilter (RT_FILTER_*), sent to every context at once: the sub-pixel camera samples of path mode"""
        self._chk(self.L.rth_renderer_set_pixel_filter(self.h, int(kind)))

    def pixel_filter(self):
        """rt_get_pixel_filter of context 0"""
        return int(self.rt.rt_get_pixel_filter(self.ctx))

    def set_lens(self, radius, focus_distance=1.0):
        """rapt::Renderer::lensRadius / focusDistance, sent to every context at once: the thin lens of the path-mode camera samples (radius 0: off)"""
        self._chk(self.L.rth_renderer_set_lens(self.h, C.c_float(radius), C.c_float(focus_distance)))

    def lens(self):
        """rt_get_lens of context 0: (radius, focus_distance)"""
        l = RtLens()
        self._rt(self.rt.rt_get_lens(self.ctx, C.byref(l)))
        return float(l.radius), float(l.focus_distance)

    def focus_at(self, x, y):
        """rapt::Renderer::FocusAt: the focus distance (np.float32) that puts what pixel (x, y) sees in focus, 0 for the sky; sets nothing"""
        d = C.c_float(0.0)
        self._chk(self.L.rth_renderer_focus_at(self.h, int(x), int(y), C.byref(d)))
        return np.float32(d.value)

    def set_shutter(self, cam_pos, top_left, top_right, bottom_left):
        """rapt::Renderer::shutter / shutterCamera, sent to every context at once: the camera at shutter close of the path-mode camera
        samples (the renderer's camera is the one at shutter open)"""
        rec = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32).reshape(3) for v in (cam_pos, top_left, top_right, bottom_left)]))
        self._chk(self.L.rth_renderer_set_shutter(self.h, _p(rec)))

    def clear_shutter(self):
        """rapt::Renderer::shutter = false on every context: the samples of a batch are taken at one instant again"""
        self._chk(self.L.rth_renderer_set_shutter(self.h, None))

    def shutter(self):
        """rt_get_shutter of context 0: the closing camera (4, 3) float32 -- cam_pos, top_left, top_right, bottom_left -- or None (off)"""
        c = RtCamera()
        rc = int(self.rt.rt_get_shutter(self.ctx, C.byref(c)))
        if rc < 0:
            self._rt(rc)
        if rc == 0:
            return None
        return np.float32([list(c.cam_pos), list(c.top_left), list(c.top_right), list(c.bottom_left)])

    def sample_rays(self, frame, seed_base=0x12345678, y0=0, y1=None):
        """rt_sample_rays: the camera rays (O, D), each (rows * width, 3), of frame 'frame' of the path samples under the context's filter"""
        y1 = self.hgt if y1 is None else y1
        O = np.zeros(((y1 - y0) * self.w, 3), dtype=np.float32)
        D = np.zeros(((y1 - y0) * self.w, 3), dtype=np.float32)
        self._rt(self.rt.rt_sample_rays(self.ctx, C.c_uint32(frame & 0xFFFFFFFF), C.c_uint32(seed_base & 0xFFFFFFFF), y0, y1, _p(O), _p(D)))
        return O, D

    def set_denoise(self, on, params=None):
        """rapt::Renderer::denoise / denoiseParams: Tick shows the denoised mean in path mode (params: dict, see denoise_params)"""
        p = denoise_params(params)
        self.L.rth_renderer_set_denoise(self.h, int(bool(on)), C.byref(p) if p is not None else None)

    def set_denoise_variance(self, on, params=None):
        """rapt::Renderer::denoiseVariance / denoiseVarParams: adaptive Ticks show the variance-guided denoised frame (params: dict, see denoise_var_params)"""
        p = denoise_var_params(params)
        self.L.rth_renderer_set_denoise_variance(self.h, int(bool(on)), C.byref(p) if p is not None else None)

    def set_adaptive(self, on, params=None):
        """rapt::Renderer::adaptive / adaptiveParams: path-mode Ticks sample only the pixels that are still noisy (params: dict, see adaptive_params)"""
        p = adaptive_params(params)
        self.L.rth_renderer_set_adaptive(self.h, int(bool(on)), C.byref(p) if p is not None else None)

    def set_adaptive_budget(self, pass_cap, max_pass_samples=0):
        """rapt::Renderer::adaptivePassCap / adaptiveMaxPassSamples: adaptive Ticks are budgeted passes (pass_cap 0: one frame per Tick, as ever)"""
        self.L.rth_renderer_set_adaptive_budget(self.h, int(pass_cap), C.c_uint32(int(max_pass_samples)))

    def set_adaptive_dilate(self, radius):
        """rapt::Renderer::adaptiveDilate: the adaptive Ticks' selections also list the pixels within 'radius' of an active one (0: as ever)"""
        self.L.rth_renderer_set_adaptive_dilate(self.h, int(radius))

    def pass_samples(self):
        """rapt::Renderer::passSamples: the samples the last adaptive Tick took"""
        return int(self.L.rth_renderer_pass_samples(self.h))

    def set_reproject(self, on, params=None):
        """rapt::Renderer::reproject / reprojectParams: an adaptive Tick answers a camera move by carrying the samples (params: dict, see reproject_params)"""
        p = reproject_params(params)
        self.L.rth_renderer_set_reproject(self.h, int(bool(on)), C.byref(p) if p is not None else None)

    def commit_instances(self):
        """rapt::Renderer::CommitInstances: the scene's instance transforms (scene.set_transforms) sent on; with reproject and adaptive set
        the next adaptive Tick carries the samples across the move (rt_reproject_motion), otherwise it clears"""
        self._chk(self.L.rth_renderer_commit_instances(self.h))

    def commit_instance_list(self):
        """rapt::Renderer::CommitInstanceList: the scene's replaced instance list (scene.set_instance_list) sent on, and the next Tick
        clears (there is no carry across a list edit: an instance index names another object afterwards)"""
        self._chk(self.L.rth_renderer_commit_instance_list(self.h))

    def commit_triangles(self, blas=-1):
        """rapt::Renderer::CommitTriangles of BLAS 'blas' (scene.commit_triangles' numbering; -1: the scene BVH): the mesh's rewritten
        triangles (scene.set_mesh_vertices) sent on; with reproject and adaptive set the next adaptive Tick carries the samples across
        the deformation (rt_reproject_deform), otherwise it clears"""
        self._chk(self.L.rth_renderer_commit_triangles(self.h, int(blas)))

    def commit_vertices(self, blas):
        """rapt::Renderer::CommitVertices of BLAS 'blas': scene.commit_vertices under commit_triangles' carry logic"""
        self._chk(self.L.rth_renderer_commit_vertices(self.h, int(blas)))

    def commit_lights(self):
        """rapt::Renderer::CommitLights: scene.commit_lights, and the next Tick clears (there is no carry across a relight)"""
        self._chk(self.L.rth_renderer_commit_look(self.h, 0))

    def commit_materials(self):
        """rapt::Renderer::CommitMaterials: scene.commit_materials, and the next Tick clears"""
        self._chk(self.L.rth_renderer_commit_look(self.h, 1))

    def commit_sky(self):
        """rapt::Renderer::CommitSky: scene.commit_sky, and the next Tick clears"""
        self._chk(self.L.rth_renderer_commit_look(self.h, 2))

    def carried_pixels(self):
        """rapt::Renderer::carriedPixels: the pixels the last reprojecting Tick carried"""
        return int(self.L.rth_renderer_carried_pixels(self.h))

    def active_pixels(self):
        """rapt::Renderer::activePixels: the pixels the last adaptive Tick sampled"""
        return int(self.L.rth_renderer_active_pixels(self.h))

    def trace_one(self, O, D, depth, path=False, energy=(1, 1, 1)):
        rgb = (C.c_float * 3)()
        self._chk(self.L.rth_renderer_trace(self.h, int(path), _f3(O), _f3(D), depth, _f3(energy), rgb))
        return np.array(list(rgb), dtype=np.float32)

    # ---- C ABI, direct ----
    def render(self, mode, frame0=0, nframes=1, seed_base=0x12345678, y0=0, y1=None, max_depth=4):
        self._rt(self.rt.rt_render(self.ctx, mode, frame0, nframes, seed_base, y0, self.hgt if y1 is None else y1, max_depth))

    def render_rows(self, mode, frame0, nframes, row_first, row_stride, row_count, seed_base=0x12345678, max_depth=4):
        self._rt(self.rt.rt_render_rows(self.ctx, mode, frame0, nframes, seed_base, row_first, row_stride, row_count, max_depth))

    def set_time(self, t):
        """Scene::SetTime with animation on: deform + refit on the GPU."""
        self._rt(self.rt.rt_set_time(self.ctx, t))

    def clear(self):
        self._rt(self.rt.rt_clear(self.ctx))

    def synchronize(self):
        self._rt(self.rt.rt_synchronize(self.ctx))

    def _rows(self, y0, y1, dtype, *tail):
        """rows [y0, y1) (y1 None: to the last row): (y1, a zeroed array of those rows, shaped (rows, width) + tail)"""
        y1 = self.hgt if y1 is None else y1
        return y1, np.zeros((y1 - y0, self.w) + tail, dtype=dtype)

    def accumulator(self, y0=0, y1=None):
        y1, out = self._rows(y0, y1, np.float32, 4)
        self._rt(self.rt.rt_download_accumulator(self.ctx, y0, y1, _p(out)))
        return out

    def resolve(self, it=1, y0=0, y1=None):
        y1, out = self._rows(y0, y1, np.uint32)
        self._rt(self.rt.rt_resolve(self.ctx, it, y0, y1, _p(out)))
        return out

    def accumulator_device_ptr(self):
        return self.rt.rt_accumulator_device_ptr(self.ctx)

    def bind_accumulator(self, device_ptr):
        self._rt(self.rt.rt_bind_accumulator(self.ctx, C.c_void_p(device_ptr)))

    def find_nearest(self, O, D, tmax=None, t_min=1e-6):
        O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(O), dtype=RT_HIT_DTYPE)
        tm = None if tmax is None else _p(np.ascontiguousarray(tmax, dtype=np.float32))
        self._rt(self.rt.rt_intersect_batch(self.ctx, len(O), _p(O), _p(D), tm, t_min, _p(out)))
        return dict(t=out["t"].copy(), obj=out["obj_idx"].copy(), mat=out["material"].copy(), normal=out["normal"].copy())

    def is_occluded(self, O, D, tmax=None):
        O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(O), dtype=np.uint8)
        tm = None if tmax is None else _p(np.ascontiguousarray(tmax, dtype=np.float32))
        self._rt(self.rt.rt_occluded_batch(self.ctx, len(O), _p(O), _p(D), tm, _p(out)))
        return out

    def build_tlas(self, bounds6):
        """rt_build_tlas: tlas::build on the device; bounds6 (n, 6) instance world boxes.  Returns the nodes as (k, 8) uint32."""
        b = np.ascontiguousarray(bounds6, dtype=np.float32).reshape(-1, 6)
        nodes = np.zeros((2 * len(b) + 1, 8), dtype=np.uint32)
        used = C.c_uint32(0)
        self._rt(self.rt.rt_build_tlas(self.ctx, _p(b), len(b), _p(nodes), C.byref(used)))
        return nodes[:used.value].copy()

    def build_bvh(self, tri_v9=None, spheres=None, planes=None, split=0):
        """rt_build_bvh_split: the reference's bvh::Build on the device (split: bvh.h:38-43, 0 = binned SAH).  tri_v9: (n, 9) vertices,
        spheres: (n, 4) pos + r, planes: (n, 4) N + d.  Returns (nodes[:nodes_used] as an (n, 8) uint32 view
        like the oracle's dump, prim_idx)."""
        tv = np.zeros((0, 9), np.float32) if tri_v9 is None else np.ascontiguousarray(tri_v9, dtype=np.float32).reshape(-1, 9)
        sp = np.zeros((0, 4), np.float32) if spheres is None else np.ascontiguousarray(spheres, dtype=np.float32).reshape(-1, 4)
        pl = np.zeros((0, 4), np.float32) if planes is None else np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 4)
        T = np.zeros(len(tv), dtype=RT_TRIANGLE_DTYPE)
        T["v0"], T["v1"], T["v2"] = tv[:, 0:3], tv[:, 3:6], tv[:, 6:9]
        S = np.zeros(len(sp), dtype=RT_SPHERE_DTYPE)
        S["pos"], S["r"] = sp[:, :3], sp[:, 3]
        P = np.zeros(len(pl), dtype=RT_PLANE_DTYPE)
        P["N"], P["d"] = pl[:, :3], pl[:, 3]
        n = len(T) + len(S) + len(P)
        nodes = np.zeros(2 * (n + 1), dtype=RT_BVH_NODE_DTYPE)
        prim = np.zeros(max(n, 1), dtype=np.uint32)
        used = C.c_uint32(0)
        self._rt(self.rt.rt_build_bvh_split(self.ctx, int(split), _p(T) if len(T) else None, len(T), _p(S) if len(S) else None, len(S),
                                      _p(P) if len(P) else None, len(P), _p(nodes), _p(prim), C.byref(used)))
        return nodes[:used.value].view(np.uint32).reshape(-1, 8).copy(), prim[:n].copy()

    # ---- moving instances (include/rt_amd.h rt_set_instances, rt_download_tlas, rt_scene_array) ----
    def set_instances(self, first, instances, bounds6=None):
        """rt_set_instances: instances is an RT_INSTANCE_DTYPE array (blas, transform, inv_transform) for instances first, first + 1, ...;
        bounds6 (count, 6) their world boxes, or None: the device computes the box of a fresh instance.  Returns the rt_status (0: done)."""
        ins = np.ascontiguousarray(instances, dtype=RT_INSTANCE_DTYPE).reshape(-1)
        b = None if bounds6 is None else np.ascontiguousarray(bounds6, dtype=np.float32).reshape(-1, 6)
        assert b is None or len(b) == len(ins)
        return int(self.rt.rt_set_instances(self.ctx, int(first), len(ins), _p(ins) if len(ins) else None, None if b is None else _p(b)))

    def set_instance_list(self, instances, bounds6=None):
        """rt_set_instance_list: the whole instance list replaced by 'instances', an RT_INSTANCE_DTYPE array of 1..256 records whose blas
        may be any uploaded BLAS; bounds6 (n, 6) their world boxes, or None: the device computes the box of a fresh instance for each.
        Returns the rt_status (0: done)."""
        ins = np.ascontiguousarray(instances, dtype=RT_INSTANCE_DTYPE).reshape(-1)
        b = None if bounds6 is None else np.ascontiguousarray(bounds6, dtype=np.float32).reshape(-1, 6)
        assert b is None or len(b) == len(ins)
        return int(self.rt.rt_set_instance_list(self.ctx, len(ins), _p(ins) if len(ins) else None, None if b is None else _p(b)))

    def download_tlas(self):
        """rt_download_tlas: the TLAS the context walks, as (nodes_used, 8) uint32 like build_tlas"""
        n = self.scene_array("scalars")[3]
        nodes = np.zeros((2 * int(n) + 1, 8), dtype=np.uint32)
        used = C.c_uint32(0)
        self._rt(self.rt.rt_download_tlas(self.ctx, _p(nodes), C.byref(used)))
        return nodes[:used.value].copy()

    # ---- deforming meshes (include/rt_amd.h rt_set_triangles, rt_blas_array, rt_set_mesh_indices, rt_set_vertices, rt_set_vertices_device) ----
    def set_triangles(self, blas, tris, ctx=None):
        """rt_set_triangles: tris is an RT_TRIANGLE_DTYPE array holding ALL triangles of BLAS 'blas' (v0, v1, v2, N, obj_idx, material).
        Returns the rt_status (0: done)."""
        t = np.ascontiguousarray(tris, dtype=RT_TRIANGLE_DTYPE).reshape(-1)
        return int(self.rt.rt_set_triangles(self.ctx if ctx is None else ctx, int(blas), _p(t) if len(t) else None, len(t)))

    def set_mesh_indices(self, blas, idx, n_vertices, ctx=None):
        """rt_set_mesh_indices: idx is an (n_tri, 3) array of 0-based vertex indices of BLAS 'blas' (None: unbind).  Returns the rt_status."""
        ctx = self.ctx if ctx is None else ctx
        if idx is None:
            return int(self.rt.rt_set_mesh_indices(ctx, int(blas), None, 0, 0))
        i = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1, 3)
        return int(self.rt.rt_set_mesh_indices(ctx, int(blas), _p(i) if len(i) else None, len(i), int(n_vertices)))

    def set_vertices(self, blas, xyz, ctx=None):
        """rt_set_vertices: xyz is the (n_vertices, 3) float32 vertex array of BLAS 'blas', whose indices are bound.  Returns the rt_status."""
        v = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        return int(self.rt.rt_set_vertices(self.ctx if ctx is None else ctx, int(blas), _p(v) if len(v) else None, len(v)))

    def set_vertices_device(self, blas, ptr, n_vertices, ctx=None):
        """rt_set_vertices_device: ptr is the address of n_vertices * 3 floats in device memory of the context's device (a torch tensor's
        data_ptr(), as with bind_accumulator); the work that produced them must be done (torch.cuda.synchronize).  Returns the rt_status."""
        return int(self.rt.rt_set_vertices_device(self.ctx if ctx is None else ctx, int(blas), C.c_void_p(ptr), int(n_vertices)))

    # ---- relighting (include/rt_amd.h rt_set_lights, rt_set_materials, rt_set_sky) ----
    def set_lights(self, lights, ctx=None):
        """rt_set_lights: lights is an RT_LIGHT_DTYPE array, the WHOLE new table (empty: no lights).  Returns the rt_status (0: done)."""
        l = np.ascontiguousarray(lights, dtype=RT_LIGHT_DTYPE).reshape(-1)
        return int(self.rt.rt_set_lights(self.ctx if ctx is None else ctx, _p(l) if len(l) else None, len(l)))

    def set_materials(self, first, materials, ctx=None):
        """rt_set_materials: materials is an RT_MATERIAL_DTYPE array replacing materials first, first + 1, ...  Returns the rt_status."""
        m = np.ascontiguousarray(materials, dtype=RT_MATERIAL_DTYPE).reshape(-1)
        return int(self.rt.rt_set_materials(self.ctx if ctx is None else ctx, int(first), len(m), _p(m) if len(m) else None))

    def set_sky(self, pixels, ctx=None):
        """rt_set_sky: pixels is an (h, w, n) uint8 array, or None: no sky.  Returns the rt_status."""
        ctx = self.ctx if ctx is None else ctx
        if pixels is None:
            return int(self.rt.rt_set_sky(ctx, None, 0, 0, 0))
        px = np.ascontiguousarray(pixels, dtype=np.uint8)
        hgt, w, n = px.shape
        return int(self.rt.rt_set_sky(ctx, _p(px), w, hgt, n))

    def blas_array(self, blas, name, ctx=None):
        """rt_blas_array: 'pairs' or 'prims' of BLAS 'blas' as the context (ctx None: context 0) holds them: the BLAS's slice of layout()'s"""
        ctx = self.ctx if ctx is None else ctx
        which = [k for k, _ in LAYOUT_ARRAYS].index(name)
        nbytes = C.c_size_t(0)
        if self.rt.rt_blas_array(ctx, int(blas), which, None, 0, C.byref(nbytes)) != 0:
            raise RuntimeError("rt_blas_array: %s" % self.rt.rt_last_error(ctx).decode())
        out = np.zeros(nbytes.value // 4, dtype=dict(LAYOUT_ARRAYS)[name])
        if nbytes.value and self.rt.rt_blas_array(ctx, int(blas), which, _p(out), nbytes.value, C.byref(nbytes)) != 0:
            raise RuntimeError("rt_blas_array: %s" % self.rt.rt_last_error(ctx).decode())
        return out

    def ctx_at(self, k):
        """context k of a renderer made with devices=[...] (context 0 is .ctx)"""
        return C.c_void_p(self.L.rth_renderer_ctx_at(self.h, int(k)))

    def scene_array(self, name, ctx=None):
        """rt_scene_array: 'pairs', 'reach', 'brute', 'inst', 'lights', 'mats' or 'scalars' as the context (ctx None: context 0) holds them, in layout()'s formats"""
        ctx = self.ctx if ctx is None else ctx
        which = [k for k, _ in LAYOUT_ARRAYS].index(name)
        nbytes = C.c_size_t(0)
        if self.rt.rt_scene_array(ctx, which, None, 0, C.byref(nbytes)) != 0:
            raise RuntimeError("rt_scene_array: %s" % self.rt.rt_last_error(ctx).decode())
        out = np.zeros(nbytes.value // 4, dtype=dict(LAYOUT_ARRAYS)[name])
        if nbytes.value and self.rt.rt_scene_array(ctx, which, _p(out), nbytes.value, C.byref(nbytes)) != 0:
            raise RuntimeError("rt_scene_array: %s" % self.rt.rt_last_error(ctx).decode())
        return out

    def upload_desc(self, desc):
        """rt_upload_scene of a caller's rt_scene_desc (a ctypes pointer, e.g. another scene's describe()) into context 0"""
        self._rt(self.rt.rt_upload_scene(self.ctx, desc))

    def primary_hits(self, t_min=1e-6):
        obj = np.zeros((self.hgt, self.w), dtype=np.int32)
        t = np.zeros((self.hgt, self.w), dtype=np.float32)
        self._rt(self.rt.rt_primary_hits(self.ctx, t_min, _p(obj), _p(t)))
        return obj, t

    # ---- G-buffer and denoiser (include/rt_amd.h rt_render_aovs .. rt_resolve_denoised) ----
    def render_aovs(self, t_min=0.001):
        self._rt(self.rt.rt_render_aovs(self.ctx, t_min))

    def aovs(self, y0=0, y1=None):
        """rows [y0, y1) of the G-buffer: dict(t, obj, mat, normal, albedo) like find_nearest plus the albedo, shaped (rows, width[, 3])"""
        y1, hits = self._rows(y0, y1, RT_HIT_DTYPE)
        alb = self._rows(y0, y1, np.float32, 3)[1]
        self._rt(self.rt.rt_download_aovs(self.ctx, y0, y1, _p(hits), _p(alb)))
        return dict(t=hits["t"].copy(), obj=hits["obj_idx"].copy(), mat=hits["material"].copy(), normal=hits["normal"].copy(), albedo=alb)

    def denoise(self, it, params=None):
        """rt_denoise of the accumulator / it (params: dict, see denoise_params; None: the library's defaults)"""
        p = denoise_params(params)
        self._rt(self.rt.rt_denoise(self.ctx, int(it), C.byref(p) if p is not None else None))

    def denoise_variance(self, params=None):
        """rt_denoise_variance of the adaptively sampled frame (params: dict, see denoise_var_params; None: the library's defaults)"""
        p = denoise_var_params(params)
        self._rt(self.rt.rt_denoise_variance(self.ctx, C.byref(p) if p is not None else None))

    def denoised(self, y0=0, y1=None):
        y1, out = self._rows(y0, y1, np.float32, 4)
        self._rt(self.rt.rt_download_denoised(self.ctx, y0, y1, _p(out)))
        return out

    def resolve_denoised(self, y0=0, y1=None):
        y1, out = self._rows(y0, y1, np.uint32)
        self._rt(self.rt.rt_resolve_denoised(self.ctx, y0, y1, _p(out)))
        return out

    # ---- adaptive sampling (include/rt_amd.h rt_stats_enable .. rt_resolve_adaptive) ----
    def stats_enable(self, on=True):
        self._rt(self.rt.rt_stats_enable(self.ctx, int(bool(on))))

    def stats(self, y0=0, y1=None):
        """rows [y0, y1) of the per-pixel statistics: (count uint32, sum_y float32, sum_yy float32), shaped (rows, width)"""
        y1, cnt = self._rows(y0, y1, np.uint32)
        sy, syy = self._rows(y0, y1, np.float32)[1], self._rows(y0, y1, np.float32)[1]
        self._rt(self.rt.rt_download_stats(self.ctx, y0, y1, _p(cnt), _p(sy), _p(syy)))
        return cnt, sy, syy

    def select_active(self, params=None):
        """rt_select_active (params: dict, see adaptive_params; None: the library's defaults): the number of pixels selected"""
        p = adaptive_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_select_active(self.ctx, C.byref(p) if p is not None else None, C.byref(n)))
        return n.value

    def set_active(self, pixels):
        """rt_set_active_pixels: pixel indices y * width + x, strictly ascending"""
        px = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        self._rt(self.rt.rt_set_active_pixels(self.ctx, _p(px) if len(px) else None, len(px)))

    def active(self, cap=None):
        """rt_download_active: (the first cap entries of the list, the list's true length); cap None: the whole frame's worth"""
        cap = self.w * self.hgt if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        n = C.c_int(-1)
        self._rt(self.rt.rt_download_active(self.ctx, _p(out), cap, C.byref(n)))
        return out[:min(cap, n.value)].copy(), n.value

    def render_active(self, frame0=0, nframes=1, seed_base=0x12345678, max_depth=4):
        self._rt(self.rt.rt_render_active(self.ctx, frame0, nframes, seed_base, max_depth))

    def resolve_adaptive(self, y0=0, y1=None):
        y1, out = self._rows(y0, y1, np.uint32)
        self._rt(self.rt.rt_resolve_adaptive(self.ctx, y0, y1, _p(out)))
        return out

    # ---- budgeted adaptive passes (include/rt_amd.h rt_select_budget .. rt_render_budget) ----
    def select_budget(self, params=None):
        """rt_select_budget (params: dict, see budget_params; None: the library's defaults): (pixels selected, samples of the pass, cap used)"""
        p = budget_params(params)
        n, total, cap = C.c_int(-1), C.c_uint32(0), C.c_int(-1)
        self._rt(self.rt.rt_select_budget(self.ctx, C.byref(p) if p is not None else None, C.byref(n), C.byref(total), C.byref(cap)))
        return n.value, total.value, cap.value

    def budgets(self, cap=None):
        """rt_download_budgets: (the first cap budgets in list order, the list's true length); cap None: the whole frame's worth"""
        cap = self.w * self.hgt if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        n = C.c_int(-1)
        self._rt(self.rt.rt_download_budgets(self.ctx, _p(out), cap, C.byref(n)))
        return out[:min(cap, n.value)].copy(), n.value

    def render_budget(self, frame_base=0, seed_base=0x12345678, max_depth=4):
        self._rt(self.rt.rt_render_budget(self.ctx, frame_base, seed_base, max_depth))

    # ---- adaptive sampling over several contexts (include/rt_amd.h rt_select_active_rows, rt_select_budget_rows, rt_gather_stats_rows, rt_gather_active)
    def select_active_rows(self, row_first, row_stride, row_count, params=None):
        """rt_select_active_rows: select_active over the pixels of rows row_first + k * row_stride, k < row_count, only"""
        p = adaptive_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_select_active_rows(self.ctx, C.byref(p) if p is not None else None, row_first, row_stride, row_count, C.byref(n)))
        return n.value

    def select_budget_rows(self, row_first, row_stride, row_count, params=None):
        """rt_select_budget_rows: select_budget over those rows only: (pixels selected, samples of the pass, cap used)"""
        p = budget_params(params)
        n, total, cap = C.c_int(-1), C.c_uint32(0), C.c_int(-1)
        self._rt(self.rt.rt_select_budget_rows(self.ctx, C.byref(p) if p is not None else None, row_first, row_stride, row_count,
                                               C.byref(n), C.byref(total), C.byref(cap)))
        return n.value, total.value, cap.value

    # ---- dilated adaptive selection (include/rt_amd.h rt_select_active_dilated, rt_select_budget_dilated) ----
    def select_active_dilated(self, radius, params=None):
        """rt_select_active_dilated: select_active plus the eligible pixels within 'radius' of an active one: the number of pixels listed"""
        p = adaptive_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_select_active_dilated(self.ctx, C.byref(p) if p is not None else None, int(radius), C.byref(n)))
        return n.value

    def select_budget_dilated(self, radius, params=None):
        """rt_select_budget_dilated: that list with select_budget's plan (1 sample where dilation alone lists): (pixels, samples, cap used)"""
        p = budget_params(params)
        n, total, cap = C.c_int(-1), C.c_uint32(0), C.c_int(-1)
        self._rt(self.rt.rt_select_budget_dilated(self.ctx, C.byref(p) if p is not None else None, int(radius), C.byref(n), C.byref(total), C.byref(cap)))
        return n.value, total.value, cap.value

    def _rt_src(self, src, rc):
        if rc != 0:  # the gathers report on the source context
            raise RuntimeError("rt_amd error %d: %s" % (rc, self.rt.rt_last_error(src.ctx).decode()))

    def gather_rows(self, src, row_first, row_stride, row_count):
        """rt_gather_rows: the accumulator rows row_first + k * row_stride, k < row_count, of HostRenderer 'src' into this renderer's context"""
        self._rt_src(src, self.rt.rt_gather_rows(self.ctx, src.ctx, row_first, row_stride, row_count))

    def gather_stats_rows(self, src, row_first, row_stride, row_count):
        """rt_gather_stats_rows: accumulator and statistics of those rows of HostRenderer 'src' into this renderer's context"""
        self._rt_src(src, self.rt.rt_gather_stats_rows(self.ctx, src.ctx, row_first, row_stride, row_count))

    def gather_active(self, src):
        """rt_gather_active: accumulator and statistics of the pixels on src's active-pixel list into this renderer's context"""
        self._rt_src(src, self.rt.rt_gather_active(self.ctx, src.ctx))

    # ---- reprojection (include/rt_amd.h rt_history_capture .. rt_download_aov_positions) ----
    def aov_positions(self, y0=0, y1=None):
        """rows [y0, y1) of the G-buffer's world positions as the device stored them, shaped (rows, width, 3)"""
        y1, out = self._rows(y0, y1, np.float32, 3)
        self._rt(self.rt.rt_download_aov_positions(self.ctx, y0, y1, _p(out)))
        return out

    def aov_instances(self, y0=0, y1=None):
        """rows [y0, y1) of the G-buffer's instance indices (int32, -1: no instance), shaped (rows, width)"""
        y1, out = self._rows(y0, y1, np.int32)
        self._rt(self.rt.rt_download_aov_instances(self.ctx, y0, y1, _p(out)))
        return out

    def aov_prims(self, y0=0, y1=None):
        """rows [y0, y1) of the G-buffer's primitive indices (int32: the record's index in the RT_LAYOUT_PRIMS array, -1: none), shaped (rows, width)"""
        y1, out = self._rows(y0, y1, np.int32)
        self._rt(self.rt.rt_download_aov_prims(self.ctx, y0, y1, _p(out)))
        return out

    def reproject_deform(self, params=None):
        """rt_reproject_deform: rt_reproject_motion that also follows the meshes deformed (rt_set_triangles, rt_set_time) since the capture"""
        p = reproject_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_reproject_deform(self.ctx, C.byref(p) if p is not None else None, C.byref(n)))
        return n.value

    def history_capture(self):
        self._rt(self.rt.rt_history_capture(self.ctx))

    def reproject_motion(self, params=None):
        """rt_reproject_motion: rt_reproject that also follows the instances moved (rt_set_instances) since the capture"""
        p = reproject_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_reproject_motion(self.ctx, C.byref(p) if p is not None else None, C.byref(n)))
        return n.value

    def reproject(self, params=None):
        """rt_reproject (params: dict, see reproject_params; None: the library's defaults): the number of pixels carried"""
        p = reproject_params(params)
        n = C.c_int(-1)
        self._rt(self.rt.rt_reproject(self.ctx, C.byref(p) if p is not None else None, C.byref(n)))
        return n.value

    def set_scene_raytracer(self, flag):
        """rt_set_scene_raytracer: -1 the flag follows the function (Trace: set, Sample: clear), 0 / 1 scene.raytracer as the caller holds it"""
        self._rt(self.rt.rt_set_scene_raytracer(self.ctx, int(flag)))

    def trace_batch(self, mode, O, D, depth=4, seed_base=0x12345678, energy=(1, 1, 1)):
        O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(O), 3), dtype=np.float32)
        self._rt(self.rt.rt_trace_batch_energy(self.ctx, mode, len(O), _p(O), _p(D), depth, seed_base, _f3(energy), _p(out)))
        return out

    def scope_nearest(self, scope, index, O, D, tmax=None):
        """rt_intersect_scope: 1 the accelerator alone, 2 BLAS index, 3 instance index"""
        O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(O), dtype=RT_HIT_DTYPE)
        tm = None if tmax is None else _p(np.ascontiguousarray(tmax, dtype=np.float32))
        self._rt(self.rt.rt_intersect_scope(self.ctx, scope, index, len(O), _p(O), _p(D), tm, C.c_float(0.0), _p(out)))
        return dict(t=out["t"].copy(), obj=out["obj_idx"].copy(), mat=out["material"].copy(), normal=out["normal"].copy())

    def scope_occluded(self, scope, index, O, D, tmax=None):
        O = np.ascontiguousarray(O, dtype=np.float32).reshape(-1, 3)
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(O), dtype=np.uint8)
        tm = None if tmax is None else _p(np.ascontiguousarray(tmax, dtype=np.float32))
        self._rt(self.rt.rt_occluded_scope(self.ctx, scope, index, len(O), _p(O), _p(D), tm, _p(out)))
        return out

    def sky_color(self, D):
        D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(D), 3), dtype=np.float32)
        self._rt(self.rt.rt_sky_color_batch(self.ctx, len(D), _p(D), _p(out)))
        return out

    def set_counting(self, on):
        """False / 0 off, True / RT_COUNT_REFERENCE the reference's walk, RT_COUNT_EXECUTED the timed kernels' walk"""
        self._rt(self.rt.rt_set_counting(self.ctx, int(on)))

    def counters(self, reset=True):
        c = np.zeros(8, dtype=np.uint64)
        self._rt(self.rt.rt_get_counters(self.ctx, _p(c), int(reset)))
        return dict(zip(COUNTER_NAMES, [int(x) for x in c]))

    def counters_split(self, reset=True):
        a = np.zeros(8, dtype=np.uint64)
        b = np.zeros(8, dtype=np.uint64)
        self._rt(self.rt.rt_get_counters_split(self.ctx, _p(a), _p(b), int(reset)))
        return dict(zip(COUNTER_NAMES, [int(x) for x in a])), dict(zip(COUNTER_NAMES, [int(x) for x in b]))

    # ---- Q-learning guided sampler (include/rt_amd.h rt_qlearn_*; no reference code: parity unpinned) ----
    def qlearn_enable(self, grid, lo, hi, alpha=0.3, epsilon=0.2, q_init=1.0, learn_mask=0):
        p = RtQlearnParams(grid, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), alpha, epsilon, q_init, learn_mask)
        self._qgrid = grid
        self._rt(self.rt.rt_qlearn_enable(self.ctx, C.byref(p)))

    def qlearn_disable(self):
        self._rt(self.rt.rt_qlearn_enable(self.ctx, None))

    def qlearn_apply(self):
        self._rt(self.rt.rt_qlearn_apply(self.ctx))

    def qlearn_sums(self):
        n = self._qgrid ** 3
        sums, cnts = np.zeros((n, 64), np.int64), np.zeros((n, 64), np.uint32)
        self._rt(self.rt.rt_qlearn_get_sums(self.ctx, _p(sums), _p(cnts)))
        return sums, cnts

    def qlearn_set_sums(self, sums, cnts):
        sums, cnts = np.ascontiguousarray(sums, np.int64), np.ascontiguousarray(cnts, np.uint32)
        self._rt(self.rt.rt_qlearn_set_sums(self.ctx, _p(sums), _p(cnts)))

    def qlearn_bind_sums(self, sums_ptr, counts_ptr):
        """rt_qlearn_bind_sums: the pending reward sums live in the caller's device arrays (data_ptr() of an int64 / int32 torch tensor
        of grid^3 * 64 elements) from here on"""
        self._rt(self.rt.rt_qlearn_bind_sums(self.ctx, C.c_void_p(sums_ptr), C.c_void_p(counts_ptr)))

    def qlearn_table(self):
        tab = np.zeros((self._qgrid ** 3, 64), np.float32)
        self._rt(self.rt.rt_qlearn_get_table(self.ctx, _p(tab)))
        return tab

    def build_info(self):
        """rt_build_info() + rt_tuning_info(): compile flags / compile-time tuning of the library and the tuning this context resolved"""
        return self.rt.rt_build_info().decode() + " | " + self.rt.rt_tuning_info(self.ctx).decode()

    def set_profiling(self, on):
        self._rt(self.rt.rt_set_profiling(self.ctx, int(on)))

    def profile(self, reset=True):
        p = RtProfile()
        self._rt(self.rt.rt_get_profile(self.ctx, C.byref(p), int(reset)))
        return {k: dict(launches=int(getattr(p, k).launches), ms=float(getattr(p, k).ms)) for k in ("generate", "extend", "shade", "connect", "query")}


# include/rt_amd.h RT_LAYOUT_*: (name, dtype) in enum order; RT_LAYOUT_SCALARS' words in their documented order
LAYOUT_ARRAYS = [("pairs", np.float32), ("prims", np.float32), ("wide", np.float32), ("wide8", np.uint32), ("leafBox", np.float32),
                 ("reach", np.float32), ("brute", np.float32), ("inst", np.uint32), ("lights", np.uint32), ("mats", np.uint32),
                 ("refitOrder", np.uint32), ("refitLevelStart", np.int32), ("rootLink", np.uint32), ("rootWide", np.uint32),
                 ("rootWide8", np.uint32), ("scalars", np.int32)]
LAYOUT_SCALARS = ["root", "tlasBase", "tlasPairs", "nInst", "reachOriginMax", "tlasLds", "stackRows", "nBruteSph", "nBrutePla",
                  "wideOK", "wide8OK", "pathUnsupported", "animSlots", "refitLevels"]


class LayoutError(RuntimeError):
    """rt_layout_build refused the description: .message is the text rt_upload_scene would report for it"""

    def __init__(self, message):
        RuntimeError.__init__(self, message)
        self.message = message


def layout(desc, wide=-1, wide8=0, tlas_lds=1):
    """rt_layout_build + rt_layout_array: the traversal layout rt_upload_scene would copy to the device for the rt_scene_desc 'desc'
    (HostScene.describe()) under RT_WIDE / RT_WIDE8 / RT_TLAS_LDS = wide / wide8 / tlas_lds, as a dict of flat numpy arrays named as in
    LAYOUT_ARRAYS (device records as uint32 words; rootLink, rootWide, rootWide8 per BLAS) plus every name of LAYOUT_SCALARS as a Python
    number ('root' is the scalar the header calls rootLink: the scene's root link).  Needs no device."""
    L = rt_lib()
    h = L.rt_layout_build(desc, int(wide), int(wide8), int(tlas_lds))
    if not h:
        raise LayoutError(L.rt_last_error(None).decode())
    try:
        out = {}
        for which, (name, dtype) in enumerate(LAYOUT_ARRAYS):
            data, nbytes = C.c_void_p(), C.c_size_t()
            if L.rt_layout_array(h, which, C.byref(data), C.byref(nbytes)) != 0:
                raise RuntimeError(L.rt_last_error(None).decode())
            out[name] = np.frombuffer(C.string_at(data, nbytes.value), dtype=dtype).copy() if nbytes.value else np.zeros(0, dtype)
        for name, v in zip(LAYOUT_SCALARS, out["scalars"]):
            out[name] = int(v)
        out["root"], out["tlasBase"] = (int(v) for v in out["scalars"].view(np.uint32)[:2])
        out["reachOriginMax"] = float(out["scalars"].view(np.float32)[4])
        return out
    finally:
        L.rt_layout_free(h)


LAUNCH_FORM_FIELDS = ["generate", "shade", "light", "light_mixed", "bt", "p", "masked", "fresh"]


def launch_form(facts, rnd):
    """rt_launch_form: what round 'rnd' of a dense path batch launches, as a dict named by LAUNCH_FORM_FIELDS.  facts: (primary table current,
    bounce table current, chain levels, RT_BOUNCE_TABLE != 0, RT_ROUND0_ENTRIES, sampler on, fisheye, rounds).  Needs no device."""
    L = rt_lib()
    f, out = (C.c_int32 * 8)(*[int(v) for v in facts]), (C.c_int32 * 8)()
    rc = L.rt_launch_form(f, int(rnd), out)
    if rc != 0:
        raise RuntimeError("rt_launch_form: %d: %s" % (rc, L.rt_last_error(None).decode()))
    return dict(zip(LAUNCH_FORM_FIELDS, out))


def any_hit_walk(counting, wide, wide8):
    """rt_any_hit_walk: 0 binary, 1 counting, 2 4-wide, 4 8-wide.  Needs no device."""
    return rt_lib().rt_any_hit_walk(int(counting), int(bool(wide)), int(bool(wide8)))


def device_pci_bus_id(device):
    """rt_device_pci_bus_id: the PCI address of HIP device 'device' (what two ranks on one GPU have in common)"""
    buf = C.create_string_buffer(64)
    rc = rt_lib().rt_device_pci_bus_id(int(device), buf, 64)
    if rc != 0:
        raise RuntimeError("rt_amd error %d: %s" % (rc, rt_lib().rt_last_error(None).decode()))
    return buf.value.decode()


def algorithmic_bytes(counters, executed=False):
    """Algorithmic bytes of a set of traversals, SURVEY.md section 8(d) literally: 64 B per BLAS inner-node visit
    (two 32-B children), 52 B per primitive test made BY THE TRAVERSAL (4-B index + 48-B triangle), 48 B per ray
    (32 in, 16 out), 64 B per TLAS inner visit and 128 B per instance entry (two mat4).  The head tests of
    Scene::FindNearest (lights, brute-force spheres / planes) run where rays are created, not in the traversal
    kernels, and are not priced here; neither are the 48-B reach records the timed kernels read per TLAS visit
    (bench.py reports those apart).  'executed' is accepted for older callers and ignored."""
    rays = counters["rays_nearest"] + counters["rays_occluded"]
    return (64 * counters["inner_visits"] + 52 * counters["prim_tests"] + 48 * rays
            + 64 * counters["tlas_inner"] + 128 * counters["instance_visits"])
