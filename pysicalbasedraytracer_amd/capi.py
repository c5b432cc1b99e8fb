"""ctypes mirror of include/pbr_hip.h (the C-ABI drop-in boundary).

The structures here are byte-for-byte the C descriptors; `load_library()` opens the in-tree
`libpbr_hip.so` and fails loudly when it is missing — there is no CPU fallback in the product.
"""
from __future__ import annotations

import ctypes as C
import os

ABI_VERSION = 5

PBR_OK = 0
PBR_E_INVALID = -1
PBR_E_HIP = -2
PBR_E_NOSCENE = -3
PBR_E_UNSUPPORTED = -4
PBR_E_NODEVICE = -5

# enum pbr_walk (pbr_hip_intersect_walk)
WALK_LANE, WALK_LANE_LDS, WALK_PACKET, WALK_REFILL, WALK_BINARY, WALK_REFILL_TR = range(6)
WALK_SEGMENTS = 2048

SHAPE_TRIANGLE_MESH, SHAPE_SPHERE = 0, 1
MAT_NONE, MAT_MATTE, MAT_MIRROR, MAT_GLASS, MAT_METAL, MAT_PLASTIC = range(6)
LIGHT_POINT, LIGHT_DIFFUSE_AREA, LIGHT_SKYBOX, LIGHT_INFINITE_AREA = 0, 1, 2, 3
INTEGRATOR_WHITTED, INTEGRATOR_PATH, INTEGRATOR_VOLPATH = 0, 1, 2
SAMPLER_HALTON, SAMPLER_SOBOL, SAMPLER_TABLE = 0, 1, 2
LIGHTS_UNIFORM, LIGHTS_POWER = 0, 1
BVH_BUILD_HOST, BVH_BUILD_DEVICE = 0, 1
SPLIT_SAH, SPLIT_HLBVH, SPLIT_MIDDLE, SPLIT_EQUAL_COUNTS = 0, 1, 2, 3
WRAP_REPEAT, WRAP_BLACK, WRAP_CLAMP = 0, 1, 2
TEX_KD, TEX_KS, TEX_KR, TEX_KT, TEX_SIGMA, TEX_ROUGHNESS = range(6)

F3 = C.c_float * 3
F16 = C.c_float * 16


class Transform(C.Structure):
    _fields_ = [("m", F16), ("m_inv", F16)]


class ShapeDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int),
        ("object_to_world", Transform),
        ("reverse_orientation", C.c_int),
        ("n_triangles", C.c_int),
        ("n_vertices", C.c_int),
        ("indices", C.POINTER(C.c_int32)),
        ("P", C.POINTER(C.c_float)),
        ("N", C.POINTER(C.c_float)),
        ("UV", C.POINTER(C.c_float)),
        ("radius", C.c_float),
        ("material", C.c_int),
        ("area_light_first", C.c_int),
        ("medium_inside", C.c_int),
        ("medium_outside", C.c_int),
    ]


class MaterialDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int),
        ("Kd", F3),
        ("sigma", C.c_float),
        ("Kr", F3),
        ("Kt", F3),
        ("Ks", F3),
        ("eta", C.c_float),
        ("metal_eta", F3),
        ("metal_k", F3),
        ("roughness", C.c_float),
        ("uroughness", C.c_float),
        ("vroughness", C.c_float),
        ("has_uv_roughness", C.c_int),
        ("remap_roughness", C.c_int),
        ("tex", C.c_int * 6),
    ]


class TextureDesc(C.Structure):
    _fields_ = [
        ("is_float", C.c_int),
        ("width", C.c_int),
        ("height", C.c_int),
        ("components", C.c_int),
        ("data", C.POINTER(C.c_float)),
        ("scale", C.c_float),
        ("gamma", C.c_int),
        ("wrap", C.c_int),
        ("trilinear", C.c_int),
        ("max_aniso", C.c_float),
        ("su", C.c_float),
        ("sv", C.c_float),
        ("du", C.c_float),
        ("dv", C.c_float),
        ("level0", C.c_int),
    ]


class LightDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int),
        ("light_to_world", Transform),
        ("I", F3),
        ("Le", F3),
        ("shape", C.c_int),
        ("triangle", C.c_int),
        ("two_sided", C.c_int),
        ("n_samples", C.c_int),
        ("medium_inside", C.c_int),
        ("medium_outside", C.c_int),
        ("world_center", F3),
        ("world_radius", C.c_float),
        ("env_width", C.c_int),
        ("env_height", C.c_int),
        ("env_components", C.c_int),
        ("env_data", C.POINTER(C.c_float)),
    ]


class MediumDesc(C.Structure):
    _fields_ = [("sigma_a", F3), ("sigma_s", F3), ("g", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int),
        ("n_shapes", C.c_int),
        ("shapes", C.POINTER(ShapeDesc)),
        ("n_materials", C.c_int),
        ("materials", C.POINTER(MaterialDesc)),
        ("n_lights", C.c_int),
        ("lights", C.POINTER(LightDesc)),
        ("n_media", C.c_int),
        ("media", C.POINTER(MediumDesc)),
        ("max_prims_in_node", C.c_int),
        ("n_textures", C.c_int),
        ("textures", C.POINTER(TextureDesc)),
        ("split_method", C.c_int),
        ("bvh_nodes", C.c_void_p),
        ("n_bvh_nodes", C.c_int),
    ]


class CameraDesc(C.Structure):
    _fields_ = [
        ("width", C.c_int),
        ("height", C.c_int),
        ("camera_to_world", Transform),
        ("use_look_at", C.c_int),
        ("eye", F3),
        ("look", F3),
        ("up", F3),
        ("fov", C.c_float),
        ("lens_radius", C.c_float),
        ("focal_distance", C.c_float),
        ("medium", C.c_int),
        ("use_raster_to_camera", C.c_int),
        ("raster_to_camera", Transform),
    ]


class Tile(C.Structure):
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("x1", C.c_int), ("y1", C.c_int)]


class RenderDesc(C.Structure):
    _fields_ = [
        ("integrator", C.c_int),
        ("max_depth", C.c_int),
        ("rr_threshold", C.c_float),
        ("light_strategy", C.c_int),
        ("sampler", C.c_int),
        ("spp", C.c_int),
        ("camera", CameraDesc),
        ("n_tiles", C.c_int),
        ("tiles", C.POINTER(Tile)),
        ("outputs_on_device", C.c_int),
        ("stream", C.c_void_p),
        ("collect_stats", C.c_int),
        ("sobol_matrices", C.POINTER(C.c_uint32)),
        ("sobol_dims", C.c_int),
        ("sample_table", C.POINTER(C.c_float)),
        ("table_dims", C.c_int),
    ]


class Adaptive(C.Structure):   # pbr_adaptive
    _fields_ = [
        ("min_samples", C.c_int),
        ("samples_per_round", C.c_int),
        ("tolerance", C.c_float),
        ("floor", C.c_float),
    ]


class AdaptiveResult(C.Structure):   # pbr_adaptive_result
    _fields_ = [
        ("rounds", C.c_int),
        ("max_samples_done", C.c_int),
        ("samples", C.c_int64),
        ("active_at_end", C.c_int64),
    ]


class RenderStats(C.Structure):
    _fields_ = [
        ("seconds", C.c_double),
        ("kernel_ms", C.c_double),
        ("film_ms", C.c_double),
        ("samples", C.c_uint64),
        ("rays", C.c_uint64),
        ("node_visits", C.c_uint64),
        ("prim_tests", C.c_uint64),
        ("shading_events", C.c_uint64),
        ("n_launches", C.c_int),
    ]


class SurfaceHit(C.Structure):
    _fields_ = [
        ("hit", C.c_int), ("prim", C.c_int), ("t", C.c_float), ("b", C.c_float * 3),
        ("p", C.c_float * 3), ("p_error", C.c_float * 3), ("n", C.c_float * 3), ("ns", C.c_float * 3),
        ("dpdu", C.c_float * 3), ("wo", C.c_float * 3), ("uv", C.c_float * 2),
        ("medium_inside", C.c_int), ("medium_outside", C.c_int),
    ]


class KernelProfile(C.Structure):
    _fields_ = [
        ("name", C.c_char * 40),
        ("launches", C.c_int),
        ("ms", C.c_double),
        ("units", C.c_uint64),
        ("bytes", C.c_uint64),
        ("counts", C.c_uint64 * 8),
    ]


KERNELS_AUTO, KERNELS_MEGAKERNEL = 0, 1
FUSE_AUTO, FUSE_OFF, FUSE_ON = 0, 1, 2


class Schedule(C.Structure):
    _fields_ = [("kernels", C.c_int), ("chunk_log2", C.c_int), ("lanes", C.c_int), ("fuse_camera", C.c_int),
                ("serial", C.c_int)]


class ChunkQuery(C.Structure):
    _fields_ = [("integrator", C.c_int), ("n_pixels", C.c_int64), ("spp", C.c_int), ("max_depth", C.c_int),
                ("n_lights", C.c_int), ("sky_light", C.c_int), ("batch", C.c_int), ("scene_fusable", C.c_int),
                ("lane_budget", C.c_double)]


class ChunkPlan(C.Structure):
    _fields_ = [("lanes", C.c_int), ("chunk_log2", C.c_int), ("chunk_pixels", C.c_int64), ("n_chunks", C.c_int64),
                ("cap", C.c_uint64), ("qcap", C.c_uint64), ("seg_cap", C.c_int), ("lane0_on_ctx_stream", C.c_int),
                ("fused_camera", C.c_int), ("reserved", C.c_int), ("bytes_per_sample", C.c_double),
                ("lane_budget", C.c_double), ("held_lane_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}
        d["lane0_on_ctx_stream"] = bool(d["lane0_on_ctx_stream"])
        d["fused_camera"] = bool(d["fused_camera"])
        return d


def plan_chunks(integrator, n_pixels, spp, max_depth, n_lights=1, sky_light=False, batch=False, lane_budget=0.0,
                scene_fusable=True, schedule: "Schedule | None" = None, lib=None) -> dict:
    """pbr_hip_plan_chunks: how the wavefront schedules would cut such a frame into chunks over lanes
    (no context, no GPU call).  lane_budget in bytes, 0 = unknown; schedule None = the defaults."""
    q = ChunkQuery(int(integrator), int(n_pixels), int(spp), int(max_depth), int(n_lights), int(bool(sky_light)),
                   int(bool(batch)), int(bool(scene_fusable)), float(lane_budget))
    out = ChunkPlan()
    rc = (lib or load_library()).pbr_hip_plan_chunks(C.byref(schedule) if schedule is not None else None, C.byref(q),
                                                     C.byref(out))
    if rc != PBR_OK:
        raise ValueError(f"plan_chunks: invalid query or schedule ({rc})")
    return out.as_dict()


AOV_CHANNELS = 8   # PBR_AOV_CHANNELS: albedo rgb, hit, shading normal xyz, t
AOV_MAX_MIRROR_BOUNCES = 16   # pbr_hip_render_aov_mirrors: max_bounces lies in 0..16


def plan_aov(n_pixels, samples, lib=None) -> list:
    """pbr_hip_plan_aov: the (first_pixel, n_pixels) launches a feature pass over n_pixels pixels of
    `samples` samples each is cut into (no context, no GPU call)."""
    fn = (lib or load_library()).pbr_hip_plan_aov
    n = C.c_int(0)
    if fn(int(n_pixels), int(samples), 0, None, None, C.byref(n)) != PBR_OK:
        raise ValueError("plan_aov: n_pixels and samples must be >= 1")
    first, count = (C.c_int64 * n.value)(), (C.c_int64 * n.value)()
    if fn(int(n_pixels), int(samples), n.value, first, count, C.byref(n)) != PBR_OK:
        raise ValueError("plan_aov: n_pixels and samples must be >= 1")
    return [(int(first[i]), int(count[i])) for i in range(n.value)]


class Denoise(C.Structure):
    """pbr_denoise: the frame and the filter's parameters (pbr_hip_denoise)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("iterations", C.c_int), ("demodulate", C.c_int),
                ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float)]


class SpatialVariance(C.Structure):
    """pbr_spatial_variance: which pixels take the denoiser's spatial variance estimate, and its window
    (pbr_hip_denoise_sv)."""
    _fields_ = [("min_count", C.c_int), ("radius", C.c_int)]


class Temporal(C.Structure):
    """pbr_temporal: the frame, the merge's parameters and the two cameras' matrices (pbr_hip_temporal)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("max_history", C.c_int), ("demodulate", C.c_int),
                ("tol_z", C.c_float), ("tol_n", C.c_float),
                ("cur_raster_to_world", F16), ("cur_eye", F3), ("prev_world_to_raster", F16), ("prev_eye", F3)]


def camera_matrices(cam: "CameraDesc", lib=None):
    """pbr_hip_camera_matrices: (raster_to_world [4, 4], world_to_raster [4, 4], eye [3]) float32 of a camera
    descriptor, from the transforms a render of it uses (no context, no GPU call)."""
    import numpy as np
    r2w, w2r, eye = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), np.zeros(3, np.float32)
    if (lib or load_library()).pbr_hip_camera_matrices(C.byref(cam), fptr(r2w), fptr(w2r), fptr(eye)) != PBR_OK:
        raise ValueError("camera_matrices: width and height must be >= 1")
    return r2w, w2r, eye


# enum pbr_bsdf_variant (pbr_hip_bsdf): the lobe mask and template source of a production shading kernel
(BSDF_VARIANT_ALL, BSDF_VARIANT_SIMPLE, BSDF_VARIANT_MATTE_MIRROR, BSDF_VARIANT_MICRO, BSDF_VARIANT_PASS_L,
 BSDF_VARIANT_PASS_R, BSDF_VARIANT_PASS_LR, BSDF_VARIANT_PASS_RT, BSDF_VARIANT_PASS_LRT, BSDF_VARIANT_MIRROR,
 BSDF_VARIANT_TEXTURED, BSDF_VARIANT_ALL_LDS, BSDF_VARIANT_ALL_GLOBAL) = range(13)
# BxDFType (Reflection.h:47-55)
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR, BSDF_ALL = 1, 2, 4, 8, 16, 31


def bsdf_query_dtype():
    """pbr_bsdf_query as a numpy record type (96 bytes)."""
    import numpy as np
    return np.dtype([("material", "i4"), ("multi_lobe", "i4"), ("type", "i4"), ("pad0", "i4"), ("n", "f4", 3), ("ns", "f4", 3),
                     ("dpdu", "f4", 3), ("uv", "f4", 2), ("wo", "f4", 3), ("wi", "f4", 3), ("u0", "f4"), ("u1", "f4"),
                     ("pad1", "f4")])


def bsdf_record_dtype():
    """pbr_bsdf_record as a numpy record type (128 bytes)."""
    import numpy as np
    return np.dtype([("no_bsdf", "i4"), ("f", "f4", 3), ("pdf", "f4"), ("f_lam", "f4", 3), ("pdf_lam", "f4"),
                     ("f_nolam", "f4", 3), ("pdf_nolam", "f4"), ("s_wi", "f4", 3), ("s_f", "f4", 3), ("s_pdf", "f4"),
                     ("s_type", "i4"), ("d_wi", "f4", 3), ("d_f", "f4", 3), ("d_pdf", "f4"), ("d_type", "i4"), ("d_ok", "i4"),
                     ("pad", "i4", 2)])


def bsdf_host(material: "MaterialDesc", variant, queries, lib=None):
    """pbr_hip_bsdf_host: the device's BSDF functions compiled for the CPU, on one constant material
    (query material 0).  queries: bsdf_query_dtype records; returns bsdf_record_dtype records.
    Raises ValueError where the library refuses (variant, mask, textured material)."""
    import numpy as np
    q = np.ascontiguousarray(queries, dtype=bsdf_query_dtype()).reshape(-1)
    out = np.zeros(q.shape[0], dtype=bsdf_record_dtype())
    rc = (lib or load_library()).pbr_hip_bsdf_host(C.byref(material), int(variant), q.shape[0], q.ctypes.data, out.ctypes.data)
    if rc != PBR_OK:
        raise ValueError(f"bsdf_host: refused ({rc})")
    return out


def mirror_step_host(hits, kr, lib=None):
    """pbr_hip_mirror_step_host: the followed feature pass's mirror step, compiled for the CPU.  hits: a
    ctypes array (or list) of SurfaceHit; kr: [n, 3] float32.  Returns (rays [n, 7] float32, followed [n]
    int32)."""
    import numpy as np
    n = len(hits)
    arr = hits if isinstance(hits, C.Array) else (SurfaceHit * max(1, n))(*hits)
    k = np.ascontiguousarray(kr, dtype=np.float32).reshape(-1, 3)
    if k.shape[0] != n:
        raise ValueError(f"mirror_step_host: {k.shape[0]} kr for {n} hits")
    if n == 0:
        k = np.zeros((1, 3), dtype=np.float32)   # (the library refuses NULL whatever n is)
    rays = np.zeros((max(1, n), 7), dtype=np.float32)
    followed = np.zeros(max(1, n), dtype=np.int32)
    rc = (lib or load_library()).pbr_hip_mirror_step_host(n, arr, k.ctypes.data, rays.ctypes.data, followed.ctypes.data)
    if rc != PBR_OK:
        raise ValueError(f"mirror_step_host: refused ({rc})")
    return rays[:n], followed[:n]


def phase_hg_host(queries, lib=None):
    """pbr_hip_phase_hg_host: [n, 9] (g, wo, wi, u0, u1) → [n, 5] (p, sampled wi, its value)."""
    import numpy as np
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 9)
    out = np.zeros((q.shape[0], 5), dtype=np.float32)
    if (lib or load_library()).pbr_hip_phase_hg_host(q.shape[0], fptr(q), fptr(out)) != PBR_OK:
        raise ValueError("phase_hg_host: refused")
    return out


def shading_query_dtype():
    """pbr_shading_query as a numpy record type (128 bytes)."""
    import numpy as np
    return np.dtype([("p", "f4", (3, 3)), ("n", "f4", (3, 3)), ("uv", "f4", (3, 2)), ("b", "f4", 3), ("has_uv", "i4"),
                     ("reverse_orientation", "i4"), ("swaps_handedness", "i4"), ("pad", "i4", 2)])


def shading_host(queries, lib=None):
    """pbr_hip_shading_host: the hit path's shading frame of a triangle with per-vertex normals,
    compiled for the CPU.  queries: shading_query_dtype records; returns [n, 3, 3] float32
    (n, shading.n, shading.dpdu)."""
    import numpy as np
    q = np.ascontiguousarray(queries, dtype=shading_query_dtype()).reshape(-1)
    out = np.zeros((q.shape[0], 3, 3), dtype=np.float32)
    if (lib or load_library()).pbr_hip_shading_host(q.shape[0], q.ctypes.data, out.ctypes.data) != PBR_OK:
        raise ValueError("shading_host: refused")
    return out


# Every symbol include/pbr_hip.h declares, with its ctypes signature.
EXPORTS = {
    "pbr_hip_shading_host": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "pbr_hip_bsdf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pbr_hip_bsdf_host": (C.c_int, [C.POINTER(MaterialDesc), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pbr_hip_phase_hg": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pbr_hip_phase_hg_host": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pbr_hip_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "pbr_hip_upload_scene": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "pbr_hip_render": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_void_p, C.c_void_p,
                                 C.POINTER(RenderStats)]),
    "pbr_hip_destroy": (C.c_int, [C.c_void_p]),
    "pbr_hip_last_error": (C.c_char_p, [C.c_void_p]),
    "pbr_hip_sync": (C.c_int, [C.c_void_p]),
    "pbr_hip_render_frames": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p)]),
    "pbr_hip_wait_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "pbr_hip_render_passes": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "pbr_hip_adaptive_select": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "pbr_hip_render_passes_list": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbr_hip_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.POINTER(Adaptive), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.POINTER(AdaptiveResult)]),
    "pbr_hip_render_aov": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pbr_hip_render_aov_mirrors": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pbr_hip_mirror_step_host": (C.c_int, [C.c_int, C.POINTER(SurfaceHit), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbr_hip_plan_aov": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int)]),
    "pbr_hip_denoise": (C.c_int, [C.c_void_p, C.POINTER(Denoise), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "pbr_hip_denoise_sv": (C.c_int, [C.c_void_p, C.POINTER(Denoise), C.POINTER(SpatialVariance), C.c_int] + [C.c_void_p] * 7),
    "pbr_hip_spatial_variance_host": (C.c_int, [C.POINTER(Denoise), C.POINTER(SpatialVariance), C.c_int] + [C.c_void_p] * 4),
    "pbr_hip_camera_matrices": (C.c_int, [C.POINTER(CameraDesc), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                          C.POINTER(C.c_float)]),
    "pbr_hip_temporal": (C.c_int, [C.c_void_p, C.POINTER(Temporal), C.c_int] + [C.c_void_p] * 12),
    "pbr_hip_temporal_host": (C.c_int, [C.POINTER(Temporal), C.c_int] + [C.c_void_p] * 9),
    "pbr_hip_get_bvh": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int)]),
    "pbr_hip_sampler_values": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "pbr_hip_sample_index": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pbr_hip_sample_dimensions": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "pbr_hip_camera_rays": (C.c_int, [C.c_void_p, C.POINTER(CameraDesc), C.c_int, C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]),
    "pbr_hip_intersect": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]),
    "pbr_hip_intersect_walk": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                         C.c_int, C.POINTER(C.c_int32)]),
    "pbr_hip_abi_version": (C.c_int, []),
    "pbr_hip_build_info": (C.c_char_p, []),
    "pbr_hip_sobol_matrices": (C.c_int, [C.c_int, C.POINTER(C.c_uint32)]),
    "pbr_hip_query": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(SurfaceHit)]),
    "pbr_hip_bounds": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "pbr_hip_li": (C.c_int, [C.c_void_p, C.POINTER(RenderDesc), C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                             C.c_int, C.POINTER(C.c_float)]),
    "pbr_hip_set_schedule": (C.c_int, [C.c_void_p, C.POINTER(Schedule)]),
    "pbr_hip_plan_chunks": (C.c_int, [C.POINTER(Schedule), C.POINTER(ChunkQuery), C.POINTER(ChunkPlan)]),
    "pbr_hip_last_chunks": (C.c_int, [C.c_void_p, C.POINTER(ChunkPlan)]),
    "pbr_hip_set_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "pbr_hip_get_profile": (C.c_int, [C.c_void_p, C.POINTER(KernelProfile), C.c_int, C.POINTER(C.c_int)]),
    "pbr_hip_set_bvh_build": (C.c_int, [C.c_void_p, C.c_int]),
    "pbr_hip_bvh_build_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double)]),
    "pbr_hip_build_bvh": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_void_p,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
}

PACKAGE_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PACKAGE_DIR, "libpbr_hip.so")

_lib = None


OPTIONAL_FOR_AB = ("pbr_hip_sync", "pbr_hip_set_profiling", "pbr_hip_get_profile", "pbr_hip_query", "pbr_hip_bounds",
                   "pbr_hip_li", "pbr_hip_set_bvh_build", "pbr_hip_bvh_build_info", "pbr_hip_build_bvh",
                   "pbr_hip_set_schedule", "pbr_hip_sample_index", "pbr_hip_sample_dimensions",
                   "pbr_hip_render_frames", "pbr_hip_wait_frame", "pbr_hip_render_passes", "pbr_hip_intersect_walk",
                   "pbr_hip_plan_chunks", "pbr_hip_last_chunks", "pbr_hip_adaptive_select", "pbr_hip_render_passes_list",
                   "pbr_hip_render_adaptive", "pbr_hip_render_aov", "pbr_hip_plan_aov", "pbr_hip_denoise", "pbr_hip_bsdf",
                   "pbr_hip_bsdf_host", "pbr_hip_phase_hg", "pbr_hip_phase_hg_host", "pbr_hip_shading_host",
                   "pbr_hip_camera_matrices", "pbr_hip_temporal", "pbr_hip_temporal_host", "pbr_hip_denoise_sv",
                   "pbr_hip_spatial_variance_host", "pbr_hip_render_aov_mirrors", "pbr_hip_mirror_step_host")


def load_library(path: str | None = None) -> C.CDLL:
    """Open the in-tree HIP library. Raises if it has not been built: no fallback exists."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"libpbr_hip.so not built at {p}; run `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: torch bundles its own libamdhip64 (same soname as /opt/rocm's).
    # Whichever loads first serves both, and torch fails to initialise ("No HIP GPUs are
    # available") on the newer system runtime, so let torch load first when it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (res, args) in EXPORTS.items():
        if path is not None and name in OPTIONAL_FOR_AB and not hasattr(lib, name):
            continue   # an older experimental build (A/B timing runs) may predate this entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    v = lib.pbr_hip_abi_version()
    # (v5 changed the texture and camera descriptors: an older build cannot take these structures)
    if v != ABI_VERSION:
        raise RuntimeError("libpbr_hip.so ABI version mismatch")
    if path is None:
        _lib = lib
    return lib


def fptr(a):
    """float32 numpy array → POINTER(c_float) (array must stay alive)."""
    return a.ctypes.data_as(C.POINTER(C.c_float))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))
