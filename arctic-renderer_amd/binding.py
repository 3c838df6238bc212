"""ctypes declarations of the C-ABI (include/arctic_hip.h -> csrc/libarctic_hip.so).

This is the binding a Python host would use; the C++ equivalent is host/renderer.hpp.
The library is never built implicitly and there is no fallback: if the shared
object is missing, lib() raises with the build command.
"""
import ctypes as C
import os
import re

from .scene import CCreateInfo, CScene, CSettings

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARCTIC_HIP_LIBRARY") or os.path.join(HERE, "csrc", "libarctic_hip.so")   # the override is for A/B timing of two builds (tools/experiments)
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "arctic_hip.h")

OPTIONS = {"keep_float_output": 1, "count_light_evals": 2, "culling": 3, "debug": 4, "antialias": 5, "hdr16": 6, "ray_refit": 7, "light_pair_runs": 8, "shadow_cache": 9, "visbuffer": 10, "item_table_floor": 11, "light_path": 12, "markers": 13, "shadow_sharded": 14, "frames_in_flight": 15, "tiles_per_wave": 16, "tile_trace": 17, "raster_owner": 18, "tile_order": 19, "order_tail": 20, "sampler": 21, "texture_tiling": 22, "cluster_cull": 23, "small_triangles": 24, "env_lighting": 25, "point_shadow_size": 26, "texture_mips": 27, "hit_model": 0}
TRACE_ANY, TRACE_BRUTE = 1, 2   # ARCTIC_TRACE_* (include/arctic_hip.h)
COMPOSE_AO, COMPOSE_REFLECTIONS = 1, 2   # ARCTIC_COMPOSE_*
TAA_LUMA_WEIGHT, TAA_SOURCE_COMPOSED = 1, 2   # ARCTIC_TAA_*
MB_DITHER, MB_SOURCE_COMPOSED, MB_SOURCE_TAA = 1, 2, 4   # ARCTIC_MB_*
DOF_SOURCE_COMPOSED, DOF_SOURCE_TAA, DOF_SOURCE_MOTION_BLUR = 1, 2, 4   # ARCTIC_DOF_*
BLOOM_SOURCE_COMPOSED, BLOOM_SOURCE_TAA, BLOOM_SOURCE_MOTION_BLUR, BLOOM_SOURCE_DOF = 1, 2, 4, 8   # ARCTIC_BLOOM_*
EXPOSURE_SOURCE_COMPOSED, EXPOSURE_SOURCE_TAA, EXPOSURE_SOURCE_MOTION_BLUR, EXPOSURE_SOURCE_DOF, EXPOSURE_SOURCE_BLOOM = 1, 2, 4, 8, 16   # ARCTIC_EXPOSURE_*
EXPOSURE_SKIP_BLACK, EXPOSURE_RESET, EXPOSURE_HOLD, EXPOSURE_METER_ONLY = 32, 64, 128, 256
FOG_SOURCE_COMPOSED = 1   # ARCTIC_FOG_*
GI_SOURCE_COMPOSED = 1   # ARCTIC_GI_*
TAA_UPSCALE_LUMA_WEIGHT, TAA_UPSCALE_SOURCE_COMPOSED, TAA_UPSCALE_NO_CLAMP, TAA_UPSCALE_JITTER_EXACT = 1, 2, 4, 0x80000000   # ARCTIC_TAA_UPSCALE_*
ERRORS = {-1: "ARCTIC_E_INVALID", -2: "ARCTIC_E_DEVICE", -3: "ARCTIC_E_NO_DEVICE", -4: "ARCTIC_E_STATE", -5: "ARCTIC_E_CAPACITY"}

_vp, _u32, _u64, _i32, _i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64
_scene, _settings = C.POINTER(CScene), C.POINTER(CSettings)

# every entry point of include/arctic_hip.h: name -> (restype, argtypes)
SIGNATURES = {
    "arctic_create": (_vp, [C.POINTER(CCreateInfo), C.c_char_p, _u64]),
    "arctic_destroy": (None, [_vp]),
    "arctic_last_error": (C.c_char_p, [_vp]),
    "arctic_resize": (_i32, [_vp, _u32, _u32]),
    "arctic_flush": (_i32, [_vp]),
    "arctic_set_stream": (_i32, [_vp, _vp]),
    "arctic_use_own_stream": (_i32, [_vp]),
    "arctic_create_material": (_i32, [_vp, _vp, _u32, _u32, _vp, _u32, _u32, _vp, _u32, _u32]),
    "arctic_create_mesh": (_i32, [_vp, _vp, _u64, _vp, _u64, _u64]),
    "arctic_set_mesh_skin": (_i32, [_vp, _u64, _vp, _u64, _u32]),
    "arctic_set_mesh_pose": (_i32, [_vp, _u64, _vp, _u32]),
    "arctic_set_mesh_morph_targets": (_i32, [_vp, _u64, _vp, _u64, _u32]),
    "arctic_set_mesh_morph_weights": (_i32, [_vp, _u64, _vp, _u32]),
    "arctic_check_morph_targets": (_i32, [_vp, _u64, _u32]),
    "arctic_morph_vertices": (_i32, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "arctic_read_mesh_vertices": (_i32, [_vp, _u64, _vp, _u64]),
    "arctic_check_mesh_skin": (_i32, [_vp, _u64, _u32]),
    "arctic_skin_vertices": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "arctic_set_material_extras": (_i32, [_vp, _u64, _vp, _vp, _u32, _u32, _vp, _u32, _u32]),
    "arctic_check_material_params": (_i32, [_vp]),
    "arctic_update_lights": (_i32, [_vp, _vp, _u64]),
    "arctic_light_pair_table": (_i32, [_vp, _u64, _i32, _vp, _vp, _vp]),
    "arctic_update_spot_lights": (_i32, [_vp, _vp, _u64]),
    "arctic_spot_light_constants": (_i32, [_vp, _u64, _vp]),
    "arctic_update_point_shadow_lights": (_i32, [_vp, _vp, _u64]),
    "arctic_point_shadow_matrices": (_i32, [_vp, _vp]),
    "arctic_pass_point_shadows": (_i32, [_vp, _scene]),
    "arctic_read_point_shadow": (_i32, [_vp, _u32, _vp]),
    "arctic_write_point_shadow": (_i32, [_vp, _u32, _vp]),
    "arctic_create_hdri": (_i32, [_vp, _vp, _u32, _u32]),
    "arctic_render_frame": (_i32, [_vp, _scene, _settings, _vp]),
    "arctic_render_frame_device": (_i32, [_vp, _scene, _settings, _vp]),
    "arctic_pass_shadow_map": (_i32, [_vp, _scene]),
    "arctic_pass_gbuffer": (_i32, [_vp, _scene]),
    "arctic_pass_shade": (_i32, [_vp, _scene, _settings, _vp]),
    "arctic_post_process": (_i32, [_vp, _vp, _u32, _u32, _settings, _vp, _vp]),
    "arctic_antialias_device": (_i32, [_vp, _vp, _vp, _u32, _u32]),
    "arctic_antialias": (_i32, [_vp, _vp, _u32, _u32, _vp]),
    "arctic_time_shade": (_i32, [_vp, _scene, _settings, _u32, _u32, _vp]),
    "arctic_read_gbuffer": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "arctic_write_gbuffer": (_i32, [_vp, _vp, _vp]),
    "arctic_read_shadow_map": (_i32, [_vp, _vp]),
    "arctic_write_shadow_map": (_i32, [_vp, _vp]),
    "arctic_read_output": (_i32, [_vp, _vp, _vp, _vp]),
    "arctic_frame_constants": (_i32, [_scene, _vp, _vp, _vp]),
    "arctic_stats": (_i32, [_vp, _vp, _u32]),
    "arctic_read_tile_trace": (_i32, [_vp, _vp, _u64, _vp, _vp]),
    "arctic_read_tile_order": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "arctic_read_bin_counts": (_i32, [_vp, _i32, _vp, _u64, _vp, _vp]),
    "arctic_read_cull_counts": (_i32, [_vp, _i32, _vp]),
    "arctic_owner_grid": (_i32, [_u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp]),
    "arctic_owner_visit": (_i32, [_u32, _u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "arctic_cluster_bounds": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "arctic_set_option": (_i32, [_vp, _u32, _i64]),
    "arctic_read_env_lighting": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "arctic_read_material_mip": (_i32, [_vp, _u32, _u32, _vp, _vp]),
    "arctic_read_lod": (_i32, [_vp, _vp]),
    "arctic_write_lod": (_i32, [_vp, _vp]),
    "arctic_trace_rays": (_i32, [_vp, _scene, _vp, _u64, _u32, _vp]),
    "arctic_trace_rays_device": (_i32, [_vp, _scene, _vp, _u64, _u32, _vp]),
    "arctic_trace_sun_visibility": (_i32, [_vp, _scene, C.c_float, _vp]),
    "arctic_trace_triangles": (_i32, [_vp, _u64, _vp, _u64, _u32, _vp]),
    "arctic_ray_scene_info": (_i32, [_vp, _vp]),
    "arctic_ray_refit_info": (_i32, [_vp, _vp]),
    "arctic_ray_scene_reset": (_i32, [_vp]),
    "arctic_read_ray_structure": (_i32, [_vp, _vp, _u64, _vp, _u64]),
    "arctic_refit_triangles": (_i32, [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _u64, _vp]),
    "arctic_ray_scene_resplit": (_i32, [_vp, _scene]),
    "arctic_ray_resplit_info": (_i32, [_vp, _vp]),
    "arctic_resplit_triangles": (_i32, [_vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _u64, _vp]),
    "arctic_trace_ambient_occlusion": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_trace_ambient_occlusion_device": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_ambient_occlusion_points": (_i32, [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _u32, _vp]),
    "arctic_hit_attributes": (_i32, [_vp, _scene, _vp, _u64, _vp, _vp]),
    "arctic_interpolate_hits": (_i32, [_vp, _u64, _vp, _u64, _vp, _vp, _u32, _u64, _vp, _u64, _vp, _vp]),
    "arctic_shade_hits": (_i32, [_vp, _scene, _vp, _vp, _u64, _u32, _vp]),
    "arctic_shade_hits_device": (_i32, [_vp, _scene, _vp, _vp, _u64, _u32, _vp]),
    "arctic_trace_reflections": (_i32, [_vp, _scene, C.c_float, _vp]),
    "arctic_trace_reflections_device": (_i32, [_vp, _scene, C.c_float, _vp]),
    "arctic_hit_shading_info": (_i32, [_vp, _vp]),
    "arctic_compose_planes_device": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp]),
    "arctic_pass_ray_effects": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp]),
    "arctic_read_composed": (_i32, [_vp, _vp, _vp, _vp]),
    "arctic_compose_pixels": (_i32, [_vp, _vp, C.c_float, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_compose_info": (_i32, [_vp, _vp]),
    "arctic_accumulate_ambient_occlusion_device": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_accumulate_ambient_occlusion": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_ao_history_reset": (_i32, [_vp]),
    "arctic_read_ao_history": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "arctic_ao_history_info": (_i32, [_vp, _vp]),
    "arctic_accumulate_pixels": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_pass_ray_effects_temporal": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_motion_vectors_device": (_i32, [_vp, _scene, _vp, _vp]),
    "arctic_motion_vectors": (_i32, [_vp, _scene, _vp, _vp, _vp, _vp]),
    "arctic_motion_reset": (_i32, [_vp]),
    "arctic_motion_info": (_i32, [_vp, _vp]),
    "arctic_motion_pixels": (_i32, [_u64, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _u32, _u32, _vp, _vp]),
    "arctic_accumulate_ambient_occlusion_motion_device": (_i32, [_vp, _scene, _vp, _vp, _vp, _vp]),
    "arctic_accumulate_ambient_occlusion_motion": (_i32, [_vp, _scene, _vp, _vp, _vp, _vp]),
    "arctic_accumulate_pixels_motion": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_pass_ray_effects_motion": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_set_camera_jitter": (_i32, [_vp, C.c_float, C.c_float]),
    "arctic_jitter_proj_view": (_i32, [_vp, _u32, _u32, C.c_float, C.c_float]),
    "arctic_taa_resolve_device": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp]),
    "arctic_taa_resolve": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp]),
    "arctic_pass_taa": (_i32, [_vp, _scene, _settings, _vp, _vp]),
    "arctic_taa_reset": (_i32, [_vp]),
    "arctic_read_taa": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "arctic_taa_info": (_i32, [_vp, _vp]),
    "arctic_taa_pixels": (_i32, [_vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_motion_blur_device": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_motion_blur": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_depth_plane_device": (_i32, [_vp, _vp]),
    "arctic_pass_motion_blur": (_i32, [_vp, _scene, _settings, _vp, _vp]),
    "arctic_read_motion_blur": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_motion_blur_info": (_i32, [_vp, _vp]),
    "arctic_motion_blur_prepare": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "arctic_motion_blur_pixels": (_i32, [_vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_dof_device": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_dof": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_pass_dof": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp]),
    "arctic_read_dof": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_dof_info": (_i32, [_vp, _vp]),
    "arctic_dof_prepare": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_dof_pixels": (_i32, [_vp, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_dof_coc_scale": (_i32, [C.c_float, C.c_float, C.c_float, C.c_float, _u32, _vp]),
    "arctic_dof_focus_at": (_i32, [_vp, C.c_float, C.c_float, _u32, _u32, _vp]),
    "arctic_bloom_device": (_i32, [_vp, _settings, _vp, _vp, _vp]),
    "arctic_bloom": (_i32, [_vp, _settings, _vp, _vp, _vp]),
    "arctic_read_bloom": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_bloom_info": (_i32, [_vp, _vp]),
    "arctic_bloom_layout": (_i32, [_u32, _u32, _u32, _vp]),
    "arctic_bloom_pyramid": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "arctic_bloom_pixels": (_i32, [_vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp]),
    "arctic_exposure_device": (_i32, [_vp, _settings, _vp, _vp, _vp]),
    "arctic_exposure": (_i32, [_vp, _settings, _vp, _vp, _vp]),
    "arctic_read_exposure": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_exposure_reset": (_i32, [_vp]),
    "arctic_exposure_info": (_i32, [_vp, _vp]),
    "arctic_exposure_layout": (_i32, [_u32, _u32, _vp]),
    "arctic_exposure_rate": (C.c_float, [C.c_float, C.c_float]),
    "arctic_exposure_histogram": (_i32, [_vp, _u32, _u32, _vp, _vp]),
    "arctic_exposure_resolve": (_i32, [_vp, _vp, _vp, _vp]),
    "arctic_exposure_pixels": (_i32, [_u64, _vp, C.c_float, _vp]),
    "arctic_fog_view": (_i32, [_scene, _u32, _u32, _vp]),
    "arctic_fog_device": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_fog": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_pass_fog": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp]),
    "arctic_read_fog": (_i32, [_vp, _vp, _vp, _vp]),
    "arctic_fog_info": (_i32, [_vp, _vp]),
    "arctic_fog_pixels": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "arctic_fog_exp2": (C.c_float, [C.c_float]),
    "arctic_fog_exp2_poly": (_i32, [_u64, _vp, _vp]),
    "arctic_taa_upscale_device": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp]),
    "arctic_taa_upscale": (_i32, [_vp, _settings, _vp, _vp, _vp, _vp]),
    "arctic_pass_taa_upscale": (_i32, [_vp, _scene, _settings, _vp, _vp]),
    "arctic_taa_upscale_reset": (_i32, [_vp]),
    "arctic_read_taa_upscale": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "arctic_taa_upscale_hdr_device": (_i32, [_vp, _vp]),
    "arctic_taa_upscale_info": (_i32, [_vp, _vp]),
    "arctic_taa_upscale_pixels": (_i32, [_vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_taa_upscale_jitter": (_i32, [_u32, _u32, _u32, _u32, _u32, _vp]),
    "arctic_trace_gi": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_trace_gi_device": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_gi_rays": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "arctic_read_gi_estimate": (_i32, [_vp, _vp, _vp]),
    "arctic_gi_info": (_i32, [_vp, _vp]),
    "arctic_accumulate_gi_device": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_accumulate_gi": (_i32, [_vp, _scene, _vp, _vp, _vp]),
    "arctic_gi_history_reset": (_i32, [_vp]),
    "arctic_read_gi_history": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "arctic_gi_compose_device": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_read_gi": (_i32, [_vp, _vp, _vp, _vp]),
    "arctic_pass_gi": (_i32, [_vp, _scene, _settings, _vp, _vp, _vp, _vp, _vp]),
    "arctic_gi_accumulate_pixels": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_gi_compose_pixels": (_i32, [_vp, C.c_float, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_gi_points": (_i32, [_vp, _vp, _u64, _vp, _vp, _u32, _vp]),
    "arctic_gi_estimate_pixels": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "arctic_version": (_i32, []),
    # include/arctic_dist.h: the multi-GPU exchange steps
    "arctic_comm_unique_id": (_i32, [_vp, _vp, _u64]),
    "arctic_comm_init": (_i32, [_vp, _vp, _i32, _i32]),
    "arctic_comm_destroy": (_i32, [_vp]),
    "arctic_gather_frame": (_i32, [_vp, _vp, _vp, _i32]),
    "arctic_assemble_frame": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    # ... and their plan as pure host functions (no device needed)
    "arctic_exchange_plan": (_i32, [_u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "arctic_exchange_row_source": (_i32, [_u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "arctic_exchange_transfers": (_i32, [_u32, _u32, _i32, _i32, _vp, _vp, _vp, _u32]),
}


class CTransfer(C.Structure):
    """ArcticTransfer (include/arctic_dist.h)"""
    _fields_ = [("peer", C.c_int32), ("is_send", C.c_int32), ("staging_offset", C.c_uint64), ("bytes", C.c_uint64)]


def header_symbols():
    """names of every function include/arctic_hip.h and include/arctic_dist.h declare."""
    text = open(HEADER_PATH).read() + open(os.path.join(os.path.dirname(HEADER_PATH), "arctic_dist.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(arctic_[a-z0-9_]+)\s*\(", text)))


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as e; e.build()'` "
                               f"(make -C arctic-renderer_amd/csrc). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        missing = [n for n in header_symbols() if not hasattr(L, n)]
        older = os.environ.get("ARCTIC_HIP_LIBRARY_OLDER") == "1"   # A/B tools only: an earlier round's build, which lacks this round's entry points
        if missing and not older:
            raise RuntimeError(f"libarctic_hip.so does not export {missing}")
        for name, (res, args) in SIGNATURES.items():
            if older and name in missing:
                continue
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib
