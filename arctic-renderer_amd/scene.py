"""POD scene types of the boundary, as numpy dtypes + ctypes structs.

Byte-compatible with include/arctic_hip.h, i.e. with the reference's
src/renderer/scene.hpp:20-110 (Camera, Vertex, Object, DirectionalLight,
PointLight, Scene, Settings).  Pure host-side data description: nothing here
computes anything on the hot path.
"""
import ctypes as C

import numpy as np

# scene.hpp:40-47 Vertex (56 B)
VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3),
                         ("bitangent", "<f4", 3), ("tex_coords", "<f4", 2)])
# scene.hpp:69-73 Object {mat4 trs (glm column-major); size_t mesh_idx}
OBJECT_DTYPE = np.dtype([("trs", "<f4", 16), ("mesh_idx", "<u8")])
# scene.hpp:88-94 PointLight (32 B)
LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("padding0", "<u4"), ("color", "<f4", 3), ("padding1", "<u4")])
# ArcticSpotLight (include/arctic_hip.h): 48 bytes, no padding
SPOT_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("range", "<f4"), ("direction", "<f4", 3), ("inner_cone_angle", "<f4"),
                             ("color", "<f4", 3), ("outer_cone_angle", "<f4")])
# ArcticPointShadowLight (include/arctic_hip.h): 32 bytes, no padding
POINT_SHADOW_LIGHT_DTYPE = np.dtype([("position", "<f4", 3), ("z_near", "<f4"), ("color", "<f4", 3), ("z_far", "<f4")])
assert VERTEX_DTYPE.itemsize == 56 and OBJECT_DTYPE.itemsize == 72 and LIGHT_DTYPE.itemsize == 32 and SPOT_LIGHT_DTYPE.itemsize == 48
assert POINT_SHADOW_LIGHT_DTYPE.itemsize == 32
# ArcticMaterialParams (include/arctic_hip.h): 48 bytes, the glTF material factors of Renderer.set_material_extras
MATERIAL_PARAMS_DTYPE = np.dtype([("base_color_factor", "<f4", 3), ("metallic_factor", "<f4"), ("roughness_factor", "<f4"), ("normal_scale", "<f4"),
                                  ("occlusion_strength", "<f4"), ("emissive_factor", "<f4", 3), ("reserved", "<f4", 2)])
assert MATERIAL_PARAMS_DTYPE.itemsize == 48
# ArcticSkinVertex (include/arctic_hip.h): 24 bytes, the per-vertex joints and weights of Renderer.set_mesh_skin
SKIN_VERTEX_DTYPE = np.dtype([("joints", "<u2", 4), ("weights", "<f4", 4)])
assert SKIN_VERTEX_DTYPE.itemsize == 24
# ArcticMorphDelta (include/arctic_hip.h): 48 bytes, one per vertex per morph target of Renderer.set_mesh_morph_targets
MORPH_DELTA_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("bitangent", "<f4", 3)])
assert MORPH_DELTA_DTYPE.itemsize == 48
# ArcticRay, ArcticHit (include/arctic_hip.h): 32 and 16 bytes, the records of Renderer.trace_rays
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("direction", "<f4", 3), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 16
# ArcticAmbientOcclusion (include/arctic_hip.h)
AO_DTYPE = np.dtype([("n_rays", "<u4"), ("pattern", "<u4"), ("radius", "<f4"), ("bias", "<f4"), ("filter", "<u4"), ("normal_cos", "<f4"), ("plane_dist", "<f4"), ("reserved", "<u4")])
assert AO_DTYPE.itemsize == 32
# ArcticGi (include/arctic_hip.h)
GI_DTYPE = np.dtype([("n_rays", "<u4"), ("pattern", "<u4"), ("max_distance", "<f4"), ("bias", "<f4"), ("clamp_max", "<f4"), ("filter", "<u4"), ("normal_cos", "<f4"), ("plane_dist", "<f4"),
                     ("reserved", "<u4", 4)])
assert GI_DTYPE.itemsize == 48
# ArcticGiHistory (ArcticAoHistory's fields) and ArcticGiCompose
GI_HISTORY_DTYPE = np.dtype([("max_history", "<f4"), ("normal_cos", "<f4"), ("plane_dist", "<f4"), ("min_weight", "<f4"), ("reserved", "<u4", 4)])
GI_COMPOSE_DTYPE = np.dtype([("flags", "<u4"), ("gi_strength", "<f4"), ("ambient_scale", "<f4"), ("reserved", "<u4", 5)])
assert GI_HISTORY_DTYPE.itemsize == 32 and GI_COMPOSE_DTYPE.itemsize == 32
# ArcticRayCompose (include/arctic_hip.h)
COMPOSE_DTYPE = np.dtype([("flags", "<u4"), ("ao_strength", "<f4"), ("reflection_strength", "<f4"), ("reflection_bias", "<f4"), ("reserved", "<u4", 4)])
assert COMPOSE_DTYPE.itemsize == 32
# ArcticAoHistory (include/arctic_hip.h)
AO_HISTORY_DTYPE = np.dtype([("max_history", "<f4"), ("normal_cos", "<f4"), ("plane_dist", "<f4"), ("min_weight", "<f4"), ("reserved", "<u4", 4)])
assert AO_HISTORY_DTYPE.itemsize == 32
# ArcticTaa: the parameters of the temporal anti-aliasing resolve (arctic_taa_resolve_device)
TAA_DTYPE = np.dtype([("flags", "<u4"), ("max_history", "<f4"), ("min_weight", "<f4"), ("jitter", "<f4", 2), ("reserved", "<u4", 3)])
assert TAA_DTYPE.itemsize == 32
# ArcticTaaUpscale: the parameters of the temporal upscaler (arctic_taa_upscale_device)
TAA_UPSCALE_DTYPE = np.dtype([("flags", "<u4"), ("max_history", "<f4"), ("min_weight", "<f4"), ("jitter", "<f4", 2), ("sharpness", "<f4"), ("confidence_floor", "<f4"),
                              ("out_width", "<u4"), ("out_height", "<u4"), ("reserved", "<u4", 3)])
assert TAA_UPSCALE_DTYPE.itemsize == 48
# ArcticMotionBlur: the parameters of the motion blur (arctic_motion_blur_device)
MOTION_BLUR_DTYPE = np.dtype([("flags", "<u4"), ("shutter", "<f4"), ("max_radius", "<f4"), ("samples", "<u4"), ("depth_extent", "<f4"), ("reserved", "<u4", 3)])
assert MOTION_BLUR_DTYPE.itemsize == 32
# ArcticDof: the parameters of depth of field (arctic_dof_device)
DOF_DTYPE = np.dtype([("flags", "<u4"), ("focus_distance", "<f4"), ("coc_scale", "<f4"), ("max_radius", "<f4"), ("samples", "<u4"), ("depth_extent", "<f4"), ("z_near", "<f4"), ("z_far", "<f4")])
assert DOF_DTYPE.itemsize == 32
# ArcticBloom: the parameters of bloom (arctic_bloom_device)
BLOOM_DTYPE = np.dtype([("flags", "<u4"), ("threshold", "<f4"), ("soft_knee", "<f4"), ("clamp_max", "<f4"), ("intensity", "<f4"), ("spread", "<f4"), ("levels", "<u4"), ("reserved", "<u4")])
assert BLOOM_DTYPE.itemsize == 32
# ArcticExposure: the parameters of auto-exposure (arctic_exposure_device), and ArcticExposureState: what it keeps on the device
EXPOSURE_DTYPE = np.dtype([("flags", "<u4"), ("low_q16", "<u4"), ("high_q16", "<u4"), ("key_value", "<f4"), ("min_exposure", "<f4"), ("max_exposure", "<f4"), ("rate_up", "<f4"),
                           ("rate_down", "<f4"), ("fallback_exposure", "<f4"), ("window", "<u4", 4), ("reserved", "<u4")])
assert EXPOSURE_DTYPE.itemsize == 56
EXPOSURE_STATE_DTYPE = np.dtype([("adapted_key", "<f8"), ("exposure", "<f4"), ("luminance", "<f4"), ("metered", "<u4"), ("valid", "<u4"), ("frames", "<u4"), ("reserved", "<u4")])
assert EXPOSURE_STATE_DTYPE.itemsize == 32
# ArcticFog: the parameters of volumetric fog (arctic_fog_device), and ArcticFogView: the camera's rays and the sun's map per frame (arctic_fog_view)
FOG_DTYPE = np.dtype([("flags", "<u4"), ("density", "<f4"), ("anisotropy", "<f4"), ("max_distance", "<f4"), ("steps", "<u4"), ("bias", "<f4"), ("scatter_color", "<f4", 3),
                      ("ambient_color", "<f4", 3), ("reserved", "<u4")])
assert FOG_DTYPE.itemsize == 52
FOG_VIEW_DTYPE = np.dtype([("eye", "<f4", 3), ("z_near", "<f4"), ("ray00", "<f4", 3), ("z_far", "<f4"), ("ray_dx", "<f4", 3), ("pad0", "<f4"), ("ray_dy", "<f4", 3), ("pad1", "<f4"),
                           ("sun_dir", "<f4", 3), ("pad2", "<f4"), ("light", "<f4", (3, 4))])
assert FOG_VIEW_DTYPE.itemsize == 128
# ArcticRayNode / ArcticRayTri: the ray structure's records as arctic_read_ray_structure and arctic_refit_triangles return them
RAY_NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("skip", "<u4"), ("bmax", "<f4", 3), ("leaf", "<u4")])
RAY_TRI_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("p2", "<f4", 3), ("prim", "<u4"), ("pad", "<u4", 2)])
assert RAY_NODE_DTYPE.itemsize == 32 and RAY_TRI_DTYPE.itemsize == 48


def neutral_material_params(n=1):
    """n records that change nothing: factors 1, normal scale 1, occlusion strength 1, no emission"""
    a = np.zeros(n, MATERIAL_PARAMS_DTYPE)
    a["base_color_factor"], a["metallic_factor"], a["roughness_factor"], a["normal_scale"], a["occlusion_strength"] = 1, 1, 1, 1, 1
    return a


def make_rays(origins, directions, t_min=0.0, t_max=np.inf):
    """n RAY_DTYPE records from (n, 3) origins and directions; t_min / t_max scalars or (n,) arrays"""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    out = np.zeros(len(o), RAY_DTYPE)
    out["origin"], out["direction"], out["t_min"], out["t_max"] = o, np.asarray(directions, np.float32).reshape(-1, 3), t_min, t_max
    return out


TM_REINHARD, TM_EXPOSURE, TM_ACES = 0, 1, 2


class CCamera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("rotation", C.c_float * 2), ("aspect", C.c_float),
                ("fov_y", C.c_float), ("z_near_far", C.c_float * 2)]


class CDirectionalLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rotation", C.c_float * 2), ("color", C.c_float * 3)]


class CScene(C.Structure):
    _fields_ = [("camera", CCamera), ("ambient", C.c_float), ("sun", CDirectionalLight),
                ("point_lights", C.c_void_p), ("n_point_lights", C.c_uint64),
                ("objects", C.c_void_p), ("n_objects", C.c_uint64)]


class CSettings(C.Structure):
    _fields_ = [("tm_method", C.c_int32), ("gamma", C.c_float), ("exposure", C.c_float)]


class CCreateInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("shadow_size", C.c_uint32),
                ("max_lights", C.c_uint32), ("device", C.c_int32), ("row_begin", C.c_uint32),
                ("row_end", C.c_uint32), ("band_rows", C.c_uint32), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32)]


class SceneDesc:
    """Scene (scene.hpp:96-103) on the Python side: owns the numpy arrays the C
    struct points into and fills any ctypes struct of the Scene layout."""

    def __init__(self, camera, ambient, sun, objects, point_lights=None):
        # camera = dict(eye, rotation, aspect, fov_y, z_near_far); sun = dict(position, rotation, color)
        self.camera, self.ambient, self.sun = dict(camera), float(ambient), dict(sun)
        self.objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        self.point_lights = (np.zeros(0, LIGHT_DTYPE) if point_lights is None
                             else np.ascontiguousarray(point_lights, dtype=LIGHT_DTYPE))

    def fill(self, s):
        s.camera.eye[:] = [float(x) for x in self.camera["eye"]]
        s.camera.rotation[:] = [float(x) for x in self.camera["rotation"]]
        s.camera.aspect = float(self.camera["aspect"])
        s.camera.fov_y = float(self.camera["fov_y"])
        s.camera.z_near_far[:] = [float(x) for x in self.camera["z_near_far"]]
        s.ambient = self.ambient
        s.sun.position[:] = [float(x) for x in self.sun["position"]]
        s.sun.rotation[:] = [float(x) for x in self.sun["rotation"]]
        s.sun.color[:] = [float(x) for x in self.sun["color"]]
        s.point_lights = self.point_lights.ctypes.data if len(self.point_lights) else None
        s.n_point_lights = len(self.point_lights)
        s.objects = self.objects.ctypes.data if len(self.objects) else None
        s.n_objects = len(self.objects)
        return s


def make_objects(items):
    """items: iterable of (trs 4x4 in math (row, col) convention or flat glm order, mesh_idx)."""
    out = np.zeros(len(items), OBJECT_DTYPE)
    for i, (trs, mesh) in enumerate(items):
        t = np.asarray(trs, np.float32)
        # a 4x4 given as math matrix M[row][col] is stored column-major like glm
        out[i]["trs"] = t.T.reshape(16) if t.shape == (4, 4) else t.reshape(16)
        out[i]["mesh_idx"] = mesh
    return out


def make_lights(positions, colors):
    positions, colors = np.asarray(positions, np.float32), np.asarray(colors, np.float32)
    out = np.zeros(len(positions), LIGHT_DTYPE)
    if len(positions):
        out["position"], out["color"] = positions, colors
    return out


def translation(x, y, z):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (x, y, z)
    return m


def scaling(x, y, z):
    return np.diag(np.array([x, y, z, 1], np.float32))


def rotation_y(deg):
    a = np.float32(np.deg2rad(deg))
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m
