"""ctypes binding of the glTF scene-loader stand-in (include/arctic_gltf.h, host/gltf_loader.cpp): what App::load_scene
(reference src/app.cpp:173-385) produces for a glTF file -- materials, meshes, objects -- as numpy arrays, ready for any
object with the Renderer surface (the HIP binding or the CPU oracle).  Host-side data loading only."""
import ctypes as C
import os
import subprocess

import numpy as np

from .scene import LIGHT_DTYPE, MATERIAL_PARAMS_DTYPE, MORPH_DELTA_DTYPE, OBJECT_DTYPE, SKIN_VERTEX_DTYPE, SPOT_LIGHT_DTYPE, VERTEX_DTYPE, neutral_material_params

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "host", "libarctic_gltf.so")
_lib = None


def build(force=False):
    src = os.path.join(HERE, "host", "gltf_loader.cpp")
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", os.path.join(HERE, "host"), "libarctic_gltf.so"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built: run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        vp, u64, u32p, u64p = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.arctic_gltf_load.restype, L.arctic_gltf_load.argtypes = vp, [C.c_char_p, C.c_char_p, u64]
        L.arctic_gltf_free.restype, L.arctic_gltf_free.argtypes = None, [vp]
        for f in ("arctic_gltf_material_count", "arctic_gltf_mesh_count", "arctic_gltf_object_count"):
            getattr(L, f).restype, getattr(L, f).argtypes = u64, [vp]
        L.arctic_gltf_material_image.restype = C.c_int
        L.arctic_gltf_material_image.argtypes = [vp, u64, C.c_int, C.POINTER(vp), u32p, u32p]
        L.arctic_gltf_material_params.restype, L.arctic_gltf_material_params.argtypes = C.c_int, [vp, u64, vp]
        L.arctic_gltf_mesh.restype = C.c_int
        L.arctic_gltf_mesh.argtypes = [vp, u64, C.POINTER(vp), u64p, C.POINTER(vp), u64p, u64p]
        L.arctic_gltf_objects.restype, L.arctic_gltf_objects.argtypes = vp, [vp]
        L.arctic_gltf_upload.restype, L.arctic_gltf_upload.argtypes = C.c_int, [vp, vp]
        for f in ("arctic_gltf_spot_lights", "arctic_gltf_point_lights"):
            getattr(L, f).restype, getattr(L, f).argtypes = vp, [vp, u64p]
        L.arctic_gltf_directional_light_count.restype, L.arctic_gltf_directional_light_count.argtypes = u64, [vp]
        for f in ("arctic_gltf_skin_count", "arctic_gltf_animation_count"):
            getattr(L, f).restype, getattr(L, f).argtypes = u64, [vp]
        L.arctic_gltf_skin_joint_count.restype, L.arctic_gltf_skin_joint_count.argtypes = u64, [vp, u64]
        L.arctic_gltf_animation_duration.restype, L.arctic_gltf_animation_duration.argtypes = C.c_double, [vp, u64]
        L.arctic_gltf_mesh_skin.restype = C.c_int
        L.arctic_gltf_mesh_skin.argtypes = [vp, u64, C.POINTER(vp), u64p, C.POINTER(C.c_int64), u32p]
        L.arctic_gltf_pose.restype, L.arctic_gltf_pose.argtypes = C.c_int, [vp, u64, C.c_int64, C.c_double, vp]
        L.arctic_gltf_mesh_morph.restype, L.arctic_gltf_mesh_morph.argtypes = C.c_int, [vp, u64, C.POINTER(vp), u64p, u32p]
        L.arctic_gltf_morph_weights.restype, L.arctic_gltf_morph_weights.argtypes = C.c_int, [vp, u64, C.c_int64, C.c_double, vp]
        L.arctic_gltf_last_error.restype, L.arctic_gltf_last_error.argtypes = C.c_char_p, [vp]
        L.arctic_png_decode.restype = vp
        L.arctic_png_decode.argtypes = [C.c_char_p, u64, u32p, u32p, C.c_char_p, u64]
        L.arctic_png_free.restype, L.arctic_png_free.argtypes = None, [vp]
        _lib = L
    return _lib


class GltfScene:
    """materials: list of (diffuse, normal, metal_rough) uint8 (h, w, 4); meshes: list of (vertices, indices, material);
    objects: OBJECT_DTYPE array -- the same three things scenes.SyntheticScene carries.  The file's KHR_lights_punctual lights:
    spot_lights (SPOT_LIGHT_DTYPE, for Renderer.update_spot_lights), point_lights (LIGHT_DTYPE, for update_lights),
    directional_lights (a count; include/arctic_gltf.h).  upload() uploads no lights.
    The glTF material model beyond the three images: material_params (MATERIAL_PARAMS_DTYPE, one record per material), emissive_images and
    occlusion_images (one entry per material: (h, w, 4) uint8 or None).  upload(material_model="gltf") applies them.
    Skins and animations: mesh_skins (one entry per mesh: None, or (SKIN_VERTEX_DTYPE records, skin index, joint count)), skin_joint_counts,
    animation_durations (seconds, one per animation).  joint_matrices() evaluates a pose, pose() hands it to a renderer.
    Morph targets: mesh_morphs (one entry per mesh: None, or (n_targets, n_vertices) MORPH_DELTA_DTYPE records as
    Renderer.set_mesh_morph_targets takes them); morph_weights() evaluates a mesh's weights, pose() sets them too."""

    def __init__(self, materials, meshes, objects, spot_lights=None, point_lights=None, directional_lights=0, material_params=None,
                 emissive_images=None, occlusion_images=None):
        self.materials, self.meshes, self.objects = materials, meshes, objects
        self.material_params = neutral_material_params(len(materials)) if material_params is None else material_params
        self.emissive_images = [None] * len(materials) if emissive_images is None else emissive_images
        self.occlusion_images = [None] * len(materials) if occlusion_images is None else occlusion_images
        self.spot_lights = np.zeros(0, SPOT_LIGHT_DTYPE) if spot_lights is None else spot_lights
        self.point_lights = np.zeros(0, LIGHT_DTYPE) if point_lights is None else point_lights
        self.directional_lights = directional_lights
        self.mesh_skins = [None] * len(meshes)
        self.mesh_morphs = [None] * len(meshes)
        self.skin_joint_counts, self.animation_durations = [], []
        self._handle = None       # the loader's handle, kept while the scene has skins to pose
        self._skinned = {}        # id(renderer) -> first_mesh its skins and morph targets were attached at

    def __del__(self):
        if getattr(self, "_handle", None):
            lib().arctic_gltf_free(self._handle)
            self._handle = None

    def joint_matrices(self, skin, animation=-1, time=0.0):
        """(n_joints, 16) float32 for Renderer.set_mesh_pose: inverse(global(mesh node)) . global(joint) . inverseBind of the file's skin
        `skin` under animation `animation` (-1: the rest pose) at `time` seconds (clamped to each sampler's range); computed in binary64 and
        rounded once (include/arctic_gltf.h: arctic_gltf_pose).  Raises ValueError with the loader's message, e.g. for a CUBICSPLINE sampler."""
        if not self._handle or not 0 <= skin < len(self.skin_joint_counts):
            raise ValueError(f"joint_matrices: the scene has no skin {skin}")
        out = np.empty((self.skin_joint_counts[skin], 16), np.float32)
        L = lib()
        if L.arctic_gltf_pose(self._handle, int(skin), int(animation), float(time), out.ctypes.data) != 0:
            raise ValueError(L.arctic_gltf_last_error(self._handle).decode())
        return out

    def morph_weights(self, mesh, animation=-1, time=0.0):
        """(n_targets,) float32 for Renderer.set_mesh_morph_weights: the weights of loader mesh `mesh` under animation `animation` (-1: the
        file's defaults -- node.weights, else mesh.weights, else zeros) at `time` seconds (clamped to the sampler's range); a + (b - a) u in
        binary64, rounded once (include/arctic_gltf.h: arctic_gltf_morph_weights).  Raises ValueError with the loader's message."""
        if not self._handle or not 0 <= mesh < len(self.mesh_morphs) or self.mesh_morphs[mesh] is None:
            raise ValueError(f"morph_weights: mesh {mesh} has no morph targets")
        out = np.empty(len(self.mesh_morphs[mesh]), np.float32)
        L = lib()
        if L.arctic_gltf_morph_weights(self._handle, int(mesh), int(animation), float(time), out.ctypes.data) != 0:
            raise ValueError(L.arctic_gltf_last_error(self._handle).decode())
        return out

    def pose(self, renderer, animation=-1, time=0.0, first_mesh=0):
        """pose every skinned mesh and set the weights of every morphed mesh of the scene on `renderer` (an object with set_mesh_skin /
        set_mesh_pose / set_mesh_morph_targets / set_mesh_morph_weights, after upload()): attaches the skins and the morph targets the first
        time it is called for that renderer, then sets each mesh's weights and pose.  first_mesh: the index upload()'s first create_mesh
        returned (0 for a renderer that held no meshes)."""
        used = sorted({ms[1] for ms in self.mesh_skins if ms is not None})
        poses = {k: self.joint_matrices(k, animation, time) for k in used}     # (evaluated first: a refused animation changes nothing)
        weights = {i: self.morph_weights(i, animation, time) for i, mm in enumerate(self.mesh_morphs) if mm is not None}
        if self._skinned.get(id(renderer)) != first_mesh:
            for i, ms in enumerate(self.mesh_skins):
                if ms is not None:
                    renderer.set_mesh_skin(first_mesh + i, ms[0], ms[2])
            for i, mm in enumerate(self.mesh_morphs):
                if mm is not None:
                    renderer.set_mesh_morph_targets(first_mesh + i, mm)
            self._skinned[id(renderer)] = first_mesh
        for i, w in weights.items():
            renderer.set_mesh_morph_weights(first_mesh + i, w)
        for i, ms in enumerate(self.mesh_skins):
            if ms is not None:
                renderer.set_mesh_pose(first_mesh + i, poses[ms[1]])
        return renderer

    def upload(self, renderer, material_model="reference"):
        """material_model "reference": the three images alone, what the reference's load_scene uploads.  "gltf": also the factors, emissive and
        occlusion of every material that is not neutral (Renderer.set_material_extras)."""
        if material_model not in ("reference", "gltf"):
            raise ValueError(f"material_model {material_model!r}: 'reference' or 'gltf'")
        neutral = neutral_material_params()[0]
        for k, (d, n, m) in enumerate(self.materials):
            i = renderer.create_material(d, n, m)
            if material_model == "gltf" and (self.material_params[k].tobytes() != neutral.tobytes() or self.emissive_images[k] is not None or self.occlusion_images[k] is not None):
                renderer.set_material_extras(i, self.material_params[k], self.emissive_images[k], self.occlusion_images[k])
        for v, i, mat in self.meshes:
            renderer.create_mesh(v, i, mat)
        return renderer


def load(path):
    L = lib()
    err = C.create_string_buffer(512)
    h = L.arctic_gltf_load(os.fsencode(path), err, 512)
    if not h:
        raise ValueError(err.value.decode())
    try:
        materials, emissive, occlusion = [], [], []
        params = np.zeros(L.arctic_gltf_material_count(h), MATERIAL_PARAMS_DTYPE)
        for i in range(L.arctic_gltf_material_count(h)):
            imgs = []
            for k in range(5):
                p, w, hh = C.c_void_p(), C.c_uint32(), C.c_uint32()
                assert L.arctic_gltf_material_image(h, i, k, C.byref(p), C.byref(w), C.byref(hh)) == 0
                imgs.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (hh.value, w.value, 4)).copy() if p.value else None)
            materials.append(tuple(imgs[:3]))
            emissive.append(imgs[3]); occlusion.append(imgs[4])
            assert L.arctic_gltf_material_params(h, i, params[i:i + 1].ctypes.data) == 0
        meshes = []
        for i in range(L.arctic_gltf_mesh_count(h)):
            pv, pi, nv, ni, mat = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            assert L.arctic_gltf_mesh(h, i, C.byref(pv), C.byref(nv), C.byref(pi), C.byref(ni), C.byref(mat)) == 0
            v = np.frombuffer(C.string_at(pv, nv.value * VERTEX_DTYPE.itemsize), dtype=VERTEX_DTYPE).copy()
            ix = np.frombuffer(C.string_at(pi, ni.value * 4), dtype=np.uint32).copy()
            meshes.append((v, ix, int(mat.value)))
        n_obj = L.arctic_gltf_object_count(h)
        objects = (np.frombuffer(C.string_at(L.arctic_gltf_objects(h), n_obj * OBJECT_DTYPE.itemsize), dtype=OBJECT_DTYPE).copy()
                   if n_obj else np.zeros(0, OBJECT_DTYPE))
        def lights(fn, dtype):
            n = C.c_uint64()
            p = fn(h, C.byref(n))
            return np.frombuffer(C.string_at(p, n.value * dtype.itemsize), dtype=dtype).copy() if n.value else np.zeros(0, dtype)
        scene = GltfScene(materials, meshes, objects, lights(L.arctic_gltf_spot_lights, SPOT_LIGHT_DTYPE),
                          lights(L.arctic_gltf_point_lights, LIGHT_DTYPE), int(L.arctic_gltf_directional_light_count(h)),
                          material_params=params, emissive_images=emissive, occlusion_images=occlusion)
        for i in range(len(meshes)):
            ps, nv, si, nj = C.c_void_p(), C.c_uint64(), C.c_int64(), C.c_uint32()
            assert L.arctic_gltf_mesh_skin(h, i, C.byref(ps), C.byref(nv), C.byref(si), C.byref(nj)) == 0
            if si.value >= 0:
                scene.mesh_skins[i] = (np.frombuffer(C.string_at(ps, nv.value * SKIN_VERTEX_DTYPE.itemsize), dtype=SKIN_VERTEX_DTYPE).copy(), int(si.value), int(nj.value))
            pd, nt = C.c_void_p(), C.c_uint32()
            assert L.arctic_gltf_mesh_morph(h, i, C.byref(pd), C.byref(nv), C.byref(nt)) == 0
            if nt.value:
                scene.mesh_morphs[i] = np.frombuffer(C.string_at(pd, nt.value * nv.value * MORPH_DELTA_DTYPE.itemsize), dtype=MORPH_DELTA_DTYPE).reshape(nt.value, nv.value).copy()
        scene.skin_joint_counts = [int(L.arctic_gltf_skin_joint_count(h, k)) for k in range(L.arctic_gltf_skin_count(h))]
        scene.animation_durations = [float(L.arctic_gltf_animation_duration(h, k)) for k in range(L.arctic_gltf_animation_count(h))]
        if scene.skin_joint_counts or any(mm is not None for mm in scene.mesh_morphs):      # arctic_gltf_pose / arctic_gltf_morph_weights need the loader's handle: the scene owns it from here on
            scene._handle, h = h, None
        return scene
    finally:
        if h:
            L.arctic_gltf_free(h)


def png_decode(data):
    L = lib()
    w, h, err = C.c_uint32(), C.c_uint32(), C.create_string_buffer(256)
    p = L.arctic_png_decode(data, len(data), C.byref(w), C.byref(h), err, 256)
    if not p:
        raise ValueError(err.value.decode())
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h.value, w.value, 4)).copy()
    finally:
        L.arctic_png_free(p)
