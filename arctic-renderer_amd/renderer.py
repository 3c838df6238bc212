"""Renderer: Python host-side mirror of Arctic::Renderer::Renderer over the C-ABI.

Same method names, argument meaning and error behaviour as the reference class
(src/renderer/renderer.hpp:100-125): init-at-construction, create_material,
create_mesh, create_hdri, update_lights, render_frame, resize, flush, cleanup.
The reference returns bool and logs; here a failed call raises ArcticError
carrying the C-ABI code and arctic_last_error().  All compute happens in
csrc/libarctic_hip.so (HIP, gfx950); numpy arrays are only the host buffers.
"""
import ctypes as C

import numpy as np

from . import binding
from .scene import (AO_DTYPE, AO_HISTORY_DTYPE, GI_DTYPE, GI_HISTORY_DTYPE, GI_COMPOSE_DTYPE, COMPOSE_DTYPE, HIT_DTYPE, RAY_DTYPE, RAY_NODE_DTYPE, RAY_TRI_DTYPE, LIGHT_DTYPE, MATERIAL_PARAMS_DTYPE, MORPH_DELTA_DTYPE, POINT_SHADOW_LIGHT_DTYPE, SKIN_VERTEX_DTYPE, SPOT_LIGHT_DTYPE, TAA_DTYPE, TAA_UPSCALE_DTYPE, MOTION_BLUR_DTYPE, DOF_DTYPE, BLOOM_DTYPE, EXPOSURE_DTYPE, EXPOSURE_STATE_DTYPE, FOG_DTYPE, FOG_VIEW_DTYPE, VERTEX_DTYPE, CCreateInfo, CScene, CSettings)


class ArcticError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"{binding.ERRORS.get(code, code)}: {message}")
        self.code = code


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Renderer:
    def __init__(self, width, height, shadow_size=4000, max_lights=16, device=0, row_begin=0, row_end=0, band_rows=0,
                 shard=(0, 1)):
        """Renderer(window, w, h) + init() (renderer.hpp:94-100); no window.  shadow_size defaults to
        ShadowMapPass::SIZE (shadow_map_pass.hpp:23), max_lights to MAX_NUM_POINT_LIGHTS (renderer.hpp:22)."""
        self.L = binding.lib()
        info = CCreateInfo(width, height, shadow_size, max_lights, device, row_begin, row_end, band_rows, shard[0], shard[1])
        err = C.create_string_buffer(512)
        self.h = self.L.arctic_create(C.byref(info), err, 512)
        if not self.h:
            raise ArcticError(-3 if b"no HIP device" in err.value else -2, err.value.decode())
        self.width, self.height, self.shadow_size, self.max_lights, self.device = width, height, shadow_size, max_lights, device
        self.row_begin, self.row_end = (row_begin, row_end) if row_end else (0, height)
        self.band_rows, self.shard = band_rows, shard
        self._options = {}   # what set_option set (read_point_shadow's shape follows "point_shadow_size")

    # ---- helpers -------------------------------------------------------------------------------
    @property
    def rows(self):
        if self.band_rows:
            from .sharding import owned_rows
            return len(owned_rows(self.height, self.shard[0], self.shard[1], self.band_rows))
        return self.row_end - self.row_begin

    def _check(self, rc):
        if rc < 0:
            raise ArcticError(rc, self.L.arctic_last_error(self.h).decode())
        return rc

    @staticmethod
    def _scene(desc):
        return desc.fill(CScene())

    @staticmethod
    def _settings(settings):
        tm, gamma, exposure = settings
        return CSettings(int(tm), float(gamma), float(exposure))

    # ---- the reference surface -------------------------------------------------------------------
    def cleanup(self):
        if getattr(self, "h", None):
            self.L.arctic_destroy(self.h)
            self.h = None

    close = cleanup

    def __del__(self):
        self.cleanup()

    def resize(self, width, height):
        self._check(self.L.arctic_resize(self.h, width, height))
        self.width, self.height, self.row_begin, self.row_end = width, height, 0, height
        self.band_rows, self.shard = 0, (0, 1)

    def flush(self):
        self._check(self.L.arctic_flush(self.h))

    def set_stream(self, hip_stream):
        """enqueue everything on a caller-owned HIP stream given as an int handle, e.g. torch.cuda.current_stream().cuda_stream
        (0 = HIP's default stream, which is what torch normally runs on); None returns to the handle's private stream."""
        if hip_stream is None:
            self._check(self.L.arctic_use_own_stream(self.h))
        else:
            self._check(self.L.arctic_set_stream(self.h, C.c_void_p(hip_stream)))

    # ---- multi-GPU exchange steps (include/arctic_dist.h) -----------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId: one process calls it, every rank of the communicator gets the bytes."""
        L = binding.lib()
        buf, err = C.create_string_buffer(128), C.create_string_buffer(512)
        rc = L.arctic_comm_unique_id(buf, err, 512)
        if rc != 0:
            raise ArcticError(rc, err.value.decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """collective: an RCCL communicator of `world` ranks owned by this handle (ncclCommInitRank) + the shard layouts."""
        assert len(unique_id) == 128
        self._check(self.L.arctic_comm_init(self.h, C.c_char_p(unique_id), rank, world))

    def comm_destroy(self):
        self._check(self.L.arctic_comm_destroy(self.h))

    def gather_frame(self, d_shard_ptr, d_frame_ptr, root=0):
        """collective, asynchronous: this rank's RGBA8 shard (device pointer; None = the handle's own output) to the root's
        row-major frame (device pointer; ignored on the other ranks)."""
        self._check(self.L.arctic_gather_frame(self.h, C.c_void_p(d_shard_ptr) if d_shard_ptr else None,
                                               C.c_void_p(d_frame_ptr) if d_frame_ptr else None, root))

    def assemble_frame(self, d_staging_ptr, d_frame_ptr, world, row_ranges=None):
        """the root's placement step alone: shards back to back in rank order -> the full frame."""
        rr = None if row_ranges is None else np.ascontiguousarray(row_ranges, dtype=np.uint32).reshape(-1)
        assert rr is None or rr.size == 2 * world
        self._check(self.L.arctic_assemble_frame(self.h, C.c_void_p(d_staging_ptr), C.c_void_p(d_frame_ptr), world, _ptr(rr)))

    def create_material(self, diffuse, normal, metal_rough):
        """three (h, w, 4) uint8 images; returns the material index."""
        d, n, m = (np.ascontiguousarray(t, dtype=np.uint8) for t in (diffuse, normal, metal_rough))
        for t in (d, n, m):
            if t.ndim != 3 or t.shape[2] != 4:
                raise ArcticError(-1, "create_material: images must be (h, w, 4) uint8")
        return self._check(self.L.arctic_create_material(self.h, _ptr(d), d.shape[1], d.shape[0], _ptr(n), n.shape[1], n.shape[0],
                                                         _ptr(m), m.shape[1], m.shape[0]))

    def set_material_extras(self, material, params=None, emissive=None, occlusion=None):
        """glTF factors, emissive and occlusion of one material (include/arctic_hip.h): params = one MATERIAL_PARAMS_DTYPE record or None (the
        neutral factors), emissive / occlusion = (h, w, 4) uint8 images or None.  Replaces what the material had; all None returns it to
        neutral.  Invalid params raise ArcticError (ARCTIC_E_INVALID) and leave the material as it was."""
        p = None if params is None else np.ascontiguousarray(params, dtype=MATERIAL_PARAMS_DTYPE).reshape(1)
        imgs = []
        for t in (emissive, occlusion):
            t = None if t is None else np.ascontiguousarray(t, dtype=np.uint8)
            if t is not None and (t.ndim != 3 or t.shape[2] != 4):
                raise ArcticError(-1, "set_material_extras: images must be (h, w, 4) uint8")
            imgs.append(t)
        e, o = imgs
        self._check(self.L.arctic_set_material_extras(self.h, int(material), _ptr(p), _ptr(e), e.shape[1] if e is not None else 0, e.shape[0] if e is not None else 0,
                                                      _ptr(o), o.shape[1] if o is not None else 0, o.shape[0] if o is not None else 0))

    def create_mesh(self, vertices, indices, material_idx):
        v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
        return self._check(self.L.arctic_create_mesh(self.h, _ptr(v), len(v), _ptr(i), len(i), int(material_idx)))

    def set_mesh_skin(self, mesh, skin, n_joints=0):
        """attach (or replace) the skin of a mesh: one SKIN_VERTEX_DTYPE record per vertex, joint indices below n_joints; None detaches the
        skin and any pose.  Invalid records raise ArcticError (ARCTIC_E_INVALID) and leave the mesh as it was."""
        if skin is None:
            self._check(self.L.arctic_set_mesh_skin(self.h, int(mesh), None, 0, 0))
            return
        s = np.ascontiguousarray(skin, dtype=SKIN_VERTEX_DTYPE)
        self._check(self.L.arctic_set_mesh_skin(self.h, int(mesh), _ptr(s), len(s), int(n_joints)))

    def set_mesh_pose(self, mesh, joint_matrices):
        """pose a skinned mesh: (n_joints, 16) float32, each matrix in glm memory order ([col][row]; a math matrix M goes in as M.T); None
        returns the mesh to its bind pose.  Asynchronous on the handle's stream, in order with the frames."""
        if joint_matrices is None:
            self._check(self.L.arctic_set_mesh_pose(self.h, int(mesh), None, 0))
            return
        j = np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1, 16)
        self._check(self.L.arctic_set_mesh_pose(self.h, int(mesh), _ptr(j), len(j)))

    def set_mesh_morph_targets(self, mesh, deltas):
        """attach (or replace) the morph targets of a mesh: (n_targets, n_vertices) MORPH_DELTA_DTYPE records; None detaches them.  All
        weights are zero afterwards.  Invalid records raise ArcticError (ARCTIC_E_INVALID) and leave the mesh as it was."""
        if deltas is None:
            self._check(self.L.arctic_set_mesh_morph_targets(self.h, int(mesh), None, 0, 0))
            return
        d = np.ascontiguousarray(deltas, dtype=MORPH_DELTA_DTYPE)
        if d.ndim != 2 or d.size == 0:                 # (an empty array is not None: it must not detach)
            raise ArcticError(-1, "set_mesh_morph_targets: deltas must be (n_targets, n_vertices) records, at least one of each")
        self._check(self.L.arctic_set_mesh_morph_targets(self.h, int(mesh), _ptr(d), d.shape[1], d.shape[0]))

    def set_mesh_morph_weights(self, mesh, weights):
        """set the weights of a mesh with morph targets: n_targets float32, used as given; None (or all zeros) returns the mesh to its own
        vertices.  Asynchronous on the handle's stream, in order with the frames."""
        if weights is None:
            self._check(self.L.arctic_set_mesh_morph_weights(self.h, int(mesh), None, 0))
            return
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        self._check(self.L.arctic_set_mesh_morph_weights(self.h, int(mesh), _ptr(w), len(w)))

    def read_mesh_vertices(self, mesh, n_vertices):
        """the vertices the next prepass reads for this mesh -- posed, else morphed, else its own: n_vertices VERTEX_DTYPE records"""
        v = np.empty(int(n_vertices), VERTEX_DTYPE)
        self._check(self.L.arctic_read_mesh_vertices(self.h, int(mesh), _ptr(v), len(v)))
        return v

    # ---- ray queries (include/arctic_hip.h: arctic_trace_rays and the definition in front of it) ---------------------------------
    def trace_rays(self, desc, rays, any_hit=False):
        """RAY_DTYPE records against the scene's triangles: HIT_DTYPE records, the closest hit of each ray (prim 0xFFFFFFFF: a miss) or, with
        any_hit, whether anything is hit (prim 0 / 0xFFFFFFFF).  Builds or refreshes the handle's acceleration structure when the scene changed."""
        s = self._scene(desc)
        ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
        hits = np.empty(len(ry), HIT_DTYPE)
        self._check(self.L.arctic_trace_rays(self.h, C.byref(s), _ptr(ry) if len(ry) else None, len(ry), binding.TRACE_ANY if any_hit else 0,
                                             _ptr(hits) if len(ry) else None))
        return hits

    def trace_rays_device(self, desc, d_rays_ptr, n, d_hits_ptr, any_hit=False):
        """the same between device buffers (int pointers, e.g. torch tensors' .data_ptr(); 32 bytes per ray, 16 per hit, 16-byte aligned);
        asynchronous on the handle's stream."""
        s = self._scene(desc)
        self._check(self.L.arctic_trace_rays_device(self.h, C.byref(s), C.c_void_p(d_rays_ptr) if d_rays_ptr else None, int(n),
                                                    binding.TRACE_ANY if any_hit else 0, C.c_void_p(d_hits_ptr) if d_hits_ptr else None))

    def trace_sun_visibility(self, desc, bias, read=True):
        """one any-hit ray per pixel of the resident G-buffer towards the sun, from world + bias * n: (rows, width) uint8, 255 = the sun is
        visible or no geometry, 0 = occluded.  read=False leaves the mask on the device and returns None (timing)."""
        s = self._scene(desc)
        mask = np.empty((self.rows, self.width), np.uint8) if read else None
        self._check(self.L.arctic_trace_sun_visibility(self.h, C.byref(s), float(bias), _ptr(mask)))
        return mask

    # ---- ambient occlusion (include/arctic_hip.h: arctic_trace_ambient_occlusion and the definition in front of it) -------------
    def trace_ambient_occlusion(self, desc, dirs, n_rays=None, pattern=None, radius=np.inf, bias=1e-3, filter=False, normal_cos=0.9, plane_dist=0.05, read=True):
        """n_rays any-hit rays of length radius per pixel of the resident G-buffer, from world + bias * m along dirs -- (P * P, n_rays, 3) float32
        local directions, z along the normal, e.g. ao_directions(n_rays, P); n_rays and pattern default to its shape: (rows, width) uint8
        visibility, 255 = open or no geometry.  filter: the edge-aware sum over the P x P window (whole frames only).  read=False leaves the
        result on the device and returns None (timing)."""
        s = self._scene(desc)
        ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist)
        out = np.empty((self.rows, self.width), np.uint8) if read else None
        self._check(self.L.arctic_trace_ambient_occlusion(self.h, C.byref(s), _ptr(ao), _ptr(d), _ptr(out)))
        return out

    def trace_ambient_occlusion_device(self, desc, dirs, d_out_ptr, n_rays=None, pattern=None, radius=np.inf, bias=1e-3, filter=False, normal_cos=0.9, plane_dist=0.05):
        """the same into device memory the caller owns (an int pointer, e.g. a torch tensor's .data_ptr(); rows * width bytes); asynchronous on
        the handle's stream."""
        s = self._scene(desc)
        ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist)
        self._check(self.L.arctic_trace_ambient_occlusion_device(self.h, C.byref(s), _ptr(ao), _ptr(d), C.c_void_p(d_out_ptr) if d_out_ptr else None))

    # ---- indirect diffuse light (include/arctic_hip.h: arctic_trace_gi and the definition in front of it) -------------------------------------
    def trace_gi(self, desc, dirs, n_rays=None, pattern=None, max_distance=np.inf, bias=1e-3, clamp_max=65504.0, filter=False, normal_cos=0.9, plane_dist=0.05, read=True):
        """n_rays rounds of one closest-hit ray per pixel of the resident G-buffer, from world + bias * m along dirs -- (P * P, n_rays, 3) float32
        local directions, z along the normal, e.g. gi_directions(n_rays, P); n_rays and pattern default to its shape --, each shaded at its hit
        (shade_hits) or by the environment map: (rows, width, 4) float32 {mean colour, rays}.  filter: the sum over the P x P window (whole
        frames only).  read=False leaves the plane on the device and returns None (timing)."""
        s = self._scene(desc)
        gi, d = gi_arguments(dirs, n_rays, pattern, max_distance, bias, clamp_max, filter, normal_cos, plane_dist)
        out = np.empty((self.rows, self.width, 4), np.float32) if read else None
        self._check(self.L.arctic_trace_gi(self.h, C.byref(s), _ptr(gi), _ptr(d), _ptr(out)))
        return out

    def trace_gi_device(self, desc, dirs, d_rgba_ptr, **kw):
        """the same into device memory the caller owns (an int pointer; rows * width * 16 bytes, 16-byte aligned); asynchronous on the handle's stream."""
        s = self._scene(desc)
        gi, d = gi_arguments(dirs, **kw)
        self._check(self.L.arctic_trace_gi_device(self.h, C.byref(s), _ptr(gi), _ptr(d), C.c_void_p(d_rgba_ptr) if d_rgba_ptr else None))

    def gi_rays(self, dirs, round, **kw):
        """round `round`'s ray records of the resident G-buffer: (rows, width) RAY_DTYPE, the all-zero record where a pixel has no ray (tests)"""
        gi, d = gi_arguments(dirs, **kw)
        out = np.empty((self.rows, self.width), RAY_DTYPE)
        self._check(self.L.arctic_gi_rays(self.h, _ptr(gi), _ptr(d), int(round), _ptr(out)))
        return out

    def read_gi_estimate(self, want=("sum", "estimate")):
        """the latest trace_gi's planes as they stand on the device: {"sum": S, "estimate": E}, (rows, width, 4) float32 each"""
        out = {k: np.empty((self.rows, self.width, 4), np.float32) for k in want}
        self._check(self.L.arctic_read_gi_estimate(self.h, _ptr(out.get("sum")), _ptr(out.get("estimate"))))
        return out

    def gi_info(self):
        """(device bytes of the table, S, E, the history and the composition's planes, launches of the stage's own kernels, tracing calls, bytes of
        the history alone): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_gi_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def accumulate_gi_device(self, desc, d_in_ptr, d_out_ptr, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0, hist=None):
        """blend a device plane of E (an int pointer: rows * width float4, 16-byte aligned) into the handle's history, reprojected through the
        previous call's camera, into d_out_ptr ({acc, N}; it may be the same plane).  Asynchronous on the handle's stream."""
        s = self._scene(desc)
        h = gi_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_accumulate_gi_device(self.h, C.byref(s), _ptr(h), vp(d_in_ptr), vp(d_out_ptr)))

    def accumulate_gi(self, desc, gi, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0, hist=None):
        """the same from and to host memory: (rows, width, 4) float32 E -> (rows, width, 4) {acc, N}; synchronous"""
        s = self._scene(desc)
        h = gi_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        a = np.ascontiguousarray(gi, dtype=np.float32)
        if a.shape != (self.rows, self.width, 4):
            raise ArcticError(-1, "accumulate_gi: the plane is not (rows, width, 4)")
        out = np.empty_like(a)
        self._check(self.L.arctic_accumulate_gi(self.h, C.byref(s), _ptr(h), _ptr(a), _ptr(out)))
        return out

    def gi_history_reset(self):
        self._check(self.L.arctic_gi_history_reset(self.h))

    def read_gi_history(self):
        """the current history, row-major: {"acc": (h, w, 3), "count": (h, w), "world": (h, w, 3), "normal": (h, w, 3)} float32"""
        n = (self.height, self.width)
        out = dict(acc=np.empty(n + (3,), np.float32), count=np.empty(n, np.float32), world=np.empty(n + (3,), np.float32), normal=np.empty(n + (3,), np.float32))
        self._check(self.L.arctic_read_gi_history(self.h, _ptr(out["acc"]), _ptr(out["count"]), _ptr(out["world"]), _ptr(out["normal"])))
        return out

    def gi_compose_device(self, desc, settings, d_hdr_ptr=None, d_gi_ptr=None, d_out_hdr_ptr=None, d_out_ptr=None, gi_strength=1.0, ambient_scale=1.0, flags=0, compose=None):
        """fold the indirect light into an HDR plane in front of the tonemapper: C (an int pointer: rows * width * 3 floats; None: the handle's
        shaded plane, under GI_SOURCE_COMPOSED the composed one) + (ambient * base) * (ambient_scale - 1) + gi_strength * (1 - metal) * base * E
        (d_gi_ptr: rows * width float4; None: the handle's estimate).  The result stays on the device -- the caller's planes or the handle's
        own: read_gi().  Asynchronous on the handle's stream."""
        s, st = self._scene(desc), self._settings(settings)
        c = gi_compose_arguments(gi_strength, ambient_scale, flags) if compose is None else compose
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_gi_compose_device(self.h, C.byref(s), C.byref(st), _ptr(c), vp(d_hdr_ptr), vp(d_gi_ptr), vp(d_out_hdr_ptr), vp(d_out_ptr)))

    def read_gi(self, want=("ldr", "hdr", "rgba8")):
        """the latest composition's planes the handle owns: {"ldr", "hdr": (rows, width, 3) float32, "rgba8": (rows, width, 4) uint8}"""
        n = (self.rows, self.width)
        out = {k: np.empty(n + ((4,) if k == "rgba8" else (3,)), np.uint8 if k == "rgba8" else np.float32) for k in want}
        self._check(self.L.arctic_read_gi(self.h, _ptr(out.get("ldr")), _ptr(out.get("hdr")), _ptr(out.get("rgba8"))))
        return out

    def pass_gi(self, desc, settings, dirs, d_out_ptr=None, hist=None, compose=None, **kw):
        """the one call: trace_gi (keywords as it takes them), accumulate when hist (a GI_HISTORY_DTYPE record, e.g. gi_history_arguments()) is
        given, compose (a GI_COMPOSE_DTYPE record; default gi_strength 1, ambient_scale 1).  Asynchronous on the handle's stream."""
        s, st = self._scene(desc), self._settings(settings)
        gi, d = gi_arguments(dirs, **kw)
        c = gi_compose_arguments() if compose is None else compose
        self._check(self.L.arctic_pass_gi(self.h, C.byref(s), C.byref(st), _ptr(gi), _ptr(d), _ptr(hist), _ptr(c), C.c_void_p(d_out_ptr) if d_out_ptr else None))

    # ---- what is at a hit (include/arctic_hip.h: arctic_hit_attributes and the text in front of it) ---------------------------------------
    def hit_attributes(self, desc, hits):
        """HIT_DTYPE records (trace_rays' answer, or hand-made) -> ((n, 18) float32 attributes in read_gbuffer's order, (n,) uint32 materials):
        the interpolated vertex output at each hit; material 0xFFFFFFFF and zeros for a miss or a prim the scene does not have."""
        s = self._scene(desc)
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).ravel()
        attrs, material = np.empty((len(h), 18), np.float32), np.empty(len(h), np.uint32)
        p = (lambda a: _ptr(a) if len(h) else None)
        self._check(self.L.arctic_hit_attributes(self.h, C.byref(s), p(h), len(h), p(attrs), p(material)))
        return attrs, material

    def set_hit_model(self, model):
        """ARCTIC_OPT_HIT_MODEL (the same as set_option("hit_model", model)): 0 = the base model at ray hits, 1 = with spot lights,
        shadow-casting point lights, image-based ambient and material extras.  shade_hits, trace_reflections, pass_ray_effects, trace_gi and
        pass_gi follow it.  Any other value raises ArcticError (ARCTIC_E_INVALID)."""
        self.set_option("hit_model", model)

    def shade_hits(self, desc, rays, hits):
        """RAY_DTYPE records and their HIT_DTYPE records -> (n, 4) float32: the forward pixel at each hit seen from the ray's origin, a = 1; for
        a miss the environment map along the ray (black without one), a = 0.  Which pixel: set_hit_model."""
        s = self._scene(desc)
        ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
        h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).ravel()
        if len(h) != len(ry):
            raise ArcticError(-1, "shade_hits: one hit per ray")
        out = np.empty((len(ry), 4), np.float32)
        p = (lambda a: _ptr(a) if len(ry) else None)
        self._check(self.L.arctic_shade_hits(self.h, C.byref(s), p(ry), p(h), len(ry), 0, p(out)))
        return out

    def shade_hits_device(self, desc, d_rays_ptr, d_hits_ptr, n, d_rgba_ptr):
        """the same between device buffers (int pointers; 32 bytes per ray, 16 per hit, 16 per result, 16-byte aligned); asynchronous on the
        handle's stream."""
        s = self._scene(desc)
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_shade_hits_device(self.h, C.byref(s), vp(d_rays_ptr), vp(d_hits_ptr), int(n), 0, vp(d_rgba_ptr)))

    def trace_reflections(self, desc, bias, read=True):
        """one mirror ray per pixel of the resident G-buffer, from world + bias * m, its closest hit shaded: (rows, width, 4) float32, a = 1 where
        the reflection shows geometry.  read=False leaves the plane on the device and returns None (timing)."""
        s = self._scene(desc)
        out = np.empty((self.rows, self.width, 4), np.float32) if read else None
        self._check(self.L.arctic_trace_reflections(self.h, C.byref(s), float(bias), _ptr(out)))
        return out

    def trace_reflections_device(self, desc, bias, d_rgba_ptr):
        """the same into device memory the caller owns (an int pointer; rows * width * 16 bytes, 16-byte aligned); asynchronous on the handle's stream."""
        s = self._scene(desc)
        self._check(self.L.arctic_trace_reflections_device(self.h, C.byref(s), float(bias), C.c_void_p(d_rgba_ptr) if d_rgba_ptr else None))

    def hit_shading_info(self):
        """(device bytes, pinned host bytes, prims in the source table, times the table was made) held for hit_attributes, shade_hits and
        trace_reflections: all 0 until the first of them"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_hit_shading_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- occlusion and reflections composed into the shaded frame (include/arctic_hip.h: arctic_compose_planes_device and the definition) -------
    def compose_planes_device(self, desc, settings, d_ao_ptr=None, d_reflection_ptr=None, ao_strength=1.0, reflection_strength=1.0, d_out_ptr=None, flags=None):
        """fold device planes the caller owns (int pointers: rows * width bytes of visibility, rows * width * 16 bytes of RGBA32F, 16-byte aligned)
        into the float HDR colour of the latest shading (set_option("keep_float_output", 1)), then tonemap; flags default to the planes given.
        The result stays on the device -- d_out_ptr (rows * width * 4 bytes) or the handle's own buffers: read_composed(); asynchronous on the
        handle's stream."""
        s, st = self._scene(desc), self._settings(settings)
        if flags is None:
            flags = (binding.COMPOSE_AO if d_ao_ptr else 0) | (binding.COMPOSE_REFLECTIONS if d_reflection_ptr else 0)
        c = _compose_arguments(flags, ao_strength, reflection_strength, 0.0)
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_compose_planes_device(self.h, C.byref(s), C.byref(st), _ptr(c), vp(d_ao_ptr), vp(d_reflection_ptr), vp(d_out_ptr)))

    def pass_ray_effects(self, desc, settings, dirs=None, reflection_bias=None, ao_strength=1.0, reflection_strength=1.0, d_out_ptr=None, read=True, n_rays=None,
                         pattern=None, radius=np.inf, bias=1e-3, filter=False, normal_cos=0.9, plane_dist=0.05):
        """the one call: the ambient occlusion (dirs and its parameters as trace_ambient_occlusion takes them; None: no occlusion), the reflection
        plane (reflection_bias; None: no reflections), then the composition into the latest shading's HDR colour and the tonemapper:
        (rows, width, 4) uint8.  read=False or a d_out_ptr leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        flags = (binding.COMPOSE_AO if dirs is not None else 0) | (binding.COMPOSE_REFLECTIONS if reflection_bias is not None else 0)
        c = _compose_arguments(flags, ao_strength, reflection_strength, 0.0 if reflection_bias is None else reflection_bias)
        ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist) if dirs is not None else (None, None)
        self._check(self.L.arctic_pass_ray_effects(self.h, C.byref(s), C.byref(st), _ptr(c), _ptr(ao), _ptr(d), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_composed(want=("rgba8",))[2] if read and not d_out_ptr else None

    def read_composed(self, want=("ldr", "hdr", "rgba8")):
        """the latest composition, shaped like read_output: (ldr, hdr, rgba8), None for what was not asked for"""
        n = (self.rows, self.width)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        self._check(self.L.arctic_read_composed(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba)))
        return ldr, hdr, rgba

    def compose_info(self):
        """(device bytes, launches of the composition kernel, pass_ray_effects calls, 0) held for the composition: all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_compose_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- temporal accumulation of the occlusion plane (include/arctic_hip.h: arctic_accumulate_ambient_occlusion_device and the definition) ------
    def accumulate_ambient_occlusion_device(self, desc, d_ao_in_ptr, d_ao_out_ptr, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0, hist=None):
        """blend the device byte plane d_ao_in_ptr (an int pointer; rows * width bytes) into the handle's history, reprojected through the previous
        call's camera, and write the accumulated plane to d_ao_out_ptr (it may be the same plane); desc's camera is kept for the next call.
        hist: an AO_HISTORY_DTYPE record instead of the four parameters.  Asynchronous on the handle's stream."""
        s = self._scene(desc)
        h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_accumulate_ambient_occlusion_device(self.h, C.byref(s), _ptr(h), vp(d_ao_in_ptr), vp(d_ao_out_ptr)))

    def accumulate_ambient_occlusion(self, desc, ao, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0, hist=None):
        """the same from and to host memory: (rows, width) uint8 -> (rows, width) uint8; synchronous"""
        s = self._scene(desc)
        h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        a = np.ascontiguousarray(ao, dtype=np.uint8)
        if a.shape != (self.rows, self.width):
            raise ArcticError(-1, f"accumulate_ambient_occlusion: expected {(self.rows, self.width)}, got {a.shape}")
        out = np.empty_like(a)
        self._check(self.L.arctic_accumulate_ambient_occlusion(self.h, C.byref(s), _ptr(h), _ptr(a), _ptr(out)))
        return out

    def ao_history_reset(self):
        """empty the history: the next accumulation is a first call.  Frees nothing."""
        self._check(self.L.arctic_ao_history_reset(self.h))

    def read_ao_history(self, want=("value", "count", "world", "normal")):
        """the history the last accumulation wrote: (value, count, world, normal) -- (rows, width) float32 twice, (rows, width, 3) float32 twice; None
        for what was not asked for.  ArcticError (STATE) while the history is empty."""
        n = (self.rows, self.width)
        value = np.empty(n, np.float32) if "value" in want else None
        count = np.empty(n, np.float32) if "count" in want else None
        world = np.empty(n + (3,), np.float32) if "world" in want else None
        normal = np.empty(n + (3,), np.float32) if "normal" in want else None
        self._check(self.L.arctic_read_ao_history(self.h, _ptr(value), _ptr(count), _ptr(world), _ptr(normal)))
        return value, count, world, normal

    def ao_history_info(self):
        """(device bytes of the two history sets, launches of the accumulation kernel, calls since the last reset, 0): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_ao_history_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def pass_ray_effects_temporal(self, desc, settings, dirs, reflection_bias=None, ao_strength=1.0, reflection_strength=1.0, d_out_ptr=None, read=True, n_rays=None,
                                  pattern=None, radius=np.inf, bias=1e-3, filter=False, normal_cos=0.9, plane_dist=0.05, max_history=32.0, history_normal_cos=0.9,
                                  history_plane_dist=0.05, min_weight=0.0):
        """pass_ray_effects with the accumulation between the occlusion and the composition: (rows, width, 4) uint8.  read=False or a d_out_ptr
        leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        flags = (binding.COMPOSE_AO if dirs is not None else 0) | (binding.COMPOSE_REFLECTIONS if reflection_bias is not None else 0)
        c = _compose_arguments(flags, ao_strength, reflection_strength, 0.0 if reflection_bias is None else reflection_bias)
        ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist) if dirs is not None else (None, None)
        h = _ao_history_arguments(max_history, history_normal_cos, history_plane_dist, min_weight)
        self._check(self.L.arctic_pass_ray_effects_temporal(self.h, C.byref(s), C.byref(st), _ptr(c), _ptr(ao), _ptr(d), _ptr(h), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_composed(want=("rgba8",))[2] if read and not d_out_ptr else None

    # ---- motion vectors and the accumulation that uses them (include/arctic_hip.h: arctic_motion_vectors_device and the definition) -------------
    def motion_vectors_device(self, desc, d_prev_world4_ptr, d_velocity2_ptr=None):
        """where every pixel's surface point lay at the previous motion call, into device planes the caller owns (int pointers: rows * width
        float4 {previous world position, flag}, and rows * width float2 offsets to where it was on the screen, or None).  desc: the scene
        that was drawn; it is what the next call compares against -- once per frame.  Asynchronous on the handle's stream."""
        s = self._scene(desc)
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_motion_vectors_device(self.h, C.byref(s), vp(d_prev_world4_ptr), vp(d_velocity2_ptr)))

    def motion_vectors(self, desc, want=("prev_world", "velocity", "bary", "source")):
        """the same to host memory, with the kernel's two further outputs: (prev_world (rows, width, 4) float32, velocity (rows, width, 2)
        float32, bary (rows, width, 3) float32, source (rows, width, 4) uint32 = {object, i0, i1, i2}); None for what was not asked for.
        Synchronous."""
        n = (self.rows, self.width)
        pw = np.empty(n + (4,), np.float32) if "prev_world" in want else None
        vel = np.empty(n + (2,), np.float32) if "velocity" in want else None
        bary = np.empty(n + (3,), np.float32) if "bary" in want else None
        src = np.empty(n + (4,), np.uint32) if "source" in want else None
        s = self._scene(desc)
        self._check(self.L.arctic_motion_vectors(self.h, C.byref(s), _ptr(pw), _ptr(vel), _ptr(bary), _ptr(src)))
        return pw, vel, bary, src

    def motion_reset(self):
        """forget what the previous motion call saw: the next call is a first call.  Frees nothing."""
        self._check(self.L.arctic_motion_reset(self.h))

    def motion_info(self):
        """(device bytes, launches of k_motion, launches of k_motion_snapshot, calls since the last reset): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_motion_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def accumulate_ambient_occlusion_motion_device(self, desc, d_prev_world4_ptr, d_ao_in_ptr, d_ao_out_ptr, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0,
                                                   hist=None):
        """accumulate_ambient_occlusion_device with the history fetched where each pixel's point WAS: d_prev_world4_ptr is the plane
        motion_vectors_device wrote for this frame.  Shares the history with the plain call.  Asynchronous on the handle's stream."""
        s = self._scene(desc)
        h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_accumulate_ambient_occlusion_motion_device(self.h, C.byref(s), _ptr(h), vp(d_prev_world4_ptr), vp(d_ao_in_ptr), vp(d_ao_out_ptr)))

    def accumulate_ambient_occlusion_motion(self, desc, prev_world4, ao, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0, hist=None):
        """the same from and to host memory: (rows, width, 4) float32 and (rows, width) uint8 -> (rows, width) uint8; synchronous"""
        s = self._scene(desc)
        h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
        a = np.ascontiguousarray(ao, dtype=np.uint8)
        pw = np.ascontiguousarray(prev_world4, dtype=np.float32)
        if a.shape != (self.rows, self.width) or pw.shape != (self.rows, self.width, 4):
            raise ArcticError(-1, f"accumulate_ambient_occlusion_motion: expected {(self.rows, self.width)} and {(self.rows, self.width, 4)}, got {a.shape} and {pw.shape}")
        out = np.empty_like(a)
        self._check(self.L.arctic_accumulate_ambient_occlusion_motion(self.h, C.byref(s), _ptr(h), _ptr(pw), _ptr(a), _ptr(out)))
        return out

    def pass_ray_effects_motion(self, desc, settings, dirs, reflection_bias=None, ao_strength=1.0, reflection_strength=1.0, d_out_ptr=None, read=True, n_rays=None,
                                pattern=None, radius=np.inf, bias=1e-3, filter=False, normal_cos=0.9, plane_dist=0.05, max_history=32.0, history_normal_cos=0.9,
                                history_plane_dist=0.05, min_weight=0.0):
        """pass_ray_effects_temporal with the motion vectors in front of the occlusion and the accumulation's motion form: (rows, width, 4)
        uint8.  read=False or a d_out_ptr leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        flags = (binding.COMPOSE_AO if dirs is not None else 0) | (binding.COMPOSE_REFLECTIONS if reflection_bias is not None else 0)
        c = _compose_arguments(flags, ao_strength, reflection_strength, 0.0 if reflection_bias is None else reflection_bias)
        ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist) if dirs is not None else (None, None)
        h = _ao_history_arguments(max_history, history_normal_cos, history_plane_dist, min_weight)
        self._check(self.L.arctic_pass_ray_effects_motion(self.h, C.byref(s), C.byref(st), _ptr(c), _ptr(ao), _ptr(d), _ptr(h), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_composed(want=("rgba8",))[2] if read and not d_out_ptr else None

    # ---- temporal anti-aliasing (include/arctic_hip.h: arctic_set_camera_jitter, arctic_taa_resolve_device and the definition) --------------------
    def set_camera_jitter(self, jx, jy):
        """the forward prepass's sub-pixel offset in pixels, each in [-1, 1]: a point at screen position s is drawn at s + (jx, jy).  (0, 0), the
        default, changes nothing.  Kept across resize."""
        self._check(self.L.arctic_set_camera_jitter(self.h, float(jx), float(jy)))

    def taa_resolve_device(self, settings, d_hdr_ptr=None, d_velocity2_ptr=None, d_out_ptr=None, jitter=(0.0, 0.0), max_history=8.0, min_weight=0.0, flags=0, taa=None):
        """blend a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own, the latest shading's or -- flags &
        TAA_SOURCE_COMPOSED -- the latest composition's) into the handle's history, fetched where d_velocity2_ptr (rows * width float2; None: zero)
        and this frame's jitter say, then tonemap.  The result stays on the device -- d_out_ptr (rows * width * 4 bytes) or the handle's own
        buffers: read_taa().  taa: a TAA_DTYPE record instead of the parameters.  Asynchronous on the handle's stream."""
        st = self._settings(settings)
        t = _taa_arguments(flags, max_history, min_weight, jitter) if taa is None else taa
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_taa_resolve_device(self.h, C.byref(st), _ptr(t), vp(d_hdr_ptr), vp(d_velocity2_ptr), vp(d_out_ptr)))

    def taa_resolve(self, settings, hdr=None, velocity2=None, jitter=(0.0, 0.0), max_history=8.0, min_weight=0.0, flags=0, taa=None, read=True):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None, velocity2 (rows, width, 2) float32 or None -> (rows, width, 4)
        uint8 (read=False: None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        t = _taa_arguments(flags, max_history, min_weight, jitter) if taa is None else taa
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        v = None if velocity2 is None else np.ascontiguousarray(velocity2, dtype=np.float32)
        if (c is not None and c.shape != (self.rows, self.width, 3)) or (v is not None and v.shape != (self.rows, self.width, 2)):
            raise ArcticError(-1, f"taa_resolve: expected {(self.rows, self.width, 3)} and {(self.rows, self.width, 2)}")
        out = np.empty((self.rows, self.width, 4), np.uint8) if read else None
        self._check(self.L.arctic_taa_resolve(self.h, C.byref(st), _ptr(t), _ptr(c), _ptr(v), _ptr(out)))
        return out

    def pass_taa(self, desc, settings, d_out_ptr=None, jitter=(0.0, 0.0), max_history=8.0, min_weight=0.0, flags=0, taa=None, read=True):
        """the one call: the frame's ONE motion call into planes the handle owns, then the resolve on the handle's HDR plane: (rows, width, 4)
        uint8.  read=False or a d_out_ptr leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        t = _taa_arguments(flags, max_history, min_weight, jitter) if taa is None else taa
        self._check(self.L.arctic_pass_taa(self.h, C.byref(s), C.byref(st), _ptr(t), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_taa(want=("rgba8",))[3] if read and not d_out_ptr else None

    def taa_reset(self):
        """empty the history: the next resolve is a first call.  Frees nothing."""
        self._check(self.L.arctic_taa_reset(self.h))

    def read_taa(self, want=("ldr", "hdr", "count", "rgba8")):
        """what the latest resolve left, row-major: (ldr (rows, width, 3), hdr (rows, width, 3), count (rows, width) float32, rgba8 (rows, width,
        4) uint8); None for what was not asked for.  ArcticError (STATE) while the history is empty."""
        n = (self.rows, self.width)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        count = np.empty(n, np.float32) if "count" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        self._check(self.L.arctic_read_taa(self.h, _ptr(ldr), _ptr(hdr), _ptr(count), _ptr(rgba)))
        return ldr, hdr, count, rgba

    def taa_info(self):
        """(device bytes, launches of k_taa_resolve, calls since the last reset, 0): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_taa_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- motion blur (include/arctic_hip.h: arctic_motion_blur_device and the definition in front of it) ------------------------------------------
    def motion_blur_device(self, settings, d_hdr_ptr=None, d_velocity2_ptr=None, d_depth_ptr=None, d_out_ptr=None, shutter=1.0, max_radius=16.0, samples=15, depth_extent=0.05,
                           flags=0, mb=None):
        """blur a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own, per flags -- the latest shading's, under
        MB_SOURCE_COMPOSED the composition's, under MB_SOURCE_TAA the anti-aliasing's history) along d_velocity2_ptr (rows * width float2,
        required), ordered by d_depth_ptr (rows * width floats; None: depth 0), then tonemap.  The result stays on the device -- d_out_ptr (rows *
        width * 4 bytes) or the handle's own buffers: read_motion_blur().  mb: a MOTION_BLUR_DTYPE record instead of the parameters.
        Asynchronous on the handle's stream."""
        st = self._settings(settings)
        m = _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent) if mb is None else mb
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_motion_blur_device(self.h, C.byref(st), _ptr(m), vp(d_hdr_ptr), vp(d_velocity2_ptr), vp(d_depth_ptr), vp(d_out_ptr)))

    def motion_blur(self, settings, hdr=None, velocity2=None, depth=None, shutter=1.0, max_radius=16.0, samples=15, depth_extent=0.05, flags=0, mb=None, read=True):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None, velocity2 (rows, width, 2) float32, depth (rows, width) float32 or
        None -> (rows, width, 4) uint8 (read=False: None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        m = _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent) if mb is None else mb
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        v = None if velocity2 is None else np.ascontiguousarray(velocity2, dtype=np.float32)
        z = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
        n = (self.rows, self.width)
        if (c is not None and c.shape != n + (3,)) or (v is not None and v.shape != n + (2,)) or (z is not None and z.shape != n):
            raise ArcticError(-1, f"motion_blur: expected {n + (3,)}, {n + (2,)} and {n}")
        out = np.empty(n + (4,), np.uint8) if read else None
        self._check(self.L.arctic_motion_blur(self.h, C.byref(st), _ptr(m), _ptr(c), _ptr(v), _ptr(z), _ptr(out)))
        return out

    def depth_plane_device(self, d_depth_ptr):
        """the visibility plane's depth of the handle's rows into a device plane (an int pointer: rows * width floats): read_gbuffer's depth.
        Asynchronous on the handle's stream."""
        self._check(self.L.arctic_depth_plane_device(self.h, C.c_void_p(d_depth_ptr) if d_depth_ptr else None))

    def pass_motion_blur(self, desc, settings, d_out_ptr=None, shutter=1.0, max_radius=16.0, samples=15, depth_extent=0.05, flags=0, mb=None, read=True):
        """the one call: the motion vectors and the depth into planes the handle owns, then the blur of the handle's HDR plane: (rows, width, 4)
        uint8.  Under MB_SOURCE_TAA no motion call: the velocity plane of the latest pass_taa.  read=False or a d_out_ptr leaves the result on
        the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        m = _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent) if mb is None else mb
        self._check(self.L.arctic_pass_motion_blur(self.h, C.byref(s), C.byref(st), _ptr(m), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_motion_blur(want=("rgba8",))[2] if read and not d_out_ptr else None

    def read_motion_blur(self, want=("ldr", "hdr", "rgba8", "tile_max", "neighbour_max", "prepared")):
        """what the latest blur left, row-major: (ldr (rows, width, 3), hdr (rows, width, 3) float32, rgba8 (rows, width, 4) uint8, tile_max and
        neighbour_max (tiles_y, tiles_x, 2), prepared (rows, width, 2) float32 {l, z}); None for what was not asked for"""
        n = (self.rows, self.width)
        t = ((self.rows + 7) // 8, (self.width + 7) // 8, 2)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        tile = np.empty(t, np.float32) if "tile_max" in want else None
        nb = np.empty(t, np.float32) if "neighbour_max" in want else None
        prep = np.empty(n + (2,), np.float32) if "prepared" in want else None
        self._check(self.L.arctic_read_motion_blur(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba), _ptr(tile), _ptr(nb), _ptr(prep)))
        return ldr, hdr, rgba, tile, nb, prep

    def motion_blur_info(self):
        """(device bytes, launches of k_motion_blur, calls, 0): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_motion_blur_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- depth of field (include/arctic_hip.h: arctic_dof_device and the definition in front of it) ------------------------------------------------
    def dof_device(self, settings, d_hdr_ptr=None, d_depth_ptr=None, taps=None, d_out_ptr=None, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, samples=16,
                   depth_extent=0.5, z_near=0.1, z_far=1000.0, flags=0, dof=None):
        """spread a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own, per flags -- the latest shading's, under
        DOF_SOURCE_COMPOSED the composition's, under DOF_SOURCE_TAA the anti-aliasing's history, under DOF_SOURCE_MOTION_BLUR the latest motion
        blur's output) over each pixel's circle of confusion, from d_depth_ptr (rows * width floats, required) and the tap table `taps` ((samples,
        2) float32 in the unit disc; None: dof_taps(samples)), then tonemap.  The result stays on the device -- d_out_ptr (rows * width * 4
        bytes) or the handle's own buffers: read_dof().  dof: a DOF_DTYPE record instead of the parameters.  Asynchronous on the handle's stream."""
        st = self._settings(settings)
        m = _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, z_near, z_far) if dof is None else dof
        t = _dof_table(taps, m)
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_dof_device(self.h, C.byref(st), _ptr(m), vp(d_hdr_ptr), vp(d_depth_ptr), _ptr(t), vp(d_out_ptr)))

    def dof(self, settings, hdr=None, depth=None, taps=None, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, samples=16, depth_extent=0.5, z_near=0.1, z_far=1000.0,
            flags=0, dof=None, read=True):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None, depth (rows, width) float32 -> (rows, width, 4) uint8
        (read=False: None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        m = _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, z_near, z_far) if dof is None else dof
        t = _dof_table(taps, m)
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        z = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
        n = (self.rows, self.width)
        if (c is not None and c.shape != n + (3,)) or (z is not None and z.shape != n):
            raise ArcticError(-1, f"dof: expected {n + (3,)} and {n}")
        out = np.empty(n + (4,), np.uint8) if read else None
        self._check(self.L.arctic_dof(self.h, C.byref(st), _ptr(m), _ptr(c), _ptr(z), _ptr(t), _ptr(out)))
        return out

    def pass_dof(self, desc, settings, d_out_ptr=None, taps=None, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, samples=16, depth_extent=0.5, flags=0, dof=None, read=True):
        """the one call: the depth into a plane the handle owns, then the gather of the handle's HDR plane per flags, under the scene's camera
        planes (the record's z_near and z_far stay 0): (rows, width, 4) uint8.  read=False or a d_out_ptr leaves the result on the device and
        returns None."""
        s, st = self._scene(desc), self._settings(settings)
        m = _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, 0.0, 0.0) if dof is None else dof
        t = _dof_table(taps, m)
        self._check(self.L.arctic_pass_dof(self.h, C.byref(s), C.byref(st), _ptr(m), _ptr(t), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_dof(want=("rgba8",))[2] if read and not d_out_ptr else None

    def read_dof(self, want=("ldr", "hdr", "rgba8", "tile_max", "neighbour_max", "prepared")):
        """what the latest depth-of-field call left, row-major: (ldr (rows, width, 3), hdr (rows, width, 3) float32, rgba8 (rows, width, 4) uint8,
        tile_max and neighbour_max (tiles_y, tiles_x), prepared (rows, width, 2) float32 {s, zv}); None for what was not asked for"""
        n = (self.rows, self.width)
        t = ((self.rows + 7) // 8, (self.width + 7) // 8)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        tile = np.empty(t, np.float32) if "tile_max" in want else None
        nb = np.empty(t, np.float32) if "neighbour_max" in want else None
        prep = np.empty(n + (2,), np.float32) if "prepared" in want else None
        self._check(self.L.arctic_read_dof(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba), _ptr(tile), _ptr(nb), _ptr(prep)))
        return ldr, hdr, rgba, tile, nb, prep

    def dof_info(self):
        """(device bytes, launches of k_dof_gather, calls, 0): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_dof_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def dof_focus_at(self, px, py, z_near, z_far):
        """autofocus: the view distance of pixel (px, py) of the handle's rows in the resident visibility plane; synchronous"""
        out = C.c_float(0.0)
        self._check(self.L.arctic_dof_focus_at(self.h, float(z_near), float(z_far), int(px), int(py), C.byref(out)))
        return float(out.value)

    # ---- bloom (include/arctic_hip.h: arctic_bloom_device and the definition in front of it) --------------------------------------------------------
    def bloom_device(self, settings, d_hdr_ptr=None, d_out_ptr=None, threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=1.0, levels=5, flags=0, bloom=None):
        """bloom of a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own, per flags -- the latest shading's, under
        BLOOM_SOURCE_COMPOSED the composition's, under BLOOM_SOURCE_TAA the anti-aliasing's history, under BLOOM_SOURCE_MOTION_BLUR the latest
        motion blur's and under BLOOM_SOURCE_DOF the latest depth of field's output): prefilter, `levels` levels down, up again, composite,
        tonemap.  The result stays on the device -- d_out_ptr (rows * width * 4 bytes) or the handle's own buffers: read_bloom().  bloom: a
        BLOOM_DTYPE record instead of the parameters.  Asynchronous on the handle's stream."""
        st = self._settings(settings)
        m = _bloom_arguments(flags, threshold, soft_knee, clamp_max, intensity, spread, levels) if bloom is None else bloom
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_bloom_device(self.h, C.byref(st), _ptr(m), vp(d_hdr_ptr), vp(d_out_ptr)))

    def bloom(self, settings, hdr=None, threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=1.0, levels=5, flags=0, bloom=None, read=True):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None -> (rows, width, 4) uint8 (read=False: None, the result stays
        in the handle's buffers); synchronous"""
        st = self._settings(settings)
        m = _bloom_arguments(flags, threshold, soft_knee, clamp_max, intensity, spread, levels) if bloom is None else bloom
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        n = (self.rows, self.width)
        if c is not None and c.shape != n + (3,):
            raise ArcticError(-1, f"bloom: expected {n + (3,)}")
        out = np.empty(n + (4,), np.uint8) if read else None
        self._check(self.L.arctic_bloom(self.h, C.byref(st), _ptr(m), _ptr(c), _ptr(out)))
        return out

    def read_bloom(self, levels, want=("ldr", "hdr", "rgba8", "down", "up")):
        """what the latest bloom call left: (ldr (rows, width, 3), hdr (rows, width, 3) float32, rgba8 (rows, width, 4) uint8, down: the list of
        D_1 .. D_L as (H_k, W_k, 3) arrays, up: the list of U_1 .. U_{L-1}); None for what was not asked for.  levels: that call's"""
        n = (self.rows, self.width)
        lay = bloom_layout(self.width, self.rows, levels)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        down = np.empty(max(lay["down_floats"], 1), np.float32) if "down" in want else None
        up = np.empty(max(lay["up_floats"], 1), np.float32) if "up" in want else None
        self._check(self.L.arctic_read_bloom(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba), _ptr(down), _ptr(up)))
        return ldr, hdr, rgba, _bloom_split(down, lay, levels), _bloom_split(up, lay, levels - 1)

    def bloom_info(self):
        """(device bytes, launches of k_bloom_composite, calls, 0): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_bloom_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- auto-exposure (include/arctic_hip.h: arctic_exposure_device and the definition in front of it) ---------------------------------------------
    def exposure_device(self, settings, d_hdr_ptr=None, d_out_ptr=None, exposure=None, **kw):
        """auto-exposure of a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own, per flags -- the latest shading's,
        or the plane EXPOSURE_SOURCE_COMPOSED, _TAA, _MOTION_BLUR, _DOF or _BLOOM names): meter, resolve, apply, tonemap.  The result stays on
        the device -- d_out_ptr (rows * width * 4 bytes) or the handle's own buffers: read_exposure().  exposure: an EXPOSURE_DTYPE record
        instead of the parameters of exposure_arguments().  Asynchronous on the handle's stream; nothing is read back."""
        st = self._settings(settings)
        m = exposure_arguments(**kw) if exposure is None else exposure
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_exposure_device(self.h, C.byref(st), _ptr(m), vp(d_hdr_ptr), vp(d_out_ptr)))

    def exposure(self, settings, hdr=None, exposure=None, read=True, **kw):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None -> (rows, width, 4) uint8 (read=False or EXPOSURE_METER_ONLY:
        None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        m = exposure_arguments(**kw) if exposure is None else exposure
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        n = (self.rows, self.width)
        if c is not None and c.shape != n + (3,):
            raise ArcticError(-1, f"exposure: expected {n + (3,)}")
        read = read and not (int(m["flags"][0]) & binding.EXPOSURE_METER_ONLY)
        out = np.empty(n + (4,), np.uint8) if read else None
        self._check(self.L.arctic_exposure(self.h, C.byref(st), _ptr(m), _ptr(c), _ptr(out)))
        return out

    def read_exposure(self, want=("ldr", "hdr", "rgba8", "hist", "state")):
        """what the latest calls left: (ldr (rows, width, 3), hdr (rows, width, 3) float32, rgba8 (rows, width, 4) uint8, hist (256,) uint32,
        state: one EXPOSURE_STATE_DTYPE record); None for what was not asked for"""
        n = (self.rows, self.width)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        hist = np.empty(256, np.uint32) if "hist" in want else None
        state = np.zeros(1, EXPOSURE_STATE_DTYPE) if "state" in want else None
        self._check(self.L.arctic_read_exposure(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba), _ptr(hist), _ptr(state)))
        return ldr, hdr, rgba, hist, state

    def exposure_reset(self):
        """forget the adaptation: the next metering call starts from an invalid state"""
        self._check(self.L.arctic_exposure_reset(self.h))

    def exposure_info(self):
        """(device bytes, launches of k_exposure_apply, calls, launches of k_exposure_meter): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_exposure_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- volumetric fog (include/arctic_hip.h: arctic_fog_device and the definition in front of it) -------------------------------------------------
    def fog_device(self, settings, view, d_hdr_ptr=None, d_depth_ptr=None, d_out_hdr_ptr=None, d_out_ptr=None, offsets=None, fog=None, **kw):
        """march a device HDR plane (an int pointer: rows * width * 3 floats; None: the handle's own -- the latest shading's, under
        FOG_SOURCE_COMPOSED the composition's) through the fog under `view` (a FOG_VIEW_DTYPE record: fog_view()), from d_depth_ptr (rows * width
        floats; None: every depth 1.0) and the handle's current sun map, then tonemap.  The result stays on the device -- d_out_hdr_ptr (rows *
        width * 3 floats) and d_out_ptr (rows * width * 4 bytes), or the handle's own buffers: read_fog().  offsets: 16 floats in [0, 1) or None
        (all 0.5); fog: a FOG_DTYPE record instead of the parameters of fog_arguments().  Asynchronous on the handle's stream."""
        st = self._settings(settings)
        m = fog_arguments(**kw) if fog is None else fog
        t = _fog_offsets(offsets)
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_fog_device(self.h, C.byref(st), _ptr(m), _ptr(view), _ptr(t), vp(d_hdr_ptr), vp(d_depth_ptr), vp(d_out_hdr_ptr), vp(d_out_ptr)))

    def fog(self, settings, view, hdr=None, depth=None, offsets=None, fog=None, read=True, **kw):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None, depth (rows, width) float32 or None -> (hdr (rows, width, 3)
        float32, rgba8 (rows, width, 4) uint8) (read=False: None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        m = fog_arguments(**kw) if fog is None else fog
        t = _fog_offsets(offsets)
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        z = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
        n = (self.rows, self.width)
        if (c is not None and c.shape != n + (3,)) or (z is not None and z.shape != n):
            raise ArcticError(-1, f"fog: expected {n + (3,)} and {n}")
        out_hdr = np.empty(n + (3,), np.float32) if read else None
        out = np.empty(n + (4,), np.uint8) if read else None
        self._check(self.L.arctic_fog(self.h, C.byref(st), _ptr(m), _ptr(view), _ptr(t), _ptr(c), _ptr(z), _ptr(out_hdr), _ptr(out)))
        return (out_hdr, out) if read else None

    def pass_fog(self, desc, settings, d_out_ptr=None, offsets=None, fog=None, read=True, **kw):
        """the one call: fog_view of the scene, the depth into a plane the handle owns, then the march of the handle's HDR plane per flags:
        (rows, width, 4) uint8.  read=False or a d_out_ptr leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        m = fog_arguments(**kw) if fog is None else fog
        t = _fog_offsets(offsets)
        self._check(self.L.arctic_pass_fog(self.h, C.byref(s), C.byref(st), _ptr(m), _ptr(t), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_fog(want=("rgba8",))[2] if read and not d_out_ptr else None

    def read_fog(self, want=("ldr", "hdr", "rgba8")):
        """what the latest fog call left, row-major: (ldr (rows, width, 3), hdr (rows, width, 3) float32, rgba8 (rows, width, 4) uint8); None for
        what was not asked for"""
        n = (self.rows, self.width)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        self._check(self.L.arctic_read_fog(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba)))
        return ldr, hdr, rgba

    def fog_info(self):
        """(device bytes, launches of k_fog_march, calls, uploads of the offset table): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_fog_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    # ---- temporal upscaling (include/arctic_hip.h: arctic_taa_upscale_device and the definition in front of it) ------------------------------------
    def taa_upscale_device(self, settings, out_size, d_hdr_ptr=None, d_velocity2_ptr=None, d_out_ptr=None, upscale=None, **kw):
        """accumulate a device HDR plane of the handle's size (an int pointer: rows * width * 3 floats; None: the handle's own, the latest
        shading's or -- flags & TAA_UPSCALE_SOURCE_COMPOSED -- the latest composition's) into the handle's history of out_size = (W, H), fetched
        where d_velocity2_ptr (rows * width float2; None: zero) and this frame's jitter say, then tonemap.  The result stays on the device --
        d_out_ptr (H * W * 4 bytes) or the handle's own buffers: read_taa_upscale().  upscale: a TAA_UPSCALE_DTYPE record instead of the
        parameters of taa_upscale_arguments().  Asynchronous on the handle's stream."""
        st = self._settings(settings)
        t = taa_upscale_arguments(out_size, **kw) if upscale is None else upscale
        vp = (lambda x: C.c_void_p(x) if x else None)
        self._check(self.L.arctic_taa_upscale_device(self.h, C.byref(st), _ptr(t), vp(d_hdr_ptr), vp(d_velocity2_ptr), vp(d_out_ptr)))

    def taa_upscale(self, settings, out_size, hdr=None, velocity2=None, upscale=None, read=True, **kw):
        """the same from and to host memory: hdr (rows, width, 3) float32 or None, velocity2 (rows, width, 2) float32 or None -> (H, W, 4) uint8
        (read=False: None, the result stays in the handle's buffers); synchronous"""
        st = self._settings(settings)
        t = taa_upscale_arguments(out_size, **kw) if upscale is None else upscale
        c = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.float32)
        v = None if velocity2 is None else np.ascontiguousarray(velocity2, dtype=np.float32)
        if (c is not None and c.shape != (self.rows, self.width, 3)) or (v is not None and v.shape != (self.rows, self.width, 2)):
            raise ArcticError(-1, f"taa_upscale: expected {(self.rows, self.width, 3)} and {(self.rows, self.width, 2)}")
        out = np.empty((int(t["out_height"][0]), int(t["out_width"][0]), 4), np.uint8) if read else None
        self._check(self.L.arctic_taa_upscale(self.h, C.byref(st), _ptr(t), _ptr(c), _ptr(v), _ptr(out)))
        return out

    def pass_taa_upscale(self, desc, settings, out_size, d_out_ptr=None, upscale=None, read=True, **kw):
        """the one call: the frame's ONE motion call into planes the handle owns, then the upscale of the handle's HDR plane: (H, W, 4) uint8.
        read=False or a d_out_ptr leaves the result on the device and returns None."""
        s, st = self._scene(desc), self._settings(settings)
        t = taa_upscale_arguments(out_size, **kw) if upscale is None else upscale
        self._check(self.L.arctic_pass_taa_upscale(self.h, C.byref(s), C.byref(st), _ptr(t), C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return self.read_taa_upscale(want=("rgba8",))[3] if read and not d_out_ptr else None

    def taa_upscale_reset(self):
        """empty the upscaler's history: the next call is a first call.  Frees nothing."""
        self._check(self.L.arctic_taa_upscale_reset(self.h))

    def read_taa_upscale(self, want=("ldr", "hdr", "count", "rgba8")):
        """what the latest upscale left, row-major at its output size: (ldr (H, W, 3), hdr (H, W, 3), count (H, W) float32, rgba8 (H, W, 4)
        uint8); None for what was not asked for.  ArcticError (STATE) while the history is empty."""
        size = self.taa_upscale_info()[3]
        n = (size >> 32, size & 0xFFFFFFFF)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        count = np.empty(n, np.float32) if "count" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        self._check(self.L.arctic_read_taa_upscale(self.h, _ptr(ldr), _ptr(hdr), _ptr(count), _ptr(rgba)))
        return ldr, hdr, count, rgba

    def taa_upscale_hdr_device(self, d_hdr_ptr):
        """the accumulated HDR colour of the latest upscale into a device plane (an int pointer: H * W * 3 floats, row-major): the explicit
        colour argument of bloom_device, exposure_device and the rest on a handle of the output size.  Asynchronous on the handle's stream."""
        self._check(self.L.arctic_taa_upscale_hdr_device(self.h, C.c_void_p(d_hdr_ptr) if d_hdr_ptr else None))

    def taa_upscale_info(self):
        """(device bytes, launches of k_taa_upscale, calls since the last reset, W | H << 32 of the history): all 0 until the first call"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_taa_upscale_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def ray_scene_info(self):
        """(triangles stored, nodes, builds so far, depth) of the cached acceleration structure"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_ray_scene_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def ray_refit_info(self):
        """(refits so far, 1 if the cached structure can be refitted, kernel launches of the latest refit, 0): set_option("ray_refit", 1)"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_ray_refit_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def ray_scene_reset(self):
        """drop the cached structure: the next query builds in full (a refitted tree that drifted far from the pose it was split for)"""
        self._check(self.L.arctic_ray_scene_reset(self.h))

    def ray_scene_resplit(self, desc):
        """put the cached structure's slots in the order a full build of the scene as it is NOW would give them, and refit: on the device, in
        stream order, nothing read back.  Falls back to a full build where the structure cannot be refitted (ray_resplit_info()[2])"""
        s = self._scene(desc)
        self._check(self.L.arctic_ray_scene_resplit(self.h, C.byref(s)))

    def ray_resplit_info(self):
        """(device re-splits so far, launches of the latest, 1 if the latest ray_scene_resplit fell back to a full build, 0)"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.arctic_ray_resplit_info(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def read_ray_structure(self):
        """the device's structure as it stands: (RAY_NODE_DTYPE nodes, RAY_TRI_DTYPE leaf triangles).  Synchronises; for tests"""
        stored, n_nodes, _, _ = self.ray_scene_info()
        nodes, tris = np.zeros(n_nodes, RAY_NODE_DTYPE), np.zeros(stored, RAY_TRI_DTYPE)
        self._check(self.L.arctic_read_ray_structure(self.h, _ptr(nodes) if n_nodes else None, n_nodes, _ptr(tris) if stored else None, stored))
        return nodes, tris

    def create_hdri(self, rgba32f):
        a = np.ascontiguousarray(rgba32f, dtype=np.float32)
        return self._check(self.L.arctic_create_hdri(self.h, _ptr(a), a.shape[1], a.shape[0]))

    def update_lights(self, lights):
        l = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self._check(self.L.arctic_update_lights(self.h, _ptr(l) if len(l) else None, len(l)))

    def update_spot_lights(self, lights):
        """replace the handle's spot lights (SPOT_LIGHT_DTYPE records; an empty array clears them).  An invalid light raises
        ArcticError (ARCTIC_E_INVALID) and leaves the previous list in place."""
        l = np.ascontiguousarray(lights, dtype=SPOT_LIGHT_DTYPE)
        self._check(self.L.arctic_update_spot_lights(self.h, _ptr(l) if len(l) else None, len(l)))

    def update_point_shadow_lights(self, lights):
        """replace the handle's shadow-casting point lights (POINT_SHADOW_LIGHT_DTYPE records; an empty array clears them).  An invalid
        light raises ArcticError (ARCTIC_E_INVALID) and leaves the previous list and faces in place."""
        l = np.ascontiguousarray(lights, dtype=POINT_SHADOW_LIGHT_DTYPE)
        self._check(self.L.arctic_update_point_shadow_lights(self.h, _ptr(l) if len(l) else None, len(l)))

    def render_frame(self, desc, settings, out=None):
        """returns the (rows, width, 4) uint8 frame (this handle's row shard)."""
        s, st = self._scene(desc), self._settings(settings)
        if out is None:
            out = np.empty((self.rows, self.width, 4), np.uint8)
        self._check(self.L.arctic_render_frame(self.h, C.byref(s), C.byref(st), _ptr(out)))
        return out

    def render_frame_device(self, desc, settings, d_out_ptr):
        """frame into caller-owned device memory (int pointer, e.g. torch tensor .data_ptr())."""
        s, st = self._scene(desc), self._settings(settings)
        self._check(self.L.arctic_render_frame_device(self.h, C.byref(s), C.byref(st), C.c_void_p(d_out_ptr)))

    # ---- passes, timing, read-back -----------------------------------------------------------------
    def pass_shadow_map(self, desc):
        s = self._scene(desc)
        self._check(self.L.arctic_pass_shadow_map(self.h, C.byref(s)))

    def pass_point_shadows(self, desc):
        s = self._scene(desc)
        self._check(self.L.arctic_pass_point_shadows(self.h, C.byref(s)))

    def pass_gbuffer(self, desc):
        s = self._scene(desc)
        self._check(self.L.arctic_pass_gbuffer(self.h, C.byref(s)))

    def prepared_pass_shade(self, desc, settings):
        """returns shade(d_out_ptr): the same call as pass_shade with the C structs built once (per-frame host cost of a
        tight loop is then one ctypes call)."""
        s, st = self._scene(desc), self._settings(settings)
        fn, h, check, ps, pst = self.L.arctic_pass_shade, self.h, self._check, C.byref(s), C.byref(st)

        def shade(d_out_ptr=None, _keep=(s, st, desc)):
            check(fn(h, ps, pst, C.c_void_p(d_out_ptr) if d_out_ptr else None))
        return shade

    def pass_shade(self, desc, settings, d_out_ptr=None):
        s, st = self._scene(desc), self._settings(settings)
        self._check(self.L.arctic_pass_shade(self.h, C.byref(s), C.byref(st), C.c_void_p(d_out_ptr) if d_out_ptr else None))

    def post_process(self, hdr_rgba, settings, want_ldr=True):
        a = np.ascontiguousarray(hdr_rgba, dtype=np.float32)
        h, w = a.shape[:2]
        st = self._settings(settings)
        out = np.empty((h, w, 4), np.uint8)
        ldr = np.empty((h, w, 3), np.float32) if want_ldr else None
        self._check(self.L.arctic_post_process(self.h, _ptr(a), w, h, C.byref(st), _ptr(out), _ptr(ldr)))
        return out, ldr

    def antialias(self, img):
        """the edge anti-aliasing filter of set_option("antialias", 1) (include/arctic_hip.h) on any (h, w, 4) uint8 image, host to host:
        returns the filtered image.  Works on every handle, whatever its size and options."""
        a = np.ascontiguousarray(img, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] == 0 or a.shape[1] == 0:
            raise ArcticError(-1, "antialias: the image must be (h, w, 4) uint8 with h, w > 0")
        out = np.empty_like(a)
        self._check(self.L.arctic_antialias(self.h, _ptr(a), a.shape[1], a.shape[0], _ptr(out)))
        return out

    def antialias_device(self, d_in_ptr, d_out_ptr, width, height):
        """the same filter between two RGBA8 device images (int pointers, e.g. torch tensors' .data_ptr()) that do not overlap; asynchronous
        on the handle's stream.  The root of a sharded frame calls it on the assembled frame."""
        self._check(self.L.arctic_antialias_device(self.h, C.c_void_p(d_in_ptr) if d_in_ptr else None, C.c_void_p(d_out_ptr) if d_out_ptr else None,
                                                   int(width), int(height)))

    def time_shade(self, desc, settings, warmup=5, iters=20):
        s, st = self._scene(desc), self._settings(settings)
        ms = np.empty(iters, np.float32)
        self._check(self.L.arctic_time_shade(self.h, C.byref(s), C.byref(st), warmup, iters, _ptr(ms)))
        return ms

    def read_gbuffer(self, want=("attrs", "material", "depth", "tri")):
        n = (self.rows, self.width)
        attrs = np.empty(n + (18,), np.float32) if "attrs" in want else None
        mat = np.empty(n, np.uint32) if "material" in want else None
        depth = np.empty(n, np.float32) if "depth" in want else None
        tri = np.empty(n, np.uint32) if "tri" in want else None
        self._check(self.L.arctic_read_gbuffer(self.h, _ptr(attrs), _ptr(mat), _ptr(depth), _ptr(tri)))
        return attrs, mat, depth, tri

    def write_gbuffer(self, attrs, material):
        a = np.ascontiguousarray(attrs, dtype=np.float32)
        m = np.ascontiguousarray(material, dtype=np.uint32)
        if a.shape != (self.rows, self.width, 18) or m.shape != (self.rows, self.width):
            raise ArcticError(-1, f"write_gbuffer: expected {(self.rows, self.width, 18)}, got {a.shape}")
        self._check(self.L.arctic_write_gbuffer(self.h, _ptr(a), _ptr(m)))

    def read_lod(self):
        """the level-of-detail plane of the G-buffer in place (set_option("texture_mips", 1)): (rows, width) float32"""
        lod = np.empty((self.rows, self.width), np.float32)
        self._check(self.L.arctic_read_lod(self.h, _ptr(lod)))
        return lod

    def write_lod(self, lod):
        """inject a level-of-detail plane next to the G-buffer in place (write_gbuffer resets it to 0)"""
        a = np.ascontiguousarray(lod, dtype=np.float32)
        if a.shape != (self.rows, self.width):
            raise ArcticError(-1, f"write_lod: expected {(self.rows, self.width)}, got {a.shape}")
        self._check(self.L.arctic_write_lod(self.h, _ptr(a)))

    def read_material_mip(self, material, level):
        """level `level` of a material's chain (arctic_read_material_mip): (h, w, 8) uint8, per texel {diffuse r, g, b, normal r, g, b,
        metal-rough g, b}; level 0 = the images as uploaded"""
        dims = np.zeros(2, np.uint32)
        self._check(self.L.arctic_read_material_mip(self.h, int(material), int(level), None, _ptr(dims)))
        t = np.empty((int(dims[1]), int(dims[0]), 8), np.uint8)
        self._check(self.L.arctic_read_material_mip(self.h, int(material), int(level), _ptr(t), _ptr(dims)))
        return t

    def read_shadow_map(self):
        d = np.empty((self.shadow_size, self.shadow_size), np.float32)
        self._check(self.L.arctic_read_shadow_map(self.h, _ptr(d)))
        return d

    def write_shadow_map(self, depth):
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.shape != (self.shadow_size, self.shadow_size):
            raise ArcticError(-1, "write_shadow_map: wrong shape")
        self._check(self.L.arctic_write_shadow_map(self.h, _ptr(d)))

    def _point_shadow_size(self):
        return self._options.get("point_shadow_size", 1024)

    def read_point_shadow(self, light):
        """the 6 faces of shadow-casting point light `light`: (6, F, F) float32, faces +X, -X, +Y, -Y, +Z, -Z"""
        F = self._point_shadow_size()
        d = np.empty((6, F, F), np.float32)
        self._check(self.L.arctic_read_point_shadow(self.h, int(light), _ptr(d)))
        return d

    def write_point_shadow(self, light, faces):
        F = self._point_shadow_size()
        d = np.ascontiguousarray(faces, dtype=np.float32)
        if d.shape != (6, F, F):
            raise ArcticError(-1, f"write_point_shadow: expected {(6, F, F)}, got {d.shape}")
        self._check(self.L.arctic_write_point_shadow(self.h, int(light), _ptr(d)))

    def read_output(self, want=("ldr", "hdr", "rgba8")):
        n = (self.rows, self.width)
        ldr = np.empty(n + (3,), np.float32) if "ldr" in want else None
        hdr = np.empty(n + (3,), np.float32) if "hdr" in want else None
        rgba = np.empty(n + (4,), np.uint8) if "rgba8" in want else None
        self._check(self.L.arctic_read_output(self.h, _ptr(ldr), _ptr(hdr), _ptr(rgba)))
        return ldr, hdr, rgba

    def stats(self):
        s = np.zeros(16, np.uint64)
        self._check(self.L.arctic_stats(self.h, _ptr(s), 16))
        return s

    def tile_trace(self):
        """(tiles_y, tiles_x, 4) uint64 of the latest shading pass under set_option("tile_trace", 1): start, end (100 MHz
        reference clock), HW_ID | XCC_ID << 32, 1 = fast tile | shader-clock ticks << 8 (arctic_read_tile_trace)."""
        tx, ty = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.arctic_read_tile_trace(self.h, None, 0, C.byref(tx), C.byref(ty)))
        out = np.zeros((ty.value, tx.value, 4), np.uint64)
        self._check(self.L.arctic_read_tile_trace(self.h, _ptr(out), tx.value * ty.value, C.byref(tx), C.byref(ty)))
        return out

    def tile_order(self):
        """(order, classes): the dispatch order arctic_pass_gbuffer left for the shading pass -- one uint32 per strip of 4 tiles,
        ty << 16 | strip column -- and the (tiles_y, tiles_x) uint8 cost classes it was built from (arctic_read_tile_order)."""
        tx, ty = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.arctic_read_tile_order(self.h, None, None, 0, C.byref(tx), C.byref(ty)))
        order = np.zeros(((tx.value + 3) // 4) * ty.value, np.uint32)
        classes = np.zeros((ty.value, tx.value), np.uint8)
        self._check(self.L.arctic_read_tile_order(self.h, _ptr(order), _ptr(classes), tx.value * ty.value, C.byref(tx), C.byref(ty)))
        return order, classes

    def bin_counts(self, shadow_pass=False):
        """(blocks_y, blocks_x) uint32: work items per 16x16 block of the latest forward / shadow prepass drawn with block
        owners (arctic_read_bin_counts)."""
        bx, by = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.arctic_read_bin_counts(self.h, int(shadow_pass), None, 0, C.byref(bx), C.byref(by)))
        out = np.zeros((by.value, bx.value), np.uint32)
        self._check(self.L.arctic_read_bin_counts(self.h, int(shadow_pass), _ptr(out), bx.value * by.value, C.byref(bx), C.byref(by)))
        return out

    def cull_counts(self, shadow_pass=False):
        """(clusters, clusters skipped, vertex blocks, vertex blocks skipped) of the latest prepass that ran under debug bit 10
        (arctic_read_cull_counts)."""
        out = np.zeros(4, np.uint32)
        self._check(self.L.arctic_read_cull_counts(self.h, int(shadow_pass), _ptr(out)))
        return out

    def read_env_lighting(self, level=None):
        """the tables of set_option("env_lighting", 1) (arctic_read_env_lighting): (sh (9, 3) float32 -- E(n) = sum_k sh[k] Y_k(n), A_l
        folded in --, lut (64, 64, 2) float32 (A, B), row = roughness cell, column = n.v cell, levels: list of (h, w, 4) float32, level 0 =
        the environment map); level=k returns only that level in the list."""
        dims = np.zeros(4, np.uint32)
        self._check(self.L.arctic_read_env_lighting(self.h, None, None, 0, None, _ptr(dims)))
        n_levels, side = int(dims[2]), int(dims[3])
        sh, lut = np.empty(27, np.float32), np.empty((side, side, 2), np.float32)
        self._check(self.L.arctic_read_env_lighting(self.h, _ptr(sh), _ptr(lut), 0, None, None))
        levels = []
        for k in (range(n_levels) if level is None else [level]):
            self._check(self.L.arctic_read_env_lighting(self.h, None, None, k, None, _ptr(dims)))
            t = np.empty((int(dims[1]), int(dims[0]), 4), np.float32)
            self._check(self.L.arctic_read_env_lighting(self.h, None, None, k, _ptr(t), None))
            levels.append(t)
        return sh.reshape(9, 3), lut, levels

    def set_option(self, name, value):
        self._check(self.L.arctic_set_option(self.h, binding.OPTIONS[name], int(value)))
        self._options[name] = int(value)


def check_material_params(params):
    """arctic_check_material_params: True when one MATERIAL_PARAMS_DTYPE record is valid (host only, no handle)"""
    p = np.ascontiguousarray(params, dtype=MATERIAL_PARAMS_DTYPE).reshape(1)
    return binding.lib().arctic_check_material_params(p.ctypes.data) == 0


def check_mesh_skin(skin, n_joints):
    """arctic_check_mesh_skin: True when the SKIN_VERTEX_DTYPE records are valid for n_joints joints (host only, no handle)"""
    s = np.ascontiguousarray(skin, dtype=SKIN_VERTEX_DTYPE)
    return binding.lib().arctic_check_mesh_skin(_ptr(s) if len(s) else None, len(s), int(n_joints)) == 0


def skin_vertices(vertices, skin, joint_matrices):
    """arctic_skin_vertices: the skinning arithmetic of include/arctic_hip.h on the host -- the posed VERTEX_DTYPE records.  Invalid input
    raises ArcticError (ARCTIC_E_INVALID)."""
    v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
    s = np.ascontiguousarray(skin, dtype=SKIN_VERTEX_DTYPE)
    j = np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1, 16)
    if len(s) != len(v):
        raise ArcticError(-1, "skin_vertices: one skin record per vertex")
    out = np.empty_like(v)
    rc = binding.lib().arctic_skin_vertices(_ptr(v), _ptr(s), len(v), _ptr(j), len(j), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "skin_vertices: invalid skin records or matrices")
    return out


def check_morph_targets(deltas):
    """arctic_check_morph_targets: True when the (n_targets, n_vertices) MORPH_DELTA_DTYPE records are valid (host only, no handle)"""
    d = np.ascontiguousarray(deltas, dtype=MORPH_DELTA_DTYPE)
    if d.ndim != 2:
        return False
    return binding.lib().arctic_check_morph_targets(_ptr(d) if d.size else None, d.shape[1], d.shape[0]) == 0


def morph_vertices(vertices, deltas, weights):
    """arctic_morph_vertices: the morph-target arithmetic of include/arctic_hip.h on the host -- the blended VERTEX_DTYPE records for
    (n_targets, n_vertices) MORPH_DELTA_DTYPE deltas and n_targets weights.  Invalid input raises ArcticError (ARCTIC_E_INVALID)."""
    v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
    d = np.ascontiguousarray(deltas, dtype=MORPH_DELTA_DTYPE)
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if d.ndim != 2 or d.shape[1] != len(v) or d.shape[0] != len(w):
        raise ArcticError(-1, "morph_vertices: deltas must be (n_targets, n_vertices) records, one weight per target")
    out = np.empty_like(v)
    rc = binding.lib().arctic_morph_vertices(_ptr(v), _ptr(d), len(v), len(w), _ptr(w), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "morph_vertices: invalid deltas or weights")
    return out


def refit_triangles(triangles_build, triangles_now, rays, any_hit=False, brute=False, structure=False):
    """arctic_refit_triangles: the refit of include/arctic_hip.h on the host -- a structure built on triangles_build, refitted to triangles_now (the
    same count, prim = the array index), walked: HIT_DTYPE records; structure=True: (hits, RAY_NODE_DTYPE nodes, RAY_TRI_DTYPE leaf triangles)."""
    a = np.ascontiguousarray(triangles_build, dtype=np.float32).reshape(-1, 9)
    b = np.ascontiguousarray(triangles_now, dtype=np.float32).reshape(-1, 9)
    if len(a) != len(b):
        raise ValueError("refit_triangles: the two triangle lists differ in length")
    ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
    hits = np.empty(len(ry), HIT_DTYPE)
    flags = (binding.TRACE_ANY if any_hit else 0) | (binding.TRACE_BRUTE if brute else 0)
    cap = len(a) if structure else 0
    nodes, tris, counts = np.zeros(2 * cap, RAY_NODE_DTYPE), np.zeros(cap, RAY_TRI_DTYPE), np.zeros(2, np.uint64)
    rc = binding.lib().arctic_refit_triangles(_ptr(a) if len(a) else None, _ptr(b) if len(b) else None, len(a), _ptr(ry) if len(ry) else None, len(ry), flags,
                                              _ptr(hits) if len(ry) else None, _ptr(nodes) if cap else None, len(nodes), _ptr(tris) if cap else None, len(tris), _ptr(counts))
    if rc < 0:
        raise ArcticError(rc, "refit_triangles")
    return (hits, nodes[:int(counts[0])].copy(), tris[:int(counts[1])].copy()) if structure else hits


def resplit_triangles(triangles_build, triangles_now, rays, any_hit=False, brute=False, structure=False):
    """arctic_resplit_triangles: the re-split of include/arctic_hip.h on the host -- a structure built on triangles_build, its slots reordered by
    the builder's rule applied to triangles_now, refitted and walked.  Returns what refit_triangles returns."""
    a = np.ascontiguousarray(triangles_build, dtype=np.float32).reshape(-1, 9)
    b = np.ascontiguousarray(triangles_now, dtype=np.float32).reshape(-1, 9)
    if len(a) != len(b):
        raise ValueError("resplit_triangles: the two triangle lists differ in length")
    ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
    hits = np.empty(len(ry), HIT_DTYPE)
    flags = (binding.TRACE_ANY if any_hit else 0) | (binding.TRACE_BRUTE if brute else 0)
    cap = len(a) if structure else 0
    nodes, tris, counts = np.zeros(2 * cap, RAY_NODE_DTYPE), np.zeros(cap, RAY_TRI_DTYPE), np.zeros(2, np.uint64)
    rc = binding.lib().arctic_resplit_triangles(_ptr(a) if len(a) else None, _ptr(b) if len(b) else None, len(a), _ptr(ry) if len(ry) else None, len(ry), flags,
                                                _ptr(hits) if len(ry) else None, _ptr(nodes) if cap else None, len(nodes), _ptr(tris) if cap else None, len(tris), _ptr(counts))
    if rc < 0:
        raise ArcticError(rc, "resplit_triangles")
    return (hits, nodes[:int(counts[0])].copy(), tris[:int(counts[1])].copy()) if structure else hits


def trace_triangles(triangles, rays, any_hit=False, brute=False):
    """arctic_trace_triangles: the ray queries of include/arctic_hip.h on the host -- (n, 9) or (n, 3, 3) float32 world-space triangles (prim = the
    array index) against RAY_DTYPE records: HIT_DTYPE records.  brute: loop over every triangle instead of the acceleration structure."""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE).ravel()
    hits = np.empty(len(ry), HIT_DTYPE)
    flags = (binding.TRACE_ANY if any_hit else 0) | (binding.TRACE_BRUTE if brute else 0)
    rc = binding.lib().arctic_trace_triangles(_ptr(t) if len(t) else None, len(t), _ptr(ry) if len(ry) else None, len(ry), flags, _ptr(hits) if len(ry) else None)
    if rc < 0:
        raise ArcticError(rc, "trace_triangles")
    return hits


def interpolate_hits(vertices, indices, trs, light_proj_view, material, first_prim, hits, attrs, material_out):
    """arctic_interpolate_hits: the hit attributes of include/arctic_hip.h on the host, for ONE object -- its mesh (VERTEX_DTYPE records, uint32
    indices), its trs and the sun's matrix (16 floats each, [col][row]), the mesh's material, the prim of its first triangle.  Fills attrs
    ((n, 18) float32) and material_out ((n,) uint32) IN PLACE for the hits whose prim is one of the object's; the others are left as they are."""
    v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE).ravel()
    ix = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    m, l = np.ascontiguousarray(trs, dtype=np.float32).reshape(16), np.ascontiguousarray(light_proj_view, dtype=np.float32).reshape(16)
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).ravel()
    assert attrs.dtype == np.float32 and attrs.flags.c_contiguous and attrs.shape == (len(h), 18)
    assert material_out.dtype == np.uint32 and material_out.flags.c_contiguous and material_out.shape == (len(h),)
    rc = binding.lib().arctic_interpolate_hits(_ptr(v) if len(v) else None, len(v), _ptr(ix) if len(ix) else None, len(ix), _ptr(m), _ptr(l), int(material),
                                               int(first_prim), _ptr(h) if len(h) else None, len(h), _ptr(attrs) if len(h) else None,
                                               _ptr(material_out) if len(h) else None)
    if rc < 0:
        raise ArcticError(rc, "interpolate_hits")


def _ao_arguments(dirs, n_rays, pattern, radius, bias, filter, normal_cos, plane_dist):
    """(one AO_DTYPE record, the table as a flat float32 array).  n_rays / pattern: from a (P * P, n_rays, 3) table where not given; the library
    checks every value"""
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if n_rays is None:
        n_rays = d.shape[1] if d.ndim == 3 else 0
    if pattern is None:
        pattern = {1: 1, 4: 2, 16: 4}.get(d.shape[0] if d.ndim == 3 else 0, 0)
    if d.size < int(pattern) ** 2 * int(n_rays) * 3:
        raise ArcticError(-1, "ambient occlusion: the direction table is smaller than pattern * pattern * n_rays * 3 floats")
    ao = np.zeros(1, AO_DTYPE)
    ao["n_rays"], ao["pattern"], ao["radius"], ao["bias"] = n_rays, pattern, radius, bias
    ao["filter"], ao["normal_cos"], ao["plane_dist"] = int(filter), normal_cos, plane_dist
    return ao, d.reshape(-1)


def ambient_occlusion_points(triangles, points, sets, dirs, n_rays=None, pattern=None, radius=np.inf, bias=1e-3, brute=False):
    """arctic_ambient_occlusion_points: the ambient occlusion of include/arctic_hip.h on the host -- how many of the n_rays rays of each point
    {world3, normal3} ((n, 6) float32) hit one of the (n, 9) world-space triangles, with direction set sets[k] of dirs: (n,) uint8.  brute: loop
    over every triangle instead of the acceleration structure."""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    st = np.ascontiguousarray(sets, dtype=np.uint32).ravel()
    if len(st) != len(p):
        raise ArcticError(-1, "ambient_occlusion_points: one set per point")
    ao, d = _ao_arguments(dirs, n_rays, pattern, radius, bias, False, 0.0, 0.0)
    hits = np.empty(len(p), np.uint8)
    rc = binding.lib().arctic_ambient_occlusion_points(_ptr(t) if len(t) else None, len(t), _ptr(p) if len(p) else None, _ptr(st) if len(p) else None, len(p),
                                                       _ptr(ao), _ptr(d), binding.TRACE_BRUTE if brute else 0, _ptr(hits) if len(p) else None)
    if rc < 0:
        raise ArcticError(rc, "ambient_occlusion_points")
    return hits


def gi_arguments(dirs, n_rays=None, pattern=None, max_distance=np.inf, bias=1e-3, clamp_max=65504.0, filter=False, normal_cos=0.9, plane_dist=0.05):
    """(one GI_DTYPE record, the table as a flat float32 array).  n_rays / pattern: from a (P * P, n_rays, 3) table where not given; the library
    checks every value"""
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if n_rays is None:
        n_rays = d.shape[1] if d.ndim == 3 else 0
    if pattern is None:
        pattern = {1: 1, 4: 2, 16: 4}.get(d.shape[0] if d.ndim == 3 else 0, 0)
    if d.size < int(pattern) ** 2 * int(n_rays) * 3:
        raise ArcticError(-1, "indirect light: the direction table is smaller than pattern * pattern * n_rays * 3 floats")
    gi = np.zeros(1, GI_DTYPE)
    gi["n_rays"], gi["pattern"], gi["max_distance"], gi["bias"], gi["clamp_max"] = n_rays, pattern, max_distance, bias, clamp_max
    gi["filter"], gi["normal_cos"], gi["plane_dist"] = int(filter), normal_cos, plane_dist
    return gi, d.reshape(-1)


def gi_history_arguments(max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0):
    """one GI_HISTORY_DTYPE record; the library checks every value"""
    h = np.zeros(1, GI_HISTORY_DTYPE)
    h["max_history"], h["normal_cos"], h["plane_dist"], h["min_weight"] = max_history, normal_cos, plane_dist, min_weight
    return h


def gi_compose_arguments(gi_strength=1.0, ambient_scale=1.0, flags=0):
    """one GI_COMPOSE_DTYPE record; the library checks every value"""
    c = np.zeros(1, GI_COMPOSE_DTYPE)
    c["flags"], c["gi_strength"], c["ambient_scale"] = flags, gi_strength, ambient_scale
    return c


def gi_accumulate_pixels(world, normal, geometry, cur, prev_proj_view=None, width=1, height=1, prev=None, hist=None, **kw):
    """arctic_gi_accumulate_pixels: stage 5 on the host for n pixels in any order -- world, normal (n, 3), geometry (n,), cur (n, 4) = E;
    prev_proj_view: the previous call's (4, 4) matrix, None = the history is empty; prev = (acc (w * h, 3), count, world, normal) row-major.
    Returns (out (n, 4) = {acc, N}, acc (n, 3), count (n,), world (n, 3), normal (n, 3)) float32."""
    f = lambda a, k: np.ascontiguousarray(a, dtype=np.float32).reshape(-1, k) if k > 1 else np.ascontiguousarray(a, dtype=np.float32).ravel()
    w, nr, c = f(world, 3), f(normal, 3), f(cur, 4)
    g = np.ascontiguousarray(geometry, dtype=np.uint8).ravel()
    n = len(w)
    if any(len(x) != n for x in (nr, g, c)):
        raise ArcticError(-1, "gi_accumulate_pixels: one entry of every array per pixel")
    h = gi_history_arguments(**kw) if hist is None else hist
    P = None if prev_proj_view is None else np.ascontiguousarray(prev_proj_view, dtype=np.float32).reshape(16)
    pa = pc = pw = pn = None
    if P is not None:
        pa, pc, pw, pn = f(prev[0], 3), f(prev[1], 1), f(prev[2], 3), f(prev[3], 3)
        if any(len(x) != int(width) * int(height) for x in (pa, pc, pw, pn)):
            raise ArcticError(-1, "gi_accumulate_pixels: the previous history is not width * height entries")
    out = np.empty((n, 4), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    p = (lambda a: _ptr(a) if n else None)
    rc = binding.lib().arctic_gi_accumulate_pixels(_ptr(h), n, p(w), p(nr), p(g), p(c), _ptr(P), int(width), int(height), _ptr(pa), _ptr(pc), _ptr(pw), _ptr(pn),
                                                   *[p(o) for o in out])
    if rc < 0:
        raise ArcticError(rc, "gi_accumulate_pixels")
    return out


def gi_compose_pixels(hdr, base, metal, gi, geometry, ambient, gi_strength=1.0, ambient_scale=1.0, flags=0, compose=None):
    """arctic_gi_compose_pixels: stage 6's two terms on the host, on channels sampled already: hdr, base (n, 3), metal (n,), gi (n, 4) = E,
    geometry (n,) -> (n, 3) float32"""
    h, b = (np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in (hdr, base))
    m, e = np.ascontiguousarray(metal, dtype=np.float32).ravel(), np.ascontiguousarray(gi, dtype=np.float32).reshape(-1, 4)
    g = np.ascontiguousarray(geometry, dtype=np.uint8).ravel()
    n = len(h)
    if any(len(x) != n for x in (b, m, e, g)):
        raise ArcticError(-1, "gi_compose_pixels: one entry of every array per pixel")
    c = gi_compose_arguments(gi_strength, ambient_scale, flags) if compose is None else compose
    out = np.empty((n, 3), np.float32)
    p = (lambda a: _ptr(a) if n else None)
    rc = binding.lib().arctic_gi_compose_pixels(_ptr(c), float(ambient), n, p(h), p(b), p(m), p(e), p(g), p(out))
    if rc < 0:
        raise ArcticError(rc, "gi_compose_pixels")
    return out


def gi_points(points, sets, dirs, round, **kw):
    """arctic_gi_points: round `round`'s ray of each point {world3, normal3} ((n, 6) float32) with direction set sets[k] of dirs: (n,) RAY_DTYPE,
    the all-zero record for a point that is not covered.  No handle, no GPU."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
    st = np.ascontiguousarray(sets, dtype=np.uint32).ravel()
    if len(st) != len(p):
        raise ArcticError(-1, "gi_points: one set per point")
    gi, d = gi_arguments(dirs, **kw)
    rays = np.empty(len(p), RAY_DTYPE)
    rc = binding.lib().arctic_gi_points(_ptr(p) if len(p) else None, _ptr(st) if len(p) else None, len(p), _ptr(gi), _ptr(d), int(round), _ptr(rays) if len(p) else None)
    if rc < 0:
        raise ArcticError(rc, "gi_points")
    return rays


def gi_estimate_pixels(rays, colors, normal=None, world=None, geometry=None, gi=None, **kw):
    """arctic_gi_estimate_pixels: stages 3 and 4 on the host.  rays (n_rays, h, w) RAY_DTYPE and colors (n_rays, h, w, 4) float32, round after
    round; with the filter normal and world (h, w, 3) and geometry (h, w) as well: -> (S, E), (h, w, 4) float32 each.  gi: a GI_DTYPE record,
    or keywords as trace_gi takes them (n_rays and pattern included: no table is read)."""
    ry = np.ascontiguousarray(rays, dtype=RAY_DTYPE)
    n_rays, h, w = ry.shape
    c = np.ascontiguousarray(colors, dtype=np.float32).reshape(n_rays, h, w, 4)
    if gi is None:
        P = int(kw.pop("pattern", 1))
        kw.pop("n_rays", None)   # (the rounds given are the rounds summed)
        gi, _ = gi_arguments(np.zeros((P * P, n_rays, 3), np.float32), n_rays=n_rays, pattern=P, **kw)
    f3 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(h, w, 3)
    nm, wd = f3(normal), f3(world)
    geo = None if geometry is None else np.ascontiguousarray(geometry, dtype=np.uint8).reshape(h, w)
    S, E = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
    rc = binding.lib().arctic_gi_estimate_pixels(_ptr(gi), w, h, _ptr(ry), _ptr(c), _ptr(nm), _ptr(wd), _ptr(geo), _ptr(S), _ptr(E))
    if rc < 0:
        raise ArcticError(rc, "gi_estimate_pixels")
    return S, E


def _compose_arguments(flags, ao_strength, reflection_strength, reflection_bias):
    """one COMPOSE_DTYPE record; the library checks every value"""
    c = np.zeros(1, COMPOSE_DTYPE)
    c["flags"], c["ao_strength"], c["reflection_strength"], c["reflection_bias"] = flags, ao_strength, reflection_strength, reflection_bias
    return c


def compose_pixels(hdr, base, metal, rough, normal, world, geometry, eye, ambient, ao=None, refl=None, ao_strength=1.0, reflection_strength=1.0, flags=None):
    """arctic_compose_pixels: the composition of include/arctic_hip.h on the host, in front of the tonemapper -- (n, 3) float32 composed HDR colours
    from (n, 3) hdr, the sampled channels base (n, 3), metal, rough (n,), the G-buffer's normal and world (n, 3), geometry (n,) bool, ao (n,) uint8
    and refl (n, 4) float32; flags default to the planes given."""
    f = lambda a, k: np.ascontiguousarray(a, dtype=np.float32).reshape((-1, k) if k > 1 else (-1,))
    h, b, m, r, nr, w = f(hdr, 3), f(base, 3), f(metal, 1), f(rough, 1), f(normal, 3), f(world, 3)
    g = np.ascontiguousarray(np.asarray(geometry) != 0, dtype=np.uint8).ravel()
    a = None if ao is None else np.ascontiguousarray(ao, dtype=np.uint8).ravel()
    rf = None if refl is None else f(refl, 4)
    n = len(h)
    if any(len(x) != n for x in (b, m, r, nr, w, g)) or (a is not None and len(a) != n) or (rf is not None and len(rf) != n):
        raise ArcticError(-1, "compose_pixels: one entry of every array per pixel")
    if flags is None:
        flags = (binding.COMPOSE_AO if a is not None else 0) | (binding.COMPOSE_REFLECTIONS if rf is not None else 0)
    c = _compose_arguments(flags, ao_strength, reflection_strength, 0.0)
    e = np.ascontiguousarray(eye, dtype=np.float32).reshape(3)
    out = np.empty((n, 3), np.float32)
    rc = binding.lib().arctic_compose_pixels(_ptr(c), _ptr(e), float(ambient), n, _ptr(h), _ptr(b), _ptr(m), _ptr(r), _ptr(nr), _ptr(w), _ptr(a), _ptr(rf), _ptr(g), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "compose_pixels")
    return out


def _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight):
    """one AO_HISTORY_DTYPE record; the library checks every value"""
    h = np.zeros(1, AO_HISTORY_DTYPE)
    h["max_history"], h["normal_cos"], h["plane_dist"], h["min_weight"] = max_history, normal_cos, plane_dist, min_weight
    return h


def accumulate_pixels(world, normal, geometry, cur, prev_proj_view=None, width=1, height=1, prev=None, max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0,
                      hist=None):
    """arctic_accumulate_pixels: the temporal accumulation of include/arctic_hip.h on the host, for n pixels in any order -- world, normal (n, 3),
    geometry (n,) bool, cur (n,) uint8; prev_proj_view: the previous call's (4, 4) matrix as frame_constants gives it, None = an empty history;
    prev: (value, count, world, normal) of the previous call's width x height frame, as read_ao_history returns them.  Returns (byte (n,) uint8,
    value (n,), N (n,), world (n, 3), normal (n, 3)): the output and the history entry written."""
    f = lambda a, k: np.ascontiguousarray(a, dtype=np.float32).reshape((-1, k) if k > 1 else (-1,))
    w, nr = f(world, 3), f(normal, 3)
    g = np.ascontiguousarray(np.asarray(geometry) != 0, dtype=np.uint8).ravel()
    c = np.ascontiguousarray(cur, dtype=np.uint8).ravel()
    n = len(w)
    if any(len(x) != n for x in (nr, g, c)):
        raise ArcticError(-1, "accumulate_pixels: one entry of every array per pixel")
    h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
    P = None if prev_proj_view is None else np.ascontiguousarray(prev_proj_view, dtype=np.float32).reshape(16)
    pv = pc = pw = pn = None
    if P is not None:
        pv, pc, pw, pn = f(prev[0], 1), f(prev[1], 1), f(prev[2], 3), f(prev[3], 3)
        if any(len(x) != int(width) * int(height) for x in (pv, pc, pw, pn)):
            raise ArcticError(-1, "accumulate_pixels: the previous history is not width * height entries")
    out = np.empty(n, np.uint8), np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    p = (lambda a: _ptr(a) if n else None)
    rc = binding.lib().arctic_accumulate_pixels(_ptr(h), n, p(w), p(nr), p(g), p(c), _ptr(P), int(width), int(height), _ptr(pv), _ptr(pc), _ptr(pw), _ptr(pn),
                                                *[p(o) for o in out])
    if rc < 0:
        raise ArcticError(rc, "accumulate_pixels")
    return out


def motion_pixels(bary, obj, prev_pos, pixel_xy, prev_trs, prev_proj_view=None, width=1, height=1):
    """arctic_motion_pixels: steps 3 to 5 of the motion vectors of include/arctic_hip.h on the host, for n pixels in any order -- bary (n, 3),
    obj (n,) uint32 (0xFFFFFFFF: no geometry), prev_pos (n, 3, 3) the previous object-space positions of the pixel's three vertices, pixel_xy
    (n, 2) int32, prev_trs (n_objects, 16) the previous call's trs by object; prev_proj_view: the previous call's (4, 4) matrix, None = M is
    empty.  Returns (prev_world4 (n, 4), velocity2 (n, 2)) float32."""
    b = np.ascontiguousarray(bary, dtype=np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(obj, dtype=np.uint32).ravel()
    q = np.ascontiguousarray(prev_pos, dtype=np.float32).reshape(-1, 9)
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    t = np.ascontiguousarray(prev_trs, dtype=np.float32).reshape(-1, 16)
    n = len(b)
    if any(len(x) != n for x in (o, q, xy)):
        raise ArcticError(-1, "motion_pixels: one entry of every array per pixel")
    P = None if prev_proj_view is None else np.ascontiguousarray(prev_proj_view, dtype=np.float32).reshape(16)
    pw, vel = np.empty((n, 4), np.float32), np.empty((n, 2), np.float32)
    p = (lambda a: _ptr(a) if len(a) else None)
    rc = binding.lib().arctic_motion_pixels(n, p(b), p(o), p(q), p(xy), p(t), len(t), _ptr(P), int(width), int(height), p(pw), p(vel))
    if rc < 0:
        raise ArcticError(rc, "motion_pixels")
    return pw, vel


def accumulate_pixels_motion(world, prev_world4, normal, geometry, cur, prev_proj_view=None, width=1, height=1, prev=None, max_history=32.0, normal_cos=0.9, plane_dist=0.05,
                             min_weight=0.0, hist=None):
    """arctic_accumulate_pixels_motion: accumulate_pixels with one more input, prev_world4 (n, 4) -- every pixel's previous point and flag as
    motion_vectors gives them.  Returns what accumulate_pixels returns."""
    f = lambda a, k: np.ascontiguousarray(a, dtype=np.float32).reshape((-1, k) if k > 1 else (-1,))
    w, pw4, nr = f(world, 3), f(prev_world4, 4), f(normal, 3)
    g = np.ascontiguousarray(np.asarray(geometry) != 0, dtype=np.uint8).ravel()
    c = np.ascontiguousarray(cur, dtype=np.uint8).ravel()
    n = len(w)
    if any(len(x) != n for x in (pw4, nr, g, c)):
        raise ArcticError(-1, "accumulate_pixels_motion: one entry of every array per pixel")
    h = _ao_history_arguments(max_history, normal_cos, plane_dist, min_weight) if hist is None else hist
    P = None if prev_proj_view is None else np.ascontiguousarray(prev_proj_view, dtype=np.float32).reshape(16)
    pv = pc = pw = pn = None
    if P is not None:
        pv, pc, pw, pn = f(prev[0], 1), f(prev[1], 1), f(prev[2], 3), f(prev[3], 3)
        if any(len(x) != int(width) * int(height) for x in (pv, pc, pw, pn)):
            raise ArcticError(-1, "accumulate_pixels_motion: the previous history is not width * height entries")
    out = np.empty(n, np.uint8), np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    p = (lambda a: _ptr(a) if n else None)
    rc = binding.lib().arctic_accumulate_pixels_motion(_ptr(h), n, p(w), p(pw4), p(nr), p(g), p(c), _ptr(P), int(width), int(height), _ptr(pv), _ptr(pc), _ptr(pw), _ptr(pn),
                                                       *[p(o) for o in out])
    if rc < 0:
        raise ArcticError(rc, "accumulate_pixels_motion")
    return out


def _taa_arguments(flags, max_history, min_weight, jitter):
    """one TAA_DTYPE record; the library checks every value"""
    t = np.zeros(1, TAA_DTYPE)
    t["flags"], t["max_history"], t["min_weight"], t["jitter"] = flags, max_history, min_weight, jitter
    return t


def taa_pixels(pixel_xy, cur, velocity2=None, prev=None, jitter=(0.0, 0.0), max_history=8.0, min_weight=0.0, flags=0, taa=None):
    """arctic_taa_pixels: steps 1 to 6 of the resolve of include/arctic_hip.h on the host, for n pixels in any order -- pixel_xy (n, 2) int32, cur
    the WHOLE frame's colour (height, width, 3), velocity2 (n, 2) or None = zero, prev the whole frame's previous {r, g, b, N} (height, width, 4)
    or None = an empty history.  Returns (n, 4) float32 {out, N}."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(cur, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "taa_pixels: cur is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    n = len(xy)
    v = None if velocity2 is None else np.ascontiguousarray(velocity2, dtype=np.float32).reshape(-1, 2)
    pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.float32)
    if (v is not None and len(v) != n) or (pv is not None and pv.shape != (height, width, 4)):
        raise ArcticError(-1, "taa_pixels: one velocity per pixel, and the previous history is (height, width, 4)")
    t = _taa_arguments(flags, max_history, min_weight, jitter) if taa is None else taa
    out = np.empty((n, 4), np.float32)
    rc = binding.lib().arctic_taa_pixels(_ptr(t), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(v) if n else None, _ptr(pv), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "taa_pixels")
    return out


def taa_upscale_arguments(out_size, jitter=(0.0, 0.0), max_history=32.0, min_weight=0.0, sharpness=1.0, confidence_floor=2.0 ** -6, flags=0):
    """one TAA_UPSCALE_DTYPE record for an output of out_size = (W, H); the library checks every value"""
    t = np.zeros(1, TAA_UPSCALE_DTYPE)
    t["flags"], t["max_history"], t["min_weight"], t["jitter"], t["sharpness"], t["confidence_floor"] = flags, max_history, min_weight, jitter, sharpness, confidence_floor
    t["out_width"], t["out_height"] = int(out_size[0]), int(out_size[1])
    return t


def taa_upscale_pixels(pixel_xy, cur, out_size, velocity2=None, prev=None, upscale=None, **kw):
    """arctic_taa_upscale_pixels: steps 1 to 6 of the upscaler of include/arctic_hip.h on the host, for n OUTPUT pixels in any order -- pixel_xy
    (n, 2) int32 inside out_size = (W, H), cur the WHOLE input frame's colour (height, width, 3), velocity2 the whole input frame's (height,
    width, 2) or None = zero, prev the whole previous {r, g, b, N} (H, W, 4) or None = an empty history.  Returns (n, 4) float32 {out, N}."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(cur, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "taa_upscale_pixels: cur is the whole input frame, (height, width, 3)")
    height, width = c.shape[:2]
    n = len(xy)
    t = taa_upscale_arguments(out_size, **kw) if upscale is None else upscale
    v = None if velocity2 is None else np.ascontiguousarray(velocity2, dtype=np.float32)
    pv = None if prev is None else np.ascontiguousarray(prev, dtype=np.float32)
    if (v is not None and v.shape != (height, width, 2)) or (pv is not None and pv.shape != (int(t["out_height"][0]), int(t["out_width"][0]), 4)):
        raise ArcticError(-1, "taa_upscale_pixels: velocity2 is (height, width, 2), and the previous history is (H, W, 4)")
    out = np.empty((n, 4), np.float32)
    rc = binding.lib().arctic_taa_upscale_pixels(_ptr(t), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(v), _ptr(pv), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "taa_upscale_pixels")
    return out


def taa_upscale_jitter(index, in_size, out_size, exact=False):
    """arctic_taa_upscale_jitter: the jitter (jx, jy) of frame `index` for an upscale from in_size = (w, h) to out_size = (W, H), as two
    float32 -- Halton(2, 3) minus one half with period 8 * ceil(W / w) * ceil(H / h), or, exact=True and a ratio of 1, 2 or 4 on both axes,
    the s * s phases that put every output pixel's centre on a sample once.  For set_camera_jitter and the upscaler's `jitter`."""
    out = np.zeros(2, np.float32)
    i = (int(index) & 0x7FFFFFFF) | (binding.TAA_UPSCALE_JITTER_EXACT if exact else 0)
    rc = binding.lib().arctic_taa_upscale_jitter(i, int(in_size[0]), int(out_size[0]), int(in_size[1]), int(out_size[1]), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "taa_upscale_jitter")
    return out


def _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent):
    """one MOTION_BLUR_DTYPE record; the library checks every value"""
    m = np.zeros(1, MOTION_BLUR_DTYPE)
    m["flags"], m["shutter"], m["max_radius"], m["samples"], m["depth_extent"] = flags, shutter, max_radius, samples, depth_extent
    return m


def motion_blur_prepare(velocity2, depth=None, shutter=1.0, max_radius=16.0, samples=15, depth_extent=0.05, flags=0, mb=None):
    """arctic_motion_blur_prepare: steps 1 to 3 of the motion blur of include/arctic_hip.h on the host, for a whole frame -- velocity2 (height,
    width, 2), depth (height, width) or None = 0.  Returns (tile_max2, neighbour_max2) of shape (tiles_y, tiles_x, 2) and P (height, width, 2)."""
    v = np.ascontiguousarray(velocity2, dtype=np.float32)
    if v.ndim != 3 or v.shape[2] != 2:
        raise ArcticError(-1, "motion_blur_prepare: velocity2 is the whole frame, (height, width, 2)")
    height, width = v.shape[:2]
    z = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
    if z is not None and z.shape != (height, width):
        raise ArcticError(-1, "motion_blur_prepare: depth is (height, width)")
    m = _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent) if mb is None else mb
    t = ((height + 7) // 8, (width + 7) // 8, 2)
    tile, nb, prep = np.empty(t, np.float32), np.empty(t, np.float32), np.empty((height, width, 2), np.float32)
    rc = binding.lib().arctic_motion_blur_prepare(_ptr(m), int(width), int(height), _ptr(v), _ptr(z), _ptr(tile), _ptr(nb), _ptr(prep))
    if rc < 0:
        raise ArcticError(rc, "motion_blur_prepare")
    return tile, nb, prep


def motion_blur_pixels(pixel_xy, rgb, prepared, neighbour_max, shutter=1.0, max_radius=16.0, samples=15, depth_extent=0.05, flags=0, mb=None):
    """arctic_motion_blur_pixels: step 4 of the motion blur on the host, for n pixels in any order -- pixel_xy (n, 2) int32, rgb the WHOLE frame's
    colour (height, width, 3), prepared and neighbour_max as motion_blur_prepare returns them.  Returns (n, 3) float32."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "motion_blur_pixels: rgb is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    p, nb = np.ascontiguousarray(prepared, dtype=np.float32), np.ascontiguousarray(neighbour_max, dtype=np.float32)
    if p.shape != (height, width, 2) or nb.shape != ((height + 7) // 8, (width + 7) // 8, 2):
        raise ArcticError(-1, "motion_blur_pixels: prepared is (height, width, 2), neighbour_max (tiles_y, tiles_x, 2)")
    m = _motion_blur_arguments(flags, shutter, max_radius, samples, depth_extent) if mb is None else mb
    n = len(xy)
    out = np.empty((n, 3), np.float32)
    rc = binding.lib().arctic_motion_blur_pixels(_ptr(m), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(p), _ptr(nb), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "motion_blur_pixels")
    return out


def _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, z_near, z_far):
    """one DOF_DTYPE record; the library checks every value"""
    m = np.zeros(1, DOF_DTYPE)
    m["flags"], m["focus_distance"], m["coc_scale"], m["max_radius"], m["samples"], m["depth_extent"] = flags, focus_distance, coc_scale, max_radius, samples, depth_extent
    m["z_near"], m["z_far"] = z_near, z_far
    return m


def _dof_table(taps, m):
    """the tap table of a call: the caller's as contiguous float32, or Vogel's spiral for the record's sample count"""
    if taps is None:
        n = int(m["samples"][0])
        return dof_taps(n) if 1 <= n <= 64 else np.zeros((1, 2), np.float32)     # (the library refuses the count)
    t = np.ascontiguousarray(taps, dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != 2 or len(t) < int(m["samples"][0]):
        raise ArcticError(-1, "dof: taps is (samples, 2)")
    return t


def dof_taps(samples):
    """a tap table for depth of field: (samples, 2) float32 in the unit disc, Vogel's spiral -- tap i at the radius sqrt((i + 0.5) / samples) and
    the angle i times the golden angle -- computed in float64 and cast.  A convenience: the library takes any table inside the disc."""
    n = int(samples)
    i = np.arange(n, dtype=np.float64)
    r, phi = np.sqrt((i + 0.5) / n), i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi)], -1).astype(np.float32)


def dof_coc_scale(f_number, focal_length_mm, sensor_height_mm, focus_distance, height_px):
    """arctic_dof_coc_scale: the thin lens' radius of the circle of confusion at infinite distance, in pixels -- ArcticDof's coc_scale"""
    out = C.c_float(0.0)
    rc = binding.lib().arctic_dof_coc_scale(float(f_number), float(focal_length_mm), float(sensor_height_mm), float(focus_distance), int(height_px), C.byref(out))
    if rc < 0:
        raise ArcticError(rc, "dof_coc_scale")
    return float(out.value)


def dof_prepare(depth, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, samples=16, depth_extent=0.5, z_near=0.1, z_far=1000.0, flags=0, dof=None):
    """arctic_dof_prepare: steps 1 to 3 of depth of field of include/arctic_hip.h on the host, for a whole frame -- depth (height, width).
    Returns (tile_max, neighbour_max) of shape (tiles_y, tiles_x) and P (height, width, 2)."""
    z = np.ascontiguousarray(depth, dtype=np.float32)
    if z.ndim != 2:
        raise ArcticError(-1, "dof_prepare: depth is the whole frame, (height, width)")
    height, width = z.shape
    m = _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, z_near, z_far) if dof is None else dof
    t = ((height + 7) // 8, (width + 7) // 8)
    tile, nb, prep = np.empty(t, np.float32), np.empty(t, np.float32), np.empty((height, width, 2), np.float32)
    rc = binding.lib().arctic_dof_prepare(_ptr(m), int(width), int(height), _ptr(z), _ptr(tile), _ptr(nb), _ptr(prep))
    if rc < 0:
        raise ArcticError(rc, "dof_prepare")
    return tile, nb, prep


def dof_pixels(pixel_xy, rgb, prepared, neighbour_max, taps=None, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, samples=16, depth_extent=0.5, z_near=0.1, z_far=1000.0,
               flags=0, dof=None):
    """arctic_dof_pixels: step 4 of depth of field on the host, for n pixels in any order -- pixel_xy (n, 2) int32, rgb the WHOLE frame's colour
    (height, width, 3), prepared and neighbour_max as dof_prepare returns them, taps (samples, 2) or None = dof_taps(samples).  Returns (n, 3) float32."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "dof_pixels: rgb is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    p, nb = np.ascontiguousarray(prepared, dtype=np.float32), np.ascontiguousarray(neighbour_max, dtype=np.float32)
    if p.shape != (height, width, 2) or nb.shape != ((height + 7) // 8, (width + 7) // 8):
        raise ArcticError(-1, "dof_pixels: prepared is (height, width, 2), neighbour_max (tiles_y, tiles_x)")
    m = _dof_arguments(flags, focus_distance, coc_scale, max_radius, samples, depth_extent, z_near, z_far) if dof is None else dof
    t = _dof_table(taps, m)
    n = len(xy)
    out = np.empty((n, 3), np.float32)
    rc = binding.lib().arctic_dof_pixels(_ptr(m), _ptr(t), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(p), _ptr(nb), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "dof_pixels")
    return out


def _bloom_arguments(flags, threshold, soft_knee, clamp_max, intensity, spread, levels):
    """one BLOOM_DTYPE record; the library checks every value"""
    m = np.zeros(1, BLOOM_DTYPE)
    m["flags"], m["threshold"], m["soft_knee"], m["clamp_max"], m["intensity"], m["spread"], m["levels"] = flags, threshold, soft_knee, clamp_max, intensity, spread, levels
    return m


def _bloom_split(packed, lay, count):
    """the first `count` levels of a packed pyramid as (H_k, W_k, 3) views"""
    if packed is None:
        return None
    return [packed[o:o + h * w * 3].reshape(h, w, 3) for (w, h), o in zip(lay["sizes"][:count], lay["offsets"][:count])]


def bloom_layout(width, height, levels):
    """arctic_bloom_layout: the pyramid of a width x height frame -- {"sizes": [(W_k, H_k)], "offsets": [floats from the start of `down` to D_k;
    U_k lies at the same offset of `up`], "down_floats", "up_floats"}"""
    n = int(levels)
    out = np.zeros(3 * max(min(n, 8), 1) + 2, np.uint64)
    rc = binding.lib().arctic_bloom_layout(int(width), int(height), n, _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "bloom_layout")
    return {"sizes": [(int(out[3 * k]), int(out[3 * k + 1])) for k in range(n)], "offsets": [int(out[3 * k + 2]) for k in range(n)],
            "down_floats": int(out[3 * n]), "up_floats": int(out[3 * n + 1])}


def bloom_pyramid(rgb, threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=1.0, levels=5, flags=0, bloom=None):
    """arctic_bloom_pyramid: steps 1 to 3 of bloom of include/arctic_hip.h on the host, for a whole frame -- rgb (height, width, 3).  Returns
    (down, up): the lists of D_1 .. D_L and U_1 .. U_{L-1} as (H_k, W_k, 3) float32 arrays."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "bloom_pyramid: rgb is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    m = _bloom_arguments(flags, threshold, soft_knee, clamp_max, intensity, spread, levels) if bloom is None else bloom
    n = int(m["levels"][0])
    lay = bloom_layout(width, height, n) if 1 <= n <= 8 and 1 <= width <= 16384 and 1 <= height <= 16384 else None     # (the library refuses the rest)
    down = np.empty(max(lay["down_floats"], 1) if lay else 1, np.float32)
    up = np.empty(max(lay["up_floats"], 1) if lay else 1, np.float32)
    rc = binding.lib().arctic_bloom_pyramid(_ptr(m), int(width), int(height), _ptr(c), _ptr(down), _ptr(up))
    if rc < 0:
        raise ArcticError(rc, "bloom_pyramid")
    return _bloom_split(down, lay, n), _bloom_split(up, lay, n - 1)


def bloom_pixels(pixel_xy, rgb, up1, threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=1.0, levels=5, flags=0, bloom=None):
    """arctic_bloom_pixels: step 4 of bloom on the host, for n pixels in any order -- pixel_xy (n, 2) int32, rgb the WHOLE frame's colour
    (height, width, 3), up1: U_1 ((height + 1) // 2, (width + 1) // 2, 3); D_1 when levels = 1.  Returns (n, 3) float32."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "bloom_pixels: rgb is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    u = np.ascontiguousarray(up1, dtype=np.float32)
    if u.shape != ((height + 1) // 2, (width + 1) // 2, 3):
        raise ArcticError(-1, "bloom_pixels: up1 is ((height + 1) // 2, (width + 1) // 2, 3)")
    m = _bloom_arguments(flags, threshold, soft_knee, clamp_max, intensity, spread, levels) if bloom is None else bloom
    n = len(xy)
    out = np.empty((n, 3), np.float32)
    rc = binding.lib().arctic_bloom_pixels(_ptr(m), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(u), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "bloom_pixels")
    return out


def exposure_arguments(flags=0, low=0.5, high=0.95, key_value=0.18, min_exposure=1.0 / 1024.0, max_exposure=1024.0, rate_up=1.0, rate_down=1.0, fallback_exposure=1.0,
                       window=(0, 0, 0, 0), low_q16=None, high_q16=None):
    """one EXPOSURE_DTYPE record; low, high: the percentile band as fractions (floored to 1/65536), or low_q16, high_q16 as they are; the
    library checks every value"""
    m = np.zeros(1, EXPOSURE_DTYPE)
    m["flags"] = flags
    m["low_q16"] = int(low * 65536.0) if low_q16 is None else low_q16
    m["high_q16"] = int(high * 65536.0) if high_q16 is None else high_q16
    m["key_value"], m["min_exposure"], m["max_exposure"], m["rate_up"], m["rate_down"], m["fallback_exposure"] = key_value, min_exposure, max_exposure, rate_up, rate_down, fallback_exposure
    m["window"][0] = window
    return m


def exposure_layout(width, height):
    """arctic_exposure_layout: the meter's launch geometry for a width x height frame -- {"groups": G, "pixels_per_trip": the pixels a workgroup
    takes per trip of its loop, "table_bytes": the bytes of T[G][256]}"""
    out = np.zeros(3, np.uint64)
    rc = binding.lib().arctic_exposure_layout(int(width), int(height), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "exposure_layout")
    return {"groups": int(out[0]), "pixels_per_trip": int(out[1]), "table_bytes": int(out[2])}


def exposure_rate(dt, speed):
    """arctic_exposure_rate: 1 - exp(-dt * speed) as a float in [0, 1], the per-call rate of an adaptation of `speed` per second"""
    return float(binding.lib().arctic_exposure_rate(float(dt), float(speed)))


def exposure_histogram(rgb, exposure=None, **kw):
    """arctic_exposure_histogram: step 1 of auto-exposure of include/arctic_hip.h on the host, for a whole frame -- rgb (height, width, 3).
    Returns H, (256,) uint32."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "exposure_histogram: rgb is the whole frame, (height, width, 3)")
    m = exposure_arguments(**kw) if exposure is None else exposure
    hist = np.empty(256, np.uint32)
    rc = binding.lib().arctic_exposure_histogram(_ptr(m), int(c.shape[1]), int(c.shape[0]), _ptr(c), _ptr(hist))
    if rc < 0:
        raise ArcticError(rc, "exposure_histogram")
    return hist


def exposure_resolve(hist, previous=None, exposure=None, **kw):
    """arctic_exposure_resolve: step 2 on the host -- hist (256,) uint32 and the state in front of the call (an EXPOSURE_STATE_DTYPE record, or
    None: invalid).  Returns the state behind it, one EXPOSURE_STATE_DTYPE record."""
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.shape != (256,):
        raise ArcticError(-1, "exposure_resolve: hist is (256,)")
    m = exposure_arguments(**kw) if exposure is None else exposure
    prev = None if previous is None else np.ascontiguousarray(previous, dtype=EXPOSURE_STATE_DTYPE).reshape(1)
    out = np.zeros(1, EXPOSURE_STATE_DTYPE)
    rc = binding.lib().arctic_exposure_resolve(_ptr(m), _ptr(h), _ptr(prev), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "exposure_resolve")
    return out


def exposure_pixels(rgb, e):
    """arctic_exposure_pixels: step 3's multiply on the host -- rgb (..., 3) float32 and the exposure E.  Returns an array of rgb's shape."""
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim < 1 or c.shape[-1] != 3:
        raise ArcticError(-1, "exposure_pixels: rgb is (..., 3)")
    out = np.empty_like(c)
    n = c.size // 3
    rc = binding.lib().arctic_exposure_pixels(n, _ptr(c) if n else None, float(e), _ptr(out) if n else None)
    if rc < 0:
        raise ArcticError(rc, "exposure_pixels")
    return out


def fog_arguments(flags=0, density=0.05, anisotropy=0.5, max_distance=100.0, steps=32, bias=0.002, scatter_color=(1.0, 1.0, 1.0), ambient_color=(0.0, 0.0, 0.0)):
    """one FOG_DTYPE record; scatter_color is the single-scattering albedo times the sun's radiance; the library checks every value"""
    m = np.zeros(1, FOG_DTYPE)
    m["flags"], m["density"], m["anisotropy"], m["max_distance"], m["steps"], m["bias"] = flags, density, anisotropy, max_distance, steps, bias
    m["scatter_color"][0], m["ambient_color"][0] = scatter_color, ambient_color
    return m


def _fog_offsets(offsets):
    """the offset table of a call: None (every entry 0.5) or 16 contiguous float32"""
    if offsets is None:
        return None
    t = np.ascontiguousarray(offsets, dtype=np.float32).ravel()
    if t.size != 16:
        raise ArcticError(-1, "fog: offsets is 16 floats")
    return t


def fog_offsets(seed=0):
    """an offset table for the fog: the 16 strata (i + 0.5) / 16 in an order shuffled by `seed`, so that the 4 x 4 pixels of a block start their
    march at 16 different depths.  A convenience: the library takes any table in [0, 1)."""
    return ((np.random.default_rng(seed).permutation(16) + 0.5) / 16.0).astype(np.float32)


def fog_view(desc, width, height):
    """arctic_fog_view: the FOG_VIEW_DTYPE record of a scene's camera and sun for a width x height frame"""
    s = desc.fill(CScene())
    out = np.zeros(1, FOG_VIEW_DTYPE)
    rc = binding.lib().arctic_fog_view(C.byref(s), int(width), int(height), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "fog_view")
    return out


def fog_pixels(pixel_xy, rgb, view, depth=None, shadow=None, offsets=None, fog=None, terms=False, **kw):
    """arctic_fog_pixels: the fog on the host, for n pixels in any order -- pixel_xy (n, 2) int32, rgb the WHOLE frame's colour (height, width,
    3), view a FOG_VIEW_DTYPE record, depth (height, width) or None, shadow (S, S) or None.  Returns (n, 3) float32, with terms=True also
    (n, 2) {T, I}."""
    xy = np.ascontiguousarray(pixel_xy, dtype=np.int32).reshape(-1, 2)
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ArcticError(-1, "fog_pixels: rgb is the whole frame, (height, width, 3)")
    height, width = c.shape[:2]
    z = None if depth is None else np.ascontiguousarray(depth, dtype=np.float32)
    sm = None if shadow is None else np.ascontiguousarray(shadow, dtype=np.float32)
    if (z is not None and z.shape != (height, width)) or (sm is not None and (sm.ndim != 2 or sm.shape[0] != sm.shape[1])):
        raise ArcticError(-1, "fog_pixels: depth is (height, width), shadow (S, S)")
    m = fog_arguments(**kw) if fog is None else fog
    t = _fog_offsets(offsets)
    n = len(xy)
    out = np.empty((n, 3), np.float32)
    tm = np.empty((n, 2), np.float32) if terms else None
    rc = binding.lib().arctic_fog_pixels(_ptr(m), _ptr(view), _ptr(t), n, _ptr(xy) if n else None, int(width), int(height), _ptr(c), _ptr(z), _ptr(sm),
                                         0 if sm is None else int(sm.shape[0]), _ptr(out) if n else None, _ptr(tm) if terms and n else None)
    if rc < 0:
        raise ArcticError(rc, "fog_pixels")
    return (out, tm) if terms else out


def fog_exp2(x):
    """arctic_fog_exp2: the fog's 2^x for x <= 0, as the kernel evaluates it"""
    return float(binding.lib().arctic_fog_exp2(float(x)))


def fog_exp2_poly(f):
    """arctic_fog_exp2_poly: the polynomial of fog_exp2 for an array of f in [0, 1]"""
    a = np.ascontiguousarray(f, dtype=np.float32).ravel()
    out = np.empty_like(a)
    rc = binding.lib().arctic_fog_exp2_poly(len(a), _ptr(a) if len(a) else None, _ptr(out) if len(a) else None)
    if rc < 0:
        raise ArcticError(rc, "fog_exp2_poly")
    return out


def jitter_proj_view(m, w, h, jx, jy):
    """arctic_jitter_proj_view: the (4, 4) [col][row] matrix m with the sub-pixel offset (jx, jy) pixels of a w x h frame applied -- the matrix
    the forward prepass draws with under set_camera_jitter(jx, jy).  Returns a new (4, 4) float32 array."""
    out = np.array(m, dtype=np.float32).reshape(16).copy()
    rc = binding.lib().arctic_jitter_proj_view(_ptr(out), int(w), int(h), float(jx), float(jy))
    if rc < 0:
        raise ArcticError(rc, "jitter_proj_view")
    return out.reshape(4, 4)


def taa_jitter(frame, period=8):
    """the sample offset of frame `frame`: point number frame % period + 1 of the Halton sequence in bases (2, 3), minus 0.5 in each coordinate --
    (jx, jy) in [-0.5, 0.5) pixels, for set_camera_jitter and for the resolve's `jitter`"""
    def halton(i, base):
        f, x = 1.0, 0.0
        while i > 0:
            f /= base
            x += f * (i % base)
            i //= base
        return x
    i = int(frame) % int(period) + 1
    return halton(i, 2) - 0.5, halton(i, 3) - 0.5


def ao_directions(n_rays, pattern, seed=0):
    """a direction table for trace_ambient_occlusion: (P * P, n_rays, 3) float32, cosine-weighted over the hemisphere z > 0, unit length.  One
    stratified point set -- (k + jitter) / n_rays against the golden-ratio sequence -- per set, each set shifted by its own Cranley-Patterson
    rotation so that the P * P sets of a window fill each other's gaps.  Deterministic in (n_rays, pattern, seed).  A convenience: the library
    takes any table."""
    n, sets = int(n_rays), int(pattern) ** 2
    rng = np.random.default_rng([int(seed), n, sets])
    k = np.arange(n, dtype=np.float64)
    out = np.zeros((sets, n, 3), np.float64)
    for s in range(sets):
        u = (k + rng.random(n)) / n                                   # stratified in the radius: one sample per ring of equal projected area
        v = (k * 0.6180339887498949 + (s + rng.random()) / sets) % 1.0   # the angle: golden-ratio steps, each set turned by its own part of a full turn
        r, phi = np.sqrt(u) * (1.0 - 1e-6), 2.0 * np.pi * v
        out[s, :, 0], out[s, :, 1] = r * np.cos(phi), r * np.sin(phi)
        out[s, :, 2] = np.sqrt(np.maximum(1.0 - r * r, 0.0))
        out[s] = out[s][rng.permutation(n)]                            # (the order inside a set carries no meaning: ray k of one set is no neighbour of ray k of another)
    out /= np.linalg.norm(out, axis=-1, keepdims=True)
    return out.astype(np.float32)


gi_directions = ao_directions
"""gi_directions(n_rays, pattern, seed=0): the direction table trace_gi expects -- ao_directions' table, under the name of its use here.  The table
MUST be cosine-weighted over the hemisphere z > 0, as this one is, for the mean of the rays' radiance to be the irradiance over pi: the estimate
weights every ray alike, so the cosine of the rendering equation has to be in the density the directions were drawn from.  The library takes any
table; with a uniform one the result is a mean radiance, not an irradiance."""


def point_shadow_matrices(light):
    """the six face matrices of one shadow-casting point light (a POINT_SHADOW_LIGHT_DTYPE record) exactly as the library builds them:
    (6, 4, 4) float32, each [col][row] like frame_constants"""
    l = np.ascontiguousarray(np.asarray(light, dtype=POINT_SHADOW_LIGHT_DTYPE).reshape(1))
    out = np.empty((6, 4, 4), np.float32)
    rc = binding.lib().arctic_point_shadow_matrices(_ptr(l), _ptr(out))
    if rc < 0:
        raise ArcticError(rc, "point_shadow_matrices: invalid light")
    return out


def cluster_bounds(vertices, indices):
    """arctic_cluster_bounds: the culling boxes create_mesh keeps for this mesh, on the host -- (tbounds (ceil(triangles / 256), 6), vbounds
    (ceil(vertices / 256), 6)) float32, {min xyz, max xyz} each; every vertex block's box contains the boxes of the clusters that read it"""
    v = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
    i = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    tb, vb = np.empty(((len(i) // 3 + 255) // 256, 6), np.float32), np.empty(((len(v) + 255) // 256, 6), np.float32)
    rc = binding.lib().arctic_cluster_bounds(_ptr(v) if len(v) else None, len(v), _ptr(i) if len(i) else None, len(i), _ptr(tb) if len(tb) else None,
                                             _ptr(vb) if len(vb) else None)
    if rc < 0:
        raise ArcticError(rc, "cluster_bounds")
    return tb, vb


def frame_constants(desc):
    """proj_view, light_proj_view ([col][row]) and sun_dir exactly as the library builds them."""
    s = desc.fill(CScene())
    pv, lpv, sd = np.empty(16, np.float32), np.empty(16, np.float32), np.empty(3, np.float32)
    rc = binding.lib().arctic_frame_constants(C.byref(s), _ptr(pv), _ptr(lpv), _ptr(sd))
    if rc < 0:
        raise ArcticError(rc, "frame_constants")
    return pv.reshape(4, 4), lpv.reshape(4, 4), sd
