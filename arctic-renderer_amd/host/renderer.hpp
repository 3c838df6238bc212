// renderer.hpp -- C++ host-side mirror of the reference's Arctic::Renderer::Renderer over the C-ABI.
//
// Same public surface as reference src/renderer/renderer.hpp:94-125 (init, cleanup, resize, render_frame,
// create_mesh, create_material, create_hdri, update_lights, flush) and the same POD scene types as
// src/renderer/scene.hpp:20-110, so src/app.cpp's calls compile against it unchanged in shape:
//   - bool-returning, [[nodiscard]], errors logged (here: kept in last_error()) -- src/renderer/dxerr.hpp:5-10
//   - glm types replaced by plain float arrays of the same bytes (glm is not a dependency of this library)
//   - no SDL window, no ImGui callback; render_frame hands back the RGBA8 frame instead of presenting it.
// Header only; link with -larctic_hip (arctic-renderer_amd/csrc/libarctic_hip.so).
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <span>
#include <string>
#include <vector>

#include "../../include/arctic_hip.h"
#include "../../include/arctic_gltf.h"   // (declarations only: nothing of the loader is linked unless apply_gltf_material_extras is used)

namespace ArcticAMD::Renderer {

using MeshIdx = size_t;
using MaterialIdx = size_t;

// scene.hpp:20-110, same member names; vec3/vec2/mat4 as float arrays (glm memory order)
struct Camera { float eye[3]; float rotation[2]; float aspect; float fov_y; std::array<float, 2> z_near_far; };
using Vertex = ArcticVertex;               // position, normal, tangent, bitangent, tex_coords
using Object = ArcticObject;               // trs (column-major mat4), mesh_idx
struct DirectionalLight { float position[3]; float rotation[2]; float color[3]; };
using PointLight = ArcticPointLight;       // position, padding0, color, padding1
using SpotLight = ArcticSpotLight;         // position, range, direction, inner_cone_angle, color, outer_cone_angle (no counterpart in the reference)
using PointShadowLight = ArcticPointShadowLight;   // position, z_near, color, z_far (no counterpart in the reference)
using SkinVertex = ArcticSkinVertex;                 // joints[4] (uint16), weights[4]: per-vertex skinning data (no counterpart in the reference)
using MorphDelta = ArcticMorphDelta;                 // position, normal, tangent, bitangent deltas: one per vertex per morph target (no counterpart in the reference)
using MaterialParams = ArcticMaterialParams;       // glTF's factors: base colour, metallic, roughness, normal scale, occlusion strength, emissive (no counterpart in the reference)
struct Scene {
    Camera camera;
    float ambient;
    DirectionalLight sun;
    std::vector<PointLight> point_lights;
    std::vector<Object> objects;
};
struct Settings { int tm_method{0}; float gamma{2.2f}; float exposure{1.0f}; };

class Renderer {
  public:
    static constexpr size_t MAX_NUM_POINT_LIGHTS = 16;   // renderer.hpp:22 (a create-time parameter here)
    static constexpr uint32_t SHADOW_MAP_SIZE = 4000;    // ShadowMapPass::SIZE, shadow_map_pass.hpp:23

    Renderer(uint32_t initial_width, uint32_t initial_height, uint32_t shadow_size = SHADOW_MAP_SIZE,
             uint32_t max_lights = MAX_NUM_POINT_LIGHTS, int device = 0)
        : m_info{initial_width, initial_height, shadow_size, max_lights, device, 0, 0} {}
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;
    ~Renderer() { cleanup(); }

    [[nodiscard]] bool init() {
        char err[512] = {0};
        m_handle = arctic_create(&m_info, err, sizeof err);
        if (!m_handle) m_error = err;
        return m_handle != nullptr;
    }
    void cleanup() { if (m_handle) { arctic_destroy(m_handle); m_handle = nullptr; } }

    [[nodiscard]] bool resize(uint32_t &out_width, uint32_t &out_height) {
        if (!ok(arctic_resize(m_handle, out_width, out_height))) return false;
        m_info.width = out_width; m_info.height = out_height;
        return true;
    }

    // out_rgba8: width*height*4 bytes, row-major, top-left origin (may be nullptr: the frame stays on the device)
    [[nodiscard]] bool render_frame(const Scene &scene, const Settings &settings, uint8_t *out_rgba8) {
        ArcticScene s{};
        std::memcpy(s.camera.eye, scene.camera.eye, sizeof s.camera.eye);
        std::memcpy(s.camera.rotation, scene.camera.rotation, sizeof s.camera.rotation);
        s.camera.aspect = scene.camera.aspect; s.camera.fov_y = scene.camera.fov_y;
        s.camera.z_near_far[0] = scene.camera.z_near_far[0]; s.camera.z_near_far[1] = scene.camera.z_near_far[1];
        s.ambient = scene.ambient;
        std::memcpy(&s.sun, &scene.sun, sizeof s.sun);
        s.point_lights = scene.point_lights.data(); s.n_point_lights = scene.point_lights.size();
        s.objects = scene.objects.data(); s.n_objects = scene.objects.size();
        ArcticSettings st{settings.tm_method, settings.gamma, settings.exposure};
        return ok(arctic_render_frame(m_handle, &s, &st, out_rgba8));
    }

    [[nodiscard]] bool create_mesh(std::span<Vertex> vertices, std::span<uint32_t> indices, MaterialIdx material_idx) {
        return ok(arctic_create_mesh(m_handle, vertices.data(), vertices.size(), indices.data(), indices.size(), material_idx));
    }
    [[nodiscard]] bool create_material(void *diffuse_data, uint32_t diffuse_width, uint32_t diffuse_height, void *normal_data,
                                       uint32_t normal_width, uint32_t normal_height, void *metalness_roughness_data,
                                       uint32_t metalness_roughness_width, uint32_t metalness_roughness_height) {
        return ok(arctic_create_material(m_handle, diffuse_data, diffuse_width, diffuse_height, normal_data, normal_width, normal_height,
                                         metalness_roughness_data, metalness_roughness_width, metalness_roughness_height));
    }
    // glTF material factors, emissive (sRGB, rgb) and occlusion (linear, R) of a material that exists (include/arctic_hip.h); replaces what it had,
    // params == nullptr and no images: back to neutral.  false = invalid params / image / index, the material stays as it was
    [[nodiscard]] bool set_material_extras(MaterialIdx material, const MaterialParams *params, const void *emissive_data = nullptr, uint32_t emissive_width = 0,
                                           uint32_t emissive_height = 0, const void *occlusion_data = nullptr, uint32_t occlusion_width = 0, uint32_t occlusion_height = 0) {
        return ok(arctic_set_material_extras(m_handle, material, params, emissive_data, emissive_width, emissive_height, occlusion_data, occlusion_width, occlusion_height));
    }
    // the glTF material model of a loaded file on top of arctic_gltf_upload (which stays the reference's load_scene): set_material_extras for every
    // material of `g` that is not neutral; first_material = the index arctic_gltf_upload's first create_material returned
    [[nodiscard]] bool apply_gltf_material_extras(const ArcticGltf *g, MaterialIdx first_material = 0) {
        const MaterialParams neutral = {{1.0f, 1.0f, 1.0f}, 1.0f, 1.0f, 1.0f, 1.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f}};
        for (uint64_t i = 0; i < arctic_gltf_material_count(g); ++i) {
            MaterialParams p;
            const uint8_t *e = nullptr, *o = nullptr;
            uint32_t ew = 0, eh = 0, ow = 0, oh = 0;
            if (arctic_gltf_material_params(g, i, &p) != ARCTIC_OK || arctic_gltf_material_image(g, i, 3, &e, &ew, &eh) != ARCTIC_OK ||
                arctic_gltf_material_image(g, i, 4, &o, &ow, &oh) != ARCTIC_OK) { m_error = "apply_gltf_material_extras: bad glTF handle"; return false; }
            if (!e && !o && std::memcmp(&p, &neutral, sizeof p) == 0) continue;
            if (!set_material_extras(first_material + i, &p, e, ew, eh, o, ow, oh)) return false;
        }
        return true;
    }
    // the culling boxes create_mesh keeps for a mesh (arctic_cluster_bounds: host only, no handle): ceil(n_indices / 3 / 256) cluster boxes and
    // ceil(n_vertices / 256) vertex-block boxes of six floats, each block's box containing the boxes of the clusters that read its vertices
    [[nodiscard]] static bool cluster_bounds(const Vertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, float *tbounds_out, float *vbounds_out) {
        return arctic_cluster_bounds(vertices, n_vertices, indices, n_indices, tbounds_out, vbounds_out) == ARCTIC_OK;
    }
    // skeletal skinning (include/arctic_hip.h; no counterpart in the reference, whose meshes are rigid): a skin -- one SkinVertex per vertex of a
    // mesh that exists, nullptr detaches it --, then a pose: n_joints matrices of 16 floats in glm memory order, nullptr / 0 = the bind pose.
    // A pose belongs to the mesh.  false = invalid records / matrices / index (the mesh stays as it was), or a pose without a skin
    [[nodiscard]] bool set_mesh_skin(MeshIdx mesh, const SkinVertex *skin, uint64_t n_vertices, uint32_t n_joints) {
        return ok(arctic_set_mesh_skin(m_handle, mesh, skin, n_vertices, n_joints));
    }
    [[nodiscard]] bool set_mesh_pose(MeshIdx mesh, const float *joint_matrices, uint32_t n_joints) { return ok(arctic_set_mesh_pose(m_handle, mesh, joint_matrices, n_joints)); }
    // the vertices the next prepass reads for this mesh, posed or not
    [[nodiscard]] bool read_mesh_vertices(MeshIdx mesh, Vertex *out, uint64_t n_vertices) { return ok(arctic_read_mesh_vertices(m_handle, mesh, out, n_vertices)); }
    [[nodiscard]] static bool check_mesh_skin(const SkinVertex *skin, uint64_t n_vertices, uint32_t n_joints) { return arctic_check_mesh_skin(skin, n_vertices, n_joints) == ARCTIC_OK; }
    [[nodiscard]] static bool skin_vertices(const Vertex *in, const SkinVertex *skin, uint64_t n_vertices, const float *joint_matrices, uint32_t n_joints, Vertex *out) {
        return arctic_skin_vertices(in, skin, n_vertices, joint_matrices, n_joints, out) == ARCTIC_OK;
    }
    // morph targets (include/arctic_hip.h): n_targets arrays of n_vertices MorphDelta, target-major, on a mesh that exists (nullptr detaches them;
    // all weights are zero afterwards), then one weight per target, used as given; nullptr / 0 = the mesh's own vertices.  Weights belong to the
    // mesh; morph first, then skin.  false = invalid records / weights / index (the mesh stays as it was), or weights without targets
    [[nodiscard]] bool set_mesh_morph_targets(MeshIdx mesh, const MorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets) {
        return ok(arctic_set_mesh_morph_targets(m_handle, mesh, deltas, n_vertices, n_targets));
    }
    [[nodiscard]] bool set_mesh_morph_weights(MeshIdx mesh, const float *weights, uint32_t n_targets) { return ok(arctic_set_mesh_morph_weights(m_handle, mesh, weights, n_targets)); }
    [[nodiscard]] static bool check_morph_targets(const MorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets) { return arctic_check_morph_targets(deltas, n_vertices, n_targets) == ARCTIC_OK; }
    [[nodiscard]] static bool morph_vertices(const Vertex *in, const MorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets, const float *weights, Vertex *out) {
        return arctic_morph_vertices(in, deltas, n_vertices, n_targets, weights, out) == ARCTIC_OK;
    }
    // the skins and one pose of a loaded file on top of arctic_gltf_upload: the first call attaches the skin of every skinned loader mesh, every
    // call sets their poses from animation `animation` (-1: the rest pose) at `time` seconds.  first_mesh = the index arctic_gltf_upload's first
    // create_mesh returned.  false with the loader's message: e.g. an animation with a CUBICSPLINE sampler (nothing is changed then)
    // Morph targets likewise, in front of the skins (morph first, then skin): attached by the first call, their weights set by every call
    [[nodiscard]] bool pose_gltf(const ArcticGltf *g, int64_t animation, double time, MeshIdx first_mesh = 0) {
        std::vector<std::vector<float>> poses(arctic_gltf_skin_count(g));
        for (uint64_t k = 0; k < poses.size(); ++k) {
            poses[k].resize(16 * arctic_gltf_skin_joint_count(g, k));
            if (arctic_gltf_pose(g, k, animation, time, poses[k].data()) != ARCTIC_OK) { m_error = arctic_gltf_last_error(g); return false; }
        }
        std::vector<std::vector<float>> weights(arctic_gltf_mesh_count(g));   // (evaluated first as well: a refused animation changes nothing)
        for (uint64_t i = 0; i < weights.size(); ++i) {
            const MorphDelta *deltas = nullptr;
            uint64_t n = 0; uint32_t n_targets = 0;
            if (arctic_gltf_mesh_morph(g, i, &deltas, &n, &n_targets) != ARCTIC_OK) { m_error = "pose_gltf: bad glTF handle"; return false; }
            weights[i].resize(n_targets);
            if (n_targets && arctic_gltf_morph_weights(g, i, animation, time, weights[i].data()) != ARCTIC_OK) { m_error = arctic_gltf_last_error(g); return false; }
        }
        const bool attach = !m_gltf_skinned;
        for (uint64_t i = 0; i < weights.size(); ++i) {   // morph first, then skin
            if (weights[i].empty()) continue;
            const MorphDelta *deltas = nullptr;
            uint64_t n = 0; uint32_t n_targets = 0;
            (void)arctic_gltf_mesh_morph(g, i, &deltas, &n, &n_targets);
            if (attach && !set_mesh_morph_targets(first_mesh + i, deltas, n, n_targets)) return false;
            if (!set_mesh_morph_weights(first_mesh + i, weights[i].data(), n_targets)) return false;
        }
        for (uint64_t i = 0; i < arctic_gltf_mesh_count(g); ++i) {
            const SkinVertex *skin = nullptr;
            uint64_t n = 0; int64_t k = -1; uint32_t n_joints = 0;
            if (arctic_gltf_mesh_skin(g, i, &skin, &n, &k, &n_joints) != ARCTIC_OK) { m_error = "pose_gltf: bad glTF handle"; return false; }
            if (k < 0) continue;
            if (attach && !set_mesh_skin(first_mesh + i, skin, n, n_joints)) return false;
            if (!set_mesh_pose(first_mesh + i, poses[(size_t)k].data(), n_joints)) return false;
        }
        m_gltf_skinned = true;
        return true;
    }
    [[nodiscard]] static bool check_material_params(const MaterialParams &params) { return arctic_check_material_params(&params) == ARCTIC_OK; }
    [[nodiscard]] bool create_hdri(float *data, uint32_t width, uint32_t height) { return ok(arctic_create_hdri(m_handle, data, width, height)); }
    void update_lights(std::span<PointLight> point_lights) { (void)ok(arctic_update_lights(m_handle, point_lights.data(), point_lights.size())); }
    // spot lights (KHR_lights_punctual's cone and range; include/arctic_hip.h): false = an invalid light, the previous list stays
    [[nodiscard]] bool update_spot_lights(std::span<SpotLight> spot_lights) { return ok(arctic_update_spot_lights(m_handle, spot_lights.data(), spot_lights.size())); }
    // shadow-casting point lights (a cube of six depth maps each; include/arctic_hip.h): false = an invalid light or no memory, the previous list stays
    [[nodiscard]] bool update_point_shadow_lights(std::span<PointShadowLight> lights) { return ok(arctic_update_point_shadow_lights(m_handle, lights.data(), lights.size())); }
    [[nodiscard]] bool pass_point_shadows(const ArcticScene &scene) { return ok(arctic_pass_point_shadows(m_handle, &scene)); }
    // the faces of light `light`: 6 x F x F floats (F = set_point_shadow_size), faces +X, -X, +Y, -Y, +Z, -Z
    [[nodiscard]] bool read_point_shadow(uint32_t light, float *faces) { return ok(arctic_read_point_shadow(m_handle, light, faces)); }
    [[nodiscard]] bool write_point_shadow(uint32_t light, const float *faces) { return ok(arctic_write_point_shadow(m_handle, light, faces)); }
    [[nodiscard]] bool set_point_shadow_size(uint32_t size) { return ok(arctic_set_option(m_handle, ARCTIC_OPT_POINT_SHADOW_SIZE, size)); }
    // the six face matrices of one light, 16 floats each in glm memory order (host only)
    [[nodiscard]] static bool point_shadow_matrices(const PointShadowLight &light, float out96[96]) { return arctic_point_shadow_matrices(&light, out96) == ARCTIC_OK; }
    [[nodiscard]] bool flush() { return ok(arctic_flush(m_handle)); }
    // image-based ambient from the HDRI (ARCTIC_OPT_ENV_LIGHTING; no counterpart in the reference, whose ps_main keeps a flat ambient):
    // false = the reference's ambient * base_color.  Safe to set before or after create_hdri, and without a map at all.
    [[nodiscard]] bool set_env_lighting(bool on) { return ok(arctic_set_option(m_handle, ARCTIC_OPT_ENV_LIGHTING, on ? 1 : 0)); }
    // its tables (arctic_read_env_lighting): any pointer may be null; dims = {w, h of `level`, levels, LUT side}
    [[nodiscard]] bool read_env_lighting(float *sh27, float *lut, uint32_t level, float *texels, uint32_t *dims) {
        return ok(arctic_read_env_lighting(m_handle, sh27, lut, level, texels, dims));
    }
    // mip-mapped material textures with trilinear filtering (ARCTIC_OPT_TEXTURE_MIPS; the reference creates one level): set BEFORE create_material -- a
    // material gets its chain when it is created -- and leave on while rendering.  The DX12 counterpart: MipLevels = 0 and a GenerateMips pass.
    [[nodiscard]] bool set_texture_mips(bool on) { return ok(arctic_set_option(m_handle, ARCTIC_OPT_TEXTURE_MIPS, on ? 1 : 0)); }
    // one level of a material's chain, 8 bytes per texel (arctic_read_material_mip); texels may be null: dims = {w, h} alone
    [[nodiscard]] bool read_material_mip(uint32_t material, uint32_t level, uint8_t *texels, uint32_t dims[2]) {
        return ok(arctic_read_material_mip(m_handle, material, level, texels, dims));
    }
    // the level-of-detail plane next to the G-buffer in place: one float per pixel, row-major over the handle's rows
    [[nodiscard]] bool read_lod(float *lod) { return ok(arctic_read_lod(m_handle, lod)); }
    [[nodiscard]] bool write_lod(const float *lod) { return ok(arctic_write_lod(m_handle, lod)); }
    // edge anti-aliasing on the RGBA8 output (ARCTIC_OPT_ANTIALIAS; the reference leaves its staircases to the swap chain): a handle that owns the
    // whole frame then filters every frame it shades; a sharded handle accepts the option and leaves its shard alone -- the root calls
    // antialias_device on the assembled frame.  The float LDR / HDR planes are never filtered.
    [[nodiscard]] bool set_antialias(bool on) { return ok(arctic_set_option(m_handle, ARCTIC_OPT_ANTIALIAS, on ? 1 : 0)); }
    // the filter on any RGBA8 image: host to host (synchronous), or between two device images that do not overlap (asynchronous on the handle's stream)
    [[nodiscard]] bool antialias(const uint8_t *rgba8, uint32_t width, uint32_t height, uint8_t *out) { return ok(arctic_antialias(m_handle, rgba8, width, height, out)); }
    [[nodiscard]] bool antialias_device(const void *d_in, void *d_out, uint32_t width, uint32_t height) { return ok(arctic_antialias_device(m_handle, d_in, d_out, width, height)); }

    // ray queries (include/arctic_hip.h: arctic_trace_rays and the definition in front of it; the reference's roadmap item "Raytracing"): n rays
    // against the scene's triangles, closest hit or -- ARCTIC_TRACE_ANY -- any hit; host buffers, synchronous.  The handle builds and caches the
    // acceleration structure; a changed object list, pose or weights rebuilds it on the next query
    [[nodiscard]] bool trace_rays(const ArcticScene &scene, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits) {
        return ok(arctic_trace_rays(m_handle, &scene, rays, n, flags, hits));
    }
    // the same between device buffers, in stream order on the handle's stream
    [[nodiscard]] bool trace_rays_device(const ArcticScene &scene, const ArcticRay *d_rays, uint64_t n, uint32_t flags, ArcticHit *d_hits) {
        return ok(arctic_trace_rays_device(m_handle, &scene, d_rays, n, flags, d_hits));
    }
    // one any-hit ray per pixel of the resident G-buffer towards the sun: mask = rows x width bytes, 255 = lit or no geometry, 0 = occluded
    [[nodiscard]] bool trace_sun_visibility(const ArcticScene &scene, float bias, uint8_t *mask) { return ok(arctic_trace_sun_visibility(m_handle, &scene, bias, mask)); }
    [[nodiscard]] bool ray_scene_info(uint64_t out4[4]) { return ok(arctic_ray_scene_info(m_handle, out4)); }
    // ARCTIC_OPT_RAY_REFIT = 1 (set_option): a moved object, a new pose or new weights are followed by a refit of the cached structure on the device, in
    // stream order, instead of a synchronous rebuild.  out4 = {refits, refittable, launches of the latest refit, 0}; ray_scene_reset drops the
    // structure so that the next query builds in full -- the remedy once the walk of a refitted tree has become slow
    [[nodiscard]] bool ray_refit_info(uint64_t out4[4]) { return ok(arctic_ray_refit_info(m_handle, out4)); }
    [[nodiscard]] bool ray_scene_reset() { return ok(arctic_ray_scene_reset(m_handle)); }
    [[nodiscard]] bool read_ray_structure(ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap) {
        return ok(arctic_read_ray_structure(m_handle, nodes, node_cap, tris, tri_cap));
    }
    // the slots of the cached structure in the order a full build of the scene as it is now would give them, then a refit: on the device, in stream
    // order (falls back to a full build where the structure cannot be refitted).  out4 = {re-splits, launches of the latest, 1 if it fell back, 0}
    [[nodiscard]] bool ray_scene_resplit(const ArcticScene &scene) { return ok(arctic_ray_scene_resplit(m_handle, &scene)); }
    [[nodiscard]] bool ray_resplit_info(uint64_t out4[4]) { return ok(arctic_ray_resplit_info(m_handle, out4)); }
    // the re-split's host arbiter: build on tris9_build, re-split to tris9_now by the definition, walk (no handle, no GPU)
    [[nodiscard]] static bool resplit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                                                ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2) {
        return arctic_resplit_triangles(tris9_build, tris9_now, n_tris, rays, n, flags, hits, nodes, node_cap, tris, tri_cap, counts2) == ARCTIC_OK;
    }
    // the refit's host arbiter: build on tris9_build, refit to tris9_now, walk; optionally the refitted structure (no handle, no GPU)
    [[nodiscard]] static bool refit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                                              ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2) {
        return arctic_refit_triangles(tris9_build, tris9_now, n_tris, rays, n, flags, hits, nodes, node_cap, tris, tri_cap, counts2) == ARCTIC_OK;
    }
    // the host arbiter: world-space triangles of 9 floats, prim = the array index; ARCTIC_TRACE_BRUTE loops over every triangle (no handle, no GPU)
    [[nodiscard]] static bool trace_triangles(const float *tris9, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits) {
        return arctic_trace_triangles(tris9, n_tris, rays, n, flags, hits) == ARCTIC_OK;
    }

    // ambient occlusion from the resident G-buffer (include/arctic_hip.h: arctic_trace_ambient_occlusion and the definition in front of it): n_rays
    // any-hit rays of length radius per pixel from dirs (P * P sets of n_rays local directions, z along the normal) -> rows x width bytes of
    // visibility, 255 = open; out = nullptr leaves it on the device.  The filter (whole frames only) sums over the P x P window of the pattern
    [[nodiscard]] bool trace_ambient_occlusion(const ArcticScene &scene, const ArcticAmbientOcclusion &ao, const float *dirs, uint8_t *out) {
        return ok(arctic_trace_ambient_occlusion(m_handle, &scene, &ao, dirs, out));
    }
    // the same into device memory the caller owns, in stream order on the handle's stream
    [[nodiscard]] bool trace_ambient_occlusion_device(const ArcticScene &scene, const ArcticAmbientOcclusion &ao, const float *dirs, uint8_t *d_out) {
        return ok(arctic_trace_ambient_occlusion_device(m_handle, &scene, &ao, dirs, d_out));
    }
    // its host arbiter: hits per point {world3, normal3} with direction set sets[k] (no handle, no GPU)
    [[nodiscard]] static bool ambient_occlusion_points(const float *tris9, uint64_t n_tris, const float *points6, const uint32_t *sets, uint64_t n_points,
                                                       const ArcticAmbientOcclusion &ao, const float *dirs, uint32_t flags, uint8_t *hits) {
        return arctic_ambient_occlusion_points(tris9, n_tris, points6, sets, n_points, &ao, dirs, flags, hits) == ARCTIC_OK;
    }
    // what is AT a hit (include/arctic_hip.h: arctic_hit_attributes and the definition in front of it): the interpolated vertex output -- 18 floats in
    // arctic_read_gbuffer's order -- and the material of every hit record; host buffers, synchronous
    [[nodiscard]] bool hit_attributes(const ArcticScene &scene, const ArcticHit *hits, uint64_t n, float *attrs, uint32_t *material) {
        return ok(arctic_hit_attributes(m_handle, &scene, hits, n, attrs, material));
    }
    // its host arbiter for one object of the scene (no handle, no GPU); hits of other objects are left as they are
    [[nodiscard]] static bool interpolate_hits(const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, const float *trs,
                                               const float *light_proj_view, uint32_t material, uint64_t first_prim, const ArcticHit *hits, uint64_t n, float *attrs,
                                               uint32_t *material_out) {
        return arctic_interpolate_hits(vertices, n_vertices, indices, n_indices, trs, light_proj_view, material, first_prim, hits, n, attrs, material_out) == ARCTIC_OK;
    }
    // which pixel the hit shading below -- and with it the reflection plane, the ray effects and the indirect light -- evaluates (ARCTIC_OPT_HIT_MODEL):
    // 0 (default) the base model; 1 also spot lights, shadow-casting point lights, image-based ambient and material extras, at level 0
    [[nodiscard]] bool set_hit_model(int model) { return ok(arctic_set_option(m_handle, ARCTIC_OPT_HIT_MODEL, model)); }
    // the forward pixel at every hit, seen from the ray's origin: rgba32f = n x {r, g, b, a}, a = 1 at a hit; a miss takes the environment map, a = 0
    [[nodiscard]] bool shade_hits(const ArcticScene &scene, const ArcticRay *rays, const ArcticHit *hits, uint64_t n, float *rgba32f) {
        return ok(arctic_shade_hits(m_handle, &scene, rays, hits, n, 0, rgba32f));
    }
    // the same between device buffers, in stream order on the handle's stream
    [[nodiscard]] bool shade_hits_device(const ArcticScene &scene, const ArcticRay *d_rays, const ArcticHit *d_hits, uint64_t n, float *d_rgba32f) {
        return ok(arctic_shade_hits_device(m_handle, &scene, d_rays, d_hits, n, 0, d_rgba32f));
    }
    // one mirror ray per pixel of the resident G-buffer, its closest hit shaded: rows x width x {r, g, b, a}; rgba32f = nullptr leaves it on the device
    [[nodiscard]] bool trace_reflections(const ArcticScene &scene, float bias, float *rgba32f) { return ok(arctic_trace_reflections(m_handle, &scene, bias, rgba32f)); }
    [[nodiscard]] bool trace_reflections_device(const ArcticScene &scene, float bias, float *d_rgba32f) {
        return ok(arctic_trace_reflections_device(m_handle, &scene, bias, d_rgba32f));
    }
    // {device bytes, pinned host bytes, prims in the source table, times the table was made}: all 0 until the first of the calls above
    [[nodiscard]] bool hit_shading_info(uint64_t out4[4]) { return ok(arctic_hit_shading_info(m_handle, out4)); }

    // occlusion and reflections composed into the shaded frame, in front of the tonemapper (include/arctic_hip.h: arctic_compose_planes_device and the
    // definition in front of it; needs ARCTIC_OPT_KEEP_FLOAT_OUTPUT and a shading pass): device planes the caller owns -- a plane whose flag is absent
    // may be nullptr -- into d_out_rgba8 or, nullptr, the handle's own buffers (read_composed); in stream order on the handle's stream
    [[nodiscard]] bool compose_planes_device(const ArcticScene &scene, const ArcticSettings &settings, const ArcticRayCompose &compose, const uint8_t *d_ao_u8,
                                             const float *d_reflection_rgba32f, uint8_t *d_out_rgba8) {
        return ok(arctic_compose_planes_device(m_handle, &scene, &settings, &compose, d_ao_u8, d_reflection_rgba32f, d_out_rgba8));
    }
    // the one call: the ambient occlusion (ao, dirs: as trace_ambient_occlusion takes them; nullptr without ARCTIC_COMPOSE_AO), the reflection plane at
    // compose.reflection_bias, then the composition
    [[nodiscard]] bool pass_ray_effects(const ArcticScene &scene, const ArcticSettings &settings, const ArcticRayCompose &compose, const ArcticAmbientOcclusion *ao,
                                        const float *dirs, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_ray_effects(m_handle, &scene, &settings, &compose, ao, dirs, d_out_rgba8));
    }
    // the latest composition, shaped like read_output; any pointer may be nullptr
    [[nodiscard]] bool read_composed(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) { return ok(arctic_read_composed(m_handle, ldr_rgb, hdr_rgb, rgba8)); }
    // its host arbiter: the composed HDR colour of n pixels from channels sampled already (no handle, no GPU)
    [[nodiscard]] static bool compose_pixels(const ArcticRayCompose &compose, const float *eye3, float ambient, uint64_t n, const float *hdr3, const float *base3,
                                             const float *metal, const float *rough, const float *normal3, const float *world3, const uint8_t *ao, const float *refl4,
                                             const uint8_t *geometry, float *out_hdr3) {
        return arctic_compose_pixels(&compose, eye3, ambient, n, hdr3, base3, metal, rough, normal3, world3, ao, refl4, geometry, out_hdr3) == ARCTIC_OK;
    }
    // {device bytes, launches of the composition kernel, pass_ray_effects calls, 0}: all 0 until the first call that passes its checks
    [[nodiscard]] bool compose_info(uint64_t out4[4]) { return ok(arctic_compose_info(m_handle, out4)); }
    // temporal accumulation of the occlusion plane (include/arctic_hip.h: arctic_accumulate_ambient_occlusion_device and the definition in front of it):
    // the device byte plane d_ao_in_u8 blended into the handle's history, reprojected through the previous call's camera, into d_ao_out_u8 (it may be
    // the same plane); in stream order on the handle's stream
    [[nodiscard]] bool accumulate_ambient_occlusion_device(const ArcticScene &scene, const ArcticAoHistory &hist, const uint8_t *d_ao_in_u8, uint8_t *d_ao_out_u8) {
        return ok(arctic_accumulate_ambient_occlusion_device(m_handle, &scene, &hist, d_ao_in_u8, d_ao_out_u8));
    }
    // the host form, synchronous
    [[nodiscard]] bool accumulate_ambient_occlusion(const ArcticScene &scene, const ArcticAoHistory &hist, const uint8_t *ao_in, uint8_t *ao_out) {
        return ok(arctic_accumulate_ambient_occlusion(m_handle, &scene, &hist, ao_in, ao_out));
    }
    // empties the history; frees nothing
    [[nodiscard]] bool ao_history_reset() { return ok(arctic_ao_history_reset(m_handle)); }
    // the history the last call wrote, row-major; any pointer may be nullptr
    [[nodiscard]] bool read_ao_history(float *value, float *count, float *world3, float *normal3) { return ok(arctic_read_ao_history(m_handle, value, count, world3, normal3)); }
    // {device bytes, launches of k_ao_accumulate, calls since the last reset, 0}
    [[nodiscard]] bool ao_history_info(uint64_t out4[4]) { return ok(arctic_ao_history_info(m_handle, out4)); }
    // its host arbiter: n pixels against a previous history given as row-major arrays (no handle, no GPU)
    [[nodiscard]] static bool accumulate_pixels(const ArcticAoHistory &hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const uint8_t *cur,
                                                const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_value, const float *prev_count,
                                                const float *prev_world3, const float *prev_normal3, uint8_t *out_u8, float *out_value, float *out_count,
                                                float *out_world3, float *out_normal3) {
        return arctic_accumulate_pixels(&hist, n, world3, normal3, geometry, cur, prev_proj_view, width, height, prev_value, prev_count, prev_world3, prev_normal3, out_u8,
                                        out_value, out_count, out_world3, out_normal3) == ARCTIC_OK;
    }
    // pass_ray_effects with the accumulation between the occlusion and the composition (compose.flags must hold ARCTIC_COMPOSE_AO)
    [[nodiscard]] bool pass_ray_effects_temporal(const ArcticScene &scene, const ArcticSettings &settings, const ArcticRayCompose &compose, const ArcticAmbientOcclusion &ao,
                                                 const float *dirs, const ArcticAoHistory &hist, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_ray_effects_temporal(m_handle, &scene, &settings, &compose, &ao, dirs, &hist, d_out_rgba8));
    }
    // motion vectors (include/arctic_hip.h: arctic_motion_vectors_device and the definition in front of it): where every pixel's surface point lay at
    // the previous motion call, into device planes the caller owns (rows*width float4; rows*width float2, may be nullptr); once per frame, after the
    // frame's pose / trs have been set and drawn; in stream order on the handle's stream
    [[nodiscard]] bool motion_vectors_device(const ArcticScene &scene, float *d_prev_world4, float *d_velocity2) {
        return ok(arctic_motion_vectors_device(m_handle, &scene, d_prev_world4, d_velocity2));
    }
    // the host form, synchronous, with the barycentrics and the source triangle of every pixel; any pointer may be nullptr
    [[nodiscard]] bool motion_vectors(const ArcticScene &scene, float *prev_world4, float *velocity2, float *bary3, uint32_t *source4) {
        return ok(arctic_motion_vectors(m_handle, &scene, prev_world4, velocity2, bary3, source4));
    }
    // forgets what the previous motion call saw; frees nothing
    [[nodiscard]] bool motion_reset() { return ok(arctic_motion_reset(m_handle)); }
    // {device bytes, launches of k_motion, launches of k_motion_snapshot, calls since the last reset}
    [[nodiscard]] bool motion_info(uint64_t out4[4]) { return ok(arctic_motion_info(m_handle, out4)); }
    // its host arbiter (no handle, no GPU)
    [[nodiscard]] static bool motion_pixels(uint64_t n, const float *bary3, const uint32_t *object, const float *prev_pos9, const int32_t *pixel_xy, const float *prev_trs,
                                            uint64_t n_objects, const float *prev_proj_view, uint32_t width, uint32_t height, float *prev_world4, float *velocity2) {
        return arctic_motion_pixels(n, bary3, object, prev_pos9, pixel_xy, prev_trs, n_objects, prev_proj_view, width, height, prev_world4, velocity2) == ARCTIC_OK;
    }
    // the accumulation with the history fetched where each pixel's point WAS (d_prev_world4: the plane motion_vectors_device wrote for this frame);
    // shares the history with accumulate_ambient_occlusion_device
    [[nodiscard]] bool accumulate_ambient_occlusion_motion_device(const ArcticScene &scene, const ArcticAoHistory &hist, const float *d_prev_world4, const uint8_t *d_ao_in_u8,
                                                                  uint8_t *d_ao_out_u8) {
        return ok(arctic_accumulate_ambient_occlusion_motion_device(m_handle, &scene, &hist, d_prev_world4, d_ao_in_u8, d_ao_out_u8));
    }
    // the host form, synchronous
    [[nodiscard]] bool accumulate_ambient_occlusion_motion(const ArcticScene &scene, const ArcticAoHistory &hist, const float *prev_world4, const uint8_t *ao_in, uint8_t *ao_out) {
        return ok(arctic_accumulate_ambient_occlusion_motion(m_handle, &scene, &hist, prev_world4, ao_in, ao_out));
    }
    // its host arbiter: accumulate_pixels with the prev_world4 array
    [[nodiscard]] static bool accumulate_pixels_motion(const ArcticAoHistory &hist, uint64_t n, const float *world3, const float *prev_world4, const float *normal3,
                                                       const uint8_t *geometry, const uint8_t *cur, const float *prev_proj_view, uint32_t width, uint32_t height,
                                                       const float *prev_value, const float *prev_count, const float *prev_world3, const float *prev_normal3, uint8_t *out_u8,
                                                       float *out_value, float *out_count, float *out_world3, float *out_normal3) {
        return arctic_accumulate_pixels_motion(&hist, n, world3, prev_world4, normal3, geometry, cur, prev_proj_view, width, height, prev_value, prev_count, prev_world3,
                                               prev_normal3, out_u8, out_value, out_count, out_world3, out_normal3) == ARCTIC_OK;
    }
    // pass_ray_effects_temporal with the motion vectors in front of the occlusion and the accumulation's motion form
    [[nodiscard]] bool pass_ray_effects_motion(const ArcticScene &scene, const ArcticSettings &settings, const ArcticRayCompose &compose, const ArcticAmbientOcclusion &ao,
                                               const float *dirs, const ArcticAoHistory &hist, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_ray_effects_motion(m_handle, &scene, &settings, &compose, &ao, dirs, &hist, d_out_rgba8));
    }

    // temporal anti-aliasing (include/arctic_hip.h: arctic_set_camera_jitter, arctic_taa_resolve_device and the definition in front of it).
    // The forward prepass's sub-pixel offset in pixels, each in [-1, 1]; (0, 0), the default, changes nothing
    [[nodiscard]] bool set_camera_jitter(float jx, float jy) { return ok(arctic_set_camera_jitter(m_handle, jx, jy)); }
    // the same offset applied to a [col][row] matrix on the host: what a host that draws with its own projection feeds it
    [[nodiscard]] static bool jitter_proj_view(float *proj_view16, uint32_t width, uint32_t height, float jx, float jy) {
        return arctic_jitter_proj_view(proj_view16, width, height, jx, jy) == ARCTIC_OK;
    }
    // the resolve on device planes (nullptr: the handle's HDR plane, zero velocity, the handle's own output); stream-ordered
    [[nodiscard]] bool taa_resolve_device(const ArcticSettings &settings, const ArcticTaa &taa, const float *d_hdr_rgb32f, const float *d_velocity2, uint8_t *d_out_rgba8) {
        return ok(arctic_taa_resolve_device(m_handle, &settings, &taa, d_hdr_rgb32f, d_velocity2, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool taa_resolve(const ArcticSettings &settings, const ArcticTaa &taa, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8) {
        return ok(arctic_taa_resolve(m_handle, &settings, &taa, hdr_rgb32f, velocity2, out_rgba8));
    }
    // the frame's ONE motion call, then the resolve on the handle's HDR plane
    [[nodiscard]] bool pass_taa(const ArcticScene &scene, const ArcticSettings &settings, const ArcticTaa &taa, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_taa(m_handle, &scene, &settings, &taa, d_out_rgba8));
    }
    // empties the history; frees nothing
    [[nodiscard]] bool taa_reset() { return ok(arctic_taa_reset(m_handle)); }
    // what the latest resolve left, row-major; any pointer may be nullptr
    [[nodiscard]] bool read_taa(float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8) { return ok(arctic_read_taa(m_handle, ldr_rgb, hdr_rgb, count, rgba8)); }
    // {device bytes, launches of k_taa_resolve, calls since the last reset, 0}
    [[nodiscard]] bool taa_info(uint64_t out4[4]) { return ok(arctic_taa_info(m_handle, out4)); }
    // the host arbiter: steps 1 to 6 for n pixels, no handle, no GPU
    [[nodiscard]] static bool taa_pixels(const ArcticTaa &taa, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb, const float *velocity2,
                                         const float *prev_rgbn, float *out_rgbn) {
        return arctic_taa_pixels(&taa, n, pixel_xy, width, height, cur_rgb, velocity2, prev_rgbn, out_rgbn) == ARCTIC_OK;
    }

    // motion blur (include/arctic_hip.h: arctic_motion_blur_device and the definition in front of it).  The blur on device planes (nullptr: the
    // handle's HDR plane per mb.flags, depth 0, the handle's own output; d_velocity2 is required); stream-ordered
    [[nodiscard]] bool motion_blur_device(const ArcticSettings &settings, const ArcticMotionBlur &mb, const float *d_hdr_rgb32f, const float *d_velocity2, const float *d_depth,
                                          uint8_t *d_out_rgba8) {
        return ok(arctic_motion_blur_device(m_handle, &settings, &mb, d_hdr_rgb32f, d_velocity2, d_depth, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool motion_blur(const ArcticSettings &settings, const ArcticMotionBlur &mb, const float *hdr_rgb32f, const float *velocity2, const float *depth, uint8_t *out_rgba8) {
        return ok(arctic_motion_blur(m_handle, &settings, &mb, hdr_rgb32f, velocity2, depth, out_rgba8));
    }
    // the visibility plane's depth as a row-major float plane on the device: arctic_read_gbuffer's depth
    [[nodiscard]] bool depth_plane_device(float *d_depth) { return ok(arctic_depth_plane_device(m_handle, d_depth)); }
    // the motion call, the depth, then the blur on the handle's planes; under ARCTIC_MB_SOURCE_TAA no motion call: pass_taa's velocity plane
    [[nodiscard]] bool pass_motion_blur(const ArcticScene &scene, const ArcticSettings &settings, const ArcticMotionBlur &mb, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_motion_blur(m_handle, &scene, &settings, &mb, d_out_rgba8));
    }
    // what the latest blur left, row-major; any pointer may be nullptr
    [[nodiscard]] bool read_motion_blur(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max2, float *neighbour_max2, float *prepared2) {
        return ok(arctic_read_motion_blur(m_handle, ldr_rgb, hdr_rgb, rgba8, tile_max2, neighbour_max2, prepared2));
    }
    // {device bytes, launches of k_motion_blur, calls, 0}
    [[nodiscard]] bool motion_blur_info(uint64_t out4[4]) { return ok(arctic_motion_blur_info(m_handle, out4)); }
    // the host arbiters: steps 1 to 3 of a whole frame, and step 4 for n pixels; no handle, no GPU
    [[nodiscard]] static bool motion_blur_prepare(const ArcticMotionBlur &mb, uint32_t width, uint32_t height, const float *velocity2, const float *depth, float *tile_max2,
                                                  float *neighbour_max2, float *prepared2) {
        return arctic_motion_blur_prepare(&mb, width, height, velocity2, depth, tile_max2, neighbour_max2, prepared2) == ARCTIC_OK;
    }
    [[nodiscard]] static bool motion_blur_pixels(const ArcticMotionBlur &mb, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                                                 const float *prepared2, const float *neighbour_max2, float *out_rgb) {
        return arctic_motion_blur_pixels(&mb, n, pixel_xy, width, height, rgb, prepared2, neighbour_max2, out_rgb) == ARCTIC_OK;
    }

    // depth of field (include/arctic_hip.h: arctic_dof_device and the definition in front of it).  The gather on device planes (nullptr: the
    // handle's HDR plane per dof.flags, the handle's own output; d_depth is required; taps2: dof.samples float2 in host memory); stream-ordered
    [[nodiscard]] bool dof_device(const ArcticSettings &settings, const ArcticDof &dof, const float *d_hdr_rgb32f, const float *d_depth, const float *taps2, uint8_t *d_out_rgba8) {
        return ok(arctic_dof_device(m_handle, &settings, &dof, d_hdr_rgb32f, d_depth, taps2, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool dof(const ArcticSettings &settings, const ArcticDof &dof, const float *hdr_rgb32f, const float *depth, const float *taps2, uint8_t *out_rgba8) {
        return ok(arctic_dof(m_handle, &settings, &dof, hdr_rgb32f, depth, taps2, out_rgba8));
    }
    // the depth, then the gather of the handle's planes under the scene's camera planes (dof.z_near == dof.z_far == 0)
    [[nodiscard]] bool pass_dof(const ArcticScene &scene, const ArcticSettings &settings, const ArcticDof &dof, const float *taps2, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_dof(m_handle, &scene, &settings, &dof, taps2, d_out_rgba8));
    }
    // what the latest call left, row-major; any pointer may be nullptr
    [[nodiscard]] bool read_dof(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max, float *neighbour_max, float *prepared2) {
        return ok(arctic_read_dof(m_handle, ldr_rgb, hdr_rgb, rgba8, tile_max, neighbour_max, prepared2));
    }
    // {device bytes, launches of k_dof_gather, calls, 0}
    [[nodiscard]] bool dof_info(uint64_t out4[4]) { return ok(arctic_dof_info(m_handle, out4)); }
    // autofocus: the view distance of one pixel of the resident visibility plane; synchronises
    [[nodiscard]] bool dof_focus_at(float z_near, float z_far, uint32_t px, uint32_t py, float *distance) { return ok(arctic_dof_focus_at(m_handle, z_near, z_far, px, py, distance)); }
    // the host arbiters and the thin lens: no handle, no GPU
    [[nodiscard]] static bool dof_prepare(const ArcticDof &dof, uint32_t width, uint32_t height, const float *depth, float *tile_max, float *neighbour_max, float *prepared2) {
        return arctic_dof_prepare(&dof, width, height, depth, tile_max, neighbour_max, prepared2) == ARCTIC_OK;
    }
    [[nodiscard]] static bool dof_pixels(const ArcticDof &dof, const float *taps2, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                                         const float *prepared2, const float *neighbour_max, float *out_rgb) {
        return arctic_dof_pixels(&dof, taps2, n, pixel_xy, width, height, rgb, prepared2, neighbour_max, out_rgb) == ARCTIC_OK;
    }
    [[nodiscard]] static bool dof_coc_scale(float f_number, float focal_length_mm, float sensor_height_mm, float focus_distance, uint32_t height_px, float *out) {
        return arctic_dof_coc_scale(f_number, focal_length_mm, sensor_height_mm, focus_distance, height_px, out) == ARCTIC_OK;
    }

    // bloom (include/arctic_hip.h: arctic_bloom_device and the definition in front of it).  The pyramid and the composite on device planes
    // (nullptr: the handle's HDR plane per bloom.flags, the handle's own output); stream-ordered
    [[nodiscard]] bool bloom_device(const ArcticSettings &settings, const ArcticBloom &bloom, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8) {
        return ok(arctic_bloom_device(m_handle, &settings, &bloom, d_hdr_rgb32f, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool bloom(const ArcticSettings &settings, const ArcticBloom &bloom, const float *hdr_rgb32f, uint8_t *out_rgba8) {
        return ok(arctic_bloom(m_handle, &settings, &bloom, hdr_rgb32f, out_rgba8));
    }
    // what the latest call left, row-major, the pyramids as bloom_layout packs them; any pointer may be nullptr
    [[nodiscard]] bool read_bloom(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *down, float *up) {
        return ok(arctic_read_bloom(m_handle, ldr_rgb, hdr_rgb, rgba8, down, up));
    }
    // {device bytes, launches of k_bloom_composite, calls, 0}
    [[nodiscard]] bool bloom_info(uint64_t out4[4]) { return ok(arctic_bloom_info(m_handle, out4)); }
    // the layout (out: 3 * levels + 2 numbers) and the host arbiters: no handle, no GPU
    [[nodiscard]] static bool bloom_layout(uint32_t width, uint32_t height, uint32_t levels, uint64_t *out) { return arctic_bloom_layout(width, height, levels, out) == ARCTIC_OK; }
    [[nodiscard]] static bool bloom_pyramid(const ArcticBloom &bloom, uint32_t width, uint32_t height, const float *rgb, float *down, float *up) {
        return arctic_bloom_pyramid(&bloom, width, height, rgb, down, up) == ARCTIC_OK;
    }
    [[nodiscard]] static bool bloom_pixels(const ArcticBloom &bloom, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb, const float *up1,
                                           float *out_rgb) {
        return arctic_bloom_pixels(&bloom, n, pixel_xy, width, height, rgb, up1, out_rgb) == ARCTIC_OK;
    }

    // auto-exposure (include/arctic_hip.h: arctic_exposure_device and the definition in front of it).  Meter, resolve and apply on device planes
    // (nullptr: the handle's HDR plane per exposure.flags, the handle's own output); stream-ordered, nothing is read back
    [[nodiscard]] bool exposure_device(const ArcticSettings &settings, const ArcticExposure &exposure, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8) {
        return ok(arctic_exposure_device(m_handle, &settings, &exposure, d_hdr_rgb32f, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool exposure(const ArcticSettings &settings, const ArcticExposure &exposure, const float *hdr_rgb32f, uint8_t *out_rgba8) {
        return ok(arctic_exposure(m_handle, &settings, &exposure, hdr_rgb32f, out_rgba8));
    }
    // what the latest calls left; any pointer may be nullptr
    [[nodiscard]] bool read_exposure(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, uint32_t *hist256, ArcticExposureState *state) {
        return ok(arctic_read_exposure(m_handle, ldr_rgb, hdr_rgb, rgba8, hist256, state));
    }
    [[nodiscard]] bool exposure_reset() { return ok(arctic_exposure_reset(m_handle)); }
    // {device bytes, launches of k_exposure_apply, calls, launches of k_exposure_meter}
    [[nodiscard]] bool exposure_info(uint64_t out4[4]) { return ok(arctic_exposure_info(m_handle, out4)); }
    // the meter's geometry (out: 3 numbers), the per-call rate and the host arbiters: no handle, no GPU
    [[nodiscard]] static bool exposure_layout(uint32_t width, uint32_t height, uint64_t *out3) { return arctic_exposure_layout(width, height, out3) == ARCTIC_OK; }
    [[nodiscard]] static float exposure_rate(float dt, float speed) { return arctic_exposure_rate(dt, speed); }
    [[nodiscard]] static bool exposure_histogram(const ArcticExposure &exposure, uint32_t width, uint32_t height, const float *rgb, uint32_t *hist256) {
        return arctic_exposure_histogram(&exposure, width, height, rgb, hist256) == ARCTIC_OK;
    }
    [[nodiscard]] static bool exposure_resolve(const ArcticExposure &exposure, const uint32_t *hist256, const ArcticExposureState *previous, ArcticExposureState *state) {
        return arctic_exposure_resolve(&exposure, hist256, previous, state) == ARCTIC_OK;
    }
    [[nodiscard]] static bool exposure_pixels(uint64_t n, const float *rgb, float exposure, float *out_rgb) { return arctic_exposure_pixels(n, rgb, exposure, out_rgb) == ARCTIC_OK; }

    // volumetric fog (include/arctic_hip.h: arctic_fog_device and the definition in front of it).  The march on device planes (nullptr: the
    // handle's HDR plane per fog.flags, every depth 1.0, the handle's own outputs; offsets16: 16 floats in host memory or nullptr); stream-ordered
    [[nodiscard]] bool fog_device(const ArcticSettings &settings, const ArcticFog &fog, const ArcticFogView &view, const float *offsets16, const float *d_hdr_rgb32f,
                                  const float *d_depth, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8) {
        return ok(arctic_fog_device(m_handle, &settings, &fog, &view, offsets16, d_hdr_rgb32f, d_depth, d_out_hdr_rgb32f, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool fog(const ArcticSettings &settings, const ArcticFog &fog, const ArcticFogView &view, const float *offsets16, const float *hdr_rgb32f, const float *depth,
                           float *out_hdr_rgb32f, uint8_t *out_rgba8) {
        return ok(arctic_fog(m_handle, &settings, &fog, &view, offsets16, hdr_rgb32f, depth, out_hdr_rgb32f, out_rgba8));
    }
    // the scene's view record, the depth plane, then the march of the handle's planes
    [[nodiscard]] bool pass_fog(const ArcticScene &scene, const ArcticSettings &settings, const ArcticFog &fog, const float *offsets16, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_fog(m_handle, &scene, &settings, &fog, offsets16, d_out_rgba8));
    }
    // what the latest call left, row-major; any pointer may be nullptr
    [[nodiscard]] bool read_fog(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) { return ok(arctic_read_fog(m_handle, ldr_rgb, hdr_rgb, rgba8)); }
    // {device bytes, launches of k_fog_march, calls, uploads of the offset table}
    [[nodiscard]] bool fog_info(uint64_t out4[4]) { return ok(arctic_fog_info(m_handle, out4)); }
    // the view record of a scene and the host arbiter: no handle, no GPU
    [[nodiscard]] static bool fog_view(const ArcticScene &scene, uint32_t width, uint32_t height, ArcticFogView *out) { return arctic_fog_view(&scene, width, height, out) == ARCTIC_OK; }
    [[nodiscard]] static bool fog_pixels(const ArcticFog &fog, const ArcticFogView &view, const float *offsets16, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height,
                                         const float *rgb, const float *depth, const float *shadow, uint32_t S, float *out_rgb, float *terms2) {
        return arctic_fog_pixels(&fog, &view, offsets16, n, pixel_xy, width, height, rgb, depth, shadow, S, out_rgb, terms2) == ARCTIC_OK;
    }
    [[nodiscard]] static float fog_exp2(float x) { return arctic_fog_exp2(x); }
    [[nodiscard]] static bool fog_exp2_poly(uint64_t n, const float *f, float *p) { return arctic_fog_exp2_poly(n, f, p) == ARCTIC_OK; }

    // temporal upscaling (include/arctic_hip.h: arctic_taa_upscale_device and the definition in front of it).  The handle's jittered frame into a
    // history of upscale.out_width x out_height on device planes (nullptr: the handle's HDR plane per upscale.flags, zero velocity, the handle's
    // own output); stream-ordered
    [[nodiscard]] bool taa_upscale_device(const ArcticSettings &settings, const ArcticTaaUpscale &upscale, const float *d_hdr_rgb32f, const float *d_velocity2, uint8_t *d_out_rgba8) {
        return ok(arctic_taa_upscale_device(m_handle, &settings, &upscale, d_hdr_rgb32f, d_velocity2, d_out_rgba8));
    }
    // the same from and to host memory; synchronous
    [[nodiscard]] bool taa_upscale(const ArcticSettings &settings, const ArcticTaaUpscale &upscale, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8) {
        return ok(arctic_taa_upscale(m_handle, &settings, &upscale, hdr_rgb32f, velocity2, out_rgba8));
    }
    // the frame's one motion call into planes the handle owns, then the upscale of the handle's HDR plane
    [[nodiscard]] bool pass_taa_upscale(const ArcticScene &scene, const ArcticSettings &settings, const ArcticTaaUpscale &upscale, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_taa_upscale(m_handle, &scene, &settings, &upscale, d_out_rgba8));
    }
    // the next call is a first call
    [[nodiscard]] bool taa_upscale_reset() { return ok(arctic_taa_upscale_reset(m_handle)); }
    // what the latest call left, row-major at the output size; any pointer may be nullptr
    [[nodiscard]] bool read_taa_upscale(float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8) { return ok(arctic_read_taa_upscale(m_handle, ldr_rgb, hdr_rgb, count, rgba8)); }
    // the accumulated HDR colour as a row-major device plane of the output size: the next stage's explicit colour, on a handle of that size
    [[nodiscard]] bool taa_upscale_hdr_device(float *d_hdr_rgb32f) { return ok(arctic_taa_upscale_hdr_device(m_handle, d_hdr_rgb32f)); }
    // {device bytes, launches of k_taa_upscale, calls since the last reset, W | H << 32}
    [[nodiscard]] bool taa_upscale_info(uint64_t out4[4]) { return ok(arctic_taa_upscale_info(m_handle, out4)); }
    // the host arbiter and the jitter sequence: no handle, no GPU
    [[nodiscard]] static bool taa_upscale_pixels(const ArcticTaaUpscale &upscale, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb,
                                                 const float *velocity2, const float *prev_rgbn, float *out_rgbn) {
        return arctic_taa_upscale_pixels(&upscale, n, pixel_xy, width, height, cur_rgb, velocity2, prev_rgbn, out_rgbn) == ARCTIC_OK;
    }
    [[nodiscard]] static bool taa_upscale_jitter(uint32_t index, uint32_t w, uint32_t W, uint32_t h, uint32_t H, float out2[2]) {
        return arctic_taa_upscale_jitter(index, w, W, h, H, out2) == ARCTIC_OK;
    }

    // indirect diffuse light (include/arctic_hip.h: arctic_trace_gi and the definition in front of it): gi.n_rays rounds of one closest-hit ray per
    // pixel of the resident G-buffer from dirs (P * P sets of n_rays local directions, z along the normal: cosine-weighted for an irradiance
    // estimate), each shaded at its hit or by the environment map -> rows x width float4 {mean colour, rays}; rgba32f = nullptr leaves it on the
    // device.  The filter (whole frames only) sums over the P x P window of the pattern
    [[nodiscard]] bool trace_gi(const ArcticScene &scene, const ArcticGi &gi, const float *dirs, float *rgba32f) { return ok(arctic_trace_gi(m_handle, &scene, &gi, dirs, rgba32f)); }
    // the same into device memory the caller owns, in stream order on the handle's stream
    [[nodiscard]] bool trace_gi_device(const ArcticScene &scene, const ArcticGi &gi, const float *dirs, float *d_rgba32f) {
        return ok(arctic_trace_gi_device(m_handle, &scene, &gi, dirs, d_rgba32f));
    }
    // round `round`'s ray records, for tests
    [[nodiscard]] bool gi_rays(const ArcticGi &gi, const float *dirs, uint32_t round, ArcticRay *rays) { return ok(arctic_gi_rays(m_handle, &gi, dirs, round, rays)); }
    // the latest call's sum and estimate planes; either may be nullptr
    [[nodiscard]] bool read_gi_estimate(float *sum_rgba32f, float *estimate_rgba32f) { return ok(arctic_read_gi_estimate(m_handle, sum_rgba32f, estimate_rgba32f)); }
    // {device bytes of the table, S and E, launches of the stage's own kernels, tracing calls, 0}
    [[nodiscard]] bool gi_info(uint64_t out4[4]) { return ok(arctic_gi_info(m_handle, out4)); }
    // the temporal accumulation of E: the device plane d_gi_in blended into the handle's history, reprojected through the previous call's camera, into
    // d_gi_out (it may be the same plane); in stream order.  accumulate_gi: the host form, synchronous
    [[nodiscard]] bool accumulate_gi_device(const ArcticScene &scene, const ArcticGiHistory &hist, const float *d_gi_in_rgba32f, float *d_gi_out_rgba32f) {
        return ok(arctic_accumulate_gi_device(m_handle, &scene, &hist, d_gi_in_rgba32f, d_gi_out_rgba32f));
    }
    [[nodiscard]] bool accumulate_gi(const ArcticScene &scene, const ArcticGiHistory &hist, const float *gi_in_rgba32f, float *gi_out_rgba32f) {
        return ok(arctic_accumulate_gi(m_handle, &scene, &hist, gi_in_rgba32f, gi_out_rgba32f));
    }
    [[nodiscard]] bool gi_history_reset() { return ok(arctic_gi_history_reset(m_handle)); }
    [[nodiscard]] bool read_gi_history(float *acc3, float *count, float *world3, float *normal3) { return ok(arctic_read_gi_history(m_handle, acc3, count, world3, normal3)); }
    // the composition: C (nullptr: the handle's shaded or composed plane) + the ambient correction + base * E (nullptr: the handle's estimate), then the
    // tonemapper, into the caller's planes or (nullptr) the handle's own: read_gi
    [[nodiscard]] bool gi_compose_device(const ArcticScene &scene, const ArcticSettings &settings, const ArcticGiCompose &compose, const float *d_hdr_rgb32f,
                                         const float *d_gi_rgba32f, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8) {
        return ok(arctic_gi_compose_device(m_handle, &scene, &settings, &compose, d_hdr_rgb32f, d_gi_rgba32f, d_out_hdr_rgb32f, d_out_rgba8));
    }
    [[nodiscard]] bool read_gi(float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) { return ok(arctic_read_gi(m_handle, ldr_rgb, hdr_rgb, rgba8)); }
    // the one call: trace, accumulate when hist is given, compose
    [[nodiscard]] bool pass_gi(const ArcticScene &scene, const ArcticSettings &settings, const ArcticGi &gi, const float *dirs, const ArcticGiHistory *hist,
                               const ArcticGiCompose &compose, uint8_t *d_out_rgba8) {
        return ok(arctic_pass_gi(m_handle, &scene, &settings, &gi, dirs, hist, &compose, d_out_rgba8));
    }
    // the host arbiters: no handle, no GPU
    [[nodiscard]] static bool gi_accumulate_pixels(const ArcticGiHistory &hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const float *cur4,
                                                   const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_acc3, const float *prev_count,
                                                   const float *prev_world3, const float *prev_normal3, float *out4, float *out_acc3, float *out_count, float *out_world3,
                                                   float *out_normal3) {
        return arctic_gi_accumulate_pixels(&hist, n, world3, normal3, geometry, cur4, prev_proj_view, width, height, prev_acc3, prev_count, prev_world3, prev_normal3, out4,
                                           out_acc3, out_count, out_world3, out_normal3) == ARCTIC_OK;
    }
    [[nodiscard]] static bool gi_compose_pixels(const ArcticGiCompose &compose, float ambient, uint64_t n, const float *hdr3, const float *base3, const float *metal,
                                                const float *gi4, const uint8_t *geometry, float *out_hdr3) {
        return arctic_gi_compose_pixels(&compose, ambient, n, hdr3, base3, metal, gi4, geometry, out_hdr3) == ARCTIC_OK;
    }
    [[nodiscard]] static bool gi_points(const float *points6, const uint32_t *sets, uint64_t n_points, const ArcticGi &gi, const float *dirs, uint32_t round, ArcticRay *rays) {
        return arctic_gi_points(points6, sets, n_points, &gi, dirs, round, rays) == ARCTIC_OK;
    }
    [[nodiscard]] static bool gi_estimate_pixels(const ArcticGi &gi, uint32_t width, uint32_t height, const ArcticRay *rays, const float *colors4, const float *normal3,
                                                 const float *world3, const uint8_t *geometry, float *sum4, float *estimate4) {
        return arctic_gi_estimate_pixels(&gi, width, height, rays, colors4, normal3, world3, geometry, sum4, estimate4) == ARCTIC_OK;
    }

    const std::string &last_error() const { return m_error; }
    ArcticRenderer *handle() const { return m_handle; }

  private:
    bool ok(int rc) {
        if (rc >= 0) return true;
        m_error = m_handle ? arctic_last_error(m_handle) : "renderer not initialised";
        return false;
    }
    ArcticCreateInfo m_info;
    ArcticRenderer *m_handle = nullptr;
    std::string m_error;
    bool m_gltf_skinned = false;   // pose_gltf has attached the file's skins
};

}  // namespace ArcticAMD::Renderer
