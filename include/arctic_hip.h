/*
 * arctic_hip.h -- C-ABI of the MI355X-native forward PBR shading path.
 *
 * This is the drop-in boundary for the per-pixel work of arctic-renderer's
 * shaders/forward.hlsl + shaders/post_process.hlsl.  The reference has no FFI;
 * the seam is the public surface of class Arctic::Renderer::Renderer
 * (reference src/renderer/renderer.hpp:94-125), the only thing src/app.cpp
 * calls.  Every entry point below names the reference call it replaces.
 *
 * Conventions
 *   - plain C: pointers + sizes only, no C++/torch types.
 *   - every fallible call returns int: >= 0 ok (an index where one is
 *     documented), < 0 an ARCTIC_E_* code.  The reference returns
 *     [[nodiscard]] bool and logs (src/renderer/dxerr.hpp:5-10); here the
 *     message is kept per handle and read with arctic_last_error().
 *   - inputs are borrowed for the duration of the call and copied to device
 *     memory synchronously (reference: blocking fence inside every upload,
 *     src/renderer/rhi.cpp:480-519); the handle owns all device memory.
 *   - a handle is not thread-safe (reference is single threaded).
 *   - matrices are 16 floats in glm memory order (column major), the same
 *     bytes the reference pushes as root constants
 *     (src/renderer/forward_pass.hpp:16-34).
 *   - there is NO CPU fallback: without a HIP device arctic_create() fails.
 */
#ifndef ARCTIC_HIP_H
#define ARCTIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes --------------------------------------------------------- */
#define ARCTIC_OK            0
#define ARCTIC_E_INVALID    -1 /* bad argument (null, zero size, index out of range) */
#define ARCTIC_E_DEVICE     -2 /* a HIP runtime call failed (message has hipGetErrorString) */
#define ARCTIC_E_NO_DEVICE  -3 /* no HIP device / device ordinal out of range */
#define ARCTIC_E_STATE      -4 /* call order (e.g. shade before any G-buffer exists) */
#define ARCTIC_E_CAPACITY   -5 /* more lights than max_lights, etc. */

/* ---- POD scene types: byte-compatible with src/renderer/scene.hpp -------- */

/* scene.hpp:20-38  Camera{vec3 eye; vec2 rotation; float aspect; float fov_y; array<float,2> z_near_far} */
typedef struct ArcticCamera {
    float eye[3];
    float rotation[2];   /* degrees: x = pitch, y = yaw (scene.cpp:9-19) */
    float aspect;
    float fov_y;         /* degrees */
    float z_near_far[2];
} ArcticCamera;

/* scene.hpp:40-47  Vertex, 14 floats = 56 B; input layout forward_pass.cpp:89-135 */
typedef struct ArcticVertex {
    float position[3];
    float normal[3];
    float tangent[3];
    float bitangent[3];
    float tex_coords[2];
} ArcticVertex;

/* scene.hpp:69-73  Object{mat4 trs; size_t mesh_idx} */
typedef struct ArcticObject {
    float    trs[16];    /* glm column-major */
    uint64_t mesh_idx;
} ArcticObject;

/* scene.hpp:75-84  DirectionalLight{vec3 position; vec2 rotation; vec3 color} */
typedef struct ArcticDirectionalLight {
    float position[3];
    float rotation[2];   /* degrees */
    float color[3];
} ArcticDirectionalLight;

/* scene.hpp:88-94  PointLight, 32 B with pads (== HLSL cbuffer packing, forward.hlsl:20-24) */
typedef struct ArcticPointLight {
    float    position[3];
    uint32_t padding0;
    float    color[3];
    uint32_t padding1;
} ArcticPointLight;

/* A spot light (no counterpart in the reference: its roadmap's "Spotlights"), 48 B, no padding.  The cone and the range follow glTF's
 * KHR_lights_punctual; see arctic_update_spot_lights for the exact semantics. */
typedef struct ArcticSpotLight {
    float position[3];
    float range;             /* > 0: the KHR window below; 0 = unlimited (KHR: range undefined) */
    float direction[3];      /* where the light points (glTF: the node's -Z); any finite non-zero length, normalised by the library */
    float inner_cone_angle;  /* radians, 0 <= inner <= outer */
    float color[3];          /* linear colour * intensity: the radiance at distance 1 on the axis (glTF: color * intensity in candela) */
    float outer_cone_angle;  /* radians, 0 < outer <= pi; pi = no cone at all (an omnidirectional light with a range) */
} ArcticSpotLight;

/* A shadow-casting point light (no counterpart in the reference: its roadmap's "Point light shadows"), 32 B, no padding: a point light
 * with a cube of six depth maps around it.  See arctic_update_point_shadow_lights for the exact semantics. */
typedef struct ArcticPointShadowLight {
    float position[3];
    float z_near;            /* the cube's near plane, > 0 */
    float color[3];          /* like ArcticPointLight.color: the radiance at distance 1 */
    float z_far;             /* the cube's far plane, > z_near; it only limits the shadow (the light itself has no range) */
} ArcticPointShadowLight;

/* scene.hpp:96-103 Scene; std::vector members flattened to pointer + count.
 * point_lights here is ignored by render_frame exactly as in the reference
 * (renderer.cpp:285-407 uses the buffer last written by update_lights). */
typedef struct ArcticScene {
    ArcticCamera            camera;
    float                   ambient;
    ArcticDirectionalLight  sun;
    const ArcticPointLight *point_lights;
    uint64_t                n_point_lights;
    const ArcticObject     *objects;
    uint64_t                n_objects;
} ArcticScene;

/* scene.hpp:105-110 Settings{int tm_method=0; float gamma=2.2; float exposure=1} */
typedef struct ArcticSettings {
    int32_t tm_method;   /* 0 Reinhard (also any other value), 1 Exposure, 2 ACES: post_process.hlsl:76-89 */
    float   gamma;
    float   exposure;
} ArcticSettings;

#define ARCTIC_TM_REINHARD 0
#define ARCTIC_TM_EXPOSURE 1
#define ARCTIC_TM_ACES     2

/* create-time parameters: every compile-time constant of the reference that
 * BASELINE.json's configs vary becomes a field here. */
typedef struct ArcticCreateInfo {
    uint32_t width, height;  /* render-target size (renderer.hpp:94, App::WINDOW_WIDTH/HEIGHT app.hpp:20-21) */
    uint32_t shadow_size;    /* ShadowMapPass::SIZE = 4000 (shadow_map_pass.hpp:23); 0 = no shadow map, shadow term 0 */
    uint32_t max_lights;     /* Renderer::MAX_NUM_POINT_LIGHTS = 16 (renderer.hpp:22) */
    int32_t  device;         /* HIP device ordinal */
    uint32_t row_begin;      /* screen-space shard: this handle renders rows [row_begin,row_end) ... */
    uint32_t row_end;        /* ... of the width x height frame; 0,0 = whole frame */
    /* or an INTERLEAVED shard (load balance: lit regions are spatially clustered): with band_rows > 0 (a multiple of 8;
     * row_begin = row_end = 0) the handle owns the rows y with (y / band_rows) % shard_count == shard_index, and its
     * output holds those rows packed in ascending order. */
    uint32_t band_rows;
    uint32_t shard_index;
    uint32_t shard_count;
} ArcticCreateInfo;

typedef struct ArcticRenderer ArcticRenderer; /* opaque */

/* ---- life cycle ---------------------------------------------------------- */

/* replaces Renderer::Renderer(window,w,h) + bool Renderer::init()
 * (renderer.hpp:94-100, renderer.cpp:22-231); no window.  On failure returns
 * NULL and, if err/err_len given, writes the message there. */
ArcticRenderer *arctic_create(const ArcticCreateInfo *info, char *err, uint64_t err_len);

/* replaces Renderer::cleanup() + destructor (renderer.hpp:102) */
void arctic_destroy(ArcticRenderer *r);

/* last error message of this handle ("" if none); valid until the next call */
const char *arctic_last_error(const ArcticRenderer *r);

/* replaces bool Renderer::resize(uint32_t&,uint32_t&) (renderer.hpp:104).  Unlike
 * the reference (which only resizes the swapchain, renderer.cpp:241-272) this
 * really reallocates the targets; the row shard is reset to the whole frame. */
int arctic_resize(ArcticRenderer *r, uint32_t width, uint32_t height);

/* replaces bool Renderer::flush() (renderer.hpp:122-125): device idle */
int arctic_flush(ArcticRenderer *r);

/* run everything on a HIP stream the caller owns (a hipStream_t passed as void*; NULL is HIP's default stream, which is
 * what torch.cuda.current_stream() usually is), e.g. the stream a following RCCL gather is enqueued on, so that no host
 * synchronisation is needed between the frame and the collective.  arctic_use_own_stream() returns to the handle's
 * private stream.  The stream in use before the switch is drained first. */
int arctic_set_stream(ArcticRenderer *r, void *hip_stream);
int arctic_use_own_stream(ArcticRenderer *r);

/* ---- scene upload -------------------------------------------------------- */

/* replaces bool Renderer::create_material(void*,w,h, void*,w,h, void*,w,h)
 * (renderer.hpp:112-116, renderer.cpp:475-553): three tightly packed RGBA8
 * images; diffuse is sRGB, the other two linear.  Returns the material index
 * (= call order, like m_materials.emplace_back). */
int arctic_create_material(ArcticRenderer *r,
                           const void *diffuse, uint32_t diffuse_w, uint32_t diffuse_h,
                           const void *normal, uint32_t normal_w, uint32_t normal_h,
                           const void *metal_rough, uint32_t mr_w, uint32_t mr_h);

/* replaces bool Renderer::create_mesh(span<Vertex>, span<uint32_t>, MaterialIdx)
 * (renderer.hpp:109-110, renderer.cpp:417-473).  Returns the mesh index. */
int arctic_create_mesh(ArcticRenderer *r,
                       const ArcticVertex *vertices, uint64_t n_vertices,
                       const uint32_t *indices, uint64_t n_indices,
                       uint64_t material_idx);

/* ---- skeletal skinning (no counterpart in the reference, whose meshes are rigid) --------------------------------------------------------
 * A mesh may carry a SKIN -- per vertex four joint indices and four weights -- and, with it, a POSE: one matrix per joint.  While a pose is
 * set, every pass reads a deformed copy of the mesh's vertex buffer, written on the device by one kernel per pose change (skin.hip, k_skin);
 * the rasterisers, the shadow maps, the cube faces and the shading see an ordinary mesh and are unchanged.
 *
 * The arithmetic, defined exactly.  Joint matrices are 16 floats each in glm memory order (m[col * 4 + row]) like ArcticObject::trs.  For a
 * vertex with joints j0..j3 and weights w0..w3, position (x, y, z) and each of its three vectors v = normal, tangent, bitangent:
 *   S[e]  = ((w0*J[j0][e] + w1*J[j1][e]) + w2*J[j2][e]) + w3*J[j3][e]          e = 0..15; only rows 0..2 (e % 4 != 3) are used
 *   pos'  = for i in 0..2: ((S[i]*x + S[4+i]*y) + S[8+i]*z) + S[12+i]*1.0f
 *   v'    = for i in 0..2:  (S[i]*v.x + S[4+i]*v.y) + S[8+i]*v.z
 *   uv'   = uv
 * Every operation is fp32 and rounds once, in the written order, without contraction: numpy in float32 reproduces the result bit for bit
 * (tests/skin_reference.py), and so does arctic_skin_vertices on the host.  Nothing is normalised here (the vertex kernel normalises the three
 * vectors as it always has), and the weights are used as given: the library does not renormalise them (weights that do not sum to 1 scale the
 * vertex).  LIMIT: the vectors go through the upper 3 x 3 of S, not through its inverse transpose.  That is exact for rigid joints and for
 * uniform scale; under non-uniform scale or shear the normals lean the wrong way.
 *
 * A pose belongs to the MESH: every object that uses the mesh shows it.  Two instances in different poses are two meshes.
 * While a mesh has a pose, the object-space cluster boxes arctic_create_mesh made for ARCTIC_OPT_CLUSTER_CULL do not describe it: the mesh is
 * then drawn with boxes that are never skipped (it is culled per triangle like any mesh under ARCTIC_OPT_CLUSTER_CULL = 0); the bind pose
 * gets its real boxes back.  arctic_render_frame's shadow caches (ARCTIC_OPT_SHADOW_CACHE) count every successful skin and pose call of a mesh
 * the scene uses as a change: the sun's map and the cube faces are redrawn.  Each rank of a sharded frame poses its own copy. */
typedef struct ArcticSkinVertex {   /* 24 bytes */
    uint16_t joints[4];   /* every index < n_joints, also in slots whose weight is 0 */
    float    weights[4];  /* finite; used as given */
} ArcticSkinVertex;

/* Attaches a skin to an existing mesh, or replaces the one it has (a replaced skin takes its pose with it: the mesh is in its bind pose until the
 * next arctic_set_mesh_pose).  skin == NULL detaches the skin and any pose.  Synchronous like arctic_create_mesh; replacing or detaching drains
 * the stream in use first.  ARCTIC_E_INVALID, the mesh left as it was: n_vertices is not the mesh's vertex count, n_joints is 0 or above 65535,
 * a joint index at or above n_joints, a weight that is not finite, a mesh that does not exist.
 * A mesh with a skin and no pose renders its own vertices, bit for bit as without the skin. */
int arctic_set_mesh_skin(ArcticRenderer *r, uint64_t mesh, const ArcticSkinVertex *skin, uint64_t n_vertices, uint32_t n_joints);

/* Poses a skinned mesh: n_joints matrices of 16 floats.  The matrices are copied before the call returns (the caller may free them at once);
 * the deformation is enqueued on the handle's stream, in order with the passes -- no host synchronisation is needed or made, and a pose set
 * between two arctic_render_frame calls applies to exactly the frames after it.  NULL, 0 returns the mesh to its bind pose (its original buffer).
 * ARCTIC_E_STATE: the mesh has no skin.  ARCTIC_E_INVALID, the previous pose kept: n_joints is not the skin's, a matrix element is not finite, a
 * mesh that does not exist.
 * Ordering: the kernel runs on the main stream, which every frame's prepass and shadow streams have been joined into, and those streams wait
 * for it before their next pass; so a frame in flight whose prepass would have run beside the previous frame's shading starts after the pose
 * instead (what that costs). */
int arctic_set_mesh_pose(ArcticRenderer *r, uint64_t mesh, const float *joint_matrices, uint32_t n_joints);

/* The vertices the next prepass will read for this mesh -- posed, else morphed, else its own (tests). n_vertices must be the mesh's vertex count.  Synchronises. */
int arctic_read_mesh_vertices(ArcticRenderer *r, uint64_t mesh, ArcticVertex *out, uint64_t n_vertices);

/* The validation arctic_set_mesh_skin applies to the records: ARCTIC_OK or ARCTIC_E_INVALID (NULL and n_vertices = 0 are invalid here).
 * Host only, no handle. */
int arctic_check_mesh_skin(const ArcticSkinVertex *skin, uint64_t n_vertices, uint32_t n_joints);

/* The arithmetic above on the host, operation for operation: out[v] = the posed in[v] (out may be in).  ARCTIC_E_INVALID (nothing written):
 * a null pointer, records arctic_check_mesh_skin refuses, a matrix element that is not finite.  Host only, no handle. */
int arctic_skin_vertices(const ArcticVertex *in, const ArcticSkinVertex *skin, uint64_t n_vertices,
                         const float *joint_matrices, uint32_t n_joints, ArcticVertex *out);

/* ---- morph targets (blend shapes; no counterpart in the reference) -----------------------------------------------------------------------
 * A mesh may carry n_targets MORPH TARGETS -- per target one ArcticMorphDelta per vertex -- and one WEIGHT per target.  While any weight is not
 * zero, every pass reads a blended copy of the mesh's vertex buffer, written on the device by one kernel per weights change (morph.hip, k_morph).
 *
 * The arithmetic, defined exactly.  With e = the 12 floats of position, normal, tangent and bitangent of vertex v, and k0 < k1 < ... the targets
 * whose weight is not 0.0f (weights of either sign of zero are skipped), in ascending target index:
 *   m[e] = base[e];   for k in k0, k1, ...:  m[e] = m[e] + w[k] * delta[k][v][e]
 *   uv'  = uv
 * Every operation is fp32: the product rounds once, then the sum rounds once, in the written order, without contraction.  numpy in float32
 * reproduces the result bit for bit (tests/morph_reference.py), and so does arctic_morph_vertices on the host.  Nothing is normalised here (the
 * vertex kernel normalises the three vectors as it always has).  Weights are used as given: negative values and values above 1 are legal.
 * SKIPPING IS PART OF THE DEFINITION, not only an optimisation: "all weights zero" is the mesh's own vertices bit for bit, a -0.0 included (adding
 * 0 * d would turn it into +0.0), and a target at rest costs no memory traffic.
 * LIMIT: the bitangent is blended linearly like the other three vectors; it is not recomputed from the blended normal and tangent.  The caller
 * supplies its delta (the glTF loader's rule: include/arctic_gltf.h).
 * ORDER WITH A SKIN: morph first, then skin, as glTF specifies.  The buffer the passes read for a morphed and posed mesh is skin(morph(base)),
 * both steps by their own definitions, so the composition is bit-defined too.
 *
 * Like a pose, weights belong to the MESH.  A mesh whose weights are not all zero is drawn with cluster boxes that are never skipped (its real
 * boxes return when the weights return to zero and there is no pose), and every successful targets or weights call counts as a change for
 * arctic_render_frame's shadow caches.  Each rank of a sharded frame morphs its own copy. */
typedef struct ArcticMorphDelta {   /* 48 bytes */
    float position[3], normal[3], tangent[3], bitangent[3];   /* finite */
} ArcticMorphDelta;

/* Attaches morph targets to an existing mesh, or replaces the ones it has.  deltas is target-major: deltas[k * n_vertices + v].  deltas == NULL
 * detaches them (n_vertices and n_targets are then ignored).  Synchronous like arctic_set_mesh_skin; replacing or detaching drains the stream in
 * use first.  All weights are zero afterwards: the mesh renders its own vertices, or -- if it is posed -- the pose of its own vertices (the pose
 * is applied again from the matrices the mesh holds).
 * ARCTIC_E_INVALID, the mesh left as it was: a mesh that does not exist, n_vertices is not the mesh's vertex count, n_targets outside 1..65535,
 * a delta that is not finite.  ARCTIC_E_DEVICE, the mesh left as it was: the n_targets * n_vertices * 48 bytes cannot be allocated. */
int arctic_set_mesh_morph_targets(ArcticRenderer *r, uint64_t mesh, const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets);

/* Sets the weights of a mesh with morph targets: n_targets floats.  The weights are copied before the call returns; the blend is enqueued on the
 * handle's stream, in order with the passes, exactly like arctic_set_mesh_pose -- no host synchronisation, no device drain, and weights set
 * between two arctic_render_frame calls apply to exactly the frames after them.  NULL, 0, or weights that are all zero, return the mesh to its
 * own vertices (the blended buffer is kept for the next call; no blend is launched).  If the mesh is posed, the pose is applied again behind the
 * blend, from the blended buffer and the matrices the mesh holds.
 * ARCTIC_E_STATE: the mesh has no targets.  ARCTIC_E_INVALID, the previous weights kept: n_targets is not the mesh's, a weight that is not
 * finite, a mesh that does not exist. */
int arctic_set_mesh_morph_weights(ArcticRenderer *r, uint64_t mesh, const float *weights, uint32_t n_targets);

/* The validation arctic_set_mesh_morph_targets applies to the records: ARCTIC_OK or ARCTIC_E_INVALID (NULL, n_vertices = 0 and n_targets
 * outside 1..65535 are invalid here).  Host only, no handle. */
int arctic_check_morph_targets(const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets);

/* The arithmetic above on the host, operation for operation: out[v] = the blended in[v] (out may be in).  ARCTIC_E_INVALID (nothing written):
 * a null pointer, records arctic_check_morph_targets refuses, a weight that is not finite.  Host only, no handle. */
int arctic_morph_vertices(const ArcticVertex *in, const ArcticMorphDelta *deltas, uint64_t n_vertices, uint32_t n_targets,
                          const float *weights, ArcticVertex *out);

/* glTF material factors, emissive and occlusion (no counterpart in the reference, whose material is three images).  Per material twelve
 * floats and two optional images. */
typedef struct ArcticMaterialParams {   /* 48 bytes */
    float base_color_factor[3];   /* linear RGB, each in [0, 1] */
    float metallic_factor;        /* [0, 1] */
    float roughness_factor;       /* [0, 1] */
    float normal_scale;           /* finite */
    float occlusion_strength;     /* [0, 1] */
    float emissive_factor[3];     /* linear RGB, finite, >= 0 (may exceed 1: emissive strength is pre-multiplied) */
    float reserved[2];            /* must be 0 */
} ArcticMaterialParams;
/* neutral = {1,1,1, 1, 1, 1, 1, 0,0,0, 0,0} and no images.
 *
 * arctic_set_material_extras may be called at any time after the material exists; it drains the stream in use first and is synchronous like
 * arctic_create_material, and it REPLACES what the material had.  params == NULL with no images returns the material to neutral (params ==
 * NULL with an image: the neutral factors and that image).  emissive_rgba8 is a tightly packed sRGB RGBA8 image of which rgb is used,
 * occlusion_rgba8 a linear one of which R is used (glTF's convention: it may be the very metal-rough image); NULL, 0, 0 = no image.
 * ARCTIC_E_INVALID, the material left as it was: a field out of range or not finite, a non-zero reserved field, an image side of 0 with a
 * non-null pointer (or a null pointer with a non-zero side), a material index that does not exist.  ARCTIC_E_CAPACITY: an image side above 65535.
 *
 * For a covered pixel start from what ps_main filters today -- base rgb (decoded per texel, then filtered), the normal-map bytes nr, ng, nb
 * on the 0..255 scale, rough and metal; ARCTIC_OPT_TEXTURE_MIPS and ARCTIC_OPT_SAMPLER bit 0 apply to these exactly as without extras.  Then
 *   base'  = base * base_color_factor                      (per channel)
 *   metal' = metal * metallic_factor      rough' = rough * roughness_factor
 *   t      = (nr*2/255 - 1, -(ng*2/255 - 1), nb*2/255 - 1) (today's tangent-space normal)
 *   n'     = normalize(T * t.x*normal_scale + B * t.y*normal_scale + N * t.z)
 *   o      = occlusion image R, linear, bilinear + WRAP, texel centres at +0.5   (no image: 1)
 *   ao     = 1 + occlusion_strength * (o - 1)
 *   e      = emissive image rgb, sRGB-decoded per texel, then filtered the same way      (no image: 1,1,1)
 *   E      = e * emissive_factor
 *   A      = ambient * base'     or, with ARCTIC_OPT_ENV_LIGHTING, ambient * ibl(n', wo, base', metal', rough')
 *   color  = Lo(base', metal', rough', n') * (1 - shadow) + A * ao + E
 * Lo is every light the handle has (sun, point, spot, shadow-casting point lights), unchanged apart from its inputs.  Occlusion scales the
 * indirect term only (glTF's rule); emission carries neither (1 - shadow) nor ao: a fully sun-shadowed pixel is A * ao + E, and without
 * ARCTIC_OPT_ENV_LIGHTING it still never loads its position or tangent frame (exact culling stays).  ARCTIC_OPT_SAMPLER bit 0 applies to
 * the two images as to the other three; ARCTIC_OPT_HDR16 rounds the final colour, emission included.  The two images are filtered at
 * LEVEL 0 under both settings of ARCTIC_OPT_TEXTURE_MIPS: they have no chains (yet).
 *
 * Nothing changes unless asked: a handle whose materials are all neutral launches exactly the kernels it launched before this call
 * existed.  While a material is not neutral every tile goes through the general tile code (kernels k_pbrlit / k_pbrlit_vis, spot, cube, ENV
 * and MIP composing as before); the pixels of a neutral material keep their bits there (the factors multiply by 1.0f and add +0.0f);
 * ARCTIC_OPT_TILE_ORDER is ignored, and ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE make a shading call return ARCTIC_E_STATE. */
int arctic_set_material_extras(ArcticRenderer *r, uint64_t material, const ArcticMaterialParams *params,
                               const void *emissive_rgba8, uint32_t ew, uint32_t eh,
                               const void *occlusion_rgba8, uint32_t ow, uint32_t oh);

/* The validation arctic_set_material_extras applies to its params: ARCTIC_OK or ARCTIC_E_INVALID (NULL is invalid here).  Host only, no handle. */
int arctic_check_material_params(const ArcticMaterialParams *params);

/* replaces void Renderer::update_lights(span<PointLight>) (renderer.hpp:120,
 * renderer.cpp:585-603): clamps to max_lights like the reference clamps to 16. */
int arctic_update_lights(ArcticRenderer *r, const ArcticPointLight *lights, uint64_t n);
/* The pair table the packed light loop walks (ARCTIC_OPT_LIGHT_PAIR_RUNS) as plain numbers, for tests; a pure host function.  slots: 2 * ceil(n / 2)
 * light indices, pair p = slots[2 p], slots[2 p + 1], 0xFFFFFFFF = the black partner of an odd count; masks: ceil(n / 2), bit c set = channel c of
 * both lights is +0.0f; run_end: 3 numbers, where the runs "skip R", "skip G" and "skip B" end (the general run ends with the table).  runs = 0: the
 * table in caller order, one general run. */
int arctic_light_pair_table(const ArcticPointLight *lights, uint64_t n, int32_t runs, uint32_t *slots, uint32_t *masks, uint32_t *run_end);

/* Spot lights (no counterpart in the reference).  Works like arctic_update_lights: replaces the handle's spot list, clamps the count to
 * max_lights; n = 0 clears the list.  A light with a NaN or inf field, a zero direction, inner > outer, outer outside (0, pi] or range < 0
 * makes the call return ARCTIC_E_INVALID, and the list the handle had stays as it was.
 * Per light the host derives, in binary64, each rounded once to fp32:
 *   s      = normalize(direction)
 *   scale  = 1 / max(1e-3, cos(inner) - cos(outer)),  offset = -cos(outer) * scale     (KHR_lights_punctual's cone formula)
 *            outer == pi: scale = 0, offset = 1 (the cone factor is exactly 1)
 *   ir2    = range > 0 ? 1 / range^2 : 0
 * A lit pixel at `world`, d = position - world, d2 = |d|^2, inv = rsq(d2), wi = d * inv, takes
 *   cd       = -dot(s, d) * inv
 *   att      = sat(cd * scale + offset)^2          (KHR cone attenuation)
 *   window   = sat(1 - (d2 * ir2)^2)               (KHR range window 1 - (dist / range)^4; with ir2 = 0 it is exactly 1)
 *   radiance = color * att * window / d2
 * into the same calculate_outgoing_radiance as a point light's (forward.hlsl:224-231), and the result into Lo.  Lo keeps the factor
 * (1 - shadow) of the sun's shadow map: a spot light does not light what the sun's shadow covers, exactly like the point lights (and fully
 * shadowed pixels skip every light).  The ambient term is unchanged, and so is the environment term of ARCTIC_OPT_ENV_LIGHTING = 1, which
 * combines with spot lights.  An omnidirectional light (outer = pi, range = 0) adds the same bits a point light with its position and
 * colour adds in the scalar light loop (ARCTIC_OPT_LIGHT_PATH = 1).  An empty list renders exactly as before.
 * With spot lights every tile goes through the general tile code (kernels k_spotlit / k_spotlit_vis), ARCTIC_OPT_TILE_ORDER is ignored,
 * and ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE make a shading call return ARCTIC_E_STATE. */
int arctic_update_spot_lights(ArcticRenderer *r, const ArcticSpotLight *lights, uint64_t n);

/* The per-light constants arctic_update_spot_lights stores on the device, 12 floats per light: position.xyz, scale, s.xyz, offset,
 * color.rgb, ir2 (semantics above).  ARCTIC_E_INVALID (nothing written) when any light is invalid.  Host only, no handle. */
int arctic_spot_light_constants(const ArcticSpotLight *lights, uint64_t n, float *out);

/* Shadow-casting point lights (no counterpart in the reference).  Works like arctic_update_spot_lights: replaces the handle's list and
 * clamps the count to max_lights; n = 0 clears it.  A light with a NaN or inf field, z_near <= 0 or z_far <= z_near makes the call return
 * ARCTIC_E_INVALID, an allocation failure ARCTIC_E_DEVICE; either way the list and faces the handle had stay as they were.  A new list
 * clears its faces to 1.0 and makes the next arctic_render_frame draw them.
 * Faces.  Light i owns 6 depth maps of F x F floats (F = ARCTIC_OPT_POINT_SHADOW_SIZE), face k = 0..5 looking along +X, -X, +Y, -Y, +Z,
 * -Z, each row-major with row 0 at clip y = +1, holding z / w of M_k = perspectiveRH_ZO(90 deg, 1, z_near, z_far) * lookAtRH(p, p + dir_k,
 * up_k), up = (0,-1,0) for +-X and +-Z, (0,0,1) for +Y, (0,0,-1) for -Y (arctic_point_shadow_matrices).  A face is drawn like the sun's
 * map: every object of the scene, front faces culled, depth LESS, cleared to 1.0.
 * Lookup, per lit pixel at `world`, d = world - p, m = max(|d.x|, |d.y|, |d.z|): the face is the axis of m (ties go to x, then y, then z)
 * and its sign;  px = 0.5 + 0.5 (s.d) / m,  py = 0.5 - 0.5 (u.d) / m,  pz = z_far / (z_far - z_near) * (1 - z_near / m), with the face's
 * lookAt rows  +X: s = -z, u = -y   -X: s = +z, u = -y   +Y: s = +x, u = +z   -Y: s = +x, u = -z   +Z: s = +x, u = -y   -Z: s = -x, u = -y.
 * If m <= z_near or pz > 1 the light is unshadowed (v = 1) and no texel is read (forward.hlsl:76: outside the map, no shadow).
 * Otherwise 2 x 2 comparison PCF with CLAMP addressing inside the face: x = px F - 0.5, y = py F - 0.5, the texels floor(x) + {0, 1} by
 * floor(y) + {0, 1} clamped to [0, F - 1], c = (pz > depth) ? 1 : 0, combined bilinearly with fx = x - floor(x), fy = y - floor(y) as
 * a + (b - a) t (four equal compares give exactly 0 or 1); v = 1 - that.  fp32 weights in every ARCTIC_OPT_SAMPLER mode; no bias (front-face
 * culling is the answer to acne, as for the sun, forward.hlsl:81): a closed occluder casts through its far side, a one-sided quad only
 * when its back faces the light.
 * The light's term is the point light's (color / |p - world|^2 into calculate_outgoing_radiance, forward.hlsl:224-231) with the colour
 * scaled by v, added to Lo behind the point and the spot lights.  Lo keeps the sun's (1 - shadow) factor: such a light does not light what
 * the sun's map covers, and fully sun-shadowed pixels skip every light, exactly like the point and spot lights.  Where v = 1 the light
 * adds the same bits as a point light with its position and colour (ARCTIC_OPT_LIGHT_PATH = 1); where v = 0 it adds nothing; an empty list
 * renders exactly as before.
 * With such lights every tile goes through the general tile code (kernels k_cubelit / k_cubelit_vis, spot lights included),
 * ARCTIC_OPT_TILE_ORDER is ignored, and ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE make a shading call return ARCTIC_E_STATE.
 * arctic_render_frame redraws the faces when the lights, F, the objects' transforms or meshes, the mesh count, ARCTIC_OPT_CLUSTER_CULL or
 * ARCTIC_OPT_SMALL_TRIANGLES changed (every frame with ARCTIC_OPT_SHADOW_CACHE = 0), on the handle's stream in front of the shading pass;
 * arctic_pass_shade uses the faces in place.  INTEGRATION.md section 5g: what a DX12 host sets. */
int arctic_update_point_shadow_lights(ArcticRenderer *r, const ArcticPointShadowLight *lights, uint64_t n);

/* The six face matrices M_k of one light (semantics above), 16 floats each in glm memory order (m[col * 4 + row]), faces in order: 96
 * floats.  fp32, camera_proj_view's helpers and operation order, with 1 / tan(45 deg) and lookAtRH's (p + dir_k) - p taken as exactly 1
 * and dir_k.  ARCTIC_E_INVALID (nothing written) for an invalid light.  Host only, no handle. */
int arctic_point_shadow_matrices(const ArcticPointShadowLight *light, float *out96);

/* replaces bool Renderer::create_hdri(float*,w,h) (renderer.hpp:118, renderer.cpp:555-583): RGBA32F equirect
 * environment map.  Pixels without geometry then take it along their view ray (skybox.hlsl:61-90);
 * without a map they are black. */
int arctic_create_hdri(ArcticRenderer *r, const float *rgba32f, uint32_t w, uint32_t h);

/* ---- frames -------------------------------------------------------------- */

/* replaces bool Renderer::render_frame(const Scene&, const Settings&, build_ui)
 * (renderer.hpp:106-107, renderer.cpp:274-415) minus ImGui/present:
 * shadow-map raster -> visibility/G-buffer prepass -> shading + skybox fill
 * (+fused tonemap) -> RGBA8.  out_rgba8 is a HOST buffer of (row_end-row_begin)*width*4 bytes,
 * row-major, top-left origin; NULL = leave the frame on the device. */
int arctic_render_frame(ArcticRenderer *r, const ArcticScene *scene,
                        const ArcticSettings *settings, uint8_t *out_rgba8);

/* same, but the RGBA8 shard is written to DEVICE memory the caller owns
 * (e.g. a torch tensor that RCCL then gathers); stream-ordered on the
 * handle's stream, call arctic_flush() before another stream reads it. */
int arctic_render_frame_device(ArcticRenderer *r, const ArcticScene *scene,
                               const ArcticSettings *settings, void *d_out_rgba8);

/* ---- the passes one by one (bench + parity tests) ------------------------ */

/* ShadowMapPass::run (shadow_map_pass.cpp:113-169, depth.hlsl): light-view
 * depth-only raster, front faces culled, into the handle's shadow map. */
int arctic_pass_shadow_map(ArcticRenderer *r, const ArcticScene *scene);

/* every face of every shadow-casting point light, drawn now (arctic_update_point_shadow_lights) */
int arctic_pass_point_shadows(ArcticRenderer *r, const ArcticScene *scene);

/* ForwardPass::run's vertex + raster work (forward_pass.cpp:161-226,
 * forward.hlsl:50-66): visibility + G-buffer (the interpolated VSOut). */
int arctic_pass_gbuffer(ArcticRenderer *r, const ArcticScene *scene);

/* ps_main (forward.hlsl:208-235) + post_process main (post_process.hlsl:59-93)
 * over the resident G-buffer.  d_out_rgba8 may be NULL (handle's own buffer). */
int arctic_pass_shade(ArcticRenderer *r, const ArcticScene *scene,
                      const ArcticSettings *settings, void *d_out_rgba8);

/* PostProcessPass::run alone (post_process_pass.cpp:73-95): tonemap + gamma of
 * a float RGBA HDR image (host, w*h*4 floats) to RGBA8 (host). */
int arctic_post_process(ArcticRenderer *r, const float *hdr_rgba32f, uint32_t w, uint32_t h,
                        const ArcticSettings *settings, uint8_t *out_rgba8, float *out_ldr_rgb);

/* time `iters` back-to-back arctic_pass_shade launches with HIP events on the
 * handle's stream (after `warmup` untimed ones); ms_each gets iters floats. */
int arctic_time_shade(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings,
                      uint32_t warmup, uint32_t iters, float *ms_each);

/* ---- read-back / injection for tests ------------------------------------- */

/* G-buffer of this shard, de-tiled to row-major: attrs = rows*width*18 floats
 * in VSOut order (uv2, tbn9 = t,b,n, world3, light_space4; forward.hlsl:41-48),
 * material = rows*width uint32 (0xFFFFFFFF = no geometry), depth = rows*width
 * floats (1.0 = clear), tri = rows*width uint32 draw-order id.  Any may be NULL. */
int arctic_read_gbuffer(ArcticRenderer *r, float *attrs, uint32_t *material, float *depth, uint32_t *tri);

/* inject a G-buffer (same row-major layout) instead of rasterising one */
int arctic_write_gbuffer(ArcticRenderer *r, const float *attrs, const uint32_t *material);

/* shadow map: shadow_size^2 floats, row-major */
int arctic_read_shadow_map(ArcticRenderer *r, float *depth);
int arctic_write_shadow_map(ArcticRenderer *r, const float *depth);

/* the faces of shadow-casting point light `light`: 6 x F x F floats in face order (+X, -X, +Y, -Y, +Z, -Z), each row-major.
 * ARCTIC_E_INVALID for an index beyond the list.  A write makes the next arctic_render_frame redraw them, as arctic_write_shadow_map does. */
int arctic_read_point_shadow(ArcticRenderer *r, uint32_t light, float *faces);
int arctic_write_point_shadow(ArcticRenderer *r, uint32_t light, const float *faces);

/* outputs of the last shade: float LDR (rows*width*3, after tonemap+gamma,
 * before the UNORM8 quantisation), float HDR (rows*width*3, ps_main's colour),
 * RGBA8 (rows*width*4).  Any may be NULL. */
int arctic_read_output(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8);

/* the per-frame constants the host builds (forward_pass.cpp:166-177 via
 * scene.cpp:41-70): proj_view[16], light_proj_view[16], sun_dir[3] */
int arctic_frame_constants(const ArcticScene *scene, float *proj_view, float *light_proj_view, float *sun_dir);

/* counters of the last frame: [0] setup triangles (forward), [1] raster work
 * items (forward), [2] setup triangles (shadow), [3] raster work items
 * (shadow), [4] with ARCTIC_OPT_COUNT_LIGHT_EVALS: (lit tile, light pair)
 * trips of the packed light loop that ran in a run which leaves out a colour
 * channel (ARCTIC_OPT_LIGHT_PAIR_RUNS; 0 with the scalar loop or the option at
 * 0); with ARCTIC_OPT_COUNT_LIGHT_EVALS: [5] point-light
 * evaluations summed over lit pixels, [6] lit pixels (1 - shadow != 0),
 * [7] evaluations with n.wi > 0 (the others contribute exactly 0,
 * forward.hlsl:191-192), [8] (tile, light) pairs whose n.wi <= 0 in every lit
 * pixel of the 8x8 tile (what a per-tile light list could skip), [9] tiles
 * with a lit pixel; [10], [11] work items of the forward / shadow pass that
 * went through the atomicMin rasteriser (all of them with
 * ARCTIC_OPT_RASTER_OWNER = 0; with block ownership those that found their
 * block's bin full or whose record takes the integer path); with
 * ARCTIC_OPT_COUNT_LIGHT_EVALS also [12] tiles of the fast path with a pixel
 * the shadow map's min/max table left undecided, [13] such pixels, [14] tiles
 * that ran the 25 PCF compares, [15] pixels that did.  n <= 16. */
int arctic_stats(ArcticRenderer *r, uint64_t *out, uint32_t n);

/* tuning / debug switches. */
#define ARCTIC_OPT_KEEP_FLOAT_OUTPUT 1 /* 1 = shade also stores float LDR+HDR planes (tests); 0 = RGBA8 only (bench) */
#define ARCTIC_OPT_COUNT_LIGHT_EVALS 2 /* 1 = the shading pass runs its counting variant: stats[5..9] (a few atomics per lit tile; slower) */
#define ARCTIC_OPT_CULLING           3 /* 0 = run the light loop for every covered pixel; 1 (default) = exact culling: fully shadowed pixels skip it
                                          (every term of ps_main carries 1 - shadow, forward.hlsl:222,230) */
#define ARCTIC_OPT_DEBUG             4 /* timing experiments only: bit 0 skip material textures, bit 1 skip shadow test, bit 2 skip tonemap (wrong images);
                                          bit 3 shadow test without the min/max table (same image); bit 4 ignored (it selected an LDS variant of the
                                          25-tap PCF path, measured slower and removed; the image is the same);
                                          bit 5 every triangle through the 64-bit integer rasteriser instead of the binary64 planes (same image: the path
                                          of triangles with snapped coordinates of 2^24 and more); bit 6 whole frames gather records and vertices through 64-bit
                                          pointers (the path of tables of 4 GiB and more) instead of 32-bit offsets (same image); bit 7 arctic_render_frame draws the
                                          shadow map on the main stream before the visibility prepass instead of beside it on a second stream (same image);
                                          bit 8 every tile through the general tile code, none through the fast tile (same image; A/B and tests);
                                          bit 9 the bins of the block owners count every work item offered, full or not (arctic_read_bin_counts as a histogram; same image);
                                          bit 10 the prepasses count the workgroups ARCTIC_OPT_CLUSTER_CULL skipped (arctic_read_cull_counts; same image) */
#define ARCTIC_OPT_HDR16             6 /* 1 = round ps_main's colour through binary16 before post_process, like the reference's
                                        R16G16B16A16_FLOAT colour target (forward_pass.cpp:149, renderer.cpp:128-144); default 0 = fp32 */
#define ARCTIC_OPT_LIGHT_PAIR_RUNS   8 /* 1 (default) = the packed loop walks its pairs in runs that leave out the sums of a colour channel both lights have as +0.0f
                                          (an exact skip; the lights are regrouped for it, so with more than two lights a frame may differ in the last bits from 0);
                                          0 = pairs in the caller's order, all sums: a parity aid.  The number is a reused one: ARCTIC_OPT_FUSED (the persistent
                                          one-kernel shading pass, measured slower and removed) had it; a client that still sets 8 to 0 gets the caller's order, which is
                                          always a correct image (numbers above 27 are not taken so that the option count stays what the ABI tests pin) */
#define ARCTIC_OPT_SHADOW_CACHE      9 /* 1 (default) = arctic_render_frame redraws the shadow map only when the sun, the objects or the mesh list changed
                                          (byte-compared); 0 = every frame like the reference (renderer.cpp:300-337).  Same image either way. */
#define ARCTIC_OPT_FRAMES_IN_FLIGHT  15 /* 2 = arctic_render_frame runs the visibility prepass of a frame on a second stream, into a second set of
                                          tables (and, when the shadow map is redrawn, into a second map), beside the shading of the frame before it; 3 (what the
                                          reference keeps, rhi.hpp:25) = three sets, consecutive prepasses on two streams, so that two prepasses overlap as well -- for
                                          small targets, whose prepass is the longer chain; 0 (default) = the library's choice: 3 below 3 Mpx, 2 above; every call
                                          still enqueues one whole frame and the output is complete after arctic_flush / in stream order on the main
                                          stream.  1 = one frame at a time on one stream.  Same images. */
#define ARCTIC_OPT_VISBUFFER        10 /* 1 (default) = arctic_render_frame shades straight from the visibility plane, no 76 B/px G-buffer round trip
                                          (bit-identical image; the G-buffer is materialised later if arctic_read_gbuffer / arctic_pass_shade ask); 0 = via the G-buffer */
#define ARCTIC_OPT_ITEM_TABLE_FLOOR 11 /* smallest size (entries) of the rasteriser's work-item table, default 4 Mi; the table grows to 4x the largest
                                          count seen.  A frame that overflows it returns ARCTIC_E_CAPACITY from the next synchronising call. */
#define ARCTIC_OPT_LIGHT_PATH       12 /* the light loop of the shading kernel: 0 = automatic (default: scalar up to 12 point lights, packed pairs above -- the
                                          measured crossover; the reference's MAX_NUM_POINT_LIGHTS is 16), 1 = scalar fp32, 2 = two lights at a time in packed
                                          fp32; both read the lights through the scalar cache.  Same formulas (images agree to fp32 rounding, ~1e-7). */
#define ARCTIC_OPT_TILES_PER_WAVE    16 /* tiles a wave of the shading pass (arctic_pass_shade) shades one after the other, 1 / n-th of the frame's height apart:
                                         lit (ALU-bound) and shadowed (latency-bound) regions are spatially clustered, and a wave that visits n distant parts of the
                                         frame carries a mix of both, so that every SIMD holds both kinds all the time, wherever in the frame the light falls
                                         (and a wave is launched once for n tiles).  0 (default) = the library's choice: 2, and 1 for targets below ~3 Mpx, where a frame is
                                         only a few rounds of the chip's wave slots.  Placement only: same image */
#define ARCTIC_OPT_TILE_TRACE        17 /* 1 = the shading pass records per 8x8 tile when its wave started and ended and where it ran (a measuring aid, default 0:
                                         the kernels then pay one wave-uniform branch at either end of a tile); read with arctic_read_tile_trace */
#define ARCTIC_OPT_RASTER_OWNER      18 /* -1 (default) = the library's choice: the forward prepass of a handle that owns 4 Mpx of the frame or more; otherwise
                                         bit 0: the forward prepass, bit 1: the shadow pass -- the rasteriser gives every 16x16 block of
                                         its target ONE owner wave: work items are handed to per-block bins, the owner merges its bin in registers and writes the
                                         block once (no clear, no early depth read, no per-pixel atomic); items that find their bin full, and records too large
                                         for the exact binary64 planes, go through the merging atomicMin rasteriser afterwards.  Bit clear = atomicMin rasteriser
                                         only (round 2; the shadow pass is instruction bound, not atomic bound: measured slower with owners).  Same visibility /
                                         shadow map, bit for bit (D3D12's fixed-function raster of forward_pass.cpp:137-151,212-224 / shadow_map_pass.cpp:96-97,157-167) */
#define ARCTIC_OPT_TILE_ORDER        19 /* 1 = arctic_pass_gbuffer leaves, next to the G-buffer, a cost class per 8x8 tile (can a pixel of it be lit at all,
                                          by the shadow map's min/max table -- the shading kernel's own first test) and from the classes the ORDER in which
                                          arctic_pass_shade hands out its work: lit tiles dealt evenly over the dispatch, shadowed ones in between, the end of
                                          the list shadowed ones only.  A hint: images never depend on it.  0 (default since round 5) = the geometric, XCD-aware
                                          order (takes effect at the next G-buffer pass; a G-buffer written by arctic_write_gbuffer has no order).  Off by default
                                          because it is a net loss as built: the order kernel is ONE workgroup (112 us per G-buffer pass at 4K) for <= 2 us of
                                          the shading pass, and strips dealt by cost no longer share an XCD's L2 with their neighbours (+83 MB of fabric reads
                                          per 4K pass: profiles/r5_a_traffic_tile_order.json) */
#define ARCTIC_OPT_ORDER_TAIL        20 /* per mille of the dispatch order, at its end, that holds cheap tiles only (default 60) */
#define ARCTIC_OPT_SAMPLER           21 /* which arithmetic stands in for the reference's D3D12 sampler (MIN_MAG_MIP_LINEAR + WRAP, forward_pass.cpp:38-51; the
                                          shadow map goes through the same sampler, forward.hlsl:84-92).  0 (default) = texel coordinates and bilinear weights in
                                          full fp32.  Bit 0: material textures with the scaled coordinate u W - 0.5 snapped to 1/256 texel (round to nearest)
                                          before it is split into texel index and weight -- 8-bit filter weights, what the D3D11.3 functional specification
                                          (3.2.4.1, 7.18.8) lets a sampler do and hardware does.  Bit 2: the same for the 25 PCF taps.  Same bits as the oracle's
                                          oracle_set_sampler_mode (its bit 1, sRGB decode after filtering, is an oracle-only bound: D3D10+ decodes first).
                                          A DX12 host comparing against captures of the real reference should pick 5; INTEGRATION.md section 7 */
#define ARCTIC_OPT_TEXTURE_TILING    22 /* how arctic_create_material stores the packed image of a material from now on: -1 (default) = the library's choice, tiles of
                                          4 x 4 texels (one 128-byte line each) for images of 2048 texels a side and more, row-major below; 0 = row-major; 1 = tiles.
                                          The reference creates one mip level (rhi.cpp:550), so large textures are minified at mip 0 and every pixel's footprint is its
                                          own cache lines: 2 in a row-major image, 1.56 on average in tiles.  A layout only: same texels, same image */
#define ARCTIC_OPT_CLUSTER_CULL      23 /* the prepasses skip whole workgroups of triangles / vertices whose object-space box (made per mesh by arctic_create_mesh) lies
                                          beyond a side of the pass's scissor rectangle, the near or the far plane -- the shard's rows for a row-range shard, the
                                          rank's slice of a sharded shadow map: 3 (default) = k_setup skips clusters of 256 triangles and k_vertex blocks of 256
                                          vertices all of whose triangles are skipped, 1 = k_setup only, 0 = off.  Conservative (geometry.hip: box_outside): same
                                          visibility plane, shadow map and counts, bit for bit.  No counterpart in the reference, which leaves culling to the
                                          hardware's clipper (forward_pass.cpp:212-224 draws every object) */
#define ARCTIC_OPT_SMALL_TRIANGLES   24 /* 1 (default) = the shadow pass draws triangles whose bounding box holds at most 64 pixels in its set-up kernel: the lanes
                                          that set a wave's triangles up share out the pixels of their boxes, the edge functions as 32-bit integers relative to the
                                          box, one atomicMin per covered pixel -- such a triangle (two thirds of what an orthographic sun sees of a tessellated
                                          scene) never becomes a record or a 16x16 work item.  0 = every triangle through the work-item rasteriser.  Same map, bit
                                          for bit (the hardware rasteriser of shadow_map_pass.cpp:96-97,157-167 / depth.hlsl:7-10 does not care either).
                                          Where the shadow pass runs with block owners (ARCTIC_OPT_RASTER_OWNER bit 1) the owners merge their bins into the map
                                          this path has drawn into, and blocks with an empty bin have no owner (measured: no faster than the atomic rasteriser) */
#define ARCTIC_OPT_MARKERS          13 /* 1 = roctx ranges around each pass, named like the reference's Tracy zones (process-wide; libroctx64 is loaded on demand) */
/* ARCTIC_OPT_ENV_LIGHTING: image-based ambient light from the environment map of arctic_create_hdri (the reference's roadmap item
 * "IBL with skybox"; forward.hlsl:13,195-206 has the hooks, ps_main :233 still ends in a flat ambient).
 *   0 (default)  ambient * base_color, as the reference renders.
 *   1            that term, and only that term, becomes
 *                  color = Lo (1 - shadow) + ambient [ (1 - F)(1 - metal) base E(n) / pi + P(R, rough) (F0 A + B) ]
 *                  F  = F0 + (max(1 - rough, F0) - F0)(1 - max(n.wo, 0))^5   (Schlick with roughness, per channel)
 *                  F0 = lerp(0.04, base, metal),  R = 2 (n.wo) n - wo,  (A, B) = LUT(max(n.wo, 0), rough)
 *                n, wo, base, metal, rough: exactly what the light loop takes (get_normal, metal-rough .g / .b, sRGB decode, every
 *                ARCTIC_OPT_SAMPLER mode); ambient (the scene's slider, app.cpp:470) scales the whole bracket.  Shadowed pixels take it too.
 *                Without an environment map mode 1 renders bit for bit as mode 0, so a host may set it unconditionally.
 * Direction <-> texel: the skybox's mapping (skybox.hlsl:74-85) with its fp32 constants 0.1591f / 0.3183f and its v flip, so that a mirror
 * reflects exactly the sky the skybox draws (the unused forward.hlsl:197 variant lacks the flip).  Texel (i, j) of a W x H map:
 * u = (i + 0.5) / W, v = (j + 0.5) / H, phi = (u - 0.5) / 0.1591f, theta = (0.5 - v) / 0.3183f, direction (cos theta cos phi, sin theta,
 * cos theta sin phi), solid angle max(cos theta, 0) dphi dtheta with dphi = 1 / (0.1591f W), dtheta = 1 / (0.3183f H).  Because the
 * constants are rounded the weights sum to 4 pi (1 + 3.5e-4), not 4 pi, and the azimuths overlap by as much at the seam (phi = +-pi, the -x
 * direction), which is weighed twice: kept, so a constant map c gives E = pi c (1 + 3.5e-4) on average and pi c (1 + 1.1e-3) towards -x.
 * Tables, built on the device in stream order on the handle's stream when both the map and mode 1 exist -- by arctic_create_hdri or by
 * arctic_set_option, whichever comes second; never by a frame.  A new map rebuilds them; arctic_resize keeps them:
 *   E(n)        9 real SH coefficients per channel (basis order 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2 with the usual normalisations),
 *               projected over the full-resolution map, Ramamoorthi-Hanrahan's A0 = pi, A1 = 2 pi / 3, A2 = pi / 4 folded in.  Summed in
 *               binary64 in a fixed order (no float atomics): the same map gives the same bits on every handle.
 *   P(R, r)     6 levels, r_k = k / 5.  Level 0 is the map (bilinear, WRAP, as the skybox samples it); level k >= 1 is an RGBA32F equirect of
 *               max(8, min(W, 512) >> (k - 1)) x max(4, min(H, 256) >> (k - 1)) texels (~2.7 MB for the stack): Karis' split-sum prefilter
 *               (N = V = R), 512 Hammersley samples, GGX with alpha = r_k^2, weight n.l, taken from the 2x2 box-filtered mip chain of the map
 *               (level m + 1 = max(1, w / 2) x max(1, h / 2), texel = mean of (2i + a, 2j + b), clamped to the last row / column) at
 *               lod = max(0, log2(Omega_s / Omega_p) / 2 + 1), Omega_s = 4 / (512 D), Omega_p = 4 pi / (W H), linear between mip levels.
 *               GGX frame around n: tangent = normalize(cross(up, n)), up = z unless |n.z| >= 0.999, then x.  At run time P is trilinear:
 *               levels floor(5 r) and floor(5 r) + 1 (the last one clamped), each bilinear with WRAP.  R and its texel coordinates are
 *               binary64 from the pixel's attributes (tangent frame, normal texel, eye - world), the filter weights and the blend fp32.
 *   (A, B)      64 x 64 RG fp32 at cell centres (n.v, r), 1024 Hammersley samples, Smith-Schlick with k = r^2 / 2 (the IBL form; the direct
 *               lights keep (r + 1)^2 / 8, on purpose); looked up bilinearly, clamped.
 * ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE do not apply in mode 1 (a shading call then returns ARCTIC_E_STATE), and
 * ARCTIC_OPT_TILE_ORDER is ignored (the geometric order).  INTEGRATION.md section 5e: what a DX12 host sets. */
#define ARCTIC_OPT_ENV_LIGHTING     25
#define ARCTIC_OPT_POINT_SHADOW_SIZE 26 /* F, the side of each cube face of the shadow-casting point lights: a multiple of 8 in [8, 4096] (default 1024),
                                          otherwise ARCTIC_E_INVALID.  A change clears the faces to 1.0 and makes the next arctic_render_frame draw them. */
/* ARCTIC_OPT_TEXTURE_MIPS: mip-mapped material textures with trilinear filtering (the reference creates one level, rhi.cpp:550, and samples
 * it with MIN_MAG_MIP_LINEAR: a minified texture aliases, and every pixel's footprint is its own cache lines).
 *   0 (default)  one level per material, sampled at level 0: as the reference renders, bit for bit, at the same speed.
 *   1            at the time of arctic_create_material ("from now on", like ARCTIC_OPT_TEXTURE_TILING): a material whose three images have
 *                equal size gets a full chain, built on the device, synchronously.  Materials with images of unequal sizes, and materials
 *                created under 0, keep one level and are sampled at level 0 in every mode.
 *                At shading time, once a material of the handle has a chain: trilinear filtering as below.  With no chain on the handle
 *                mode 1 shades with the kernels of mode 0.
 * The chain.  levels = 1 + floor(log2(max(w, h))); level k has w_k = max(1, w >> k), h_k = max(1, h >> k).  Texel (x, y) of level k + 1 is made
 * from the four texels of level k in columns min(2x, w_k - 1), min(2x + 1, w_k - 1) and rows min(2y, h_k - 1), min(2y + 1, h_k - 1): an odd
 * side drops its last row / column (it is never read: 2x + 1 <= 2 (w_k >> 1) - 1 < w_k - 1), and a side of 1 repeats its only texel.
 *   normal .rgb, metal-rough .gb (UNORM8):  (a + b + c + d + 2) >> 2.
 *   diffuse .rgb (sRGB8):  m = the mean of the four DECODED values, decoded with the 256-entry fp32 table the kernels use (code c ->
 *     x = c / 255.0f; x <= 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f)), taken in binary64, where the sum of four such values
 *     is exact.  The stored code is the one whose table value is nearest to m, the lower code on a tie (m against the binary64 midpoints
 *     of neighbouring table entries: exact again).  Four equal codes give that code back; no pow on the way.
 *   Level 0 is the image as uploaded (row-major or 4 x 4-texel tiles, ARCTIC_OPT_TEXTURE_TILING); levels 1.. are row-major.  A layout only.
 *   The chain lives in one allocation of less than 2^32 bytes (8 bytes per texel, a one-texel border per level); a material whose chain
 *   does not fit fails with ARCTIC_E_CAPACITY and leaves the handle as it was.
 * The level of detail, per covered pixel (px, py) of a material with a chain: uv00 = the texture coordinates interpolated for the pixel;
 * uv10, uv01 = the SAME triangle's perspective-correct interpolation evaluated at (px + 1, py) and (px, py + 1), extrapolated past the
 * triangle's edge where the neighbour is outside it (what a GPU's helper lanes do; never a difference between two triangles).
 *   rho^2 = max((w du_x)^2 + (h dv_x)^2, (w du_y)^2 + (h dv_y)^2),  du_x = u10 - u00 and so on, w, h the level-0 size;
 *   lambda = 0.5 log2(rho^2) clamped to [0, levels - 1], a NaN giving 0.  Pixels without geometry and pixels of materials with one level: 0.
 * arctic_pass_gbuffer leaves lambda in one more plane next to the G-buffer (arctic_read_lod / arctic_write_lod), arctic_render_frame computes
 * it in the shading kernel with the same operations: the two paths agree bit for bit, as they do in mode 0.
 * Sampling: l0 = floor(lambda), f = lambda - l0, l1 = min(l0 + 1, levels - 1).  Each of the two levels is sampled by the bilinear rule of
 * mode 0 with that level's size (texel centres at +0.5, WRAP, sRGB decoded per texel before filtering, ARCTIC_OPT_SAMPLER bit 0 applying to
 * the bilinear weights); the eight filtered channels (base colour rgb, normal rgb, roughness, metalness) blend as a + (b - a) f in fp32 with
 * the full-precision f in every sampler mode; ps_main continues unchanged.  f == 0 returns level l0's bits: a plane of zeroes renders the
 * bits of mode 0.
 * Composes with ARCTIC_OPT_ENV_LIGHTING, spot lights and shadow-casting point lights.  ARCTIC_OPT_COUNT_LIGHT_EVALS and ARCTIC_OPT_TILE_TRACE
 * do not apply while mode 1 shades with a chain (a shading call then returns ARCTIC_E_STATE), ARCTIC_OPT_TILE_ORDER is ignored (the geometric
 * order).  Not provided: anisotropic filtering, a LOD bias, chains for the environment map, the shadow maps or materials with images of
 * unequal sizes, a chain supplied by the caller.  INTEGRATION.md section 5h: what a DX12 host sets. */
#define ARCTIC_OPT_TEXTURE_MIPS     27
/* ARCTIC_OPT_ANTIALIAS: an edge anti-aliasing pass on the finished RGBA8 image (no counterpart in the reference, which left its staircases to the
 * swap chain and the display's scaling).  The renderer takes one sample per pixel; this filter is FXAA's structure -- the 3 x 3 orientation
 * test, a search along the edge with a quarter-gradient stop, the offset 1/2 - d / span and the 0.75 smoothstep^2 sub-pixel term -- restated
 * in integers, with whole-pixel steps and fixed-point quantities, so that it is DEFINED bit for bit (tests/antialias_reference.py).
 *   0 (default)  no pass: the image is what it was, byte for byte, at the same speed.
 *   1            a handle that owns the whole frame applies the filter below to the RGBA8 image of every arctic_pass_shade,
 *                arctic_render_frame and arctic_render_frame_device: the shading kernels then always write the handle's own RGBA8 buffer and
 *                the filter writes the destination -- the caller's d_out, or a second buffer of the handle, which arctic_render_frame,
 *                arctic_read_output and arctic_gather_frame (d_shard = NULL) then read for rgba8.  The float LDR / HDR planes of
 *                ARCTIC_OPT_KEEP_FLOAT_OUTPUT stay what shading wrote: they are NOT filtered.  arctic_time_shade stays the shading kernel alone.
 *   any other value: ARCTIC_E_INVALID.
 * Sharded handles.  A handle that owns only part of the frame (a row range, or interleaved bands of more than one shard) accepts the option and
 * does NOT apply it: its shard lacks the neighbouring rows.  The root filters the assembled frame with arctic_antialias_device.
 * The number 5 is the lowest unused one (ARCTIC_OPT_BANDS of the early two-kernel shading pass had it and left with that pass; no library
 * since has known it); 27 stays the highest.
 *
 * The filter.  Input: a W x H RGBA8 image C, row-major.  Addressing: every read at a coordinate outside the image is clamped per axis to
 * [0, W - 1] x [0, H - 1].  Arithmetic: all integers; nothing below needs more than 32 bits unsigned, or signed for the differences.
 * Luma: Y(p) = 77 R + 150 G + 29 B, range 0 .. 65280.  Fixed constants: K = 12, T_MIN = 4096.
 * For each pixel p = (x, y), with N = (x, y - 1), S = (x, y + 1), W = (x - 1, y), E = (x + 1, y) and M = p:
 *   1. Early exit.  hi / lo are the max / min of Y over {M, N, S, W, E}, and rng = hi - lo.  If rng < max(T_MIN, hi >> 3) the output pixel is
 *      the input pixel; the rest is skipped.
 *   2. Orientation, with the corner lumas NW, NE, SW, SE:
 *        eh = |NW + SW - 2 W| + 2 |N + S - 2 M| + |NE + SE - 2 E|
 *        ev = |NW + NE - 2 N| + 2 |W + E - 2 M| + |SW + SE - 2 S|
 *      The edge is horizontal iff eh >= ev.
 *   3. Side.  (a, b) = (N, S) if horizontal, else (W, E).  ga = |Y(a) - Y(M)|, gb = |Y(b) - Y(M)|, g = max(ga, gb).  The side is a (step -1
 *      along the normal axis) iff ga >= gb, else b (step +1).  n is that unit step, Ls the side pixel's luma, avg2 = Y(M) + Ls, and t the
 *      unit step along the edge: (1, 0) if horizontal, else (0, 1).
 *   4. Search, once per direction s in {-1, +1}.  For i = 1 .. K: q = clamp(p + s i t), e = Y(q) + Y(clamp(q + n)) - avg2.  The first i with
 *      2 |e| >= g ends the search: d_s = i, e_s = e.  If none ends it, d_s = K and e_s is the e of i = K.
 *   5. Edge offset.  span = d- + d+, d = min(d-, d+), e_end = e- if d- < d+, else e+.  good = (e_end < 0) != (Y(M) < Ls).
 *      off_e = good ? floor(128 (span - 2 d) / span) : 0.
 *   6. Sub-pixel offset.  A = |2 (N + S + E + W) + NW + NE + SW + SE - 12 M| (lumas).  s1 = min(256, floor(256 A / (12 rng))),
 *      s2 = (s1 s1 (768 - 2 s1)) >> 16,  off_s = (s2 s2 3) >> 10.
 *   7. Blend.  off = max(off_e, off_s), at most 192.  Cn = C(clamp(p + n)).  For each of R, G, B: out = (C (256 - off) + Cn off + 128) >> 8.
 *      Alpha is copied from the input pixel.
 * Not provided: filtering in front of the tonemapper, other thresholds or search lengths (one preset), a halo exchange between shards,
 * temporal or multi-sample methods.  INTEGRATION.md section 5j: which buffer holds what, and the sharded case. */
#define ARCTIC_OPT_ANTIALIAS         5
int arctic_set_option(ArcticRenderer *r, uint32_t option, int64_t value);

/* The filter of ARCTIC_OPT_ANTIALIAS on any RGBA8 device image of width x height pixels (row-major, tightly packed, 4-byte aligned), whatever
 * the handle's own size and options: d_in -> d_out, asynchronous on the handle's stream (arctic_flush before another stream reads d_out).
 * This is what the root of a sharded frame calls on the assembled image.  ARCTIC_E_INVALID: a null pointer, a zero size, a pointer that is
 * not 4-byte aligned, or d_in / d_out ranges that overlap (a pixel reads its neighbours: the filter cannot run in place). */
int arctic_antialias_device(ArcticRenderer *r, const void *d_in, void *d_out, uint32_t width, uint32_t height);

/* The same, host to host and synchronous: rgba8 and out are width x height x 4 bytes (they may be the same host buffer); staged through the
 * handle's staging buffer like arctic_post_process. */
int arctic_antialias(ArcticRenderer *r, const uint8_t *rgba8, uint32_t width, uint32_t height, uint8_t *out);

/* Level `level` of a material's chain (ARCTIC_OPT_TEXTURE_MIPS; level 0 = the images as uploaded), for tests: dims = {w, h} of the level,
   texels = w x h x 8 bytes, row-major, no border, per texel {diffuse r, g, b, normal r, g, b, metal-rough g, b}.  texels may be NULL (the size
   alone).  ARCTIC_E_INVALID for a material that does not exist or has images of unequal sizes, and for a level beyond the material's
   (a material without a chain has one).  Synchronises. */
int arctic_read_material_mip(ArcticRenderer *r, uint32_t material, uint32_t level, uint8_t *texels, uint32_t dims[2]);

/* The level-of-detail plane of the G-buffer in place (ARCTIC_OPT_TEXTURE_MIPS = 1): one float per pixel, row-major over the handle's rows
   like arctic_read_gbuffer.  arctic_write_gbuffer resets the plane to 0 (an injected G-buffer has no triangles); arctic_write_lod after it
   injects one (values outside [0, levels - 1] are clamped when they are used, a NaN counts as 0).  ARCTIC_E_STATE with the option off, and
   without a G-buffer.  Both synchronise. */
int arctic_read_lod(ArcticRenderer *r, float *lod);
int arctic_write_lod(ArcticRenderer *r, const float *lod);

/* The tables of ARCTIC_OPT_ENV_LIGHTING (no counterpart in the reference): sh27 = the 27 coefficients of E(n), coefficient k of channel c
   at 3 k + c (A_l folded in); lut = 64 x 64 x 2 floats, row = roughness cell; texels = specular level `level` (0 = the map), w x h x 4
   floats; dims = {w, h of that level, levels (6), LUT side (64)}.  Any pointer may be NULL.  ARCTIC_E_STATE when no tables exist.
   Synchronises. */
int arctic_read_env_lighting(ArcticRenderer *r, float *sh27, float *lut, uint32_t level, float *texels, uint32_t *dims);

/* The trace of the latest shading pass under ARCTIC_OPT_TILE_TRACE: 4 x uint64 per tile, tile-row major over the handle's tile
   grid (tiles_x x tiles_y, returned too): the 100 MHz reference clock (s_memrealtime) when the tile's wave started, when it ended,
   HW_ID | XCC_ID << 32 (XCD / SE / CU / SIMD / wave slot it ran on), and 1 = shaded by the fast tile code | shader-clock ticks between
   start and end << 8.  out == NULL only reports the grid.  Synchronises.  No counterpart in
   the reference (its GPU timing is Tracy zones per pass, renderer.cpp:285-357); tools/experiments/tile_trace.py reads it. */
int arctic_read_tile_trace(ArcticRenderer *r, uint64_t *out, uint64_t capacity_tiles, uint32_t *tiles_x, uint32_t *tiles_y);

/* The dispatch order arctic_pass_gbuffer left for arctic_pass_shade (ARCTIC_OPT_TILE_ORDER) and the cost classes it was built from:
   order = ceil(tiles_x / 4) * tiles_y entries, one per strip of 4 horizontally adjacent tiles, ty << 16 | strip column, in the order
   the shading pass hands them out; tile_class = one byte per tile, row-major over the handle's tile grid, 1 = a pixel of the tile
   can be lit (or takes the environment lookup).  Either pointer may be NULL; both NULL only reports the grid; capacity_tiles >=
   tiles_x * tiles_y.  Synchronises.  A hint for the pass's scheduling, never part of a result; no counterpart in the reference
   (its pixel shader is scheduled by the GPU's fixed function, forward_pass.cpp:212-224). */
int arctic_read_tile_order(ArcticRenderer *r, uint32_t *order, uint8_t *tile_class, uint64_t capacity_tiles, uint32_t *tiles_x, uint32_t *tiles_y);

/* Work items per 16x16 block of the latest forward (shadow_pass = 0) or shadow (1) prepass drawn with block owners
   (ARCTIC_OPT_RASTER_OWNER): blocks_x x blocks_y counters, row-major over the whole target; a block's owner drew the first 32, the
   atomicMin rasteriser the rest.  out == NULL only reports the grid.  Synchronises.  A measuring aid (load balance of the owner
   waves, choice of the bin size); no counterpart in the reference, whose rasteriser is the GPU's fixed function
   (forward_pass.cpp:212-224). */
int arctic_read_bin_counts(ArcticRenderer *r, int shadow_pass, uint32_t *out, uint64_t capacity_blocks, uint32_t *blocks_x, uint32_t *blocks_y);

/* What ARCTIC_OPT_CLUSTER_CULL skipped in the latest forward (shadow_pass = 0) or shadow (1) prepass that ran under ARCTIC_OPT_DEBUG bit 10:
   out[0] = clusters of 256 triangles in the scene, out[1] = of them skipped by k_setup, out[2] = blocks of 256 vertices, out[3] = of them skipped by
   k_vertex.  Synchronises.  A measuring aid; no counterpart in the reference (forward_pass.cpp:212-224 draws every object). */
int arctic_read_cull_counts(ArcticRenderer *r, int shadow_pass, uint32_t *out);

/* ---- ray queries (no counterpart in the reference: its roadmap's "Raytracing") ------------------------------------------------------------------
 * What does this ray hit?  The handle keeps an acceleration structure over the scene's triangles in world space, built on the host and walked on
 * the device by ordinary vector code (trace.hip; the MI355X has no ray accelerator).  The answer is DEFINED bit for bit: a walk that prunes gives
 * exactly what a loop over every triangle gives, numpy in float32 reproduces it (tests/ray_reference.py), and so does arctic_trace_triangles on
 * the host.  Nothing in the passes uses it (yet): shading, shadow maps and every existing bit are unchanged.
 *
 * THE DEFINITION.  Everything is fp32; each operation rounds once, in the written order, without contraction; division is IEEE division.
 *   min(a, b) = b < a ? b : a      max(a, b) = a < b ? b : a        (of two equal operands, zeros of either sign included, the first)
 *   cross(a, b)[0] = a[1]*b[2] - a[2]*b[1], cyclically: two rounded products, then the rounded difference
 *   dot(a, b)      = (a[0]*b[0] + a[1]*b[1]) + a[2]*b[2]
 * Scene triangles.  The objects in ArcticScene::objects order, each object's triangles in index-buffer order; `prim` is the running index of the
 *   triangle over the whole scene.  An object whose mesh does not exist has no triangles (the passes skip it too).  The triangle at an index
 *   out of range is skipped as the rasteriser skips it, and still takes a prim number.  More than 2^32 - 2 triangles: ARCTIC_E_CAPACITY (and the
 *   structure stores at most 2^29 - 1 triangles that can be hit: ARCTIC_E_CAPACITY as well).  A world vertex is the vertex kernel's transform of
 *   the mesh's vertices IN USE (posed, else morphed, else its own: arctic_read_mesh_vertices) with w = 1 and M = the object's trs:
 *     p[i] = ((M[i]*x + M[4+i]*y) + M[8+i]*z) + M[12+i]*1.0f                        i = 0..2: what arctic_read_gbuffer returns as attributes 11..13
 *   A triangle with a world vertex that is not finite is never hit.
 * Ray (o, d) against a box (bmin, bmax).  Per axis a:
 *     d[a] == 0:  the axis contributes (-inf, +inf) when bmin[a] <= o[a] <= bmax[a]; otherwise the box is missed.
 *     else:       inv = 1.0f / d[a];  l = (bmin[a] - o[a]) * inv;  h = (bmax[a] - o[a]) * inv;  lo = min(l, h);  hi = max(l, h).
 *                 If l or h is a NaN the axis contributes (-inf, +inf) instead.  (That is 0 * inf: a d[a] so small that inv is infinite, and an
 *                 origin in one of the box's planes -- the inclusive rule of d[a] == 0.  No other NaN can arise from finite operands.)
 *     tn = max(max(lo[0], lo[1]), lo[2]);  tf = min(min(hi[0], hi[1]), hi[2]).  The box is met iff no axis missed it and tn <= tf.
 *   The test is MONOTONE in box inclusion (rounding is monotone, and so is a multiplication by one fixed factor): a ray that meets a box B meets
 *   every box that contains B, with tn' <= tn and tf' >= tf.  The whole design rests on this.
 * Ray against triangle (p0, p1, p2).
 *   1. The triangle's own box: bmin = min(min(p0, p1), p2), bmax = max(max(p0, p1), p2), component-wise.  (tn, tf) is its interval; a box that is
 *      not met is a miss.
 *   2. Moeller-Trumbore:  e1 = p1 - p0;  e2 = p2 - p0;  pv = cross(d, e2);  det = dot(e1, pv);  inv = 1.0f / det;  tv = o - p0;
 *      u = dot(tv, pv) * inv;  qv = cross(tv, e1);  v = dot(d, qv) * inv;  tm = dot(e2, qv) * inv.
 *      A miss unless  det != 0 && u >= 0 && u <= 1 && v >= 0 && u + v <= 1;  every comparison is false for a NaN, and a NaN tm is a miss too.
 *   3. t = min(max(tm, tn), tf): Moeller-Trumbore's parameter CLAMPED INTO THE TRIANGLE'S OWN BOX INTERVAL.  A hit iff t_min <= t && t <= t_max.
 *   Step 3 is what makes a pruned walk EXACTLY equal to the loop over every triangle, with no epsilon anywhere: a hit's t lies inside its
 *   triangle's interval, so -- by monotonicity -- inside the interval of every box that contains the triangle; a node of the structure with
 *   max(tn_node, t_min) > min(tf_node, t_max, t_best) therefore holds no hit at or below t_best.  The comparison is strict: a tie must still be found.
 *   For an axis-aligned triangle (floors, walls) the box has no thickness and t is the slab's value, which is also better conditioned at grazing
 *   angles than tm.
 * Closest hit: among all triangles that are hit the smallest t (-0 == +0), among equal t the smallest prim; reported {t, u, v, prim} of that triangle.
 * Any hit (ARCTIC_TRACE_ANY): only whether a triangle is hit at all: {0, 0, 0, 0}.
 * A miss is {t = 0, u = 0, v = 0, prim = 0xFFFFFFFF}, under either flag.  A ray whose origin or direction has a component that is not finite, or
 * whose direction is zero, is a miss, not an error; t_min and t_max are used as given (t_max = +inf: no far limit; a NaN limit admits no hit).
 * KNOWN LIMITS.  The test is two-sided (no back-face culling).  It is NOT watertight: a ray through a shared edge can slip between the two
 * triangles' rounded u and v.
 *
 * THE STRUCTURE.  A binary tree over the triangles that can be hit, at most 4 per leaf, built deterministically (median split on the widest
 * centroid axis, ties by prim), boxes the exact fp32 unions -- no padding: the paragraph on step 3 is why none is needed.  Nodes are stored in
 * depth-first order with a skip link, 32 bytes each; leaf triangles are stored by leaf, pre-transformed, 48 bytes each.  The device walk is
 * i = descend ? i + 1 : skip[i]: the index strictly increases and the loop ends at the node count -- no stack, and termination by construction.
 * The host checks every node before anything is uploaded (index < skip <= nodes, first + count <= triangles, a child's box inside its parent's).
 * The structure is cached in the handle and rebuilt -- synchronously, draining the stream in use, reading deformed meshes back -- by the next
 * query after the bytes of the objects, the mesh count, or the shape of a mesh in use changed (every successful skin, pose, morph-targets and
 * weights call counts: the rule of arctic_render_frame's shadow cache).  Each rank of a sharded frame keeps its own full copy. */
typedef struct ArcticRay { float origin[3]; float t_min; float direction[3]; float t_max; } ArcticRay;   /* 32 bytes */
typedef struct ArcticHit { float t, u, v; uint32_t prim; } ArcticHit;                                    /* 16 bytes */
#define ARCTIC_TRACE_ANY   1u   /* any hit instead of the closest */
#define ARCTIC_TRACE_BRUTE 2u   /* arctic_trace_triangles only: loop over every triangle, no structure */

/* n rays against the scene's triangles: hits[k] answers rays[k].  Host buffers, synchronous.  ARCTIC_E_INVALID: a null scene, null rays or hits
 * with n > 0, a flag other than ARCTIC_TRACE_ANY.  ARCTIC_E_CAPACITY: n above 2^32 - 1, or a scene too large (above).  n = 0 only builds. */
int arctic_trace_rays(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits);

/* The same between DEVICE buffers the caller owns (16-byte aligned), stream-ordered on the handle's stream like arctic_render_frame_device: call
 * arctic_flush() before another stream reads d_hits.  (A rebuild of the structure, when one is due, is synchronous.) */
int arctic_trace_rays_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *d_rays, uint64_t n, uint32_t flags, ArcticHit *d_hits);

/* One any-hit ray per pixel of the handle's RESIDENT G-buffer (arctic_pass_gbuffer, arctic_write_gbuffer, or the latest frame), towards the sun:
 *   o[i] = world[i] + bias * n[i]   (the product rounds, then the sum),   d = -sun_dir,   t_min = 0,   t_max = +inf
 * world and n are attributes 11..13 and 8..10 of arctic_read_gbuffer's order, sun_dir is arctic_frame_constants' sun_dir for `scene`.
 * mask = rows * width bytes, row-major over the handle's rows like arctic_read_gbuffer: 255 where the sun is visible or the pixel has no
 * geometry, 0 where a triangle is hit.  mask == NULL leaves the result on the device and does not synchronise (timing).  A sharded handle answers
 * for its own rows.  ARCTIC_E_STATE without a G-buffer; ARCTIC_E_INVALID for a null scene or a bias that is not finite. */
int arctic_trace_sun_visibility(ArcticRenderer *r, const ArcticScene *scene, float bias, uint8_t *mask);

/* The host arbiter: the same definition, the same structure and the same walk on the CPU -- or, with ARCTIC_TRACE_BRUTE, the loop over every
 * triangle.  tris9 = n_tris world-space triangles of 9 floats (p0, p1, p2); prim is the array index.  No handle, no GPU.
 * ARCTIC_E_INVALID: a null pointer with a non-zero count, an unknown flag.  ARCTIC_E_CAPACITY: n_tris above 2^32 - 2. */
int arctic_trace_triangles(const float *tris9, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits);

/* The cached structure: out4 = {triangles stored (those that can be hit), nodes, builds so far, depth (nodes on the longest path; 0: empty)}. */
int arctic_ray_scene_info(ArcticRenderer *r, uint64_t *out4);

/* ---- refit: the structure follows a scene that MOVES without being rebuilt ------------------------------------------------------------------------
 * ARCTIC_OPT_RAY_REFIT = 1 (arctic_set_option; default 0: everything above, bit for bit and call for call; any other value: ARCTIC_E_INVALID).
 * When the geometry moved and the topology stayed, the next query REFITS the cached structure on the device (ray_refit.hip) instead of building
 * a new one on the host: in stream order on the handle's stream, without synchronising, without reading anything back.  By the paragraph on step 3
 * a pruned walk equals the loop over every triangle for ANY tree whose boxes contain their triangles, so a refitted tree gives the same bits as a
 * fresh one; only the speed of the walk can degrade, as the boxes of a tree split for another pose overlap more -- arctic_ray_scene_reset is the
 * caller's remedy.
 *
 * A REFITTED STRUCTURE, defined:
 * Topology.  The node count, every skip, every leaf word, the order of the slots (the stored triangle records) and every slot's prim are those
 *   of the last full build.
 * Slot contents.  Slot k holds the world vertices of its prim, by the formula above ("A world vertex is ...": the same operations, contraction
 *   off) from the mesh's vertices in use NOW and the object's trs NOW.  If any of the nine floats is not finite the slot is DEAD: nine quiet NaNs
 *   (0x7FC00000), prim kept.  A dead slot is never hit (the ray against triangle test as written: with a d[a] == 0 its box is missed because
 *   bmin <= o is false for a NaN; with every d[a] != 0 the box is met with (-inf, +inf), but u is a NaN and u >= 0 is false).  It comes back to
 *   life at the next refit whose vertices are finite again.
 * Leaf boxes.  The union (min / max as defined above) of the boxes of the leaf's LIVE triangles; a leaf with none has the EMPTY box
 *   bmin = +inf, bmax = -inf.
 * Interior boxes.  The union of the two children's boxes; the empty box is the identity.  The node test only has to stay conservative, and on an
 *   empty box it is: (+inf - o) and (-inf - o) times a reciprocal that is never zero and never a NaN (zero direction components count as
 *   +inf) are +inf and -inf in some order, the interval (-inf, +inf) on every axis -- the node is visited, and holds dead slots only.
 * Zero signs.  min / max of finite values are exact, so a box is the same VALUE in whatever order it is formed; the sign of a zero bound is not
 *   defined.  Compare boxes by value, triangles by bytes.
 * Eligibility, decided on the host without synchronising.  The next query refits when ALL hold: the option was 1 at the last full build; that
 *   build left out no in-range triangle for being non-finite; n_objects and every object's mesh_idx equal that build's; every such mesh still
 *   exists -- and anything else the structure depends on changed (a trs, a pose, weights).  In every other case it builds in full, as above.  A
 *   structure built under option 0 is not refittable.  A refit does not count as a build in arctic_ray_scene_info. */
#define ARCTIC_OPT_RAY_REFIT 7
typedef struct ArcticRayNode { float bmin[3]; uint32_t skip; float bmax[3]; uint32_t leaf; } ArcticRayNode;                 /* 32 bytes */
typedef struct ArcticRayTri { float p0[3], p1[3], p2[3]; uint32_t prim; uint32_t pad[2]; } ArcticRayTri;                    /* 48 bytes */

/* out4 = {refits so far, 1 if the cached structure can be refitted, kernel launches of the latest refit, 0}. */
int arctic_ray_refit_info(ArcticRenderer *r, uint64_t *out4);

/* Drops the cached structure: the next query builds in full (under the option in force then).  For a refitted tree that has drifted far from
 * the pose it was split for. */
int arctic_ray_scene_reset(ArcticRenderer *r);

/* The device's nodes and leaf triangles as they stand (for tests; synchronises).  Either pointer may be NULL; counts: arctic_ray_scene_info.
 * ARCTIC_E_CAPACITY: too little room (nothing written).  ARCTIC_E_STATE: no structure. */
int arctic_read_ray_structure(ArcticRenderer *r, ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap);

/* The host arbiter of the refit (no handle, no GPU): builds on tris9_build, refits to tris9_now -- n_tris triangles each, prim = the array
 * index -- by the definition above, walks the refitted tree, and optionally returns it (nodes / tris may be NULL; counts2, if given, receives
 * {nodes, stored triangles}).  With ARCTIC_TRACE_BRUTE the hits come from the loop over every triangle of tris9_now instead of the walk.  Refuses what
 * arctic_trace_triangles refuses, and ARCTIC_E_CAPACITY for too little room; a refused call writes nothing. */
int arctic_refit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                           ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2);

/* ---- re-split: the structure is split again for the pose the scene has NOW, on the device ------------------------------------------------------
 * A refit keeps the order of the triangles in the slots from the pose the tree was split for, and the walk of such a tree slows down as the scene
 * moves on.  arctic_ray_scene_resplit puts the slots in the order a full build of the current pose would give them and refits -- in stream order
 * on the handle's stream, without synchronising, without reading anything back (ray_resplit.hip).  The builder splits [lo, hi) at
 * lo + (hi - lo) / 2 and stops at hi - lo <= 4, so the node count, every skip, every leaf word and the depth depend on the NUMBER of stored
 * triangles alone; the geometry decides only which triangle sits in which slot.
 *
 * A RE-SPLIT STRUCTURE, defined:
 * Topology.  The node count, every skip and every leaf word are those of the last full build; the set of stored triangles (prims) is that build's.
 * World vertices and centroids.  A stored triangle's world vertices are those of "A world vertex is ..." above, from the mesh's vertices in use
 *   NOW and the object's trs NOW.  Its centroid is that of its box, per axis c = 0.5f*lo + 0.5f*hi (lo = min, hi = max of the three vertices;
 *   the products round, then the sum: contraction off).
 * Dead triangles.  A triangle with a world vertex that is not finite now is DEAD.  On every axis a dead triangle orders behind every live one;
 *   among dead triangles the order is by prim.
 * Per segment [lo, hi) of slots, the root's being [0, stored):  hi - lo <= 4 is a LEAF, its slots ordered by prim.  Otherwise the axis is the one
 *   with the widest centroid extent over the segment's LIVE members, fp32 cmax - cmin under a strict >: on a tie the lowest axis wins; an extent
 *   that overflows to +inf still orders; a segment with no live member takes axis 0.  The members are ordered by (c[axis], prim) under < on
 *   floats -- -0 and +0 tie and fall to the prim --, dead members last; with mid = lo + (hi - lo) / 2 the lower mid - lo members form [lo, mid),
 *   the others [mid, hi), and the rule applies to each half.  (Only the two SETS matter: each half is ordered again by its own rule.)
 * Slot contents and boxes.  Those of a refit to the current pose ("A REFITTED STRUCTURE" above), dead slots and empty boxes included.
 * Consequence: with every stored triangle finite now, a re-split structure EQUALS the structure a full build of the current world triangles
 *   makes (bvh.cpp: bvh_build) -- triangles, skip and leaf compare by bytes, boxes compare by value.
 * arctic_ray_scene_resplit(r, scene).  When the cached structure could follow `scene` by a refit (Eligibility above: the option was 1 at the last
 *   full build, and so on) the re-split and the refit are enqueued -- also when nothing moved.  Otherwise the call does what
 *   arctic_ray_scene_reset and the build of the next query do.  A re-split counts neither as a build in arctic_ray_scene_info nor as a refit in
 *   arctic_ray_refit_info; later refits keep the order it left.  Its workspace (about 100 bytes per stored triangle) is allocated by the first
 *   re-split of a structure and kept; a handle that never makes the call allocates nothing and behaves as before.  Each rank of a sharded frame
 *   re-splits its own copy.  ARCTIC_E_INVALID: a null handle or scene. */
int arctic_ray_scene_resplit(ArcticRenderer *r, const ArcticScene *scene);

/* out4 = {device re-splits so far, launches of the latest one (its kernels and fills, each radix sort counted as one, and the refit's stages),
 * 1 if the latest arctic_ray_scene_resplit fell back to a full build on the host, 0}. */
int arctic_ray_resplit_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter of the re-split (no handle, no GPU), shaped like arctic_refit_triangles: builds on tris9_build, re-splits to tris9_now by the
 * definition above -- carried out directly, dead triangles included, not by a second build --, walks the result and optionally returns it.
 * With ARCTIC_TRACE_BRUTE the hits come from the loop over every triangle of tris9_now.  The same refusals; a refused call writes nothing. */
int arctic_resplit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                             ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2);

/* ---- ambient occlusion from the resident G-buffer (no counterpart in the reference: its one ambient term is the flat ambient * base_color) ---------
 * How open is each pixel?  n_rays short any-hit rays per pixel over the hemisphere of its normal, against the structure of the ray queries above
 * (built, refitted and re-split as described there), walked by ordinary vector code (ray_ao.hip).  The answer is DEFINED bit for bit: numpy in
 * float32 reproduces it (tests/ao_reference.py), and so does arctic_ambient_occlusion_points on the host.  Nothing in the passes uses the plane:
 * shading and every existing bit are unchanged; arctic_compose_planes_device and arctic_pass_ray_effects (below) fold it into the shaded frame.
 *
 * THE DEFINITION.  Everything is fp32, one rounding per operation, in the written order, no contraction; division and square root are IEEE
 * (correctly rounded); dot, min, max as the ray-query section defines them.
 * dirs = P*P*n_rays*3 floats: direction k of set s sits at dirs[(s*n_rays + k)*3 ..]: LOCAL directions, z along the normal, used as given -- not
 *   normalised, no sign check (a table may reach below the horizon, or weight by length through radius); every component must be finite.
 *   Pixel (x, y) OF THE FRAME uses set (y % P) * P + x % P, so that a P x P window holds every set once and the filter below turns P*P*n_rays
 *   directions into one estimate.
 * Per pixel, with world = attributes 11..13 and n = attributes 8..10 of arctic_read_gbuffer's order:
 *   1. len = sqrt((n0*n0 + n1*n1) + n2*n2);  m[i] = n[i] / len.  The pixel is NOT COVERED if it has no geometry, if len is zero or not finite, or
 *      if any m[i] is not finite: its hits are 0 and its result is 255.  (The G-buffer's normals are interpolated, so they are not unit vectors;
 *      the frame below is orthonormal only for one that is.)
 *   2. The frame, from m alone (Duff et al., "Building an Orthonormal Basis, Revisited", branchless):
 *        s = copysign(1.0f, m2);  a = -1.0f / (s + m2);  b = (m0*m1)*a;
 *        t  = { 1.0f + ((s*m0)*m0)*a,  s*b,  (-s)*m0 };     bt = { b,  s + (m1*m1)*a,  -m1 }
 *      (m2 = -0.0 takes s = -1: a = 1, a frame like any other.)
 *   3. Ray k, with l = the local direction:  o[i] = world[i] + bias*m[i]  (the product rounds, then the sum);
 *        d[i] = (t[i]*l0 + bt[i]*l1) + m[i]*l2;   t_min = 0;   t_max = radius;
 *      any hit, by the ray definition above unchanged.  A ray that is invalid by that definition (a world position that is not finite, a
 *      direction that comes out zero) is a miss.
 *   4. hits = the number of the n_rays rays that hit.
 * Unfiltered result (u8):  (510*(n_rays - hits) + n_rays) / (2*n_rays), integer division: visibility on 0..255, rounded to nearest.
 * Filtered result for a covered pixel p at frame position (x, y):  the window is the pixels (x+i, y+j) with i, j in [-(P/2), P-1-P/2] -- offsets
 *   -2..1 for P = 4, -1..0 for P = 2, 0 for P = 1 --, which holds every direction set exactly once.  p itself is always accepted.  Another pixel q
 *   is accepted iff q lies inside the frame, q is covered, dot(m_p, m_q) >= normal_cos, and fabs(dot(m_p, w_q - w_p)) <= plane_dist, where the
 *   difference rounds per component first.  With V = the sum of (n_rays - hits_q) over the accepted pixels and T = n_rays * accepted, the result
 *   is (510*V + T) / (2*T).  A pixel that is not covered gives 255.
 * Sharded handles.  The pattern uses the row of the FRAME: a handle that owns a row range or interleaved bands returns exactly its rows of the
 *   whole frame's unfiltered result.  filter = 1 on a handle that does not own the whole frame is refused with ARCTIC_E_STATE and writes nothing
 *   -- the rule of ARCTIC_OPT_ANTIALIAS: the shard lacks its neighbours' rows.
 * KNOWN LIMITS.  Those of the ray definition (two-sided, not watertight); the bias is along the shading normal, so a ray of a strongly
 *   interpolated normal can start below its own surface. */
typedef struct ArcticAmbientOcclusion {   /* 32 bytes */
    uint32_t n_rays;      /* rays per pixel, 1..64 */
    uint32_t pattern;     /* P = 1, 2 or 4: pixel (x, y) OF THE FRAME uses direction set (y % P) * P + x % P */
    float    radius;      /* every ray's t_max: > 0, +inf allowed */
    float    bias;        /* finite */
    uint32_t filter;      /* 0: per-pixel result; 1: reconstruction over the P x P window */
    float    normal_cos;  /* filter only, finite */
    float    plane_dist;  /* filter only, >= 0 */
    uint32_t reserved;    /* 0 */
} ArcticAmbientOcclusion;

/* The result for every pixel of the handle's RESIDENT G-buffer (arctic_pass_gbuffer, arctic_write_gbuffer, or the latest frame): rows*width
 * bytes, row-major over the handle's rows like arctic_trace_sun_visibility.  out == NULL leaves the result on the device and does not
 * synchronise (timing).  Once the handle is warm a call allocates nothing; the table is sent again only when its bytes changed.
 * Refusals, in this order; a refused call writes nothing.  ARCTIC_E_INVALID: a null scene, ao or dirs; n_rays outside 1..64; pattern not 1, 2 or
 * 4; radius not > 0 (a NaN included); a bias that is not finite; filter > 1 or reserved != 0; with the filter on, a normal_cos that is not finite
 * or a plane_dist that is negative or a NaN; a direction component that is not finite.  ARCTIC_E_STATE: no G-buffer; the filter on a shard. */
int arctic_trace_ambient_occlusion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *out);

/* The same into DEVICE memory the caller owns (rows*width bytes), stream-ordered on the handle's stream: call arctic_flush() before another
 * stream reads d_out.  dirs stays a host pointer.  ARCTIC_E_INVALID also for a null d_out. */
int arctic_trace_ambient_occlusion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *d_out);

/* The host arbiter (no handle, no GPU): hits[k] for point k = {world3, normal3} of points6, using direction set sets[k] -- steps 1 to 4 above,
 * 0 for a point that is not covered; filter, normal_cos and plane_dist are checked and otherwise unused.  tris9 as in arctic_trace_triangles;
 * flags: 0 (the structure and the walk of the device) or ARCTIC_TRACE_BRUTE (the loop over every triangle).  Refuses what the call above refuses
 * with ARCTIC_E_INVALID, and an unknown flag, a null pointer with a non-zero count and a sets[k] >= P*P; ARCTIC_E_CAPACITY: n_tris above 2^32 - 2. */
int arctic_ambient_occlusion_points(const float *tris9, uint64_t n_tris, const float *points6, const uint32_t *sets, uint64_t n_points,
                                    const ArcticAmbientOcclusion *ao, const float *dirs, uint32_t flags, uint8_t *hits);

/* ---- what is AT a hit: attributes, shading, and a reflection plane (no counterpart in the reference: its roadmap's "Raytracing") ---------------------
 * A ray query answers {t, u, v, prim}.  The three layers below turn that into the interpolated vertex output at the hit, into the colour the
 * forward pass would give that point seen along the ray, and into a plane of mirror reflections of the resident G-buffer.  Each is usable alone.
 * Nothing in the passes uses them: shading, shadow maps and every existing bit are unchanged, and a handle that never makes these calls
 * allocates nothing for them; arctic_compose_planes_device and arctic_pass_ray_effects (below) fold the reflection plane into the shaded frame.
 *
 * 1. HIT ATTRIBUTES, DEFINED bit for bit: numpy in float32 reproduces them (tests/hit_reference.py), and so does arctic_interpolate_hits on the host.
 * Everything is fp32; each operation rounds once, in the written order, without contraction; division and square root are IEEE.
 * prim -> source.  `prim` is the running triangle index of the ray-query definition above: the objects in ArcticScene::objects order, each
 *   object's triangles in index-buffer order, an object whose mesh does not exist having none.  The result is material = 0xFFFFFFFF and eighteen
 *   zeros for prim == 0xFFFFFFFF (a miss), for a prim at or above the scene's count, and for the triangle with an index out of range, which is
 *   skipped but numbered.  Otherwise material is the mesh's material, as arctic_read_gbuffer reports it.
 * Per vertex, exactly what the vertex kernel writes, from the mesh's vertices IN USE (posed, else morphed, else its own) and the object's trs NOW:
 *     world[i] = ((M[i]*x + M[4+i]*y) + M[8+i]*z) + M[12+i]*1.0f         i = 0..3, M = trs (i = 3 is the w the next product takes: 1 for an affine trs)
 *     t, b, n  = the stored tangent, bitangent, normal, each times  inv = 1.0f / sqrt((v0*v0 + v1*v1) + v2*v2)  -- NOT transformed by trs
 *     light_space[i] = ((L[i]*world0 + L[4+i]*world1) + L[8+i]*world2) + L[12+i]*world3,   L = arctic_frame_constants' light_proj_view for `scene`
 *     uv = the stored texture coordinates
 * Interpolation.  w0 = (1.0f - u) - v.  Each of the 18 attributes -- arctic_read_gbuffer's order: uv2, t3, b3, n3, world3, light_space4 -- is
 *     (w0*a0 + u*a1) + v*a2      a0, a1, a2 = the attribute at the triangle's first, second, third index
 *   u and v are used as given (not clamped); t is not used.  A NaN u or v propagates: the attributes it reaches are NaNs, of a sign and payload
 *   that are not defined -- compare those as NaNs, everything else by bytes.
 * The handle keeps a table, indexed by prim, of where every triangle takes its vertices from.  It depends on the topology alone, is made by the
 * first of these calls behind the ray structure and made again only behind a full build of it: the calls keep working, without a rebuild, after a
 * refit and after arctic_ray_scene_resplit. */

/* attrs[18 k ..] and material[k] for hits[k].  Host buffers, synchronous; builds or refreshes the ray structure like arctic_trace_rays.
 * ARCTIC_E_INVALID: a null scene, a null pointer with n > 0.  ARCTIC_E_CAPACITY: n above 2^32 - 1, or a scene too large (above). */
int arctic_hit_attributes(ArcticRenderer *r, const ArcticScene *scene, const ArcticHit *hits, uint64_t n, float *attrs, uint32_t *material);

/* The host arbiter (no handle, no GPU) for ONE object: its mesh (n_indices / 3 triangles), its trs (16 floats), the sun's matrix (16 floats) and
 * the mesh's material.  The object's triangles are prims first_prim .. first_prim + n_indices / 3 - 1; a hit whose prim lies there gets its
 * attributes and material (eighteen zeros and 0xFFFFFFFF for the triangle with an index out of range), every other hit's entries are LEFT AS THEY
 * ARE -- so a caller fills the outputs with zeros and 0xFFFFFFFF and chains the scene's objects.  ARCTIC_E_INVALID: a null pointer with a non-zero
 * count, null trs or matrix.  ARCTIC_E_CAPACITY: more than 2^32 - 1 vertices, prims beyond 2^32 - 2. */
int arctic_interpolate_hits(const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, const float *trs,
                            const float *light_proj_view, uint32_t material, uint64_t first_prim, const ArcticHit *hits, uint64_t n, float *attrs,
                            uint32_t *material_out);

/* 2. HIT SHADING (hit_shade.hip: k_shade_hits).  rgba32f[4 k ..] for ray k and its hit:
 * A hit (a prim that resolves, above):  rgb = ps_main (forward.hlsl:208-235) on the attributes of layer 1 with eye := rays[k].origin, so
 *   wo = normalize(origin - world);  a = 1.  The material's textures are sampled at LEVEL 0 with the default sampler -- full-fp32 bilinear
 *   weights, WRAP, sRGB decoded per texel before filtering -- whatever ARCTIC_OPT_SAMPLER says.  calculate_shadow takes its 25 taps on the
 *   handle's resident sun map (shadow_size == 0: shadow 0).  The point lights are those last given to arctic_update_lights, in caller order;
 *   ambient and sun come from `scene`.  A back face is shaded with the stored frame, without a flip.  The hit's t is not used.
 * A miss or a prim that does not resolve:  with an environment map (arctic_create_hdri), its level 0 along d / |d| under the skybox's mapping
 *   (uv = (atan2(d.z, d.x) * 0.1591f + 0.5, -(asin(d.y) * 0.3183f + 0.5)), bilinear, WRAP), a = 0.  Without a map, or for a direction that is
 *   zero or has a component that is not finite: {0, 0, 0, 0}.
 * Held to the shading pass's standing bar against float64 (tests/test_gpu_hit_shading.py), not defined bit for bit.
 * OUT OF SCOPE at hits: spot lights, shadow-casting point lights, image-based ambient (ARCTIC_OPT_ENV_LIGHTING), material extras
 *   (arctic_set_material_extras) and mip chains (ARCTIC_OPT_TEXTURE_MIPS) do not take part; a handle that has them still answers ARCTIC_OK with
 *   the base model above.  That is ARCTIC_OPT_HIT_MODEL = 0, the default.
 * ARCTIC_OPT_HIT_MODEL = 1 (hit_shade_ext.hip: k_shade_hits_ext) shades the hit with the forward pass's whole pixel, each part by the definition
 *   that stands next to its call or option above, with eye := rays[k].origin, one light at a time in the caller's order:
 *     Lo    = sun + sum(point) + sum(spot: colour att window / d2) + sum(cube: colour v / d2)
 *     rgb   = Lo (1 - shadow) + A ao + E,      A = ambient * base'  or, with image-based ambient active, ambient * ibl(n', wo, base', metal', rough')
 *   material extras (only while a material of the handle is not neutral): the factors on base, metal and rough, normal_scale on the tangent-space x
 *     and y, E = the sRGB-decoded emissive image * emissive_factor -- not multiplied by (1 - shadow) --, ao = 1 + occlusion_strength (o - 1) on the
 *     ambient term only; both images bilinear with WRAP at level 0, whichever way the handle stores them.
 *   spot lights (arctic_update_spot_lights) behind the point lights: att = sat(cd scale + offset)^2, window = sat(1 - (d2 ir2)^2).
 *   shadow-casting point lights (arctic_update_point_shadow_lights) behind the spots: the face of the largest |d| (ties x, then y, then z), the
 *     lookAt rows above, four clamped texels, compare then bilinear, v = 1 inside the near and beyond the far plane; their sum stands under the
 *     sun's (1 - shadow) like every other light's.
 *   image-based ambient, when ARCTIC_OPT_ENV_LIGHTING = 1 and a map are both there: the bracket of that option from the resident tables in place of
 *     ambient * base; never multiplied by the sun's shadow.
 *   Mip chains STAY OUT under both values: a hit has no pixel footprint, so every image is sampled at level 0; so do ARCTIC_OPT_SAMPLER's modes.
 *   A hit AT the ray's origin (world == origin by bits: t = 0 on a surface the origin lies on) has wo = 0 / 0 under both models, and its colour is
 *   not a number wherever wo is used: the base model does not use it where the sun's shadow is total, the image-based ambient always does.
 *   Alpha, misses and invalid directions are those of the base model.  A handle with no spot light, no shadow-casting point light, only neutral
 *   materials and no active image-based ambient gets the base model's bytes.  Every consumer of the hit shading follows the option:
 *   arctic_shade_hits(_device), arctic_trace_reflections(_device), arctic_pass_ray_effects*, arctic_trace_gi, arctic_pass_gi.  Held to the same bar
 *   against float64 (tests/test_gpu_hit_model.py).  A handle that never sets the option allocates nothing for it.
 * Refusals, before the device is touched; a refused call writes nothing.  ARCTIC_E_INVALID: a null scene, flags != 0, a null pointer with n > 0.
 *   ARCTIC_E_CAPACITY: n above 2^32 - 1 (or a scene too large).  ARCTIC_E_STATE: the handle has a sun map (shadow_size != 0) that was never
 *   drawn or written, or that is sharded (ARCTIC_OPT_SHADOW_SHARDED); under ARCTIC_OPT_HIT_MODEL = 1 also a non-empty list of shadow-casting
 *   point lights whose faces were neither drawn (arctic_pass_point_shadows, a frame) nor written (arctic_write_point_shadow) since the list or
 *   ARCTIC_OPT_POINT_SHADOW_SIZE was set.  That state is ONE flag for the whole list, like the sun map's: arctic_write_point_shadow of one light
 *   sets it for all (the others' faces are then the cleared 1.0: everything lit), and a drawn face whose rasteriser table overflowed (the
 *   ARCTIC_E_CAPACITY of the next synchronising call) still counts as drawn -- render again, as that error says. */
#define ARCTIC_OPT_HIT_MODEL         0 /* 0 (default) = the base model at hits (k_shade_hits); 1 = the extended model above; anything else: ARCTIC_E_INVALID.
                                          (Its number is 0: 1 .. 27 are taken -- 14 in arctic_dist.h -- and 0 was the free one that is not above them.) */
int arctic_shade_hits(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *rays, const ArcticHit *hits, uint64_t n, uint32_t flags, float *rgba32f);

/* The same between DEVICE buffers the caller owns (16-byte aligned), stream-ordered on the handle's stream like arctic_trace_rays_device: call
 * arctic_flush() before another stream reads d_rgba32f.  ARCTIC_E_INVALID also for a pointer that is not 16-byte aligned. */
int arctic_shade_hits_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *d_rays, const ArcticHit *d_hits, uint64_t n, uint32_t flags,
                             float *d_rgba32f);

/* 3. THE REFLECTION PLANE.  One mirror ray per pixel of the handle's RESIDENT G-buffer (arctic_pass_gbuffer, arctic_write_gbuffer, or the latest
 * frame), its closest hit shaded by layer 2: three launches over buffers the handle owns (k_reflect_rays, the ray queries' walk, k_shade_hits).
 * Per pixel, with world = attributes 11..13, n = attributes 8..10 and eye = scene->camera.eye; fp32, one rounding per operation, no contraction:
 *   m = n / len as in step 1 of the ambient occlusion.  A pixel without geometry or NOT COVERED by that step has no ray.
 *   i[j] = world[j] - eye[j];   k = dot(m, i)  (the ray queries' dot);   k >= 0 (the surface faces away): no ray.
 *   d[j] = i[j] - (2.0f*k)*m[j];   o[j] = world[j] + bias*m[j]  (the product rounds, then the sum);   t_min = 0;   t_max = +inf
 *   The result is layer 2's for that ray and its closest hit.  A pixel without a ray is {0, 0, 0, 0}: it stands in the ray buffer as the
 *   all-zero record, whose direction is zero.  So a = 1 where the reflection shows geometry, 0 elsewhere.
 * The normal is the INTERPOLATED VERTEX NORMAL, as in the ambient occlusion, not the normal-mapped one.
 * rgba32f = rows * width * 4 floats, row-major over the handle's rows like arctic_trace_sun_visibility; a sharded handle answers for its own
 * rows.  rgba32f == NULL leaves the plane on the device and does not synchronise (timing).
 * ARCTIC_E_INVALID: a null scene, a bias that is not finite.  ARCTIC_E_STATE: no G-buffer; the sun map's states of layer 2. */
int arctic_trace_reflections(ArcticRenderer *r, const ArcticScene *scene, float bias, float *rgba32f);

/* The same into DEVICE memory the caller owns (rows * width * 16 bytes, 16-byte aligned), stream-ordered on the handle's stream.
 * ARCTIC_E_INVALID also for a null or misaligned d_rgba32f. */
int arctic_trace_reflections_device(ArcticRenderer *r, const ArcticScene *scene, float bias, float *d_rgba32f);

/* What the three layers hold on this handle: out4 = {bytes of device memory (the source table, the object records, the host forms' buffers and
 * the plane's rays, hits and colours, at their capacities), bytes of pinned host memory (the object records' ring), prims in the source table,
 * times the source table was made}.  {0, 0, 0, 0} until the first arctic_hit_attributes, arctic_shade_hits(_device) or
 * arctic_trace_reflections(_device) that passes its checks.  Touches no device. */
int arctic_hit_shading_info(ArcticRenderer *r, uint64_t *out4);

/* ---- occlusion and reflections composed into the shaded frame (no counterpart in the reference: the last stage of its roadmap's "Raytracing") -------
 * The ambient occlusion's byte plane and the reflection plane above, folded into the frame the shading pass left, IN FRONT OF the tonemapper: one
 * streaming kernel (compose.hip: k_compose) over the handle's rows, and the one call that traces both planes and composes them.  Nothing in the
 * passes changes: a handle that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Everything is fp32.  For every pixel of the handle's rows:
 *   hdr  = the float HDR colour the last shading left (what arctic_read_output returns as hdr_rgb; needs ARCTIC_OPT_KEEP_FLOAT_OUTPUT);
 *   the resident G-buffer: uv = attributes 0..1, n = attributes 8..10, world = attributes 11..13 of arctic_read_gbuffer's order, and material;
 *   ao   = a byte, visibility on 0..255 (arctic_trace_ambient_occlusion's result);   refl = four floats (arctic_trace_reflections' result).
 * A pixel without geometry (material == 0xFFFFFFFF, or an index the handle has no material for -- the shading pass's own test):  C = hdr.
 * Otherwise base, metal, rough = the material's channels at uv, sampled exactly as layer 2 of the hit shading samples them: level 0, the default
 *   sampler (full-fp32 bilinear weights, WRAP, sRGB decoded per texel before filtering), all three image layouts, whatever ARCTIC_OPT_SAMPLER says.
 * Occlusion (ARCTIC_COMPOSE_AO):
 *     vis = ao / 255;   ka = 1 - ao_strength * (1 - vis);   C = hdr + (ambient * base) * (ka - 1)          ambient = scene->ambient
 *   This scales ps_main's ambient term (forward.hlsl:233) by ka and touches nothing that carries 1 - shadow.  ao == 255 or ao_strength == 0 adds
 *   an exact zero.
 * Reflection (ARCTIC_COMPOSE_REFLECTIONS), present only where refl.a > 0:
 *     m  = n / len as in step 1 of the ambient occlusion: the INTERPOLATED VERTEX NORMAL the mirror ray used, not the normal-mapped one;
 *     wo = normalize(eye - world)   (eye = scene->camera.eye);      c = max(dot(m, wo), 0);
 *     F0 = 0.04 + (base - 0.04) * metal;      F = F0 + (1 - F0) * (1 - c)^5;
 *     g  = (1 - rough)^2      -- a single mirror ray stands for the specular lobe only as far as the surface is smooth;
 *     C += reflection_strength * refl.a * g * F * refl.rgb
 *   The term is a SELECT, not a product by zero: where refl.a is 0 (or a NaN), or the pixel is NOT COVERED by the occlusion's step 1, nothing of
 *   m or refl.rgb is looked at -- a NaN there does not reach C.
 * Tonemap.  post_process (post_process.hlsl:59-93) of C under `settings` gives the float LDR colour and RGBA8, by the operations arctic_post_process
 *   carries out.
 * Not defined bit for bit (the sampler, a fifth power, the tonemapper): held to the shading pass's two standing bars against float64,
 *   |hdr - want| / (|want| + 1e-3) <= 1e-4 and |ldr - want| <= 1e-4 (tests/test_gpu_compose.py).
 * That the HDR plane and the resident G-buffer belong to the same frame is the caller's business when the passes are driven one by one; after
 *   arctic_render_frame it holds by construction (the G-buffer is resolved on demand from the frame's visibility plane).
 * ARCTIC_OPT_ANTIALIAS is not applied to the composed image: a caller runs arctic_antialias_device on it.
 * Sharded handles compose their own rows: the kernel needs no neighbours.
 * Refusals, in this order, before the device is touched; a refused call writes nothing.
 *   ARCTIC_E_INVALID: a null scene, settings or block; flags 0 or with unknown bits; ao_strength outside [0, 1] or a NaN; reflection_strength
 *     negative or not finite; reserved != 0; a null plane that a flag needs, or a float plane that is not 16-byte aligned (the byte plane may be
 *     at any address).
 *   ARCTIC_E_STATE: no G-buffer; ARCTIC_OPT_KEEP_FLOAT_OUTPUT off, or no shading since it was turned on or since the last resize;
 *     ARCTIC_OPT_HDR16 = 1; with ARCTIC_COMPOSE_AO: ARCTIC_OPT_ENV_LIGHTING on, ARCTIC_OPT_TEXTURE_MIPS = 1, or a material that is not neutral
 *     (arctic_set_material_extras) -- the ambient term of such a frame is not ambient * base at level 0, and the occlusion would scale something the
 *     frame does not hold; it is refused, not approximated. */
#define ARCTIC_COMPOSE_AO          1u
#define ARCTIC_COMPOSE_REFLECTIONS 2u
typedef struct ArcticRayCompose {   /* 32 bytes */
    uint32_t flags;                /* ARCTIC_COMPOSE_AO | ARCTIC_COMPOSE_REFLECTIONS, at least one */
    float    ao_strength;          /* 0..1: 0 leaves the frame as it is, 1 takes the ambient term of a closed pixel (ao = 0) away */
    float    reflection_strength;  /* >= 0, finite */
    float    reflection_bias;      /* arctic_pass_ray_effects only: the bias of arctic_trace_reflections */
    uint32_t reserved[4];          /* 0 */
} ArcticRayCompose;

/* k_compose alone, on DEVICE planes the caller owns: d_ao_u8 (rows*width bytes) and d_reflection_rgba32f (rows*width*16 bytes, 16-byte aligned),
 * row-major over the handle's rows; a plane whose flag is absent may be NULL.  d_out_rgba8: rows*width*4 bytes of device memory (4-byte aligned: ARCTIC_E_INVALID otherwise), or NULL = the
 * handle's own buffer (arctic_read_composed).  The float LDR and the composed HDR go to the handle's own buffers.  Stream-ordered on the handle's
 * stream: call arctic_flush() before another stream reads d_out_rgba8.  Once the handle is warm a call allocates nothing. */
int arctic_compose_planes_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                 const uint8_t *d_ao_u8, const float *d_reflection_rgba32f, uint8_t *d_out_rgba8);

/* The one call.  With ARCTIC_COMPOSE_AO: arctic_trace_ambient_occlusion_device with `ao` and `dirs` as that call takes them, into the handle's own
 * plane.  With ARCTIC_COMPOSE_REFLECTIONS: arctic_trace_reflections_device with the bias compose->reflection_bias, into the handle's own plane.
 * Then k_compose on those planes.  Byte for byte what the three public calls give when made by hand.  ao and dirs may be NULL without
 * ARCTIC_COMPOSE_AO.  Every refusal of the three calls is unchanged (the occlusion's filter on a shard and the sun map's states of the hit shading
 * among them), and all of them come before anything is enqueued: a refused call writes nothing. */
int arctic_pass_ray_effects(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                            const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *d_out_rgba8);

/* The last composed planes, shaped like arctic_read_output: rows*width*3 floats, rows*width*3 floats, rows*width*4 bytes; any may be NULL.
 * Synchronises.  ARCTIC_E_STATE: nothing composed yet (or not since the last resize); rgba8 asked for when the last call wrote the caller's
 * buffer. */
int arctic_read_composed(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8);

/* The host arbiter (no handle, no GPU): the composed HDR colour of n pixels from channels the caller has sampled already -- the definition's two
 * terms by the very functions the kernel runs, without the sampler and without the tonemapper.  Per pixel k: hdr3, base3, metal, rough, the G-buffer's
 * normal3 (not normalised: step 1 is carried out here) and world3, ao, refl4, and geometry[k] != 0 where the pixel has geometry.  ao may be NULL
 * without ARCTIC_COMPOSE_AO, refl4 without ARCTIC_COMPOSE_REFLECTIONS.  The same ARCTIC_E_INVALID refusals (the float plane needs no alignment
 * beyond a float's), also for a null eye3 and a null array with n > 0; a refused call writes nothing. */
int arctic_compose_pixels(const ArcticRayCompose *compose, const float *eye3, float ambient, uint64_t n, const float *hdr3, const float *base3,
                          const float *metal, const float *rough, const float *normal3, const float *world3, const uint8_t *ao, const float *refl4,
                          const uint8_t *geometry, float *out_hdr3);

/* What the composition holds on this handle: out4 = {bytes of device memory (the composed RGBA8, LDR and HDR buffers, at their capacities),
 * launches of k_compose, calls of arctic_pass_ray_effects that passed their checks, 0}.  {0, 0, 0, 0} until the first call that passes its checks.
 * Touches no device. */
int arctic_compose_info(ArcticRenderer *r, uint64_t *out4);

/* ---- temporal accumulation of the ambient occlusion's byte plane (no counterpart in the reference) --------------------------------------------------
 * One occlusion ray per pixel gives 0 or 255; these calls carry the estimate from frame to frame: reproject it through the PREVIOUS call's camera,
 * reject history that belongs to another surface, blend the new byte into it.  A caller who turns the direction table every frame
 * (ao_directions(n, P, seed = frame)) gets the quality of tens of rays per pixel for one ray and one streaming kernel (ao_history.hip:
 * k_ao_accumulate).  Nothing in the passes or in the other ray calls changes: a handle that never makes these calls renders the same bytes and
 * allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit, like the occlusion itself: fp32 throughout, one rounding per operation in the written order, no contraction,
 * IEEE division and square root.
 * STATE.  The handle keeps a history H of its frame: per pixel {world3, value} and {m3, count}, two float4 planes, 32 bytes per pixel, and TWO sets
 *   of them (a call reads one and writes the other): 64 bytes per pixel, 531 MB at 3840 x 2160, allocated by the first call that passes its checks
 *   (arctic_ao_history_info).  It also keeps the proj_view (16 floats, arctic_frame_constants' layout [col][row]) and the frame size of the call
 *   that wrote H.  H is EMPTY before the first call, after arctic_ao_history_reset and after arctic_resize.
 * INPUTS.  The resident G-buffer (n = attributes 8..10, world = attributes 11..13, material), `scene` (its camera gives THIS call's proj_view, kept
 *   for the next call), the current byte plane ao_in, and ArcticAoHistory.
 * PER PIXEL p.  cur = (float)ao_in[p];  W, H = the frame's width and height as floats.
 *   1. m_p = n / len as in step 1 of the ambient occlusion, w_p = world.  No geometry (material == 0xFFFFFFFF) or NOT COVERED by that step:
 *      the output byte is 255 and the entry written is all zero (count 0: never accepted as a tap).
 *   2. H is empty:  N = 1, value = cur.
 *   3. Otherwise reproject with the PREVIOUS call's matrix P (the vertex kernel's product order, setup_triangle's projection):
 *        c[i] = ((P[i]*w0 + P[4+i]*w1) + P[8+i]*w2) + P[12+i]
 *        reject everything unless c3 > 0 and c0, c1, c3 are finite;
 *        iw = 1 / c3;  nx = c0*iw;  ny = c1*iw;  sx = (nx + 1) * (0.5*W);  sy = (1 - ny) * (0.5*H)
 *        gx = sx - 0.5;  gy = sy - 0.5;  ix = floor(gx);  iy = floor(gy);  ax = gx - ix;  ay = gy - iy
 *        reject everything, tested in float before any conversion, unless -1 <= ix <= W-1 and -1 <= iy <= H-1.
 *      "Reject everything": N = 1, value = cur, as in step 5.
 *   4. The four taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1), in this order, weigh (1-ax)*(1-ay), ax*(1-ay), (1-ax)*ay, ax*ay.
 *      A tap q is ACCEPTED iff it lies inside the frame, count_q > 0 and the occlusion filter's test holds on the STORED m_q, w_q of the previous
 *      call:  dot(m_p, m_q) >= normal_cos  and  |dot(m_p, w_q - w_p)| <= plane_dist.
 *      A rejected tap's weight is 0 and its history is not looked at -- a SELECT, not a product by zero: a NaN there does not reach the result.
 *        S = ((k0 + k1) + k2) + k3;   V, C = the same ordered sums of k*value_q and k*count_q.
 *   5. !(S > min_weight):  N = 1, value = cur.
 *   6. Otherwise  hv = V / S;  hn = C / S;  N = min(hn + 1, max_history);  a = 1 / N;  value = hv + (cur - hv) * a.
 *   7. The output byte is (uint8)min(max(floor(value + 0.5), 0), 255); the entry written is {w_p, value}, {m_p, N}.
 * KNOWN LIMITS, stated and not worked around.  There are no per-object motion vectors: a moving object is handled only as far as the two
 *   rejections catch it (the motion form below, arctic_accumulate_ambient_occlusion_motion_device, is the call that has them).  Only the occlusion
 *   plane is accumulated; the mirror reflection is one deterministic ray per pixel and is not.
 * Refusals, in this order; a refused call writes nothing and leaves H as it was.
 *   ARCTIC_E_INVALID: a null scene, hist or plane; max_history outside [1, 65536] or a NaN; normal_cos not finite; plane_dist negative or a NaN;
 *     min_weight outside [0, 1) or a NaN; reserved != 0.
 *   ARCTIC_E_STATE: no G-buffer; a handle that does not own the whole frame (the rule of the occlusion's filter: the taps' rows are elsewhere). */
typedef struct ArcticAoHistory {   /* 32 bytes */
    float    max_history;   /* N's cap: 1 <= max_history <= 65536, finite; 1 = no accumulation */
    float    normal_cos;    /* the acceptance test's bound on dot(m_p, m_q), finite */
    float    plane_dist;    /* the acceptance test's bound on |dot(m_p, w_q - w_p)|, >= 0 */
    float    min_weight;    /* history is used only if the accepted taps' weight S > min_weight; in [0, 1) */
    uint32_t reserved[4];   /* 0 */
} ArcticAoHistory;

/* One call of the definition on DEVICE planes the caller owns, rows*width bytes each, row-major.  d_ao_in_u8 == d_ao_out_u8 is allowed (a pixel
 * reads only its own current byte); the planes may not overlap otherwise.  Stream-ordered on the handle's stream.  The first call that passes its
 * checks allocates the two history sets (64 bytes per pixel); from then on a call allocates nothing and does not synchronise. */
int arctic_accumulate_ambient_occlusion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const uint8_t *d_ao_in_u8,
                                               uint8_t *d_ao_out_u8);

/* The host form: ao_in and ao_out are rows*width bytes of host memory (they may be the same).  Synchronous. */
int arctic_accumulate_ambient_occlusion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const uint8_t *ao_in, uint8_t *ao_out);

/* Empties H (the next call is a first call) and sets the calls counter to 0.  Frees nothing, touches no device. */
int arctic_ao_history_reset(ArcticRenderer *r);

/* The history the last call WROTE, row-major: value and count rows*width floats, world3 and normal3 (the stored m) rows*width*3 floats.  Any
 * pointer may be NULL.  Synchronises.  ARCTIC_E_STATE while H is empty. */
int arctic_read_ao_history(ArcticRenderer *r, float *value, float *count, float *world3, float *normal3);

/* What the accumulation holds on this handle: out4 = {bytes of device memory (the two history sets, at their capacities), launches of
 * k_ao_accumulate, calls since the last reset, 0}.  {0, 0, 0, 0} until the first call that passes its checks.  Touches no device. */
int arctic_ao_history_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter (no handle, no GPU): the definition for n pixels in any order, by the very functions the kernel runs.  Per pixel k: world3,
 * normal3 (not normalised: step 1 is carried out here), geometry[k] != 0 where the pixel has geometry, and cur[k], its current byte.
 * prev_proj_view: the previous call's matrix, NULL = the history is empty; width, height: the frame (1..16384 each); prev_value, prev_count,
 * prev_world3, prev_normal3: the previous history as arctic_read_ao_history returns it (ignored while prev_proj_view is NULL).  Outputs: the byte
 * (required with n > 0), and -- each may be NULL -- value, N, and the stored w_p and m_p (all zero for step 1's pixels).  No output may overlap
 * the previous history.  The same ARCTIC_E_INVALID refusals, also for a frame size out of range and a null array that is needed. */
int arctic_accumulate_pixels(const ArcticAoHistory *hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const uint8_t *cur,
                             const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_value, const float *prev_count,
                             const float *prev_world3, const float *prev_normal3, uint8_t *out_u8, float *out_value, float *out_count, float *out_world3,
                             float *out_normal3);

/* arctic_pass_ray_effects with the accumulation between the occlusion and k_compose: arctic_trace_ambient_occlusion_device into the handle's own
 * plane, arctic_accumulate_ambient_occlusion_device on that plane in place, the reflection plane if ARCTIC_COMPOSE_REFLECTIONS is set, then
 * k_compose.  Requires ARCTIC_COMPOSE_AO (ARCTIC_E_INVALID without it).  Byte for byte the public calls made by hand.  Every refusal of those calls
 * is unchanged and comes before anything is enqueued: a refused call writes nothing and leaves H as it was.  arctic_pass_ray_effects itself is
 * what it was. */
int arctic_pass_ray_effects_temporal(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                     const ArcticAmbientOcclusion *ao, const float *dirs, const ArcticAoHistory *hist, uint8_t *d_out_rgba8);

/* ---- per-pixel motion vectors, and the accumulation that uses them (no counterpart in the reference) ------------------------------------------------
 * "Where was this surface point in the previous frame": for every pixel of the current visibility plane the world position its surface point had
 * at the PREVIOUS motion call -- through that call's trs and that call's pose or morph weights -- and the offset on the screen to where it was
 * seen then.  It is what lets the occlusion's history follow an object that moves (a changed trs, arctic_set_mesh_pose,
 * arctic_set_mesh_morph_weights), and what temporal anti-aliasing and the motion blur (below) read first.  Nothing in the passes or in the other calls
 * changes: a handle that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division.
 * STATE.  The handle keeps M, what the previous motion call saw: per entry o of that call's object list its mesh handle and the 16 floats of its
 *   trs; that call's proj_view (arctic_frame_constants' layout [col][row]) and the frame size; and per mesh the object-space positions its vertices
 *   in use held when that call was enqueued.  A mesh that was neither posed nor morphed then needs nothing (its own vertices never change); any other
 *   gets a snapshot, one float4 {x, y, z, 0} per vertex, written by k_motion_snapshot at the END of the call in stream order behind k_motion, and only
 *   when the mesh's shape has changed since the snapshot was last written -- one buffer per mesh: a call reads pose N-1 from it, then overwrites it
 *   with pose N.  M is EMPTY before the first call, after arctic_motion_reset and after arctic_resize.
 * INPUTS.  The visibility plane of the current frame with the records of its prepass -- exactly what resolves the G-buffer --, so after
 *   arctic_pass_gbuffer or a frame; and `scene`, the scene that was DRAWN (its objects give this call's trs and meshes, its camera this call's
 *   proj_view: both kept for the next call).
 * PER PIXEL p = (px, py), in the frame's coordinates whatever rows the handle owns.  A pixel reads no neighbour.
 *   1. No triangle covers p:  prev_world4 = {0, 0, 0, 0}, velocity2 = {0, 0}, bary3 = {0, 0, 0}, source4 = {0xFFFFFFFF, 0, 0, 0}.
 *   2. Otherwise B = the perspective-correct barycentrics of p in its SOURCE triangle, the three weights every one of the 18 attributes of
 *      arctic_read_gbuffer is interpolated with; o = the triangle's entry in the scene's object list; i0, i1, i2 = its three indices into the
 *      mesh's vertices.  bary3 = B, source4 = {o, i0, i1, i2}.
 *   3. Entry o HAS A PREVIOUS iff M is not empty, o is below the previous call's object count, and that call's entry o named the same mesh.
 *      Without a previous:  prev_world4 = {0, 0, 0, 0}, velocity2 = {0, 0}.
 *   4. X_k = prev_trs[o] * (prevpos[i_k], 1), rows 0..2, in the vertex kernel's product order:
 *        X_k[j] = ((T[j]*x + T[4+j]*y) + T[8+j]*z) + T[12+j]*1
 *      pw[j] = (B0*X_0[j] + B1*X_1[j]) + B2*X_2[j], the attributes' order.   prev_world4 = {pw, flag}.
 *   5. The velocity, through the PREVIOUS call's matrix P (the accumulation's operations up to sx, sy):
 *        c[i] = ((P[i]*pw0 + P[4+i]*pw1) + P[8+i]*pw2) + P[12+i]
 *        c3 > 0 and c0, c1, c3 finite:  iw = 1 / c3;  nx = c0*iw;  ny = c1*iw;  sx = (nx + 1) * (0.5*W);  sy = (1 - ny) * (0.5*H);
 *          velocity2 = {sx - (px + 0.5), sy - (py + 0.5)}, flag = 2.
 *        otherwise:  velocity2 = {0, 0}, flag = 1.
 *      The vector points from this pixel's centre to where the point WAS: the offset a consumer adds to fetch history.
 *   The flag (prev_world4's w): 0 = nothing known, 1 = the previous point alone, 2 = the point and its velocity.
 * WHAT FOLLOWS.  With no trs, pose or weights changed since the previous call, pw equals the G-buffer's world (attributes 11..13) bit for bit.
 * An object whose mesh does not exist and a triangle with an index out of range never reach a pixel (the prepass skips both); every index is
 *   bounded by the mesh's vertex count before a position is read.
 * Refusals, in this order; a refused call writes nothing and leaves M as it was.
 *   ARCTIC_E_INVALID: a null handle, scene or prev_world4 plane (the device form: also a prev_world4 that is not 16-byte aligned, a velocity2
 *     that is not 8-byte aligned).
 *   ARCTIC_E_STATE: no visibility plane -- nothing drawn yet, or the G-buffer in place was written by arctic_write_gbuffer. */

/* One call of the definition into DEVICE planes the caller owns, row-major, in the handle's own rows: rows*width float4 (prev_world4) and
 * rows*width float2 (velocity2, may be NULL).  Stream-ordered on the handle's stream.  The per-object table of the call travels through a ring of
 * pinned buffers; a warm call on a scene without a posed or morphed mesh allocates nothing and does not synchronise.  After enqueueing, M is this
 * call's scene: make the call ONCE per frame, after the frame's pose / trs have been set and drawn. */
int arctic_motion_vectors_device(ArcticRenderer *r, const ArcticScene *scene, float *d_prev_world4, float *d_velocity2);

/* The host form: the same kernel into host memory, with its two further outputs -- bary3 (rows*width*3 floats) and source4 (rows*width*4
 * uint32: {o, i0, i1, i2}) -- which let a caller restate the pass without a rasteriser of its own.  Any pointer may be NULL.  Synchronous. */
int arctic_motion_vectors(ArcticRenderer *r, const ArcticScene *scene, float *prev_world4, float *velocity2, float *bary3, uint32_t *source4);

/* Empties M (the next call is a first call) and sets the calls counter to 0.  Frees nothing, touches no device. */
int arctic_motion_reset(ArcticRenderer *r);

/* What the motion calls hold on this handle: out4 = {bytes of device memory (the snapshots, the table, and the planes of the host form and of
 * arctic_pass_ray_effects_motion, at their capacities), launches of k_motion, launches of k_motion_snapshot, calls since the last reset}.
 * {0, 0, 0, 0} until the first call that passes its checks.  Touches no device. */
int arctic_motion_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter (no handle, no GPU): steps 3 to 5 for n pixels in any order, by the very functions the kernel runs.  Per pixel k: bary3 (B),
 * object[k] (its entry o; 0xFFFFFFFF = no geometry), prev_pos9 (the previous object-space positions of its three vertices, x y z each), and
 * pixel_xy (px, py).  prev_trs: n_objects x 16 floats, the previous call's trs by entry (an object[k] at or above n_objects has no previous);
 * prev_proj_view: the previous call's matrix, NULL = M is empty; width, height: the frame (1..16384 each).  Outputs: prev_world4 (n*4 floats,
 * required with n > 0) and velocity2 (n*2 floats, may be NULL).  ARCTIC_E_INVALID: a frame size out of range, a null array that is needed. */
int arctic_motion_pixels(uint64_t n, const float *bary3, const uint32_t *object, const float *prev_pos9, const int32_t *pixel_xy, const float *prev_trs,
                         uint64_t n_objects, const float *prev_proj_view, uint32_t width, uint32_t height, float *prev_world4, float *velocity2);

/* THE ACCUMULATION WITH MOTION.  arctic_accumulate_ambient_occlusion_device's definition with two changes, pw_p and flag_p being pixel p's entry
 * of a prev_world4 plane (row-major, rows*width float4, as arctic_motion_vectors_device writes it):
 *   Step 3 reprojects pw_p in place of w_p; unless flag_p >= 1 (a NaN is not) it rejects everything.
 *   Step 4's plane test is |dot(m_p, w_q - pw_p)| <= plane_dist: both positions lie in the previous frame.
 * The normal test and the entry written ({w_p, value}, {m_p, N}) are unchanged, so both calls share H and may be mixed from frame to frame (the
 * launches arctic_ao_history_info counts are those of either kernel, k_ao_accumulate or k_ao_accumulate_motion).  The refusals are the plain
 * call's, plus ARCTIC_E_INVALID for a null prev_world4 plane (the device form: or one that is not 16-byte aligned).
 * KNOWN LIMIT, stated and not worked around: a surface that ROTATES between frames is tested with this frame's normal m_p against the stored m_q
 * of the previous frame; normal_cos is what tolerates that. */
int arctic_accumulate_ambient_occlusion_motion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const float *d_prev_world4,
                                                      const uint8_t *d_ao_in_u8, uint8_t *d_ao_out_u8);

/* The host form: prev_world4 is rows*width*4 floats, ao_in and ao_out rows*width bytes of host memory (they may be the same).  Synchronous. */
int arctic_accumulate_ambient_occlusion_motion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const float *prev_world4, const uint8_t *ao_in,
                                               uint8_t *ao_out);

/* Its host arbiter: arctic_accumulate_pixels with one more input array, prev_world4 (n*4 floats: pw and the flag of every pixel). */
int arctic_accumulate_pixels_motion(const ArcticAoHistory *hist, uint64_t n, const float *world3, const float *prev_world4, const float *normal3, const uint8_t *geometry,
                                    const uint8_t *cur, const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_value, const float *prev_count,
                                    const float *prev_world3, const float *prev_normal3, uint8_t *out_u8, float *out_value, float *out_count, float *out_world3,
                                    float *out_normal3);

/* arctic_pass_ray_effects_temporal with two differences: arctic_motion_vectors_device goes into a plane the handle owns, in front of the occlusion,
 * and the accumulation is the motion form on that plane.  Byte for byte the public calls made by hand.  Every refusal of those calls comes before
 * anything is enqueued: a refused call writes nothing and leaves H and M as they were.  arctic_pass_ray_effects and
 * arctic_pass_ray_effects_temporal are what they were. */
int arctic_pass_ray_effects_motion(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                   const ArcticAmbientOcclusion *ao, const float *dirs, const ArcticAoHistory *hist, uint8_t *d_out_rgba8);

/* ---- temporal anti-aliasing: camera jitter and a history resolve (no counterpart in the reference) ------------------------------------------------
 * The frame is point-sampled at pixel centres.  Two pieces turn a sequence of frames into an anti-aliased one: a sub-pixel offset of the sample
 * position that changes from frame to frame, and a resolve in front of the tonemapper that blends each frame's float HDR colour into a history
 * fetched where the surface point WAS (velocity2 of arctic_motion_vectors_device).  Nothing in the passes or in the other calls changes: a handle
 * that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE JITTER.  ArcticCamera is byte-compatible with the reference and has no room for it, so the handle keeps it. */

/* Sets the handle's camera jitter (jx, jy), in pixels; both finite and in [-1, 1], else ARCTIC_E_INVALID.  The default is (0, 0).  It applies to
 * the forward prepass only (arctic_pass_gbuffer, and so arctic_render_frame): the matrix that is drawn is arctic_jitter_proj_view of the
 * camera's, and the cluster culling tests against that matrix.  The shadow pass, the cube faces, arctic_frame_constants, the motion calls and the
 * occlusion history keep the unjittered matrix.  arctic_resize keeps the jitter.  With (0, 0) arctic_jitter_proj_view is NOT CALLED: the matrix,
 * and so every byte of every path, is what it was.  Touches no device.
 * KNOWN LIMIT, stated and not worked around: the occlusion history and k_motion reproject through unjittered matrices, so under jitter their
 * screen positions are off by less than one pixel from the drawn samples.  velocity2 of a still scene is -j, and the resolve's step 3 adds j back. */
int arctic_set_camera_jitter(ArcticRenderer *r, float jx, float jy);

/* A pure host function (no device, no handle), the one the forward prepass calls: in arctic_frame_constants' layout [col][row], for c = 0..3
 *     m[4c+0] = m[4c+0] + kx * m[4c+3]          m[4c+1] = m[4c+1] - ky * m[4c+3]          kx = (2*jx)/W,  ky = (2*jy)/H
 * in fp32, one rounding per operation.  A point the unjittered matrix puts at screen position s is drawn at s + j.  ARCTIC_E_INVALID (nothing
 * written): a null matrix, a frame size outside 1..16384, a jitter that is not finite or outside [-1, 1]. */
int arctic_jitter_proj_view(float *proj_view16, uint32_t width, uint32_t height, float jx, float jy);

/* THE RESOLVE: THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division.
 * min(a, b) is (b < a) ? b : a and max(a, b) is (a < b) ? b : a.
 * STATE.  T is one float4 plane per pixel, {r, g, b, N}: the resolved HDR colour and the number of frames it stands for.  There are TWO SETS, and
 *   a call reads one and writes the other: 32 bytes per pixel, allocated by the first call that passes its checks.  T is EMPTY before the first
 *   call, after arctic_taa_reset and after arctic_resize.
 * INPUTS.  The current HDR colour plane C (rows x width x 3 floats, row-major); optionally velocity2 as arctic_motion_vectors_device writes it
 *   (NULL: all zero); and ArcticTaa.  The resolve reads NO G-BUFFER: it works after every shading variant (image-based ambient, mip chains,
 *   material extras, spot and cube lights) and refuses none of them.
 * PER PIXEL p = (px, py); W and H are the frame size as floats.
 *   1. c = C[p].  The neighbourhood box: for dy = -1, 0, 1 and dx = -1, 0, 1, in that order, q = (clamp(px+dx, 0, W-1), clamp(py+dy, 0, H-1));
 *      lo and hi start at the first C[q] and fold per channel, lo = (x < lo) ? x : lo and hi = (x > hi) ? x : hi: a NaN neighbour is ignored.
 *   2. T is empty:  N = 1, out = c.
 *   3. Otherwise v = velocity2[p], or (0, 0).  hx = ((px + 0.5) + vx) + jx, hy likewise, j being ArcticTaa::jitter.  gx = hx - 0.5;
 *      ix = floor(gx); ax = gx - ix; y likewise.  Reject everything (N = 1, out = c) unless hx and hy are finite, -1 <= ix <= W-1 and
 *      -1 <= iy <= H-1, tested in float before any conversion.
 *   4. Four taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the weights (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax*ay.  A tap is accepted iff
 *      it lies inside the frame and its stored N_q > 0; a rejected tap is a SELECT: its weight is 0 and its history is not looked at.
 *      S = ((k0 + k1) + k2) + k3; R, G, B and Cn are the same ordered sums of k*r_q, k*g_q, k*b_q and k*N_q.
 *      If !(S > min_weight):  N = 1, out = c.
 *   5. Otherwise h = {R, G, B} / S and hn = Cn / S, then the clamp, per channel with selects: h = (h < lo) ? lo : h, then h = (h > hi) ? hi : h.
 *   6. N = min(hn + 1, max_history); a = 1 / N.
 *      Without ARCTIC_TAA_LUMA_WEIGHT:  out = h + (c - h) * a.
 *      With it:  wc = 1 / (1 + max(max(max(c.r, c.g), c.b), 0)), wh the same of h;  kc = a * wc;  kh = (1 - a) * wh;
 *        out = (c*kc + h*kh) / (kc + kh)  -- which keeps one HDR sample from owning an edge.
 *   7. Store {out, N}.  Then post_process of `out` under `settings`, as k_compose carries it out: float LDR and RGBA8.
 *   {out, N} is defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4 of the float64 post_process).
 * WHAT FOLLOWS.  On a still scene drawn with jitter j, velocity2 is -j and step 3 lands on the pixel's own centre: with max_history at or above
 *   the frame count and no luma weight, `out` is the running mean of the frames.
 * KNOWN LIMITS, stated and not worked around.  A pixel without geometry has velocity2 = 0, so the sky is not reprojected under camera rotation;
 *   the box clamp bounds what it keeps.  There is no sharpening (the motion blur is a stage of its own behind the resolve, below), and a shard cannot resolve (no halo exchange).
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing and leaves T as it was.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticTaa; unknown flag bits; a field outside the ranges below, or a NaN; a device plane that
 *     is misaligned: 4 bytes for C and RGBA8, 8 bytes for velocity2.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame (the taps' rows are elsewhere); and, with a NULL colour plane:
 *     ARCTIC_OPT_KEEP_FLOAT_OUTPUT off; no shading since it was turned on or since the last resize; under ARCTIC_TAA_SOURCE_COMPOSED no
 *     composition since the last resize; ARCTIC_OPT_HDR16 = 1. */
#define ARCTIC_TAA_LUMA_WEIGHT      1u
#define ARCTIC_TAA_SOURCE_COMPOSED  2u   /* C = the latest composition's HDR plane instead of the latest shading's */
typedef struct ArcticTaa {               /* 32 bytes */
    uint32_t flags;
    float max_history;                   /* 1..65536, finite; 1 = no accumulation */
    float min_weight;                    /* [0, 1) */
    float jitter[2];                     /* THIS frame's jitter, pixels, finite, |j| <= 1 */
    uint32_t reserved[3];                /* 0 */
} ArcticTaa;

/* One call of the definition on DEVICE planes, in the handle's rows.  d_hdr_rgb32f: rows*width*3 floats, NULL = the handle's own plane (the
 * latest shading's, or under ARCTIC_TAA_SOURCE_COMPOSED the latest composition's); d_velocity2: rows*width float2, NULL = zero; d_out_rgba8:
 * rows*width*4 bytes, NULL = the handle's own buffer (arctic_read_taa).  No plane may alias another.  Stream-ordered on the handle's stream; a
 * warm call allocates nothing and does not synchronise. */
int arctic_taa_resolve_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaa *taa, const float *d_hdr_rgb32f, const float *d_velocity2,
                              uint8_t *d_out_rgba8);

/* The host form: the same kernel from and to host memory (any pointer but settings and taa may be NULL, with the meanings above; a NULL output:
 * the result stays in the handle's buffers).  Synchronous. */
int arctic_taa_resolve(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaa *taa, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8);

/* The one call: arctic_motion_vectors_device into planes the handle owns, then the resolve on the handle's HDR plane with that velocity2.  Byte
 * for byte the two calls made by hand.  It is the frame's ONE motion call: a caller who also wants arctic_pass_ray_effects_motion drives the
 * calls by hand and shares the planes.  Every refusal of both calls comes before anything is enqueued. */
int arctic_pass_taa(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticTaa *taa, uint8_t *d_out_rgba8);

/* Empties T (the next call is a first call) and sets the calls counter to 0.  Frees nothing, touches no device. */
int arctic_taa_reset(ArcticRenderer *r);

/* What the latest resolve left, row-major whatever the layout on the device: float LDR and the resolved HDR colour (rows*width*3 floats each), N
 * (rows*width floats) and the handle's own RGBA8.  Any pointer may be NULL.  Synchronises.  ARCTIC_E_STATE while T is empty, and for rgba8 when
 * the latest resolve wrote the caller's buffer. */
int arctic_read_taa(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_taa_resolve, calls since the last reset, 0}.  All 0 until the
 * first call that passes its checks.  Touches no device. */
int arctic_taa_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter (no handle, no GPU): steps 1 to 6 for n pixels in any order, by the very functions the kernel runs.  pixel_xy: (px, py) per
 * pixel, inside the frame; cur_rgb: the WHOLE frame's C (height*width*3 floats, row-major); velocity2: n*2 floats, one per listed pixel, or NULL
 * = zero; prev_rgbn: the whole frame's previous T (height*width*4 floats, row-major) or NULL = T is empty; out_rgbn: n*4 floats {out, N}.
 * ARCTIC_E_INVALID (nothing written): what the resolve refuses of ArcticTaa, a frame size outside 1..16384, a pixel outside the frame, a null
 * array that is needed. */
int arctic_taa_pixels(const ArcticTaa *taa, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb, const float *velocity2,
                      const float *prev_rgbn, float *out_rgbn);

/* ---- motion blur: tile velocity maxima and a depth-aware gather (no counterpart in the reference) -------------------------------------------------
 * A fast object is smeared over the path it covered while the shutter was open: the reconstruction filter of McGuire et al., "A Reconstruction
 * Filter for Plausible Motion Blur" (2012) -- tile maximum, neighbourhood maximum, and a depth-aware gather with cone and cylinder weights --
 * restated so that it is defined bit for bit like every stage in front of the tonemapper here.  It reads the float HDR colour (the shading's, the
 * composition's, or the anti-aliasing's history), velocity2 of arctic_motion_vectors_device and the prepass depth.  Nothing in the passes or in
 * the other calls changes: a handle that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division and square root.
 * min(a, b) is (b < a) ? b : a and max(a, b) is (a < b) ? b : a.  clamp01(x) = !(x > 0) ? 0 : (x > 1 ? 1 : x): a NaN gives 0.
 * INPUTS.  C: the HDR colour, rows x width x 3 floats, row-major.  velocity2 as arctic_motion_vectors_device writes it (REQUIRED).  Depth: rows x
 *   width floats, smaller means nearer, in the units arctic_read_gbuffer returns (arctic_depth_plane_device); NULL: every pixel has depth 0.
 *   W and H are the frame size; a tile is 8 x 8 pixels, tile(p) = (px / 8, py / 8), and the tile grid is ceil(W / 8) x ceil(H / 8).
 *   1. HALF VELOCITY.  h_p = velocity2[p] * (0.5 * shutter) per component.  If either component of h_p is not finite, h_p = (0, 0).
 *      len = sqrt(hx*hx + hy*hy).  If len > max_radius:  s = max_radius / len,  h_p = h_p * s.  l2_p = hx*hx + hy*hy of the final h_p, and
 *      l_p = max(sqrt(l2_p), 0.5).  The prepared plane is P[p] = {l_p, z_p} (float2, row-major), z_p the pixel's depth.
 *   2. TILE MAXIMUM.  tile_max2[tile] = the h_p with the largest l2_p over the tile's pixels inside the frame; among equals the pixel with the
 *      lowest lane index (py & 7) * 8 + (px & 7) wins.
 *   3. NEIGHBOURHOOD MAXIMUM.  Rt = ceil(max_radius / 8) tiles.  neighbour_max2[(tx, ty)] = the tile_max2 with the largest hx*hx + hy*hy among
 *      the tiles (tx+dx, ty+dy), |dx|, |dy| <= Rt, that lie inside the tile grid, visited row-major (dy outer); the first among equals wins.
 *   4. THE GATHER, for pixel p = (px, py) with d = neighbour_max2[tile(p)] and dl = sqrt(dx*dx + dy*dy):
 *      If !(dl > 0.5):  out = C[p], bit for bit -- tiles that nothing fast can reach are copied.
 *      Otherwise w = 1 / l_p, acc = C[p] * w, and for i = 0 .. samples-1 in order:
 *        o = ((B[py & 3][px & 3] + 0.5) / 16) - 0.5 under ARCTIC_MB_DITHER, else 0; B is the 4 x 4 Bayer matrix with the rows
 *          {0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}.
 *        t = (((i + 0.5) + o) / samples) * 2 - 1.   sx = (px + 0.5) + t*dx, sy = (py + 0.5) + t*dy;  qx = floor(sx), qy = floor(sy).
 *        The tap is inside iff 0 <= qx <= W-1 and 0 <= qy <= H-1, tested in float before any conversion; a NaN fails.
 *        dist = |t| * dl.  With {l_q, z_q} = P[q]:
 *          f = clamp01(1 - (z_q - z_p) / depth_extent)          b = clamp01(1 - (z_p - z_q) / depth_extent)
 *          cone(l) = clamp01(1 - dist / l)
 *          cyl(l) = 1 - (s*s) * (3 - 2*s)  with  s = clamp01((dist - 0.95*l) / (0.1*l))
 *          a = (f * cone(l_q) + b * cone(l_p)) + (cyl(l_q) * cyl(l_p)) * 2
 *        A tap outside the frame is a SELECT with weight 0: nothing of it is read.  A tap whose a is not > 0 is a SELECT too: its colour does
 *        not enter, so a NaN colour never spreads through a zero weight.  Otherwise w = w + a and acc = acc + C[q] * a per channel.
 *      out = acc / w.
 *   5. Store out (float3, row-major).  Then post_process of `out` under `settings`, as k_compose and k_taa_resolve carry it out: float LDR and
 *      RGBA8.  tile_max2, neighbour_max2, P and out are defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4
 *      of the float64 post_process).
 * KNOWN LIMITS, stated and not worked around.  The depth is the prepass's non-linear depth, so depth_extent is in those units.  The sky has
 *   velocity2 = 0.  Only whole frames are handled: a shard's taps lie on other ranks, so a shard is refused as the resolve refuses it.  The
 *   minimum length 0.5 lets a still pixel inside a fast tile's window take up to one pixel of its neighbour along d: the paper's behaviour.
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticMotionBlur; unknown flag bits, or both source flags; a field outside the ranges below,
 *     or a NaN; a null velocity2; a device plane that is misaligned: 4 bytes for C, the depth and RGBA8, 8 bytes for velocity2.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame; and, with a NULL colour plane: under ARCTIC_MB_SOURCE_TAA an empty T
 *     (arctic_read_taa's condition) -- nothing else, the history is float whatever made it --, otherwise what arctic_taa_resolve_device refuses
 *     of the handle's HDR plane: ARCTIC_OPT_KEEP_FLOAT_OUTPUT off; no shading since it was turned on or since the last resize; under
 *     ARCTIC_MB_SOURCE_COMPOSED no composition since the last resize; ARCTIC_OPT_HDR16 = 1. */
#define ARCTIC_MB_DITHER           1u   /* the taps of a pixel are offset by its entry of the Bayer matrix */
#define ARCTIC_MB_SOURCE_COMPOSED  2u   /* a NULL colour = the latest composition's HDR plane instead of the latest shading's */
#define ARCTIC_MB_SOURCE_TAA       4u   /* a NULL colour = the anti-aliasing's history T; excludes ARCTIC_MB_SOURCE_COMPOSED */
typedef struct ArcticMotionBlur {       /* 32 bytes */
    uint32_t flags;
    float shutter;                      /* [0, 4], finite: the fraction of the frame interval that is exposed */
    float max_radius;                   /* [1, 64], finite: pixels */
    uint32_t samples;                   /* 1..64: taps per pixel */
    float depth_extent;                 /* > 0, finite: the soft extent of the depth comparison */
    uint32_t reserved[3];               /* 0 */
} ArcticMotionBlur;

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_mb_tile_max, k_mb_neighbour_max, k_motion_blur.
 * d_hdr_rgb32f: rows*width*3 floats, NULL = the handle's own plane per `flags`; d_velocity2: rows*width float2, required; d_depth: rows*width
 * floats, NULL = depth 0; d_out_rgba8: rows*width*4 bytes, NULL = the handle's own buffer (arctic_read_motion_blur).  No plane may alias
 * another.  Stream-ordered on the handle's stream; a warm call allocates nothing and does not synchronise. */
int arctic_motion_blur_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticMotionBlur *mb, const float *d_hdr_rgb32f, const float *d_velocity2,
                              const float *d_depth, uint8_t *d_out_rgba8);

/* The host form: the same kernels from and to host memory (hdr_rgb32f, depth and out_rgba8 may be NULL, with the meanings above; a NULL output:
 * the result stays in the handle's buffers).  Synchronous. */
int arctic_motion_blur(ArcticRenderer *r, const ArcticSettings *settings, const ArcticMotionBlur *mb, const float *hdr_rgb32f, const float *velocity2,
                       const float *depth, uint8_t *out_rgba8);

/* The visibility plane's depth of the handle's rows as a device plane: d_depth, rows*width floats, row-major, 4-byte aligned -- the values
 * arctic_read_gbuffer returns as `depth`, a pixel without geometry 1.0.  Stream-ordered.  ARCTIC_E_INVALID: a null handle or plane, or a
 * misaligned one.  ARCTIC_E_STATE: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none). */
int arctic_depth_plane_device(ArcticRenderer *r, float *d_depth);

/* The one call: arctic_motion_vectors_device, then arctic_depth_plane_device, then the blur of the handle's HDR plane, all on planes the handle
 * owns.  Byte for byte the calls made by hand.  It is then the frame's ONE motion call.  Under ARCTIC_MB_SOURCE_TAA it makes NO motion call:
 * it reads the velocity plane the latest arctic_pass_taa left in the handle, and returns ARCTIC_E_STATE unless the handle's latest
 * anti-aliasing call since the last resize or reset was arctic_pass_taa.  So blur behind anti-aliasing is: render, arctic_pass_taa,
 * arctic_pass_motion_blur with the flag -- and the frame still has one motion call.  Every refusal of every step comes before anything is
 * enqueued. */
int arctic_pass_motion_blur(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticMotionBlur *mb, uint8_t *d_out_rgba8);

/* What the latest blur left, row-major: float LDR and the blurred HDR colour (rows*width*3 floats each), the handle's own RGBA8, tile_max2 and
 * neighbour_max2 (one float2 per tile of the tile grid, row-major) and P (rows*width float2).  Any pointer may be NULL.  Synchronises.
 * ARCTIC_E_STATE before the first call and after a resize, and for rgba8 when the latest call wrote the caller's buffer. */
int arctic_read_motion_blur(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max2, float *neighbour_max2, float *prepared2);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_motion_blur, calls, 0}.  All 0 until the first call that
 * passes its checks.  Touches no device. */
int arctic_motion_blur_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiters (no handle, no GPU), by the very functions the kernels run.  arctic_motion_blur_prepare: steps 1 to 3 of a WHOLE frame --
 * velocity2 (height*width*2 floats), depth (height*width floats or NULL = 0) in; tile_max2, neighbour_max2 (2 floats per tile) and prepared2
 * (P: height*width*2 floats) out.  arctic_motion_blur_pixels: step 4 for n pixels in any order -- pixel_xy: (px, py) per pixel, inside the frame;
 * rgb: the WHOLE frame's C (height*width*3 floats, row-major); prepared2 and neighbour_max2 as the first writes them; out_rgb: n*3 floats.
 * ARCTIC_E_INVALID (nothing written): what the blur refuses of ArcticMotionBlur, a frame size outside 1..16384, a pixel outside the frame, a
 * null array that is needed. */
int arctic_motion_blur_prepare(const ArcticMotionBlur *mb, uint32_t width, uint32_t height, const float *velocity2, const float *depth, float *tile_max2,
                               float *neighbour_max2, float *prepared2);
int arctic_motion_blur_pixels(const ArcticMotionBlur *mb, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                              const float *prepared2, const float *neighbour_max2, float *out_rgb);

/* ---- depth of field: circle-of-confusion tile maxima and a disc gather (no counterpart in the reference) -------------------------------------------
 * The lens of the camera stage whose shutter is the motion blur above: a pixel away from the focus plane is spread over a disc whose radius
 * follows the thin lens, in front of the tonemapper and BEHIND the motion blur.  It reads the float HDR colour (the shading's, the
 * composition's, the anti-aliasing's history or the motion blur's output) and the prepass depth, nothing else.  Nothing in the passes or in the
 * other calls changes: a handle that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division and square root.
 * min, max and clamp01 are the motion blur's.  |x| clears the sign bit.
 * INPUTS.  C: the HDR colour, rows x width x 3 floats, row-major.  Depth: rows x width floats as arctic_depth_plane_device writes them
 *   (REQUIRED: without a depth there is nothing to focus on).  taps2: `samples` float2 offsets in the unit disc, HOST memory in every form of
 *   the call, as the occlusion's direction table is; renderer.py's dof_taps gives Vogel's spiral.  W and H are the frame size; a tile is 8 x 8
 *   pixels, tile(p) = (px / 8, py / 8), and the tile grid is ceil(W / 8) x ceil(H / 8).
 *   1. VIEW DISTANCE AND SIGNED RADIUS.  With n = z_near, f = z_far and d = depth[p]:  den = f - d * (f - n);  zv = (n * f) / den if den > 0,
 *      else zv = f (a NaN fails the test).  This inverts the camera's projection as the library draws it (perspectiveRH_ZO: a point at the
 *      distance `dist` along the view axis has the depth f / (f - n) * (1 - n / dist)), so zv is that distance; a pixel without geometry
 *      (depth 1.0) has zv = f up to rounding.
 *      s = coc_scale * (1 - focus_distance / zv): negative in front of the focus plane.  If s is not finite, s = 0.  Then
 *      s = min(max(s, -max_radius), max_radius).  a_p = max(|s_p|, A0) with A0 = 0.5641896f, which is 1 / sqrt(pi): a sharp pixel's disc has
 *      the area of one pixel.  The prepared plane is P[p] = {s_p, zv_p} (float2, row-major).
 *   2. TILE MAXIMUM.  tile_max[tile] = the largest |s_p| over the tile's pixels inside the frame: one float per tile.
 *   3. NEIGHBOURHOOD MAXIMUM.  Rt = ceil(max_radius / 8) tiles.  neighbour_max[(tx, ty)] = the largest tile_max among the tiles
 *      (tx+dx, ty+dy), |dx|, |dy| <= Rt, that lie inside the tile grid.
 *   4. THE GATHER, for pixel p = (px, py) with R = neighbour_max[tile(p)]:
 *      If !(R > 0.5):  out = C[p], bit for bit -- tiles that nothing out of focus can reach are copied.
 *      Otherwise k = (R * R) / samples, w = 0.31830987f / (a_p * a_p), acc = C[p] * w, entered = false, and for i = 0 .. samples-1 in order,
 *      with u = taps2[i]:
 *        ox = u.x * R, oy = u.y * R.   qx = floor((px + 0.5) + ox), qy = floor((py + 0.5) + oy).
 *        The tap is inside iff 0 <= qx <= W-1 and 0 <= qy <= H-1, tested in float before any conversion; a NaN fails.
 *        dist = sqrt(ox*ox + oy*oy).  With {s_q, z_q} = P[q] and a_q = max(|s_q|, A0):
 *          behind = clamp01((z_q - z_p) / depth_extent)
 *          e = a_q - behind * (a_q - min(a_q, a_p))
 *          cover = clamp01(e - dist)
 *          a = (cover * k) / (a_q * a_q)
 *        A tap behind the centre cannot spread further than the centre's own disc, so a blurred background does not bleed onto a sharp
 *        foreground; a blurred foreground does spread over a sharp background.  A tap stands for R*R*pi / samples of area and a disc of radius
 *        a_q has the density 1 / (pi * a_q * a_q): that is a; the centre is one pixel of area at its own density: that is the first w.
 *        A tap outside the frame is a SELECT: nothing of it is read.  A tap whose a is not > 0 is a SELECT too: its colour does not enter,
 *        so a NaN colour never spreads through a zero weight.  Otherwise w = w + a, acc = acc + C[q] * a per channel, entered = true.
 *      out = entered ? acc / w : C[p].  The second select makes "a pixel that nothing covers keeps its bits" exact.
 *   5. Store out (float3, row-major).  Then post_process of `out` under `settings`, as k_motion_blur carries it out: float LDR and RGBA8.
 *      tile_max, neighbour_max, P and out are defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4 of the
 *      float64 post_process).
 * KNOWN LIMITS, stated and not worked around.  The gather radius is the tile neighbourhood's, so a mildly blurred pixel near a strongly
 *   blurred one is sampled sparsely.  Weights are normalised, not alpha-composited.  The sky sits at about z_far.  Only whole frames are
 *   handled: a shard's taps lie on other ranks, so a shard is refused as the motion blur refuses it.
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticDof; unknown flag bits, or more than one source flag; a field outside the ranges
 *     below, or a NaN; a null depth; a null taps2, a tap with a component that is not finite or with x*x + y*y > 1 in fp32; a device plane
 *     that is misaligned: 4 bytes for C, the depth and RGBA8.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame; and, with a NULL colour plane: under ARCTIC_DOF_SOURCE_MOTION_BLUR no motion
 *     blur since the last resize (arctic_read_motion_blur's condition); under ARCTIC_DOF_SOURCE_TAA and ARCTIC_DOF_SOURCE_COMPOSED, and with
 *     no flag, what the motion blur refuses under ARCTIC_MB_SOURCE_TAA, ARCTIC_MB_SOURCE_COMPOSED and with no flag. */
#define ARCTIC_DOF_SOURCE_COMPOSED     1u   /* a NULL colour = the latest composition's HDR plane instead of the latest shading's */
#define ARCTIC_DOF_SOURCE_TAA          2u   /* a NULL colour = the anti-aliasing's history T */
#define ARCTIC_DOF_SOURCE_MOTION_BLUR  4u   /* a NULL colour = the latest motion blur's HDR output; at most one of the three */
typedef struct ArcticDof {                  /* 32 bytes */
    uint32_t flags;
    float focus_distance;                   /* > 0, finite: the view distance that is sharp */
    float coc_scale;                        /* [0, 4096], finite: pixels of radius at infinite distance (arctic_dof_coc_scale) */
    float max_radius;                       /* [1, 64]: pixels */
    uint32_t samples;                       /* 1..64: taps per pixel */
    float depth_extent;                     /* > 0, finite: the soft extent of the occlusion test, in view distance */
    float z_near;                           /* > 0: the camera's planes, as the frame was drawn with */
    float z_far;                            /* > z_near, finite */
} ArcticDof;

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_dof_prepare, k_dof_neighbour_max, k_dof_gather.
 * d_hdr_rgb32f: rows*width*3 floats, NULL = the handle's own plane per `flags`; d_depth: rows*width floats, required; taps2: samples float2
 * in HOST memory, read before the call returns and sent through the handle's staged-upload ring when it differs from the table last sent;
 * d_out_rgba8: rows*width*4 bytes, NULL = the handle's own buffer (arctic_read_dof).  No plane may alias another.  Stream-ordered on the
 * handle's stream; a warm call allocates nothing and does not synchronise. */
int arctic_dof_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticDof *dof, const float *d_hdr_rgb32f, const float *d_depth, const float *taps2,
                      uint8_t *d_out_rgba8);

/* The host form: the same kernels from and to host memory (hdr_rgb32f and out_rgba8 may be NULL, with the meanings above; a NULL output: the
 * result stays in the handle's buffers).  Synchronous. */
int arctic_dof(ArcticRenderer *r, const ArcticSettings *settings, const ArcticDof *dof, const float *hdr_rgb32f, const float *depth, const float *taps2, uint8_t *out_rgba8);

/* The one call: arctic_depth_plane_device into a plane the handle owns, then the gather of the handle's HDR plane per `flags`.  Byte for
 * byte the calls made by hand.  The block's z_near and z_far must both be 0 -- the call takes scene->camera.z_near_far, the planes the frame
 * was drawn with -- and only this call accepts zeros there.  Behind the motion blur: render, arctic_pass_motion_blur, arctic_pass_dof with
 * ARCTIC_DOF_SOURCE_MOTION_BLUR.  Every refusal of every step comes before anything is enqueued. */
int arctic_pass_dof(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticDof *dof, const float *taps2, uint8_t *d_out_rgba8);

/* What the latest call left, row-major: float LDR and the HDR colour (rows*width*3 floats each), the handle's own RGBA8, tile_max and
 * neighbour_max (one float per tile of the tile grid, row-major) and P (rows*width float2).  Any pointer may be NULL.  Synchronises.
 * ARCTIC_E_STATE before the first call and after a resize, and for rgba8 when the latest call wrote the caller's buffer. */
int arctic_read_dof(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max, float *neighbour_max, float *prepared2);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_dof_gather, calls, 0}.  All 0 until the first call that
 * passes its checks.  Touches no device. */
int arctic_dof_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiters (no handle, no GPU), by the very functions the kernels run.  arctic_dof_prepare: steps 1 to 3 of a WHOLE frame -- depth
 * (height*width floats) in; tile_max, neighbour_max (1 float per tile) and prepared2 (P: height*width*2 floats) out.  arctic_dof_pixels: step
 * 4 for n pixels in any order -- taps2: samples float2; pixel_xy: (px, py) per pixel, inside the frame; rgb: the WHOLE frame's C
 * (height*width*3 floats, row-major); prepared2 and neighbour_max as the first writes them; out_rgb: n*3 floats.  ARCTIC_E_INVALID (nothing
 * written): what the gather refuses of ArcticDof and of taps2, a frame size outside 1..16384, a pixel outside the frame, a null array that is
 * needed. */
int arctic_dof_prepare(const ArcticDof *dof, uint32_t width, uint32_t height, const float *depth, float *tile_max, float *neighbour_max, float *prepared2);
int arctic_dof_pixels(const ArcticDof *dof, const float *taps2, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                      const float *prepared2, const float *neighbour_max, float *out_rgb);

/* The thin lens in pixels -- a pure host function, no handle: the radius of the circle of confusion of a point at infinite distance, which is
 * ArcticDof::coc_scale.  In fp32, in this order, with focus_distance in metres:  fl = focal_length_mm * 0.001;
 * c = (fl * fl) / (f_number * (focus_distance - fl))  [the diameter on the sensor, metres];
 * *out = ((0.5 * c) / (sensor_height_mm * 0.001)) * height_px.  A point at the distance D then has the radius *out * |1 - focus_distance / D|:
 * step 1's s.  ARCTIC_E_INVALID (nothing written): a null out; f_number, focal_length_mm or sensor_height_mm not finite and above 0;
 * height_px outside 1..16384; focus_distance not finite or not above fl; a result that is not finite. */
int arctic_dof_coc_scale(float f_number, float focal_length_mm, float sensor_height_mm, float focus_distance, uint32_t height_px, float *out);

/* Autofocus: step 1's zv of pixel (px, py) of the handle's rows (py counts from the handle's first row) of the resident visibility plane,
 * under the planes z_near and z_far.  Synchronises.  ARCTIC_E_INVALID: a null handle or distance, planes outside ArcticDof's ranges, a pixel
 * outside the handle's rows.  ARCTIC_E_STATE: no visibility plane (arctic_depth_plane_device's condition). */
int arctic_dof_focus_at(ArcticRenderer *r, float z_near, float z_far, uint32_t px, uint32_t py, float *distance);

/* ---- bloom: a thresholded mip pyramid composed in front of the tonemapper (no counterpart in the reference) ----------------------------------------
 * The glow of the lens: what is brighter than a threshold is spread over a pyramid of ever coarser planes and added back, the LAST stage in
 * front of the tonemapper, BEHIND the depth of field.  The filters are Jimenez's ("Next Generation Post Processing in Call of Duty: Advanced
 * Warfare", 2014): a 13-tap downsample with Karis' luminance weights on the first level, and a 3 x 3 tent on the way up -- restated on integer
 * texels so that they are defined bit for bit like every stage in front of the tonemapper here.  It reads the float HDR colour (the shading's,
 * the composition's, the anti-aliasing's history, the motion blur's or the depth of field's output), nothing else.  Nothing in the passes or
 * in the other calls changes: a handle that never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division.
 * min and max are the motion blur's.  Every clamp(i, lo, hi) of an index is an integer clamp.
 * INPUTS.  C: the HDR colour, rows x width x 3 floats, row-major.  The frame is W x H.  Level sizes: W_0 = W, H_0 = H,
 *   W_k = (W_{k-1} + 1) / 2, H_k = (H_{k-1} + 1) / 2 in integer division; a level of 1 x 1 is valid, and so is every level below it.
 *   `levels` is L, 1..8.  Every plane of the pyramid is row-major float3.
 *   1. PREFILTER, per pixel q of the frame.  Per channel x = C[q] > 0 ? min(C[q], clamp_max) : 0 -- a NaN fails the test and becomes 0, +inf
 *      becomes clamp_max, a negative value becomes 0.  br = max(x.r, max(x.g, x.b)).  knee = threshold * soft_knee.
 *      t = br - (threshold - knee).  t = min(max(t, 0), 2 * knee).  soft = (t * t) / (4 * knee + 1e-5f).  m = max(soft, br - threshold).
 *      contrib = min(m / max(br, 1e-5f), 1).  b[q] = x * contrib per channel.
 *   2. DOWN(S, Ws, Hs) at destination pixel (x, y).  The footprint is S~(i, j) = S[clamp(2x - 2 + i, 0, Ws - 1), clamp(2y - 2 + j, 0, Hs - 1)],
 *      i, j = 0..5.  Box(a, b) = ((S~(a,b) + S~(a+1,b)) + (S~(a,b+1) + S~(a+1,b+1))) * 0.25.
 *      Group(a, b) = ((Box(a,b) + Box(a+2,b)) + (Box(a,b+2) + Box(a+2,b+2))) * 0.25.
 *      G0 = Group(1,1), G1 = Group(0,0), G2 = Group(2,0), G3 = Group(0,2), G4 = Group(2,2): the 13 bilinear taps of Jimenez's downsample on
 *      integer texels, 36 texels and 13 distinct boxes.
 *      Plain form: out = G0 * 0.5 + ((G1 + G2) + (G3 + G4)) * 0.125.
 *      Karis form, for the first level only, to suppress fireflies: l_g = (0.2126f * G.r + 0.7152f * G.g) + 0.0722f * G.b;
 *      w_0 = 0.5f / (1 + l_0), w_g = 0.125f / (1 + l_g) for g = 1..4; num = w_0 * G0 + ((w_1 * G1 + w_2 * G2) + (w_3 * G3 + w_4 * G4));
 *      den = w_0 + ((w_1 + w_2) + (w_3 + w_4)); out = num / den.
 *      D_1 = DOWN_karis(b, W, H), and D_k = DOWN(D_{k-1}, W_{k-1}, H_{k-1}) for k = 2..L.
 *   3. UP(T, Wt, Ht) at destination pixel (x, y) of the next finer level.  With h = x >> 1: even x has base = h - 2 and
 *      wx = (0.0625f, 0.3125f, 0.4375f, 0.1875f); odd x has base = h - 1 and wx = (0.1875f, 0.4375f, 0.3125f, 0.0625f).  The same rule
 *      applies in y.  This is the 3 x 3 tent of bilinear taps one coarse texel apart, restated; its weights are exact sixteenths.
 *      T~(i, j) = T[clamp(bx + i, 0, Wt - 1), clamp(by + j, 0, Ht - 1)], i, j = 0..3.
 *      r_j = (wx0 * T~(0,j) + wx1 * T~(1,j)) + (wx2 * T~(2,j) + wx3 * T~(3,j)).  out = (wy0 * r_0 + wy1 * r_1) + (wy2 * r_2 + wy3 * r_3).
 *      U_L = D_L.  For k = L-1 .. 1, U_k = D_k + spread * UP(U_{k+1}) at level k's size.
 *   4. COMPOSITE, per pixel p.  B = UP(U_1, W_1, H_1) at the frame's size.  a = intensity * B per channel.  out = a > 0 ? C[p] + a : C[p].
 *      The composite is a SELECT, so a pixel that no bloom reaches keeps its bits, a NaN included.
 *   5. Store out (float3, row-major).  Then post_process of `out` under `settings`, exactly as k_dof_gather carries it out: float LDR and
 *      RGBA8.  The D_k, U_k and out are defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4 of the
 *      float64 post_process).
 * EXACT PROPERTIES.  Every D_k and U_k is finite and >= 0 whatever C holds: step 1 removes NaN, infinity and negatives, and everything after
 *   it is a bounded sum.  If every pixel has br <= threshold - knee, every plane is +0 and out equals C by bits.
 * KNOWN LIMITS, stated and not worked around.  The footprint is corner-centred, so a single pixel's glow is not symmetric about it.  There is
 *   no lens dirt and no per-level tint.  Only whole frames are handled: a shard's footprint lies on other ranks, so a shard is refused as the
 *   blur and the lens refuse it.
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticBloom; unknown flag bits, or more than one source flag; a field outside the ranges
 *     below, or a NaN; reserved != 0; a device plane that is misaligned: 4 bytes for C and RGBA8.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame; and, with a NULL colour plane: under ARCTIC_BLOOM_SOURCE_DOF no depth of field
 *     since the last resize (arctic_read_dof's condition); under the other three flags and with no flag, what arctic_dof_device refuses under
 *     ARCTIC_DOF_SOURCE_MOTION_BLUR, ARCTIC_DOF_SOURCE_TAA, ARCTIC_DOF_SOURCE_COMPOSED and with no flag. */
#define ARCTIC_BLOOM_SOURCE_COMPOSED     1u   /* a NULL colour = the latest composition's HDR plane instead of the latest shading's */
#define ARCTIC_BLOOM_SOURCE_TAA          2u   /* a NULL colour = the anti-aliasing's history T */
#define ARCTIC_BLOOM_SOURCE_MOTION_BLUR  4u   /* a NULL colour = the latest motion blur's HDR output */
#define ARCTIC_BLOOM_SOURCE_DOF          8u   /* a NULL colour = the latest depth of field's HDR output; at most one of the four */
#define ARCTIC_BLOOM_MAX_LEVELS          8u
typedef struct ArcticBloom {                  /* 32 bytes */
    uint32_t flags;
    float threshold;                          /* [0, 65504], finite: the brightness where the glow begins */
    float soft_knee;                          /* [0, 1]: the part of the threshold below it over which the glow fades in */
    float clamp_max;                          /* (0, 65504]: no channel enters the pyramid above it */
    float intensity;                          /* [0, 16]: the composite's factor */
    float spread;                             /* [0, 1]: what every coarser level adds to the next finer one */
    uint32_t levels;                          /* 1..8: L */
    uint32_t reserved;                        /* must be 0 */
} ArcticBloom;

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_bloom_down_first, L-1 times k_bloom_down, L-1 times
 * k_bloom_up, k_bloom_composite -- 2L launches.  d_hdr_rgb32f: rows*width*3 floats, NULL = the handle's own plane per `flags`;
 * d_out_rgba8: rows*width*4 bytes, NULL = the handle's own buffer (arctic_read_bloom).  No plane may alias another.  Stream-ordered on the
 * handle's stream; a warm call allocates nothing and does not synchronise. */
int arctic_bloom_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticBloom *bloom, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8);

/* The host form: the same kernels from and to host memory (hdr_rgb32f and out_rgba8 may be NULL, with the meanings above; a NULL output: the
 * result stays in the handle's buffers).  Synchronous. */
int arctic_bloom(ArcticRenderer *r, const ArcticSettings *settings, const ArcticBloom *bloom, const float *hdr_rgb32f, uint8_t *out_rgba8);

/* What the latest call left, row-major: float LDR and `out` (rows*width*3 floats each), the handle's own RGBA8, and the two pyramids as
 * arctic_bloom_layout packs them for that call's `levels`: `down` holds D_1 .. D_L and `up` holds U_1 .. U_{L-1} (U_L is D_L; nothing is
 * written to `up` when L = 1).  Any pointer may be NULL.  Synchronises.  ARCTIC_E_STATE before the first call and after a resize, and for
 * rgba8 when the latest call wrote the caller's buffer. */
int arctic_read_bloom(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *down, float *up);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_bloom_composite, calls, 0}.  All 0 until the first call
 * that passes its checks.  Touches no device. */
int arctic_bloom_info(ArcticRenderer *r, uint64_t *out4);

/* The pyramid's layout -- a pure host function, no handle.  out: 3 * levels + 2 numbers: {W_k, H_k, offset_k} for k = 1 .. levels, where
 * offset_k counts FLOATS from the start of `down` to D_k (the levels are packed in level order, W_k * H_k * 3 floats each), then the floats
 * of `down` and the floats of `up`.  U_k lies at offset_k of `up`.  ARCTIC_E_INVALID (nothing written): a null out, a frame size outside
 * 1..16384, levels outside 1..8. */
int arctic_bloom_layout(uint32_t width, uint32_t height, uint32_t levels, uint64_t *out);

/* The host arbiters (no handle, no GPU), by the very functions the kernels run.  arctic_bloom_pyramid: steps 1 to 3 of a WHOLE frame -- rgb
 * (height*width*3 floats) in; `down` and `up` out, as arctic_bloom_layout packs them (`up` may be NULL when levels = 1).
 * arctic_bloom_pixels: step 4 for n pixels in any order -- pixel_xy: (px, py) per pixel, inside the frame; rgb: the WHOLE frame's C; up1: U_1
 * (H_1*W_1*3 floats; D_1 when levels = 1); out_rgb: n*3 floats.  ARCTIC_E_INVALID (nothing written): what the call refuses of ArcticBloom, a
 * frame size outside 1..16384, a pixel outside the frame, a null array that is needed. */
int arctic_bloom_pyramid(const ArcticBloom *bloom, uint32_t width, uint32_t height, const float *rgb, float *down, float *up);
int arctic_bloom_pixels(const ArcticBloom *bloom, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb, const float *up1,
                        float *out_rgb);

/* ---- auto-exposure: a luminance histogram, eye adaptation and the exposed frame in front of the tonemapper (no counterpart in the reference) -----
 * The meter of the chain: the frame's luminance is binned into a 256-bin histogram, a percentile band of it gives a mean log luminance, the
 * mean is adapted over time, and the frame is multiplied by the exposure E that maps the adapted luminance to `key_value` -- the LAST stage in
 * front of the tonemapper, BEHIND bloom.  It reads the float HDR colour (the shading's, the composition's, the anti-aliasing's history, the
 * motion blur's, the depth of field's or bloom's output), nothing else.  The histogram, the adapted state and E stay in device memory: the
 * three launches of a call are stream-ordered and nothing is read back.  Nothing in the passes or in the other calls changes: a handle that
 * never makes these calls renders the same bytes and allocates nothing for them.
 *
 * THE DEFINITION.  Bit for bit: fp32 unless marked binary64, one rounding per operation in the written order, no contraction, IEEE division.
 * There is no transcendental in it: the logarithm and its inverse are the float's own bit pattern.  min and max are the motion blur's.
 * INPUTS.  C: the HDR colour, rows x width x 3 floats, row-major.  The frame is W x H.  The metering window is [x0, x1) x [y0, y1): the
 *   record's `window`, or the whole frame when all four are zero.  The state record (ArcticExposureState) of the handle, valid or not.
 *   1. METER, per pixel q inside the window.  Per channel x = C[q] > 0 ? min(C[q], 65504.0f) : 0 -- a NaN fails the test and becomes 0, +inf
 *      becomes 65504, a negative value becomes 0.  l = (0.2126f * x.r + 0.7152f * x.g) + 0.0722f * x.b.  key = bits(l) >> 20: the sign is 0, so
 *      keys are monotone in l, 8 keys per octave.  bin = clamp(key - 888, 0, 255) as an integer clamp; 888 = (127 - 16) * 8.  Bin 0 is "black",
 *      everything below 1.125 * 2^-16; bin 255 ends just under 2^16, which 65504 cannot exceed.  H[bin] += 1, H being uint32[256]: the counts
 *      are integers, so H does not depend on the order of the additions or on the launch geometry.
 *   2. RESOLVE.  Under ARCTIC_EXPOSURE_SKIP_BLACK H' is H with H'[0] = 0, otherwise H' = H.  N = sum H' in uint64.
 *      lo = (N * low_q16) >> 16 and hi = (N * high_q16) >> 16.  P_0 = 0, P_{b+1} = P_b + H'[b].
 *      c_b = max(0, min(P_{b+1}, hi) - max(P_b, lo)): the pixels of bin b whose rank lies in [lo, hi).  M = sum c_b and S = sum b * c_b, uint64.
 *      If M == 0 there is no measurement: adapted_key, luminance, valid and frames of the state are left as they are (an invalid state stays
 *      invalid, with adapted_key = 0 and luminance = 0), metered = 0, and E = min(max(fallback_exposure, min_exposure), max_exposure).
 *      Otherwise, in binary64: m = (double)S / (double)M and a_t = m + 888.5.  If the state is invalid or ARCTIC_EXPOSURE_RESET is set, a = a_t
 *      and frames = 1.  Else rate = a_t > a_prev ? rate_up : rate_down, a = a_prev + (a_t - a_prev) * (double)rate -- two roundings, no fma --
 *      and frames += 1.  L = float_from_bits((uint32)(a * 1048576.0)): the product is exact and the cast truncates; L is the float whose key is
 *      the adapted mean key, at the middle of its bin.  E = min(max(key_value / L, min_exposure), max_exposure).
 *      The state becomes {adapted_key = a, exposure = E, luminance = L, metered = M saturated at 2^32 - 1, valid = 1, frames, reserved = 0}.
 *   3. APPLY, per pixel of the WHOLE frame, not the window.  out = C * E per channel: one multiply; a NaN stays a NaN, a -0 stays a -0.
 *      Store out (float3, row-major).  Then post_process of `out` under `settings`, exactly as k_bloom_composite ends: float LDR and RGBA8.
 *      settings->exposure keeps its meaning for tm_exposure and is independent of E.
 *   H, the state and out are defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4 of the float64
 *   post_process of the kernel's own out, RGBA8 within one step).
 * EXACT PROPERTIES.  (i) H sums to the window's pixel count whatever C holds.  (ii) Scaling a frame by 2^k shifts every key by 8k; when no
 *   pixel touches bin 0, bin 255 or the 65504 clamp before or after and ARCTIC_EXPOSURE_RESET is set, a_t shifts by 8k (exactly when M is a
 *   power of two, else to the last place of the binary64 division), L scales by exactly 2^k, E by exactly 2^-k, and out is the same bytes.  (iii) A constant grey l inside the range gives |L / l - 1| <= 1/16: L is the
 *   middle of l's bin.  (iv) The state after n calls on one frame is binary64 arithmetic; a moves monotonically towards a_t.
 * KNOWN LIMITS, stated and not worked around.  The logarithm is piecewise linear, at most 0.0861 octaves off log2; with the bin's half width
 *   L lies within 2^(2 * 0.0861 + 1/16) = 1.177 of the true geometric mean of the band.  Adaptation is linear in the key domain at the
 *   caller's per-frame rates (arctic_exposure_rate is the convenience).  Metering is uniform inside the window.  Bloom's threshold is applied
 *   in front of this stage, so it sees unexposed radiance.  Only whole frames are handled: a shard is refused as the blur, the lens and bloom
 *   refuse it.
 * FLAGS.  ARCTIC_EXPOSURE_HOLD: no meter and no resolve, the E the latest metering call left is applied with one launch.
 *   ARCTIC_EXPOSURE_METER_ONLY: no apply, and no output plane is allocated or written -- for a host that feeds E to its own tonemapper.
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing, the state included.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticExposure; unknown flag bits, or more than one source flag; ARCTIC_EXPOSURE_HOLD
 *     together with ARCTIC_EXPOSURE_METER_ONLY or ARCTIC_EXPOSURE_RESET; a field outside the ranges below, or a NaN; a window that is neither
 *     all zero nor inside the frame; reserved != 0; a device plane that is misaligned: 4 bytes for C and RGBA8.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame; with a NULL colour plane: under ARCTIC_EXPOSURE_SOURCE_BLOOM no bloom since
 *     the last resize (arctic_read_bloom's condition); under the other four flags and with no flag, what arctic_bloom_device refuses under
 *     ARCTIC_BLOOM_SOURCE_DOF, _MOTION_BLUR, _TAA, _COMPOSED and with no flag; and under ARCTIC_EXPOSURE_HOLD: no metering call since the
 *     handle was created, since arctic_exposure_reset or since the last resize. */
#define ARCTIC_EXPOSURE_SOURCE_COMPOSED     1u   /* a NULL colour = the latest composition's HDR plane instead of the latest shading's */
#define ARCTIC_EXPOSURE_SOURCE_TAA          2u   /* a NULL colour = the anti-aliasing's history T */
#define ARCTIC_EXPOSURE_SOURCE_MOTION_BLUR  4u   /* a NULL colour = the latest motion blur's HDR output */
#define ARCTIC_EXPOSURE_SOURCE_DOF          8u   /* a NULL colour = the latest depth of field's HDR output */
#define ARCTIC_EXPOSURE_SOURCE_BLOOM        16u  /* a NULL colour = the latest bloom's HDR output; at most one of the five */
#define ARCTIC_EXPOSURE_SKIP_BLACK          32u  /* bin 0 does not count */
#define ARCTIC_EXPOSURE_RESET               64u  /* this call adapts at once: a = a_t */
#define ARCTIC_EXPOSURE_HOLD                128u /* apply the held E; nothing is metered */
#define ARCTIC_EXPOSURE_METER_ONLY          256u /* meter and resolve; nothing is applied */
typedef struct ArcticExposure {                  /* 56 bytes */
    uint32_t flags;
    uint32_t low_q16;                            /* 0 <= low_q16 < high_q16 <= 65536: the percentile band in 1/65536 */
    uint32_t high_q16;
    float key_value;                             /* (0, 65504]: the mid grey the mean luminance is mapped to, exposure compensation folded in */
    float min_exposure;                          /* 0 < min_exposure <= max_exposure <= 65504 */
    float max_exposure;
    float rate_up;                               /* [0, 1]: the part of the way a moves per call when a_t lies above it */
    float rate_down;                             /* [0, 1]: ... and when it does not */
    float fallback_exposure;                     /* (0, 65504]: E of a call that measured nothing */
    uint32_t window[4];                          /* x0, y0, x1, y1; all zero = the whole frame; else x0 < x1 <= W, y0 < y1 <= H */
    uint32_t reserved;                           /* must be 0 */
} ArcticExposure;
typedef struct ArcticExposureState {             /* 32 bytes, on the device */
    double adapted_key;                          /* a */
    float exposure;                              /* E of the latest metering call */
    float luminance;                             /* L */
    uint32_t metered;                            /* M of the latest metering call, saturated */
    uint32_t valid;                              /* a and L hold a measurement */
    uint32_t frames;                             /* measurements folded into a since it last began at a_t */
    uint32_t reserved;
} ArcticExposureState;

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_exposure_meter, k_exposure_resolve, k_exposure_apply
 * (HOLD: the last alone; METER_ONLY: the first two).  d_hdr_rgb32f: rows*width*3 floats, NULL = the handle's own plane per `flags`;
 * d_out_rgba8: rows*width*4 bytes, NULL = the handle's own buffer (arctic_read_exposure).  No plane may alias another.  Stream-ordered on
 * the handle's stream; a warm call allocates nothing and does not synchronise. */
int arctic_exposure_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticExposure *exposure, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8);

/* The host form: the same kernels from and to host memory (hdr_rgb32f and out_rgba8 may be NULL, with the meanings above; a NULL output: the
 * result stays in the handle's buffers).  Synchronous. */
int arctic_exposure(ArcticRenderer *r, const ArcticSettings *settings, const ArcticExposure *exposure, const float *hdr_rgb32f, uint8_t *out_rgba8);

/* What the latest calls left: float LDR and `out` (rows*width*3 floats each) and the handle's own RGBA8 of the latest call that applied; H
 * (256 counts) and the state record of the latest call that metered.  Any pointer may be NULL.  Synchronises.  ARCTIC_E_STATE: nothing of
 * what is asked for since the handle was created, arctic_exposure_reset or the last resize; and for rgba8 when the latest call wrote the
 * caller's buffer. */
int arctic_read_exposure(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, uint32_t *hist256, ArcticExposureState *state);

/* Forgets the adaptation: the next metering call starts from an invalid state, and ARCTIC_EXPOSURE_HOLD is refused until then.  Nothing is
 * enqueued and nothing freed. */
int arctic_exposure_reset(ArcticRenderer *r);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_exposure_apply, calls, launches of k_exposure_meter}.
 * All 0 until the first call that passes its checks.  Touches no device. */
int arctic_exposure_info(ArcticRenderer *r, uint64_t *out4);

/* The meter's launch geometry -- a pure host function, no handle.  out3 = {G: the workgroups of k_exposure_meter and the rows of its partials
 * table T[G][256], the pixels a workgroup takes per trip of its loop, the bytes of T}.  ARCTIC_E_INVALID (nothing written): a null out3, a
 * frame size outside 1..16384. */
int arctic_exposure_layout(uint32_t width, uint32_t height, uint64_t *out3);

/* The per-call rate of an adaptation of `speed` per second over a frame of dt seconds: 1 - exp(-dt * speed) as a float, clamped to [0, 1]
 * (a NaN: 0).  A pure host function. */
float arctic_exposure_rate(float dt, float speed);

/* The host arbiters (no handle, no GPU), by the very functions the kernels run.  arctic_exposure_histogram: step 1 of a WHOLE frame -- rgb
 * (height*width*3 floats) in, H (256 counts) out.  arctic_exposure_resolve: step 2 -- H and the state in front of the call (NULL: invalid) in,
 * the state behind it out.  arctic_exposure_pixels: step 3's multiply for n pixels -- rgb and out_rgb: n*3 floats.  ARCTIC_E_INVALID
 * (nothing written): what the call refuses of ArcticExposure (arctic_exposure_resolve takes any window a frame of 16384 x 16384 admits), a
 * frame size outside 1..16384, a null array that is needed. */
int arctic_exposure_histogram(const ArcticExposure *exposure, uint32_t width, uint32_t height, const float *rgb, uint32_t *hist256);
int arctic_exposure_resolve(const ArcticExposure *exposure, const uint32_t *hist256, const ArcticExposureState *previous, ArcticExposureState *state);
int arctic_exposure_pixels(uint64_t n, const float *rgb, float exposure, float *out_rgb);

/* ---- Volumetric fog: sun shafts marched through the sun's shadow map (no counterpart in the reference) ------------------------------------------
 * The first stage behind the shading or the composition and in front of the anti-aliasing: a homogeneous participating medium lit by the sun.
 * Every pixel's view ray is marched from the eye to its surface in `steps` samples; each sample asks the sun's shadow map whether it is lit.
 * The stages behind it have no flag for it: the calls take an optional caller-owned HDR output plane, and that plane is chained into
 * arctic_taa_resolve_device, arctic_motion_blur_device and the rest through their explicit colour argument.
 *
 * THE DEFINITION.  Bit for bit: fp32, one rounding per operation in the written order, no contraction (no fma), IEEE division and square root,
 * no library transcendental.  min(a, b) is b < a ? b : a.
 * INPUTS.  C: the float HDR colour, row-major, 3 floats per pixel.  depth: the prepass depth plane (arctic_depth_plane_device), one float per
 *   pixel; a NULL plane means every depth is 1.0.  The sun's map: S x S floats, row-major; S = 0 means no map, and every sample is lit.
 *   offsets16: a caller's HOST table of 16 floats in [0, 1), interleaved over 4 x 4 pixels: pixel (px, py) uses entry (py & 3) * 4 + (px & 3);
 *   NULL means every entry is 0.5.  The two records below; N = steps, g = anisotropy.
 * 1. RAY.  fx = px + 0.5, fy = py + 0.5.  Per component D = (ray00 + fx * ray_dx) + fy * ray_dy.  len = sqrt((D.x*D.x + D.y*D.y) + D.z*D.z).
 *   zv = the depth of field's view distance of `depth` under z_near and z_far: den = z_far - depth * (z_far - z_near), zv = den > 0 ?
 *   (z_near * z_far) / den : z_far, so a NaN depth gives z_far.  z_end = min(zv, max_distance).  dz = z_end / (float)N.
 * 2. EXTINCTION.  x = -((density * 1.442695f) * len) * dz.  a = fog_exp2(x).  T_0 = 1, and T_{k+1} = T_k * a.
 *   fog_exp2(x) for x <= 0: x = x > -126 ? x : -126 (a NaN becomes -126); n = floor(x); f = x - n, which lies in [0, 1], and 1 is reached
 *   after rounding; p = Horner from the top with separate multiply and add, ((((((c6 * f + c5) * f + c4) * f + c3) * f + c2) * f + c1) * f + c0,
 *   c0..c6 = 0x1p+0, 0x1.62e428p-1, 0x1.ebfdf2p-3, 0x1.c67f5p-5, 0x1.3d54d8p-7, 0x1.44d4d2p-10, 0x1.ca8f0ap-13;
 *   r = float_from_bits(bits(p) + (n << 23)) in two's complement; a = min(r, 1.0f).  Over every float f of [0, 1] p differs from 2^f by at most
 *   8.4e-8 relative and lies in [1, 2]; the test holds 1.2e-7 and 1 <= p < 4, which the bit addition needs (tests/test_fog_reference.py).
 * 3. MARCH, for k = 0 .. N-1.  z = ((float)k + offset) * dz.  Per component P = eye + D * z.
 *   u = ((light[0][0]*P.x + light[0][1]*P.y) + light[0][2]*P.z) + light[0][3]; v and w likewise from rows 1 and 2.
 *   tu = floor(u * (float)S), tv = floor(v * (float)S).  The sample is inside when tu >= 0 && tu <= S-1 && tv >= 0 && tv <= S-1 && !(w > 1.0f);
 *   a NaN fails, and nothing is read.  Inside: V_k = (w - bias > map[tv][tu]) ? 0 : 1.  Outside, or with S = 0: V_k = 1.
 *   I = I + V_k * (T_k - T_{k+1}), as a select on V_k, in order of k from I = 0.
 * 4. PHASE AND OUTPUT.  cos_t = -((D.x*sun_dir.x + D.y*sun_dir.y) + D.z*sun_dir.z) / len.  q = (1 + g*g) - (2*g) * cos_t.
 *   ph = ((1 - g*g) * 0.07957747f) / (q * sqrt(q)) (Henyey-Greenstein).  T = T_N.  If !(T < 1.0f): out = C by bits -- zero density, zero
 *   length and a NaN T.  Otherwise per channel out = (C * T + (scatter_color * ph) * I) + ambient_color * (1 - T).
 *   Then the tonemapper of `out` exactly as k_dof_gather carries it out: float HDR, float LDR and RGBA8.
 * EXACT PROPERTIES.  a <= 1, so the T_k never rise and every term of I is >= 0.  0 <= I <= 1 - T up to the sum's rounding.  Density 0 returns
 *   C by bits, NaN and -0 included (for a finite len).  A NaN in C stays in its own pixel: the stage reads no neighbour.  No lookup is made
 *   outside the map for any light rows or any view record.
 * KNOWN LIMITS, stated and not worked around.  Homogeneous medium.  Single scattering from the sun only: point, spot and cube-shadow lights do
 *   not light the fog.  One nearest-texel compare per sample.  The ray ignores the anti-aliasing's sub-pixel jitter.  Whole frames only: a
 *   shard is refused with ARCTIC_E_STATE.  ARCTIC_OPT_HDR16 is refused (ARCTIC_E_STATE) when the colour is the handle's.
 * REFUSALS, all ARCTIC_E_INVALID, in this order, and every refusal comes before anything is enqueued: a null argument; unknown flag bits; a
 *   field out of range or NaN; reserved != 0 or a pad that is not 0; a view record that is not finite or has z_near >= z_far (or z_near <= 0);
 *   an offset outside [0, 1); a misaligned plane.  Then ARCTIC_E_STATE: a shard; with a NULL colour no float HDR plane of this size (or none
 *   composed under the flag); a sun map (shadow_size != 0) that is sharded or was never drawn or written, the rule of arctic_shade_hits.  A
 *   refused call writes nothing and leaves the counters and buffers as they were. */
#define ARCTIC_FOG_SOURCE_COMPOSED 1u                /* a NULL colour = the composition's HDR plane, not the shading's */
typedef struct ArcticFog {                       /* 52 bytes */
    uint32_t flags;
    float density;                               /* [0, 64]: sigma, the extinction per world unit */
    float anisotropy;                            /* [-0.95, 0.95]: g of the phase function; above 0 scatters forward */
    float max_distance;                          /* (0, 65504]: the march ends here, in view distance */
    uint32_t steps;                              /* 1..128: N */
    float bias;                                  /* [0, 1]: in shadow-map depth */
    float scatter_color[3];                      /* [0, 65504]: the single-scattering albedo times the sun's radiance; the caller sets it */
    float ambient_color[3];                      /* [0, 65504]: what the medium emits or in-scatters from the sky */
    uint32_t reserved;                           /* must be 0 */
} ArcticFog;
typedef struct ArcticFogView {                   /* 128 bytes; every field finite, the pads 0, 0 < z_near < z_far */
    float eye[3];
    float z_near;
    float ray00[3];                              /* the ray of the frame's corner (0, 0), at view distance 1 */
    float z_far;
    float ray_dx[3];                             /* ... and what a pixel to the right adds */
    float pad0;
    float ray_dy[3];                             /* ... and a pixel down */
    float pad1;
    float sun_dir[3];                            /* the direction in which the light travels, of length 1 */
    float pad2;
    float light[3][4];                           /* three affine rows: a world point to the map's (u, v, depth) */
} ArcticFogView;

/* The view record of a scene's camera and sun for a width x height frame -- a pure host function, no handle.  The formulas are those of the
 * camera's and the sun's matrices (perspectiveRH_ZO * lookAtRH, orthoRH_ZO(-16, 16, -16, 16, 0.1, 50) * lookAtRH) on the fp32 direction the
 * library derives from the rotations, evaluated in binary64 and rounded once to fp32.  D at view distance 1 is f + x_ndc * aspect *
 * tan(fov_y / 2) * s + y_ndc * tan(fov_y / 2) * u with x_ndc = 2 fx / width - 1 and y_ndc = 1 - 2 fy / height, which falls as py rises.
 * light row 0 is 0.5 * clip_x + 0.5, row 1 is 0.5 - 0.5 * clip_y, row 2 is clip_z.  ARCTIC_E_INVALID (nothing written): a null pointer, a
 * frame size outside 1..16384, a scene whose record is not finite or has not 0 < z_near < z_far. */
int arctic_fog_view(const ArcticScene *scene, uint32_t width, uint32_t height, ArcticFogView *out);

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_fog_march, one launch.  d_hdr_rgb32f: rows*width*3
 * floats, NULL = the shading's plane (the composition's under ARCTIC_FOG_SOURCE_COMPOSED), which needs ARCTIC_OPT_KEEP_FLOAT_OUTPUT; d_depth:
 * rows*width floats or NULL; d_out_hdr_rgb32f (rows*width*3 floats) and d_out_rgba8 (rows*width*4 bytes): NULL = the handle's own
 * (arctic_read_fog).  offsets16 is a HOST pointer; the table is sent again only when it differs from the one last sent.  It reads the
 * handle's current sun map.  No plane may alias another.  Stream-ordered on the handle's stream; a warm call allocates nothing and does not
 * synchronise. */
int arctic_fog_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, const float *d_hdr_rgb32f,
                      const float *d_depth, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8);

/* The host form: the same kernel from and to host memory (every plane may be NULL, with the meanings above; a NULL output: the result stays in
 * the handle's buffers).  Synchronous. */
int arctic_fog(ArcticRenderer *r, const ArcticSettings *settings, const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, const float *hdr_rgb32f,
               const float *depth, float *out_hdr_rgb32f, uint8_t *out_rgba8);

/* The one call: arctic_fog_view of the scene at the handle's size, then arctic_depth_plane_device into a plane the handle owns, then the march
 * of the handle's HDR plane per fog->flags into the handle's HDR plane and d_out_rgba8 (NULL: the handle's own).  Its bytes equal the same
 * calls made by hand.  Also ARCTIC_E_INVALID for a null scene or one that arctic_fog_view refuses, ARCTIC_E_STATE without a visibility plane;
 * every refusal comes before anything is enqueued. */
int arctic_pass_fog(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticFog *fog, const float *offsets16, uint8_t *d_out_rgba8);

/* What the latest call left: float LDR and `out` (rows*width*3 floats each) and RGBA8, the latter two when that call wrote the handle's own.
 * Any pointer may be NULL.  Synchronises.  ARCTIC_E_STATE: no fog since the handle was created or the last resize; hdr_rgb or rgba8 when the
 * latest call wrote the caller's plane. */
int arctic_read_fog(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_fog_march, calls, uploads of the offset table}.  All 0 until
 * the first call that passes its checks.  Touches no device. */
int arctic_fog_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter (no handle, no GPU), by the very functions the kernel runs: steps 1 to 4 for n pixels in any order.  pixel_xy: n int2; rgb:
 * the WHOLE frame's colour (height*width*3 floats); depth: height*width floats or NULL; shadow: S*S floats (S = 0: none); out_rgb: n*3 floats;
 * terms2: NULL or n float2 {T, I}.  ARCTIC_E_INVALID (nothing written): what the calls refuse of the records and the table, a frame size
 * outside 1..16384 or S above 16384, a pixel outside the frame, a null array that is needed.
 * arctic_fog_exp2 is step 2's function and arctic_fog_exp2_poly its polynomial p of n values f, for the test that measures them. */
int arctic_fog_pixels(const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height,
                      const float *rgb, const float *depth, const float *shadow, uint32_t S, float *out_rgb, float *terms2);
float arctic_fog_exp2(float x);
int arctic_fog_exp2_poly(uint64_t n, const float *f, float *p);

/* ---- Temporal upscaling: low-resolution jittered frames into a larger history (no counterpart in the reference) ----------------------------------
 * Every stage behind the shading runs at the handle's frame size, and the ray stages' cost scales with the pixel count.  This stage lets a
 * caller trace and shade w x h pixels and show W x H: it accumulates the handle's jittered frames into a history of the OUTPUT size, in front
 * of the tonemapper.  It is the resolve above (arctic_taa_resolve_device) with three differences: the history lives on a larger grid, each
 * frame's sample carries a confidence that falls with its distance from the output pixel's centre, and the box comes from the input pixels
 * around the nearest sample.  Nothing in the passes or in the other calls changes: a handle that never makes these calls renders the same
 * bytes and allocates nothing for them.
 *
 * THE UPSCALER: THE DEFINITION.  Bit for bit: fp32 throughout, one rounding per operation in the written order, no contraction, IEEE division.
 * min(a, b) is (b < a) ? b : a and max(a, b) is (a < b) ? b : a.
 * SIZES.  The input is the handle's frame, w x h.  The output is W x H = out_width x out_height with w <= W <= 4w, h <= H <= 4h and both in
 *   1..16384; the two axes may have different ratios.  rx = (float)w / (float)W, ry = (float)h / (float)H.
 * STATE.  U is one float4 {r, g, b, N} per OUTPUT pixel: the accumulated HDR colour and the confidence it stands for.  There are TWO SETS, and a
 *   call reads one and writes the other: 32 bytes per output pixel, tile-major like T, allocated by the first call that passes its checks and
 *   re-allocated when W x H changes.  U is EMPTY before the first call, after arctic_taa_upscale_reset, after arctic_resize and after a change
 *   of W x H.  U is not T: this stage and the resolve never touch each other's state.
 * INPUTS.  The handle-size HDR colour plane C (h x w x 3 floats, row-major), exactly as the resolve takes it; optionally the handle-size
 *   velocity2 (NULL: all zero), in INPUT pixels as arctic_motion_vectors_device writes it; and ArcticTaaUpscale, j being its jitter in INPUT pixels.
 * PER OUTPUT PIXEL p = (px, py), x written out and y likewise:
 *   1. THE NEAREST SAMPLE.  ux = (px + 0.5) * rx is the pixel's centre in input pixels.  Input pixel q's centre shows the unjittered position
 *      (q + 0.5) - j, so the sample nearest to p is qx = clamp(floor(ux + jx), 0, w-1) -- the floor of the ROUNDED sum, clamped in float before
 *      the conversion.  Its offset in OUTPUT pixels: Dx = (((qx + 0.5) - jx) - ux) / rx.
 *   2. c = C[q].  The box lo, hi over the 3 x 3 INPUT pixels around q is the resolve's step 1 with q in the place of p: dy then dx from -1 to
 *      1, clamped at the input frame's edge, lo = (x < lo) ? x : lo and hi = (x > hi) ? x : hi, so a NaN neighbour is ignored.
 *   3. THE CONFIDENCE of this frame's sample for this pixel: beta = max(0, 1 - sharpness * (Dx*Dx + Dy*Dy)).
 *   4. U is empty:  out = c, N = max(beta, confidence_floor).  This is also what every rejection below gives.
 *   5. Otherwise v = velocity2[q], or (0, 0).  hx = ((px + 0.5) + vx / rx) + jx / rx.  From here the resolve's steps 3 to 5 ON THE OUTPUT
 *      GRID: gx = hx - 0.5; ix = floor(gx); ax = gx - ix; reject unless hx and hy are finite, -1 <= ix <= W-1 and -1 <= iy <= H-1, tested in
 *      float before any conversion.  Four taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) of U with the weights (1-ax)(1-ay), ax(1-ay),
 *      (1-ax)ay, ax*ay; a tap is accepted iff it lies inside the OUTPUT frame and its stored N_q > 0; a rejected tap is a SELECT: its weight is
 *      0 and its history is not looked at.  S = ((k0 + k1) + k2) + k3; R, G, B and Cn the same ordered sums of k*r_q, k*g_q, k*b_q, k*N_q.
 *      If !(S > min_weight): reject.  h = {R, G, B} / S and hn = Cn / S, then, unless ARCTIC_TAA_UPSCALE_NO_CLAMP, per channel
 *      h = (h < lo) ? lo : h, then h = (h > hi) ? hi : h.  (NO_CLAMP is meant for still scenes and ground-truth accumulation.)
 *   6. N = min(hn + beta, max_history); a = beta / N.
 *      beta == 0 is a SELECT: out = h -- a NaN in c does not enter a pixel that this frame does not sample.
 *      Otherwise, if hn + beta == beta (the history's confidence vanishes beside the sample's, which only a history that has seen nothing
 *      but confidence_floor does): a SELECT too, out = c.  At ratio 1 it never fires: every stored N is 1 or more there.
 *      Otherwise the resolve's step 6 with this a.  Without ARCTIC_TAA_UPSCALE_LUMA_WEIGHT: out = h + (c - h) * a.  With it:
 *      wc = 1 / (1 + max(max(max(c.r, c.g), c.b), 0)), wh the same of h; kc = a * wc; kh = (1 - a) * wh; out = (c*kc + h*kh) / (kc + kh).
 *   7. Store {out, N}.  Then post_process of `out` under `settings`, as k_taa_resolve carries it out: float LDR and RGBA8, row-major at W x H.
 *   {out, N} is defined bit for bit; the tonemapped planes are held to the project's standing bar (1e-4 of the float64 post_process).
 * WHAT FOLLOWS, each a test.
 *   P1.  With W = w, H = h, sharpness = 0, |j| < 0.5 and no NO_CLAMP, {out, N} is the resolve's (arctic_taa_pixels) by bytes: rx = 1, q = p,
 *     beta = 1, and v / 1 and j / 1 are v and j.  (floor(ux + jx) is px as long as the sum does not round up to px + 1: |j| <= 0.499 does at
 *     every frame size.)
 *   P2.  With U empty every output pixel is C[q], the nearest sample; no output byte is left unwritten for any size pair.
 *   P3.  A still scene (velocity2 = -j), a power-of-two integer ratio s, NO_CLAMP, sharpness >= 1, confidence_floor <= 2^-25 and the s*s
 *     jitters of arctic_taa_upscale_jitter's exact sequence: every D is a whole number of output pixels, so beta is 1 where the sample lies
 *     on the pixel's centre and 0 elsewhere; hx is px + 0.5 exactly.  After s*s frames `out` is, for every output pixel, the colour sampled
 *     at its own centre, by bits -- the frame point-sampled at W x H -- and after k*s*s frames it still is, with N = min(k, max_history).
 *   P4.  A NaN, infinite or far-out-of-frame velocity rejects that pixel alone.  A NaN in C[q'] enters, through c, only the pixels whose q is
 *     q' (the box ignores it); what a history that holds a NaN does is the resolve's: a tap's weight times it.  Nothing is read outside a
 *     plane for any record that passes the checks.
 * KNOWN LIMITS, stated and not worked around.  The motion blur and the depth of field read the low-resolution handle's depth and velocity, so
 *   they run IN FRONT of the upscaler, on its input.  There is no LOD bias for ARCTIC_OPT_TEXTURE_MIPS at the reduced size.  The sky is not
 *   reprojected under camera rotation (the resolve's limit).  A shard cannot upscale.
 * Refusals, in this order; every refusal comes before anything is enqueued, and a refused call writes nothing and leaves U as it was.
 *   ARCTIC_E_INVALID: a null handle, settings or ArcticTaaUpscale; unknown flag bits; a field outside the ranges below, or a NaN; reserved
 *     words that are not 0; an output size outside 1..16384, below the handle's or above four times it; a device plane that is misaligned:
 *     4 bytes for C and RGBA8, 8 bytes for velocity2.
 *   ARCTIC_E_STATE: a handle that does not own the whole frame; and, with a NULL colour plane, the resolve's four conditions:
 *     ARCTIC_OPT_KEEP_FLOAT_OUTPUT off; no shading since it was turned on or since the last resize; under ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED
 *     no composition since the last resize; ARCTIC_OPT_HDR16 = 1. */
#define ARCTIC_TAA_UPSCALE_LUMA_WEIGHT      1u
#define ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED  2u   /* C = the latest composition's HDR plane instead of the latest shading's */
#define ARCTIC_TAA_UPSCALE_NO_CLAMP         4u   /* step 5 without the clamp to the box */
typedef struct ArcticTaaUpscale {        /* 48 bytes */
    uint32_t flags;
    float max_history;                   /* 1..65536, finite */
    float min_weight;                    /* [0, 1) */
    float jitter[2];                     /* THIS frame's jitter, INPUT pixels, finite, |j| <= 1 */
    float sharpness;                     /* [0, 65536]; 0: every frame counts fully for every pixel */
    float confidence_floor;              /* (0, 1]: the N of a pixel that only a distant sample has reached */
    uint32_t out_width;                  /* W */
    uint32_t out_height;                 /* H */
    uint32_t reserved[3];                /* 0 */
} ArcticTaaUpscale;

/* One call of the definition on DEVICE planes of a handle that owns the whole frame: k_taa_upscale, one launch.  d_hdr_rgb32f: h*w*3 floats,
 * NULL = the handle's own plane (the latest shading's, or under ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED the latest composition's); d_velocity2:
 * h*w float2, NULL = zero; d_out_rgba8: H*W*4 bytes, NULL = the handle's own buffer (arctic_read_taa_upscale).  No plane may alias another.
 * Stream-ordered on the handle's stream; a warm call allocates nothing and does not synchronise. */
int arctic_taa_upscale_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, const float *d_hdr_rgb32f, const float *d_velocity2,
                              uint8_t *d_out_rgba8);

/* The host form: the same kernel from and to host memory (any pointer but settings and upscale may be NULL, with the meanings above; a NULL
 * output: the result stays in the handle's buffers).  Synchronous. */
int arctic_taa_upscale(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8);

/* The one call: arctic_motion_vectors_device into planes the handle owns, then the upscale of the handle's HDR plane with that velocity2.  Byte
 * for byte the two calls made by hand.  It is the frame's ONE motion call.  Every refusal of both calls comes before anything is enqueued. */
int arctic_pass_taa_upscale(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, uint8_t *d_out_rgba8);

/* Empties U (the next call is a first call) and sets the calls counter to 0.  Frees nothing, touches no device. */
int arctic_taa_upscale_reset(ArcticRenderer *r);

/* What the latest call left, row-major at W x H whatever the layout on the device: float LDR and the accumulated HDR colour (H*W*3 floats
 * each), N (H*W floats) and the handle's own RGBA8 (H*W*4 bytes).  Any pointer may be NULL.  Synchronises.  ARCTIC_E_STATE while U is empty,
 * and for rgba8 when the latest call wrote the caller's buffer. */
int arctic_read_taa_upscale(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8);

/* The accumulated HDR colour of the latest call as a DEVICE plane of the output size, row-major, H*W*3 floats (4-byte aligned): what the stages
 * behind the upscaler take as their explicit colour argument -- arctic_bloom_device, arctic_exposure_device and the rest on a handle of the
 * OUTPUT size.  One small launch (k_taa_upscale_hdr), stream-ordered on the handle's stream, allocates nothing.  ARCTIC_E_INVALID: a null or
 * misaligned plane.  ARCTIC_E_STATE while U is empty.  It does not count as a call or a launch of arctic_taa_upscale_info. */
int arctic_taa_upscale_hdr_device(ArcticRenderer *r, float *d_hdr_rgb32f);

/* What the calls hold on this handle: out4 = {bytes of device memory, launches of k_taa_upscale, calls since the last reset, W | H << 32 of the
 * history (0 before the first call)}.  All 0 until the first call that passes its checks.  Touches no device. */
int arctic_taa_upscale_info(ArcticRenderer *r, uint64_t *out4);

/* The host arbiter (no handle, no GPU): steps 1 to 6 for n OUTPUT pixels in any order, by the very function the kernel runs.  pixel_xy:
 * (px, py) per pixel, inside the output frame; width, height: the INPUT frame; cur_rgb: the whole input frame's C (height*width*3 floats);
 * velocity2: the whole input frame's (height*width*2 floats) or NULL = zero; prev_rgbn: the whole previous U (H*W*4 floats, row-major) or NULL
 * = U is empty; out_rgbn: n*4 floats {out, N}.  ARCTIC_E_INVALID (nothing written): what the calls refuse of ArcticTaaUpscale and of the
 * sizes, a pixel outside the output frame, a null array that is needed. */
int arctic_taa_upscale_pixels(const ArcticTaaUpscale *upscale, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb,
                              const float *velocity2, const float *prev_rgbn, float *out_rgbn);

/* The jitter of frame `index` for an upscale from w x h to W x H -- a pure host function; set it with arctic_set_camera_jitter and pass it in
 * ArcticTaaUpscale::jitter.  In fp32, one rounding per operation:
 *   Without ARCTIC_TAA_UPSCALE_JITTER_EXACT in `index`: L = 8 * ceil(W / w) * ceil(H / h); i = index % L + 1; out2 = {halton(i, 2) - 0.5,
 *     halton(i, 3) - 0.5}, halton(i, b): f = 1, x = 0; while i > 0: f = f / b; x = x + f * (float)(i % b); i = i / b.
 *   With it (the sequence of P3), for W = s*w and H = s*h with s = 1, 2 or 4 alone: i = (index & 0x7FFFFFFF) % (s*s); kx = i % s, ky = i / s;
 *     out2 = {0.5 - (kx + 0.5) / s, 0.5 - (ky + 0.5) / s}: phase i puts the centres of the output pixels (s*qx + kx, s*qy + ky) on samples.
 * ARCTIC_E_INVALID (nothing written): a null pointer, sizes outside what the upscaler takes, the flag with any other ratio. */
#define ARCTIC_TAA_UPSCALE_JITTER_EXACT 0x80000000u
int arctic_taa_upscale_jitter(uint32_t index, uint32_t w, uint32_t W, uint32_t h, uint32_t H, float *out2);

/* ---- Indirect diffuse light: one bounce from the resident G-buffer (no counterpart in the reference: its one ambient term is the flat ambient * base_color) --
 * What light arrives at each pixel from the rest of the scene?  n_rays rays per pixel over the hemisphere of its normal, each walked to its
 * CLOSEST hit and shaded there by layer 2 of the hit section (arctic_shade_hits), a miss taking the environment map; the mean of those colours
 * is the estimate E.  With a COSINE-WEIGHTED direction table the mean of the radiance is the irradiance over pi, which is what a diffuse surface
 * multiplies its base colour by.  Nothing in the passes uses the plane: shading and every existing bit are unchanged, and a handle that never
 * makes these calls allocates nothing for them.
 *
 * THE DEFINITION.  Everything is fp32, one rounding per operation, in the written order, no contraction; division and square root are IEEE
 * (correctly rounded).  dirs has the ambient occlusion's layout, P*P*n_rays*3 floats, direction k of set s at dirs[(s*n_rays + k)*3 ..], used as
 * given; pixel (x, y) OF THE FRAME uses set (y % P) * P + x % P.  The work is done in n_rays ROUNDS k = 0 .. n_rays-1 over the reflection plane's
 * own buffers (one ray, one hit and one colour per pixel: 64 bytes, once, not n_rays times); S and E are row-major float4 planes.
 *   1. Rays (k_gi_rays, round k).  Per pixel, with world = attributes 11..13 and n = attributes 8..10: steps 1 to 3 of the ambient occlusion
 *      unchanged -- m, the frame t and bt, o[i] = world[i] + bias*m[i], d[i] = (t[i]*l0 + bt[i]*l1) + m[i]*l2 with l = direction k of the pixel's
 *      set -- and t_min = 0, t_max = max_distance.  A pixel without geometry, or one NOT COVERED by step 1, gets the all-zero record, as in the
 *      reflection plane.  A pixel HAD A RAY in the round iff its record's t_max > 0.
 *   2. Radiance.  The ray queries' closest-hit walk and layer 2's k_shade_hits on those records, unchanged: a hit gives the forward pixel there
 *      seen from the ray's origin, a miss the environment map along d, or zeros without a map.  OUT OF SCOPE at the hits, as in layer 2: spot
 *      lights, shadow-casting point lights, image-based ambient, material extras and mip chains do not take part.
 *   3. Sum (k_gi_add, round k).  Each channel l of the round's colour is sanitised by selects:  L = l > clamp_max ? clamp_max : (l > 0 ? l : 0)
 *      -- a NaN becomes 0, +inf becomes clamp_max, a negative becomes 0.  For a pixel that had a ray,
 *      S[p] = {S.r + L.r, S.g + L.g, S.b + L.b, S.cnt + 1};  round 0 starts from {0, 0, 0, 0} (it stores, it does not add), so the plane needs
 *      no clearing; a pixel without a ray keeps its S (in round 0: zeros).
 *   4. Estimate (k_gi_estimate).  Unfiltered:  E = {S.r / S.cnt, S.g / S.cnt, S.b / S.cnt, S.cnt} where S.cnt > 0, else {0, 0, 0, 0}.
 *      Filtered (filter = 1), for a covered pixel p: the ambient occlusion filter's window, pixel order (rows of the window outside, columns
 *      inside) and acceptance test -- p itself always accepted; another pixel q accepted iff inside the frame, covered,
 *      dot(m_p, m_q) >= normal_cos and fabs(dot(m_p, w_q - w_p)) <= plane_dist.  A = {0, 0, 0, 0};  for every accepted pixel q IN WINDOW ORDER,
 *      p at its own place:  A = {A.r + S_q.r, A.g + S_q.g, A.b + S_q.b, A.cnt + S_q.cnt};  E = A's estimate by the unfiltered formula, so E.a is
 *      the accepted ray count.  A rejected pixel's S is not looked at (a select, not a product by zero: a NaN there stays there).  A pixel that
 *      is not covered gives {0, 0, 0, 0}.
 * Sharded handles.  The pattern uses the row of the FRAME; filter = 1 on a handle that does not own the whole frame is refused with
 *   ARCTIC_E_STATE, by the occlusion's rule.
 * KNOWN LIMITS.  Those of the ray definition and of layer 2; the normal is the interpolated vertex normal; one bounce: the radiance at a hit holds
 *   the flat ambient term there, not a second bounce.  The calls use the reflection plane's rays, hits and colours as a round's scratch: a
 *   reflection plane left on the device (arctic_trace_reflections with a NULL output) is overwritten. */
typedef struct ArcticGi {   /* 48 bytes */
    uint32_t n_rays;       /* rays per pixel = rounds, 1..16 */
    uint32_t pattern;      /* P = 1, 2 or 4: pixel (x, y) OF THE FRAME uses direction set (y % P) * P + x % P */
    float    max_distance; /* every ray's t_max: > 0, +inf allowed */
    float    bias;         /* finite */
    float    clamp_max;    /* the upper bound of a sanitised channel: > 0, finite */
    uint32_t filter;       /* 0: per-pixel estimate; 1: the sum over the P x P window */
    float    normal_cos;   /* filter only, finite */
    float    plane_dist;   /* filter only, >= 0 */
    uint32_t reserved[4];  /* 0 */
} ArcticGi;

/* E for every pixel of the handle's RESIDENT G-buffer: rows * width * 4 floats, row-major over the handle's rows like arctic_trace_reflections.
 * rgba32f == NULL leaves the plane on the device and does not synchronise (timing).  Once the handle is warm a call allocates nothing; the
 * table is sent again only when its bytes changed.
 * Refusals, in this order; a refused call writes nothing and enqueues nothing.  ARCTIC_E_INVALID: a null scene, gi or dirs; n_rays outside
 * 1..16; pattern not 1, 2 or 4; max_distance not > 0 (a NaN included); a bias that is not finite; a clamp_max that is not > 0 and finite;
 * filter > 1 or a reserved word != 0; with the filter on, a normal_cos that is not finite or a plane_dist that is negative or a NaN; a direction
 * component that is not finite.  ARCTIC_E_STATE: no G-buffer; the sun map's states of layer 2; the filter on a shard. */
int arctic_trace_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticGi *gi, const float *dirs, float *rgba32f);

/* The same into DEVICE memory the caller owns (rows * width * 16 bytes, 16-byte aligned), stream-ordered on the handle's stream.  dirs stays a host
 * pointer.  ARCTIC_E_INVALID also, first, for a null or misaligned d_rgba32f. */
int arctic_trace_gi_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticGi *gi, const float *dirs, float *d_rgba32f);

/* For tests: the records of round `round` (stage 1 alone), rows * width of them, row-major.  Needs no scene.  ARCTIC_E_INVALID: what the call
 * above refuses for gi and dirs, then a round >= n_rays or a null output.  ARCTIC_E_STATE: no G-buffer. */
int arctic_gi_rays(ArcticRenderer *r, const ArcticGi *gi, const float *dirs, uint32_t round, ArcticRay *rays);

/* The latest arctic_trace_gi(_device)'s S and E as they stand on the device (either may be NULL).  ARCTIC_E_STATE: nothing traced yet, or not since
 * the last resize; E asked for when the latest call wrote the caller's plane. */
int arctic_read_gi_estimate(ArcticRenderer *r, float *sum_rgba32f, float *estimate_rgba32f);

/* out4 = {bytes of device memory held for the table, S, E, the history and the composition's planes (the rays, hits and colours are the reflection
 * plane's: arctic_hit_shading_info), launches of this section's own kernels so far, tracing calls so far, bytes of the history alone}.
 * {0, 0, 0, 0} until the first call that passes its checks. */
int arctic_gi_info(ArcticRenderer *r, uint64_t *out4);

/* 5. TEMPORAL ACCUMULATION of E (k_gi_accumulate).  Steps 1 to 6 of arctic_accumulate_ambient_occlusion_device's definition word for word, with
 * `value` a three-channel colour: the reprojection of the pixel's world position through the PREVIOUS call's proj_view, the four taps, the
 * acceptance of a tap q on its STORED m_q and w_q, the weights w_q, S = the accepted weights' sum, min_weight, N = min(hn + 1, max_history) and
 * a = 1 / N are all unchanged.  What changes:  V becomes three ordered sums, V_c = ((k0*acc_c,0 + k1*acc_c,1) + k2*acc_c,2) + k3*acc_c,3 over the
 * accepted taps;  hv_c = V_c / S;  acc_c = hv_c + (cur_c - hv_c) * a, with cur = E.rgb of the plane given.  A pixel whose E.a is 0 is treated as
 * NOT COVERED: its output is {0, 0, 0, 0} and the entry written is all zero.  The output is {acc.rgb, N}; without an accepted history
 * (S <= min_weight, or the first call) it is {E.rgb, 1}.
 * The history is three float4 planes per pixel -- {w, N}, {m, 0}, {acc, 0} -- in two sets, tile-major like the occlusion's: 96 bytes per pixel,
 * allocated by the first call, reported by arctic_gi_info, emptied by arctic_gi_history_reset and by a resize.  It is this section's own: the
 * occlusion's history is not touched.  Whole frames only (ARCTIC_E_STATE on a shard, by the occlusion's rule).
 * KNOWN LIMITS.  The plain form's: the reprojection follows the camera alone, so a moving or deforming object drags its history until the normal
 *   and plane tests reject it; the motion-vector form (arctic_accumulate_ambient_occlusion_motion_device's) is OUT OF SCOPE here.  Light that
 *   changes is followed at the rate 1 / max_history. */
typedef struct ArcticGiHistory {   /* 32 bytes: ArcticAoHistory's fields and refusals */
    float    max_history;  /* in [1, 65536] */
    float    normal_cos;   /* finite */
    float    plane_dist;   /* >= 0 */
    float    min_weight;   /* in [0, 1) */
    uint32_t reserved[4];  /* 0 */
} ArcticGiHistory;

/* d_gi_in_rgba32f (E: rows * width float4, row-major, 16-byte aligned, e.g. arctic_trace_gi_device's output) blended into the handle's history,
 * the result {acc, N} into d_gi_out_rgba32f (it may be the same plane); stream-ordered on the handle's stream.
 * Refusals, in this order; a refused call writes nothing.  ARCTIC_E_INVALID: a null scene; null parameters or plane; a plane that is not 16-byte
 * aligned; max_history outside [1, 65536]; a normal_cos that is not finite; a plane_dist that is negative or a NaN; min_weight outside [0, 1);
 * reserved != 0.  ARCTIC_E_STATE: no G-buffer; a handle that does not own the whole frame. */
int arctic_accumulate_gi_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticGiHistory *hist, const float *d_gi_in_rgba32f, float *d_gi_out_rgba32f);

/* The same from and to host memory; synchronous. */
int arctic_accumulate_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticGiHistory *hist, const float *gi_in_rgba32f, float *gi_out_rgba32f);

/* Empties the history (the next call is a first call); frees nothing. */
int arctic_gi_history_reset(ArcticRenderer *r);

/* The current history, row-major (any pointer may be NULL): acc3 and world3 and normal3 = height * width * 3 floats, count = height * width.
 * ARCTIC_E_STATE: the history is empty. */
int arctic_read_gi_history(ArcticRenderer *r, float *acc3, float *count, float *world3, float *normal3);

/* 6. COMPOSITION (k_gi_compose, a kernel and a call of its own: arctic_compose_planes_device is what it was).  Per pixel WITH GEOMETRY (a material
 * the handle has), with base, metal sampled exactly as k_compose samples them (level 0, the default sampler, the G-buffer's uv and material):
 *   C = the HDR colour: the caller's plane (rows * width * 3 floats, row-major), or with NULL the handle's shaded plane, or under
 *       ARCTIC_GI_SOURCE_COMPOSED the composed one -- the refusals of those sources are the post stages' (ARCTIC_OPT_KEEP_FLOAT_OUTPUT, ...).
 *   Ambient correction:   C_c = C_c + (ambient * base_c) * (ambient_scale - 1)      -- the occlusion's form with ka = ambient_scale:
 *       ambient_scale = 1 adds an exact zero, ambient_scale = 0 takes the flat ambient term out, so that E replaces it.
 *   Where E.a > 0 (a select; E.rgb is not looked at elsewhere):   C_c = C_c + (gi_strength * (1 - metal)) * (base_c * E_c)
 *   then the shared tonemapper to float LDR and RGBA8.  A pixel without geometry keeps its C.
 * E is the caller's plane (arctic_trace_gi_device's or arctic_accumulate_gi_device's output) or, with NULL, the handle's own estimate.  Written:
 * the handle's own HDR, LDR and RGBA8 planes (arctic_read_gi), or the caller's d_out_hdr_rgb32f / d_out_rgba8.  The later stages take the
 * result through their explicit colour argument, as they take the fog's: there is no *_SOURCE_GI flag.  Shards compose their own rows.
 * Indirect SPECULAR light is out of scope: the reflection plane is that term.
 * Refusals, in this order; a refused call writes nothing.  ARCTIC_E_INVALID: a null scene or settings; null parameters; unknown flag bits; a
 * gi_strength that is negative or not finite; ambient_scale outside [0, 1]; reserved != 0; a misaligned plane (E: 16 bytes, the others 4).
 * ARCTIC_E_STATE: no G-buffer; with a NULL C the source's states; with a NULL E no estimate on the handle; with ambient_scale != 1 what refuses
 * ARCTIC_COMPOSE_AO (ARCTIC_OPT_ENV_LIGHTING, ARCTIC_OPT_TEXTURE_MIPS = 1, a material that is not neutral), and with ARCTIC_GI_SOURCE_COMPOSED
 * a latest composition that had ARCTIC_COMPOSE_AO: it has scaled the term already. */
#define ARCTIC_GI_SOURCE_COMPOSED 1u   /* a NULL colour plane means the composed HDR plane, not the shaded one */
typedef struct ArcticGiCompose {   /* 32 bytes */
    uint32_t flags;         /* 0 or ARCTIC_GI_SOURCE_COMPOSED */
    float    gi_strength;   /* >= 0, finite */
    float    ambient_scale; /* in [0, 1]: what is left of the flat ambient term */
    uint32_t reserved[5];   /* 0 */
} ArcticGiCompose;

int arctic_gi_compose_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticGiCompose *compose, const float *d_hdr_rgb32f,
                             const float *d_gi_rgba32f, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8);

/* What the latest composition left in the handle's own planes (any pointer may be NULL).  ARCTIC_E_STATE: nothing composed yet, or not since the
 * last resize; a plane asked for that the latest call wrote into the caller's memory instead. */
int arctic_read_gi(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8);

/* The one call: arctic_trace_gi into the handle's own estimate, arctic_accumulate_gi_device on that plane in place when hist != NULL, then
 * arctic_gi_compose_device with a NULL colour and the handle's estimate -- byte for byte the calls made by hand.  Every refusal of the three comes
 * before anything is enqueued, in the order: gi and dirs, hist, compose (ARCTIC_E_INVALID); then the states of the trace, of the accumulation and
 * of the composition (ARCTIC_E_STATE). */
int arctic_pass_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticGi *gi, const float *dirs, const ArcticGiHistory *hist,
                   const ArcticGiCompose *compose, uint8_t *d_out_rgba8);

/* The host arbiters (no handle, no GPU), running the functions the kernels run.  arctic_gi_points: round `round`'s record for point k =
 * {world3, normal3} of points6, which has geometry, using direction set sets[k]; the all-zero record for a point that is not covered.  Refuses
 * what arctic_trace_gi refuses for gi and dirs, a round >= n_rays, a null pointer with a non-zero count and a sets[k] >= P*P. */
int arctic_gi_points(const float *points6, const uint32_t *sets, uint64_t n_points, const ArcticGi *gi, const float *dirs, uint32_t round, ArcticRay *rays);

/* Stages 3 and 4 for a whole frame of width x height pixels: rays and colors4 hold n_rays rounds of width*height records / float4 colours, round
 * after round; normal3, world3 (attributes 8..10 and 11..13) and geometry (0: none) are read with the filter on only and may be NULL without it.
 * sum4 and estimate4 receive S and E.  Refuses what arctic_trace_gi refuses for gi, a width or height of 0 or above 16384 and a null pointer. */
int arctic_gi_estimate_pixels(const ArcticGi *gi, uint32_t width, uint32_t height, const ArcticRay *rays, const float *colors4, const float *normal3,
                              const float *world3, const uint8_t *geometry, float *sum4, float *estimate4);

/* Stage 5 for n pixels in any order, shaped like arctic_accumulate_pixels: cur4 = the pixels' E; prev_proj_view = the previous call's matrix
 * (NULL: the history is empty) and the previous history as row-major arrays of a width x height frame; out4 = {acc, N}, and the entry written
 * (any of the four may be NULL).  Refuses what arctic_accumulate_gi_device refuses for hist, a width or height of 0 or above 16384, a matrix
 * without its four arrays, and a null array with n > 0. */
int arctic_gi_accumulate_pixels(const ArcticGiHistory *hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const float *cur4,
                                const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_acc3, const float *prev_count,
                                const float *prev_world3, const float *prev_normal3, float *out4, float *out_acc3, float *out_count, float *out_world3,
                                float *out_normal3);

/* Stage 6's two terms for n pixels on channels sampled already, like arctic_compose_pixels: out_hdr3 = C after the ambient correction and the
 * indirect term.  Refuses what arctic_gi_compose_device refuses for compose, and a null array with n > 0. */
int arctic_gi_compose_pixels(const ArcticGiCompose *compose, float ambient, uint64_t n, const float *hdr3, const float *base3, const float *metal, const float *gi4,
                             const uint8_t *geometry, float *out_hdr3);

/* The owner grid of a forward prepass as plain numbers -- pure host functions, no device, no handle (the library's kernels use the
   same definitions).  A handle created with these sizes (row range [row_begin, row_end), or -- band_rows > 0 -- the interleaved
   shard shard_index of shard_count) launches grid[0] x grid[1] owner waves, one per 16x16 block; arctic_owner_visit: grid row
   `grid_row` visits block row *block_row of the frame and stores its upper / lower 8-pixel tile row as the shard's tile row
   local_tile_rows[0] / [1] (-1: that tile row is not this shard's).  Every tile row a shard stores must be visited exactly once:
   tests/test_owner_grid.py checks that for worlds 1..8, bands of odd and even numbers of tile rows and row ranges that cut blocks. */
int arctic_owner_grid(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t shard_index, uint32_t shard_count, uint32_t *grid);
int arctic_owner_visit(uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end, uint32_t band_rows, uint32_t shard_index, uint32_t shard_count,
                       uint32_t grid_row, uint32_t *block_row, int32_t *local_tile_rows);

/* The object-space boxes of ARCTIC_OPT_CLUSTER_CULL as plain numbers -- a pure host function, no device, no handle: the function
   arctic_create_mesh makes a mesh's boxes with.  Triangle t is indices[3 t .. 3 t + 2]; it is VALID when its three indices are below n_vertices
   (any other triangle draws nothing and bounds nothing).  A box is six floats {min x, min y, min z, max x, max y, max z}; the infinite box is
   {-inf, -inf, -inf, inf, inf, inf} and is never skipped.
     tbounds_out: ceil(n_indices / 3 / 256) boxes.  Box c bounds the positions of the valid triangles 256 c .. 256 c + 255 (a cluster: one workgroup
       of the set-up kernel).  Infinite if one of those positions is not finite, or if the cluster has no valid triangle.
     vbounds_out: ceil(n_vertices / 256) boxes.  Box b is the union of tbounds[t / 256] over every valid triangle t that uses one of the vertices
       256 b .. 256 b + 255 (a vertex block: one workgroup of the vertex kernel) -- so it CONTAINS the box of every cluster that reads one of the
       block's vertices, and is infinite when one of them is.  Infinite as well if no valid triangle uses the block.
   min and max of floats round nothing: both tables are exact.  An empty index list or vertex list is accepted (no clusters / no blocks).
   ARCTIC_E_INVALID (nothing written): a null array with a count above 0, an index count that is no multiple of 3, a null output for a table that
   is not empty.  ARCTIC_E_CAPACITY (nothing written): more than 2^31 - 1 vertices or 2^32 - 16 indices, arctic_create_mesh's limits. */
int arctic_cluster_bounds(const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, float *tbounds_out, float *vbounds_out);

/* library/ABI version: major*10000 + minor*100 + patch */
int arctic_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ARCTIC_HIP_H */
