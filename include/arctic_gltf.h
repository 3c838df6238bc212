/* arctic_gltf.h -- C ABI of the scene-loader stand-in.
 *
 * Replaces, on Linux and without assimp / stb, what App::load_scene does above the renderer boundary
 * (reference src/app.cpp:173-385): read a glTF 2.0 file and hand the renderer materials (three RGBA8 images each),
 * meshes (Vertex + uint32 index arrays) and objects (model matrix + mesh index).  The conventions of that function are
 * restated, quirks included:
 *   - one mesh per glTF primitive, materials in file order (assimp's glTF2 importer), triangles only;
 *   - aiProcess_FlipUVs: v -> 1 - v; tangents from the file's TANGENT attribute (bitangent = cross(n, t) * w) or, without
 *     it, computed per triangle from the UV gradients and orthogonalised against the normal (aiProcess_CalcTangentSpace,
 *     without assimp's cross-vertex smoothing);
 *   - missing textures fall back to a white image / a flat normal map (assets/white.png, assets/normal.png);
 *   - node matrices go through assimp_to_mat4 (app.cpp:540-564), which feeds assimp's row-major elements to glm's
 *     column-major constructor, i.e. TRANSPOSES them, and are accumulated as parent * child in that transposed form.
 * Supported: .gltf (JSON) with external or base64 buffers and .glb containers, float / normalised-integer attributes,
 * u8/u16/u32 indices, skins and animations (below), images by uri or bufferView: PNG (1-16 bit, grey / RGB / palette / alpha, non-interlaced) and
 * baseline JPEG (8 bit, 1 or 3 components, sampling up to 2x2, restart intervals; float IDCT and replicated chroma, so an
 * LSB or two away from stb_image's integer pipeline).  Sparse accessors are read everywhere an
 * accessor is (below).  Not supported: progressive JPEG, Draco.
 * Nothing here runs on the GPU; parity with assimp's output is unpinned (assimp is not available offline).
 */
#ifndef ARCTIC_GLTF_H
#define ARCTIC_GLTF_H
#include <stdint.h>
#include "arctic_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ArcticGltf ArcticGltf;

/* NULL on failure with a message in err. */
ArcticGltf *arctic_gltf_load(const char *path, char *err, uint64_t err_len);
void arctic_gltf_free(ArcticGltf *g);

uint64_t arctic_gltf_material_count(const ArcticGltf *g);
uint64_t arctic_gltf_mesh_count(const ArcticGltf *g);
uint64_t arctic_gltf_object_count(const ArcticGltf *g);

/* image k of material i: 0 diffuse, 1 normal, 2 metal-rough; RGBA8, row-major (what stbi_load(..., 4) returns).
 * k = 3 emissive (sRGB, rgb), k = 4 occlusion (linear, R; glTF files often name the metal-rough image here): not read by load_scene.  An
 * absent image returns ARCTIC_OK with *rgba = NULL, *w = *h = 0. */
int arctic_gltf_material_image(const ArcticGltf *g, uint64_t i, int k, const uint8_t **rgba, uint32_t *w, uint32_t *h);
/* The factors of material i as arctic_set_material_extras takes them (not read by load_scene): pbrMetallicRoughness.baseColorFactor (rgb;
 * alpha ignored), metallicFactor, roughnessFactor, normalTexture.scale, occlusionTexture.strength, and emissiveFactor multiplied by
 * extensions.KHR_materials_emissive_strength.emissiveStrength (binary64, rounded once).  Defaults are glTF's: 1,1,1 / 1 / 1 / 1 / 1 / 0,0,0
 * / 1.  A wrong type, a wrong array length, a value outside ArcticMaterialParams' ranges or a texture index out of range refuse the file.
 * texCoord is ignored as for the other three textures.  arctic_gltf_upload does NOT apply them (it stays load_scene): the caller hands
 * them, with images 3 and 4, to arctic_set_material_extras for every material that is not neutral. */
int arctic_gltf_material_params(const ArcticGltf *g, uint64_t i, ArcticMaterialParams *out);
int arctic_gltf_mesh(const ArcticGltf *g, uint64_t i, const ArcticVertex **vertices, uint64_t *n_vertices,
                     const uint32_t **indices, uint64_t *n_indices, uint64_t *material);
const ArcticObject *arctic_gltf_objects(const ArcticGltf *g);
/* KHR_lights_punctual (not read by the reference's load_scene): the root's extensions.KHR_lights_punctual.lights, placed by every node whose
 * extensions.KHR_lights_punctual.light names one, with the node's accumulated matrix M exactly as a mesh on that node gets it
 * (assimp_to_mat4's transpose included): position = (M (0,0,0,1)).xyz, direction = (M (0,0,-1,0)).xyz.  One entry per (node, light), in
 * the node walk's order.  Defaults of the extension: color (1,1,1), intensity 1, innerConeAngle 0, outerConeAngle pi/4, no range.
 * colour = color * intensity (binary64, rounded once).  A spot light -> ArcticSpotLight; a point light without a range -> ArcticPointLight;
 * a point light with a range -> an omnidirectional ArcticSpotLight (outer = pi, inner = 0), so its range is kept.  Directional lights are
 * only counted (the sun stays the host's); unknown types are skipped.  A light index out of range, a range <= 0, cone angles outside
 * 0 <= inner <= outer <= pi/2 (outer > 0; the extension asks inner < outer, equality is accepted), a negative or non-finite colour or
 * intensity, or a non-numeric field refuse the file.  The arrays live as long as g; n receives the count (NULL result when it is 0).
 * arctic_gltf_upload uploads no lights: hand them to arctic_update_spot_lights / arctic_update_lights. */
const ArcticSpotLight *arctic_gltf_spot_lights(const ArcticGltf *g, uint64_t *n);
const ArcticPointLight *arctic_gltf_point_lights(const ArcticGltf *g, uint64_t *n);
uint64_t arctic_gltf_directional_light_count(const ArcticGltf *g);

/* Skins and animations (not read by the reference's load_scene, whose meshes are rigid): JOINTS_0 (u8 / u16) and WEIGHTS_0 (float or
 * normalised u8 / u16) of a primitive, the file's skins (joints; inverseBindMatrices, identity when absent) and animations (translation /
 * rotation / scale channels, LINEAR and STEP, rotations by slerp along the shorter arc).  A file without them loads exactly as before: the
 * same meshes and objects in the same order.  A node's `skin` attaches to the loader meshes of its `mesh`; the same glTF mesh met under a
 * SECOND skin becomes a second set of loader meshes, appended behind the file's, and its objects name those (met twice under one skin it
 * stays one set: a pose belongs to the mesh, and it is relative to the first node that carried it).  A primitive without JOINTS_0 stays
 * rigid under any skin.  Refused files: a joint that is not a node, a vertex that names a joint the skin does not have, JOINTS_0 without
 * WEIGHTS_0, attribute counts that differ, inverseBindMatrices with fewer matrices than joints or with an element that is not finite, a
 * weight that is not finite, sampler inputs that are not finite, negative or not strictly increasing, outputs whose count does not match,
 * a node with two parents (only checked in files that have skins).  A CUBICSPLINE sampler, or a `weights` channel on a node whose mesh
 * has no morph targets, does NOT refuse the file: only arctic_gltf_pose / arctic_gltf_morph_weights with that animation fail.  Keyframe quaternions are normalised when the file is read; one of
 * length zero is taken as the identity rotation.
 * arctic_gltf_mesh_skin: the records of loader mesh i as arctic_set_mesh_skin takes them, the skin it belongs to and that skin's joint
 * count; a rigid mesh returns ARCTIC_OK with *skin = NULL, *skin_index = -1. */
uint64_t arctic_gltf_skin_count(const ArcticGltf *g);
uint64_t arctic_gltf_skin_joint_count(const ArcticGltf *g, uint64_t skin);
uint64_t arctic_gltf_animation_count(const ArcticGltf *g);
double arctic_gltf_animation_duration(const ArcticGltf *g, uint64_t animation);   /* the latest keyframe of its channels, seconds; -1: no such animation */
int arctic_gltf_mesh_skin(const ArcticGltf *g, uint64_t i, const ArcticSkinVertex **skin, uint64_t *n_vertices, int64_t *skin_index, uint32_t *n_joints);
/* The joint matrices of `skin` as arctic_set_mesh_pose takes them (16 floats per joint, glm memory order) into out:
 *   inverse(global(mesh node)) * global(joint) * inverseBind,   global(n) = global(parent(n)) * local(n)  in glTF's own (untransposed) convention,
 * evaluated in binary64 and rounded once to fp32.  animation = -1: the rest pose (the nodes as the file has them); otherwise the animation's
 * channels replace the translation / rotation / scale of the nodes they target at `time` seconds, clamped to each sampler's range.  The mesh
 * node is the node the skin's first loader mesh was met on (identity when no mesh uses the skin).
 * ARCTIC_E_INVALID with a message in arctic_gltf_last_error: an index out of range, a time that is not finite, an animation with a
 * CUBICSPLINE sampler or a weights channel without morph targets, a singular mesh-node transform, a result that is not finite in fp32. */
int arctic_gltf_pose(const ArcticGltf *g, uint64_t skin, int64_t animation, double time, float *out);
const char *arctic_gltf_last_error(const ArcticGltf *g);

/* Sparse accessors: accessor.sparse = {count, indices {bufferView, byteOffset, componentType u8 / u16 / u32}, values {bufferView, byteOffset}}
 * replaces `count` elements of the dense base -- the accessor's bufferView, or zeros when it has none (such an accessor may hold at most 2^26
 * elements).  Refused: a sparse count above the accessor's, an index at or above the accessor's count, indices that do not increase strictly,
 * a view too short for its count.
 *
 * Morph targets (not read by the reference's load_scene): primitives[].targets with POSITION, NORMAL and TANGENT displacements, each optional
 * (absent = zero) and each float VEC3 with the primitive's vertex count; every primitive of a mesh has the same number of targets (at most
 * 65535).  arctic_gltf_mesh_morph gives the records of loader mesh i as arctic_set_mesh_morph_targets takes them (target-major); a mesh
 * without targets returns ARCTIC_OK with *deltas = NULL, *n_vertices = *n_targets = 0.  The derived parts of a delta follow one rule -- THE
 * VALUE WITH TARGET k ALONE AT WEIGHT 1, MINUS THE BASE VALUE:
 *   - primitive with a TANGENT attribute: tangent delta = the file's; bitangent delta = cross(n + dn, t + dt) * w - b, in the loader's fp32 order;
 *   - primitive without one: the tangents are computed again (aiProcess_CalcTangentSpace as above) on the mesh with target k applied; tangent
 *     and bitangent deltas are the differences to the base mesh's (a TANGENT displacement in the target is checked and not used).
 * LIMITS: a target without NORMAL keeps the base normal (normals are not re-derived); the bitangent is blended linearly (arctic_hip.h).
 * Weights: node.weights overrides mesh.weights, the default is zeros; a length that is not the target count refuses the file.  Weights belong
 * to the node and a deformation to the loader mesh, so a glTF mesh with targets gets one set of loader meshes per node it is met on: the first
 * node keeps the file's, every further node a copy appended behind them (as under a second skin).
 * `weights` animation channels: LINEAR and STEP, output SCALAR (float or normalised integers) with keyframes x targets values.
 * arctic_gltf_morph_weights: the n_targets weights of loader mesh i into out -- animation = -1: the file's defaults; otherwise a weights channel
 * on the mesh's node replaces them, a + (b - a) * u with u = (t - t0) / (t1 - t0) in binary64 (STEP: a), time clamped to the sampler's range,
 * rounded once to fp32.  A mesh without targets: ARCTIC_OK, nothing written.  ARCTIC_E_INVALID with a message in arctic_gltf_last_error: an
 * index out of range, a time that is not finite, an animation arctic_gltf_pose refuses too.  An animation with joint channels and weights
 * channels poses both: arctic_gltf_pose reads the former, this call the latter.  arctic_gltf_upload stays load_scene: it attaches nothing. */
int arctic_gltf_mesh_morph(const ArcticGltf *g, uint64_t i, const ArcticMorphDelta **deltas, uint64_t *n_vertices, uint32_t *n_targets);
int arctic_gltf_morph_weights(const ArcticGltf *g, uint64_t i, int64_t animation, double time, float *out);

/* convenience: create_material / create_mesh for everything in the file, in order (what load_scene does). */
int arctic_gltf_upload(const ArcticGltf *g, ArcticRenderer *r);

/* the image decoders alone (tests): PNG or baseline JPEG by signature; returns a malloc'ed RGBA8 image, NULL on failure */
uint8_t *arctic_png_decode(const uint8_t *data, uint64_t size, uint32_t *w, uint32_t *h, char *err, uint64_t err_len);
void arctic_png_free(uint8_t *p);

#ifdef __cplusplus
}
#endif
#endif
