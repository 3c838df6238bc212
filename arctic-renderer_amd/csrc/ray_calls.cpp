// ray_calls.cpp -- the ray family of the C-ABI (include/arctic_hip.h): ray queries, refit and re-split of their structure, sun visibility, ambient
// occlusion and its temporal accumulation, hit attributes, hit shading, the reflection plane, the composition of the two planes into the shaded frame,
// and the motion vectors with the accumulation that uses them.  The post stages that read these planes are units of their own (renderer_state.h).
//
// Owns, of the handle (renderer_state.h): ArcticRenderer::RayScene, AmbientOcclusion, AoHistory, HitScene, Compose and Motion -- nothing outside this
// unit touches them but arctic_set_option, which writes RayScene::refit_opt, a resize, which empties the histories, the post stages' one calls,
// which make the motion call through motion_refusal and motion_planes into Motion::d_plane, and post_source.cpp, which reads Compose's HDR plane.
// Reads, of the handle's other state: the G-buffer planes (resolved here from the visibility plane when a frame was shaded from it), the shadow
// map, the lights, the textures, the environment, the meshes and -- the composition -- the float HDR plane of the latest shading.  Enqueues on
// r->stream only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "renderer_state.h"
#include "ray_query.h"
#include "ray_ao.h"
#include "hit_shade.h"
#include "hit_shade_ext.h"
#include "compose.h"
#include "ao_history.h"
#include "motion.h"

namespace arctic {   // (renderer_state.h: gi_calls.cpp calls these as well)

// "The call needs a G-buffer", in two steps: ambient occlusion and the reflections have a refusal of their own between them, and no call
// resolves anything in front of a refusal.  gbuffer_refusal: the refusal alone, no side effect ...
int gbuffer_refusal(ArcticRenderer *r, const char *who) {
    if (!r->have_gbuffer && !r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no G-buffer (arctic_pass_gbuffer, arctic_write_gbuffer or a frame first)", who);
    return ARCTIC_OK;
}
// ... and gbuffer_in_place, behind it: the planes are resolved now when the frame was shaded from the visibility plane
int gbuffer_in_place(ArcticRenderer *r) { return r->have_gbuffer ? ARCTIC_OK : resolve_gbuffer(r); }
// what keeps a call from correcting the frame's ambient term (ARCTIC_COMPOSE_AO; the indirect light's ambient_scale)
const char *ambient_term_refusal(const ArcticRenderer *r) {
    return r->env_lighting == 1 ? "ARCTIC_OPT_ENV_LIGHTING is on" : r->texture_mips == 1 ? "ARCTIC_OPT_TEXTURE_MIPS = 1" : r->has_extras() ? "a material is not neutral (arctic_set_material_extras)" : nullptr;
}

}  // namespace arctic

extern "C" {

// ---- ray queries (the definition: include/arctic_hip.h; the arithmetic: ray_query.h; the builder: bvh.cpp; the kernels: trace.hip) ----------------
namespace {
// everything the structure is a function of, as bytes (shadow_inputs' rule: the objects, the mesh count, the shape of every mesh in use)
void ray_inputs(const ArcticRenderer *r, const ArcticScene *sc, std::vector<uint8_t> &k) {
    k.clear();
    auto put = [&](const void *p, size_t n) { const uint8_t *b = static_cast<const uint8_t *>(p); k.insert(k.end(), b, b + n); };
    const uint64_t head[2] = {(uint64_t)r->meshes.size(), sc->n_objects};
    put(head, sizeof head);
    put_objects(r, sc, k);
}

// may the cached structure follow `sc` by a refit?  Host state only (include/arctic_hip.h: "Eligibility")
bool ray_refit_eligible(const ArcticRenderer *r, const ArcticScene *sc) {
    const ArcticRenderer::RayScene &R = r->ray;
    if (!R.built || !R.refittable || sc->n_objects != R.built_meshes.size()) return false;
    for (uint64_t i = 0; i < sc->n_objects; ++i)
        if (sc->objects[i].mesh_idx != R.built_meshes[i] || sc->objects[i].mesh_idx >= r->meshes.size()) return false;
    return true;
}

// the refit: the per-object table (trs and vertices in use NOW) through the ring, then the stages.  Everything is enqueued on the handle's stream,
// behind the k_morph / k_skin that wrote the vertices and behind the queries that still walk the structure in place; nothing waits for the device
// (the ring's event is that of the copy OBJ_RING refits ago).  resplit: arctic_ray_scene_resplit -- between the table and the stages the slots are put
// in the order a fresh build of this pose would give them (ray_resplit.hip), so the stages write that build's structure
int refit_ray_scene(ArcticRenderer *r, const ArcticScene *sc, std::vector<uint8_t> &key, bool resplit = false) {
    ArcticRenderer::RayScene &R = r->ray;
    const size_t n_obj = (size_t)sc->n_objects, bytes = std::max<size_t>(n_obj, 1) * sizeof(RefitObject);
    RefitObject *h_objs = nullptr;
    HIPCHECK(r, R.objs_ring.stage(bytes, &h_objs));   // (a slot grows to fit)
    for (size_t i = 0; i < n_obj; ++i) {
        const ArcticObject &o = sc->objects[i];
        const Mesh &m = r->meshes[o.mesh_idx];   // (ray_refit_eligible: it exists)
        RefitObject &d = h_objs[i];
        for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) d.m[3 * c + k] = o.trs[4 * c + k];
        d.vertices = m.vertices_in_use(); d.n_vertices = m.n_vertices; d.pad = 0;
    }
    HIPCHECK(r, R.objs_ring.send(R.d_objs.p, n_obj * sizeof(RefitObject), r->stream));   // (no object: nothing is sent, the ring moves on)
    const RefitTablesDev T = {R.d_head.as<uint32_t>(), R.d_inputs.as<uint32_t>(), R.d_interior.as<RefitInterior>(), R.d_src.as<RefitSource>()};
    uint32_t launches = 0, split_launches = 0;
    if (resplit) {
        const hipError_t es = launch_ray_resplit(R.d_resplit.p, R.resplit_bytes, R.d_tris.p, (uint32_t)R.n_tris, R.d_src.as<RefitSource>(), R.d_objs.as<RefitObject>(), (uint32_t)n_obj,
                                                 r->stream, &split_launches);
        if (es != hipSuccess) { R.built = false; HIPCHECK(r, es); }   // (the order may be half written: the structure is dropped, the next query builds)
    }
    const hipError_t e = launch_ray_refit(T, R.stage_first.data(), (uint32_t)R.stage_first.size() - 1, R.d_nodes.p, (uint32_t)R.n_nodes, R.d_tris.p, (uint32_t)R.n_tris,
                                          R.d_objs.as<RefitObject>(), (uint32_t)n_obj, r->stream, &launches);
    if (e != hipSuccess) { R.built = false; HIPCHECK(r, e); }   // (some stages may have run: the structure is dropped, the next query builds)
    R.key.swap(key);
    if (resplit) { ++R.resplits; R.resplit_launches = (uint64_t)split_launches + launches; }
    else { ++R.refits; R.refit_launches = launches; }
    return ARCTIC_OK;
}
}  // namespace
}  // extern "C"
namespace arctic {   // (renderer_state.h)
// the structure for `sc`, resident on the device: built, validated and uploaded when its inputs changed (synchronous: it reads the meshes back) -- or,
// under ARCTIC_OPT_RAY_REFIT, refitted in stream order when only the geometry moved.
int ensure_ray_scene(ArcticRenderer *r, const ArcticScene *sc) {
    std::vector<uint8_t> key;
    ray_inputs(r, sc, key);
    if (r->ray.built && key == r->ray.key) return ARCTIC_OK;
    if (ray_refit_eligible(r, sc)) return refit_ray_scene(r, sc, key);
    const bool with_refit = r->ray.refit_opt == 1;
    std::vector<RefitSource> sources;
    // the vertices in use are written by k_morph / k_skin on the main stream; the structure in place may still be read by a query on it
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    std::vector<float> tris9;
    std::vector<uint32_t> prims;
    std::vector<std::vector<float>> verts(r->meshes.size());
    std::vector<std::vector<uint32_t>> inds(r->meshes.size());
    uint64_t prim = 0;
    for (uint64_t i = 0; i < sc->n_objects; ++i) {
        const ArcticObject &o = sc->objects[i];
        if (o.mesh_idx >= r->meshes.size()) continue;   // (skipped by the passes as well: upload_pass_tables)
        const Mesh &m = r->meshes[o.mesh_idx];
        if (prim + m.n_indices / 3 > 0xFFFFFFFEull) return r->fail(ARCTIC_E_CAPACITY, "ray queries: more than 2^32 - 2 triangles in the scene");
        if (verts[o.mesh_idx].empty()) {
            verts[o.mesh_idx].resize((size_t)m.n_vertices * 14); inds[o.mesh_idx].resize(m.n_indices);
            HIPCHECK(r, hipMemcpy(verts[o.mesh_idx].data(), m.vertices_in_use(), (size_t)m.n_vertices * sizeof(ArcticVertex), hipMemcpyDeviceToHost));
            HIPCHECK(r, hipMemcpy(inds[o.mesh_idx].data(), m.d_indices.p, (size_t)m.n_indices * 4, hipMemcpyDeviceToHost));
        }
        prim = ray_world_triangles(o.trs, verts[o.mesh_idx].data(), m.n_vertices, inds[o.mesh_idx].data(), m.n_indices / 3, prim, tris9, prims);
        if (with_refit) ray_triangle_sources((uint32_t)i, m.n_vertices, inds[o.mesh_idx].data(), m.n_indices / 3, sources);
    }
    Bvh b;
    if (!bvh_build(tris9.data(), prims.size(), prims.data(), b))
        return r->fail(ARCTIC_E_CAPACITY, "ray queries: %llu triangles to store, the structure holds 2^29 - 1", (unsigned long long)prims.size());
    if (!bvh_validate(b)) return r->fail(ARCTIC_E_INVALID, "internal: the ray structure failed its validation (%zu nodes, %zu triangles); nothing was uploaded", b.nodes.size(), b.tris.size());
    // Refittable: built under the option, no in-range triangle left out for being non-finite (it would have no slot to come back to), every
    // object's mesh there, and an object index that fits the source records.  The tables: where every stored slot's vertices come from -- copied
    // from the index buffers read above, found by the slot's prim (ascending in `prims`) -- and the schedule; both checked before anything is uploaded
    bool refittable = with_refit && b.tris.size() == prims.size() && sources.size() == prims.size() && sc->n_objects <= 0xFFFFFFFFull;
    for (uint64_t i = 0; refittable && i < sc->n_objects; ++i) refittable = sc->objects[i].mesh_idx < r->meshes.size();
    std::vector<RefitSource> slot_src;
    RefitSchedule sched;
    if (refittable) {
        slot_src.resize(b.tris.size());
        for (size_t k = 0; k < b.tris.size(); ++k) {
            const auto it = std::lower_bound(prims.begin(), prims.end(), b.tris[k].prim);
            if (it == prims.end() || *it != b.tris[k].prim) return r->fail(ARCTIC_E_INVALID, "internal: a stored triangle's prim %u is not one of the scene's", b.tris[k].prim);
            const RefitSource &s = slot_src[k] = sources[(size_t)(it - prims.begin())];
            const uint32_t nv = s.object < sc->n_objects ? r->meshes[sc->objects[s.object].mesh_idx].n_vertices : 0u;
            if (!(s.i0 < nv && s.i1 < nv && s.i2 < nv)) return r->fail(ARCTIC_E_INVALID, "internal: the refit's source record %zu is out of range; nothing was uploaded", k);
        }
        refit_schedule(b, sched);
        if (!refit_schedule_validate(b, sched)) return r->fail(ARCTIC_E_INVALID, "internal: the refit's schedule failed its validation (%zu nodes, %zu tasks); nothing was uploaded", b.nodes.size(), sched.head.size());
    }
    r->ray.built = false; r->ray.refittable = false;
    if (refittable) {
        const auto upload = [&](DevBuf &d, const void *p, size_t bytes) -> hipError_t {
            hipError_t e = d.ensure(std::max<size_t>(bytes, 16));
            if (e == hipSuccess && bytes) e = hipMemcpy(d.p, p, bytes, hipMemcpyHostToDevice);
            return e;
        };
        HIPCHECK(r, upload(r->ray.d_src, slot_src.data(), slot_src.size() * sizeof(RefitSource)));
        HIPCHECK(r, upload(r->ray.d_head, sched.head.data(), sched.head.size() * sizeof(uint32_t)));
        HIPCHECK(r, upload(r->ray.d_inputs, sched.inputs.data(), sched.inputs.size() * sizeof(uint32_t)));
        HIPCHECK(r, upload(r->ray.d_interior, sched.interior.data(), sched.interior.size() * sizeof(RefitInterior)));
        HIPCHECK(r, r->ray.d_objs.ensure(std::max<size_t>((size_t)sc->n_objects, 1) * sizeof(RefitObject)));
        r->ray.stage_first = sched.stage_first;
        r->ray.built_meshes.resize((size_t)sc->n_objects);
        for (uint64_t i = 0; i < sc->n_objects; ++i) r->ray.built_meshes[(size_t)i] = sc->objects[i].mesh_idx;
    }
    HIPCHECK(r, r->ray.d_nodes.ensure(std::max<size_t>(sizeof(RayNode), b.nodes.size() * sizeof(RayNode))));
    HIPCHECK(r, r->ray.d_tris.ensure(std::max<size_t>(sizeof(RayTri), b.tris.size() * sizeof(RayTri))));
    if (!b.nodes.empty()) HIPCHECK(r, hipMemcpy(r->ray.d_nodes.p, b.nodes.data(), b.nodes.size() * sizeof(RayNode), hipMemcpyHostToDevice));
    if (!b.tris.empty()) HIPCHECK(r, hipMemcpy(r->ray.d_tris.p, b.tris.data(), b.tris.size() * sizeof(RayTri), hipMemcpyHostToDevice));
    r->ray.key.swap(key);
    r->ray.n_tris = b.tris.size(); r->ray.n_nodes = b.nodes.size(); r->ray.depth = b.depth;
    ++r->ray.builds;
    r->ray.built = true; r->ray.refittable = refittable;
    return ARCTIC_OK;
}
}  // namespace arctic
extern "C" {
namespace {

int trace_checks(ArcticRenderer *r, const ArcticScene *sc, const void *rays, uint64_t n, uint32_t flags, const void *hits, const char *who) {
    if (!valid_scene(sc)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (flags & ~ARCTIC_TRACE_ANY) return r->fail(ARCTIC_E_INVALID, "%s: flags %#x (ARCTIC_TRACE_ANY or 0; ARCTIC_TRACE_BRUTE belongs to arctic_trace_triangles)", who, flags);
    if (n && (!rays || !hits)) return r->fail(ARCTIC_E_INVALID, "%s: null rays or hits", who);
    if (n > 0xFFFFFFFFull) return r->fail(ARCTIC_E_CAPACITY, "%s: %llu rays in one call (2^32 - 1 at most)", who, (unsigned long long)n);
    return ARCTIC_OK;
}
}  // namespace

int arctic_trace_rays_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *d_rays, uint64_t n, uint32_t flags, ArcticHit *d_hits) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = trace_checks(r, scene, d_rays, n, flags, d_hits, "trace_rays_device");
    if (rc) return rc;
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return r->fail(ARCTIC_E_INVALID, "trace_rays_device: rays and hits must be 16-byte aligned");
    if ((rc = select_device(r)) != ARCTIC_OK || (rc = ensure_ray_scene(r, scene)) != ARCTIC_OK) return rc;
    HIPCHECK(r, launch_trace(d_rays, n, r->ray.d_nodes.p, r->ray.d_tris.p, (uint32_t)r->ray.n_nodes, (flags & ARCTIC_TRACE_ANY) != 0, d_hits, r->stream));
    return ARCTIC_OK;
}

int arctic_trace_rays(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = trace_checks(r, scene, rays, n, flags, hits, "trace_rays");
    if (rc) return rc;
    if ((rc = select_device(r)) != ARCTIC_OK || (rc = ensure_ray_scene(r, scene)) != ARCTIC_OK) return rc;
    if (n == 0) return ARCTIC_OK;
    HIPCHECK(r, r->ray.d_rays.ensure(n * sizeof(ArcticRay)));
    HIPCHECK(r, r->ray.d_hits.ensure(n * sizeof(ArcticHit)));
    HIPCHECK(r, hipMemcpyAsync(r->ray.d_rays.p, rays, n * sizeof(ArcticRay), hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_trace(r->ray.d_rays.p, n, r->ray.d_nodes.p, r->ray.d_tris.p, (uint32_t)r->ray.n_nodes, (flags & ARCTIC_TRACE_ANY) != 0, r->ray.d_hits.p, r->stream));
    return read_back(r, hits, r->ray.d_hits, n * sizeof(ArcticHit));
}

int arctic_trace_sun_visibility(ArcticRenderer *r, const ArcticScene *scene, float bias, uint8_t *mask) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "trace_sun_visibility: null scene");
    if (!std::isfinite(bias)) return r->fail(ARCTIC_E_INVALID, "trace_sun_visibility: the bias is not finite");
    int rc = select_device(r);
    if (rc) return rc;
    if ((rc = gbuffer_refusal(r, "trace_sun_visibility")) != ARCTIC_OK || (rc = gbuffer_in_place(r)) != ARCTIC_OK) return rc;
    if ((rc = ensure_ray_scene(r, scene)) != ARCTIC_OK) return rc;
    float sun[3];
    dir_from_rot(scene->sun.rotation, sun);
    const float minus_sun[3] = {-sun[0], -sun[1], -sun[2]};
    const size_t bytes = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->ray.d_mask.ensure(std::max<size_t>(bytes, 16)));
    HIPCHECK(r, launch_trace_sun(r->gbuffer(), r->tiles_x, r->tiles_y, r->width, r->rows(), r->row0_in_tile, bias, minus_sun, r->ray.d_nodes.p, r->ray.d_tris.p,
                                 (uint32_t)r->ray.n_nodes, r->ray.d_mask.as<uint8_t>(), r->stream));
    return mask ? read_back(r, mask, r->ray.d_mask, bytes, FROM_FRAME) : ARCTIC_OK;
}

namespace {
// the checks, the G-buffer, the structure, the table and the launches of both ambient-occlusion calls; d_out: the caller's device memory, or null = the handle's own
int trace_ambient_occlusion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *d_out, const char *who) {
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    AoDesc d;
    if (ao) std::memcpy(&d, ao, sizeof d);
    if (const char *why = ao_refusal(ao ? &d : nullptr, dirs)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    int rc = select_device(r);
    if (rc || (rc = gbuffer_refusal(r, who)) != ARCTIC_OK) return rc;
    if (d.filter && r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the filter needs the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    if ((rc = gbuffer_in_place(r)) != ARCTIC_OK || (rc = ensure_ray_scene(r, scene)) != ARCTIC_OK) return rc;
    ArcticRenderer::AmbientOcclusion &A = r->ao;
    const size_t n_floats = (size_t)d.pattern * d.pattern * d.n_rays * 3, bytes = (size_t)r->rows() * r->width;
    const size_t table_bytes = 16 * AO_MAX_RAYS * 3 * sizeof(float);   // the largest table: the slot and d_dirs are made once
    if (A.n_floats != n_floats || std::memcmp(A.dirs_ring.slot[0].h.p, dirs, n_floats * sizeof(float)) != 0) {   // (n_floats != 0: an empty A holds no table)
        float *h_dirs = nullptr;
        HIPCHECK(r, A.dirs_ring.stage(table_bytes, &h_dirs));
        HIPCHECK(r, A.d_dirs.ensure(table_bytes));
        A.n_floats = 0;
        std::memcpy(h_dirs, dirs, n_floats * sizeof(float));
        HIPCHECK(r, A.dirs_ring.send(A.d_dirs.p, n_floats * sizeof(float), r->stream));
        A.n_floats = n_floats;
    }
    if (d.filter) HIPCHECK(r, A.d_hits.ensure(std::max<size_t>(bytes, 16)));
    if (!d_out) { HIPCHECK(r, A.d_out.ensure(std::max<size_t>(bytes, 16))); d_out = A.d_out.as<uint8_t>(); }
    const GBuffer g = r->gbuffer();
    // (a band's first row is a multiple of 8 in the frame and in the shard alike, so the shard's row and the frame's agree modulo the pattern)
    const uint32_t frame_row0 = r->band_rows ? 0u : r->row_begin;
    HIPCHECK(r, launch_trace_ao(g.b, g.c, g.e, r->tiles_x, r->tiles_y, r->width, r->rows(), r->row0_in_tile, frame_row0, d, A.d_dirs.as<float>(), r->ray.d_nodes.p, r->ray.d_tris.p,
                                (uint32_t)r->ray.n_nodes, d.filter ? 0 : 1, d.filter ? A.d_hits.as<uint8_t>() : d_out, r->stream));
    if (d.filter) HIPCHECK(r, launch_ao_filter(g.b, g.c, g.e, r->tiles_x, r->tiles_y, r->width, r->rows(), d, A.d_hits.as<uint8_t>(), d_out, r->stream));
    return ARCTIC_OK;
}
}  // namespace

int arctic_trace_ambient_occlusion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *out) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = trace_ambient_occlusion(r, scene, ao, dirs, nullptr, "trace_ambient_occlusion");
    if (rc || !out) return rc;
    return read_back(r, out, r->ao.d_out, (size_t)r->rows() * r->width, FROM_FRAME);
}

int arctic_trace_ambient_occlusion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *d_out) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_out) return r->fail(ARCTIC_E_INVALID, "trace_ambient_occlusion_device: null output");
    return trace_ambient_occlusion(r, scene, ao, dirs, d_out, "trace_ambient_occlusion_device");
}

int arctic_ray_scene_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "ray_scene_info: null");
    out4[0] = r->ray.n_tris; out4[1] = r->ray.n_nodes; out4[2] = r->ray.builds; out4[3] = r->ray.depth;
    return ARCTIC_OK;
}

int arctic_ray_refit_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "ray_refit_info: null");
    out4[0] = r->ray.refits; out4[1] = r->ray.built && r->ray.refittable ? 1 : 0; out4[2] = r->ray.refit_launches; out4[3] = 0;
    return ARCTIC_OK;
}

int arctic_ray_scene_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->ray.drop();   // (the buffers stay: a query in flight may still walk them, and the build reuses them)
    return ARCTIC_OK;
}

int arctic_ray_scene_resplit(ArcticRenderer *r, const ArcticScene *scene) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "ray_scene_resplit: null scene");
    int rc = select_device(r);
    if (rc) return rc;
    ArcticRenderer::RayScene &R = r->ray;
    if (!ray_refit_eligible(r, scene)) {   // what a reset and the next query's build do (under the option in force now)
        R.drop();
        R.resplit_fell_back = 1;
        return ensure_ray_scene(r, scene);
    }
    if (R.resplit_slots != R.n_tris) {
        size_t bytes = 0;
        HIPCHECK(r, ray_resplit_workspace((uint32_t)R.n_tris, &bytes));
        HIPCHECK(r, R.d_resplit.ensure(std::max<size_t>(bytes, 256)));
        R.resplit_bytes = bytes; R.resplit_slots = R.n_tris;
    }
    std::vector<uint8_t> key;
    ray_inputs(r, scene, key);
    R.resplit_fell_back = 0;
    return refit_ray_scene(r, scene, key, true);
}

int arctic_ray_resplit_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "ray_resplit_info: null");
    out4[0] = r->ray.resplits; out4[1] = r->ray.resplit_launches; out4[2] = r->ray.resplit_fell_back; out4[3] = 0;
    return ARCTIC_OK;
}

int arctic_read_ray_structure(ArcticRenderer *r, ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap) {
    if (!r) return ARCTIC_E_INVALID;
    static_assert(sizeof(ArcticRayNode) == sizeof(RayNode) && sizeof(ArcticRayTri) == sizeof(RayTri), "the public records are the internal ones");
    if (!r->ray.built) return r->fail(ARCTIC_E_STATE, "read_ray_structure: no structure (a query builds it)");
    if ((nodes && node_cap < r->ray.n_nodes) || (tris && tri_cap < r->ray.n_tris))
        return r->fail(ARCTIC_E_CAPACITY, "read_ray_structure: %llu nodes and %llu triangles", (unsigned long long)r->ray.n_nodes, (unsigned long long)r->ray.n_tris);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (nodes && r->ray.n_nodes) HIPCHECK(r, hipMemcpy(nodes, r->ray.d_nodes.p, r->ray.n_nodes * sizeof(RayNode), hipMemcpyDeviceToHost));
    if (tris && r->ray.n_tris) HIPCHECK(r, hipMemcpy(tris, r->ray.d_tris.p, r->ray.n_tris * sizeof(RayTri), hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

// ---- hit attributes (the definition: include/arctic_hip.h; the arithmetic: hit_attributes.h; the kernel: hit_shade.hip) ---------------------------
namespace {
// the structure for `sc`, the source table of its topology and this call's object records, all on the device; enqueues on the handle's stream
int ensure_hit_scene(ArcticRenderer *r, const ArcticScene *sc) {
    int rc = ensure_ray_scene(r, sc);
    if (rc) return rc;
    ArcticRenderer::HitScene &H = r->hit;
    if (H.sources_of != r->ray.builds) {   // (a refit and a re-split keep the objects' meshes, and a mesh keeps its index buffer)
        HIPCHECK(r, hipStreamSynchronize(r->stream));   // a call in flight may still read the table in place
        std::vector<HitSource> sources;
        std::vector<std::vector<uint32_t>> inds(r->meshes.size());
        for (uint64_t i = 0; i < sc->n_objects; ++i) {
            const ArcticObject &o = sc->objects[i];
            if (o.mesh_idx >= r->meshes.size()) continue;   // (no triangles: ensure_ray_scene)
            const Mesh &m = r->meshes[o.mesh_idx];
            std::vector<uint32_t> &ix = inds[o.mesh_idx];
            if (ix.empty() && m.n_indices) {
                ix.resize(m.n_indices);
                HIPCHECK(r, hipMemcpy(ix.data(), m.d_indices.p, (size_t)m.n_indices * 4, hipMemcpyDeviceToHost));
            }
            hit_triangle_sources((uint32_t)i, m.n_vertices, ix.data(), m.n_indices / 3, sources);   // (at most 2^32 - 2 in all: ensure_ray_scene)
        }
        HIPCHECK(r, H.d_src.ensure(std::max<size_t>(sources.size(), 1) * sizeof(HitSource)));
        if (!sources.empty()) HIPCHECK(r, hipMemcpy(H.d_src.p, sources.data(), sources.size() * sizeof(HitSource), hipMemcpyHostToDevice));
        H.n_prims = sources.size();
        H.sources_of = r->ray.builds;
        ++H.tables_made;
    }
    const size_t n_obj = (size_t)sc->n_objects, bytes = std::max<size_t>(n_obj, 1) * sizeof(HitObject);
    HitObject *h_objs = nullptr;
    HIPCHECK(r, H.objs_ring.stage(bytes, &h_objs));
    HIPCHECK(r, H.d_objs.ensure(bytes));
    for (size_t i = 0; i < n_obj; ++i) {
        const ArcticObject &o = sc->objects[i];
        HitObject &d = h_objs[i];
        std::memcpy(d.trs, o.trs, sizeof d.trs);
        const bool there = o.mesh_idx < r->meshes.size();   // (an object without a mesh has no prim: its record is never read)
        d.vertices = there ? r->meshes[o.mesh_idx].vertices_in_use() : nullptr;
        d.n_vertices = there ? r->meshes[o.mesh_idx].n_vertices : 0u;
        d.material = there ? (uint32_t)r->meshes[o.mesh_idx].material : HIT_NO_MATERIAL;
    }
    HIPCHECK(r, H.objs_ring.send(H.d_objs.p, n_obj * sizeof(HitObject), r->stream));
    return ARCTIC_OK;
}
}  // namespace

int arctic_hit_attributes(ArcticRenderer *r, const ArcticScene *scene, const ArcticHit *hits, uint64_t n, float *attrs, uint32_t *material) {
    if (!r) return ARCTIC_E_INVALID;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "hit_attributes: null scene");
    if (n && (!hits || !attrs || !material)) return r->fail(ARCTIC_E_INVALID, "hit_attributes: null hits, attrs or material");
    if (n > 0xFFFFFFFFull) return r->fail(ARCTIC_E_CAPACITY, "hit_attributes: %llu hits in one call (2^32 - 1 at most)", (unsigned long long)n);
    int rc;
    if ((rc = select_device(r)) != ARCTIC_OK || (rc = ensure_hit_scene(r, scene)) != ARCTIC_OK) return rc;
    if (n == 0) return ARCTIC_OK;
    ArcticRenderer::HitScene &H = r->hit;
    float lpv[16];
    sun_proj_view(scene->sun.position, scene->sun.rotation, lpv);
    HIPCHECK(r, H.d_hits.ensure(n * sizeof(ArcticHit)));
    HIPCHECK(r, H.d_attrs.ensure(n * HIT_ATTRS * sizeof(float)));
    HIPCHECK(r, H.d_material.ensure(n * sizeof(uint32_t)));
    HIPCHECK(r, hipMemcpyAsync(H.d_hits.p, hits, n * sizeof(ArcticHit), hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, launch_hit_attributes(H.d_hits.p, n, H.d_src.as<HitSource>(), (uint32_t)H.n_prims, H.d_objs.as<HitObject>(), lpv, H.d_attrs.as<float>(),
                                      H.d_material.as<uint32_t>(), r->stream));
    HIPCHECK(r, hipMemcpyAsync(attrs, H.d_attrs.p, n * HIT_ATTRS * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    return read_back(r, material, H.d_material, n * sizeof(uint32_t));
}

// ---- hit shading and the reflection plane (include/arctic_hip.h; the kernels: hit_shade.hip) -------------------------------------------------------
}  // extern "C"
namespace arctic {   // (renderer_state.h: gi_calls.cpp runs the hit shading between kernels of its own)
// the sun's map as k_shade_hits (and k_shade_hits_ext) needs it: whole, and drawn or written at least once
int sun_map_ready(ArcticRenderer *r, const char *who) {
    if (r->shadow_size && r->shadow_sharded)
        return r->fail(ARCTIC_E_STATE, "%s: the sun's map is sharded (ARCTIC_OPT_SHADOW_SHARDED): a hit may lie in rows this handle never draws", who);
    if (r->shadow_size && !r->shadow_written_set[r->scur])
        return r->fail(ARCTIC_E_STATE, "%s: the sun's map was never drawn or written (arctic_pass_shadow_map, arctic_write_shadow_map or a frame first)", who);
    // ... and, under ARCTIC_OPT_HIT_MODEL = 1, the cube lights' faces as k_shade_hits_ext needs them: drawn or written since the list was set
    if (r->hit_model == 1 && r->n_cubes && !r->cube_faces_filled)
        return r->fail(ARCTIC_E_STATE, "%s: ARCTIC_OPT_HIT_MODEL = 1 and the shadow-casting point lights' faces were neither drawn nor written since the list was set "
                       "(arctic_pass_point_shadows, arctic_write_point_shadow or a frame first)", who);
    return ARCTIC_OK;
}
// the structure, the tables and the launch: device pointers throughout.  Every caller has asked sun_map_ready in front of its first launch
int shade_hits(ArcticRenderer *r, const ArcticScene *sc, const void *d_rays, const void *d_hits, uint64_t n, float4 *d_out) {
    int rc = ensure_hit_scene(r, sc);
    if (rc || n == 0) return rc;
    HitShadeParams p = {};
    p.src = r->hit.d_src.as<HitSource>(); p.objs = r->hit.d_objs.as<HitObject>(); p.n_prims = (uint32_t)r->hit.n_prims;
    p.tex = r->d_tex.as<TexDesc>(); p.srgb_lut = r->d_lut.as<float>();
    p.shadow_map = r->shadow_size ? r->d_shadow().as<float>() : nullptr; p.shadow_size = r->shadow_size;
    p.lights = r->d_lights.as<float4>(); p.n_lights = r->n_lights;
    p.env = r->env_w ? r->d_env.as<float4>() : nullptr; p.env_w = r->env_w; p.env_h = r->env_h;
    p.ambient = sc->ambient;
    dir_from_rot(sc->sun.rotation, p.sun_dir);
    std::memcpy(p.sun_color, sc->sun.color, sizeof p.sun_color);
    sun_proj_view(sc->sun.position, sc->sun.rotation, p.lpv);
    if (r->hit_model == 1) {   // the same block, and the handle's other tables as they stand (hit_shade_ext.h)
        HitShadeExtParams q = {};
        q.base = p;
        if (r->n_spots) { q.spots = r->d_spots.as<float4>(); q.n_spots = r->n_spots; }
        if (r->n_cubes) { q.cubes = r->d_cubes.as<float4>(); q.n_cubes = r->n_cubes; q.cube_size = r->cube_size; }
        if (r->has_extras()) q.extras = p.tex + r->tex.size();   // one MaterialExtra per material behind the 3 n_materials descriptors (common.h)
        if (r->env_active()) q.env_tables = r->d_env_tables.as<EnvTables>();
        HIPCHECK(r, launch_shade_hits_ext(d_rays, d_hits, n, q, d_out, r->stream));
        return ARCTIC_OK;
    }
    HIPCHECK(r, launch_shade_hits(d_rays, d_hits, n, p, d_out, r->stream));
    return ARCTIC_OK;
}
}  // namespace arctic
extern "C" {
namespace {
// what both forms of arctic_shade_hits refuse before the device is touched
int shade_checks(ArcticRenderer *r, const ArcticScene *sc, const void *rays, const void *hits, uint64_t n, uint32_t flags, const void *out, const char *who) {
    if (!valid_scene(sc)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (flags) return r->fail(ARCTIC_E_INVALID, "%s: flags %#x (0)", who, flags);
    if (n && (!rays || !hits || !out)) return r->fail(ARCTIC_E_INVALID, "%s: null rays, hits or output", who);
    if (n > 0xFFFFFFFFull) return r->fail(ARCTIC_E_CAPACITY, "%s: %llu rays in one call (2^32 - 1 at most)", who, (unsigned long long)n);
    return sun_map_ready(r, who);
}
}  // namespace

int arctic_shade_hits_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *d_rays, const ArcticHit *d_hits, uint64_t n, uint32_t flags, float *d_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = shade_checks(r, scene, d_rays, d_hits, n, flags, d_rgba32f, "shade_hits_device");
    if (rc) return rc;
    if (((uintptr_t)d_rays | (uintptr_t)d_hits | (uintptr_t)d_rgba32f) & 15u) return r->fail(ARCTIC_E_INVALID, "shade_hits_device: rays, hits and output must be 16-byte aligned");
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    return shade_hits(r, scene, d_rays, d_hits, n, reinterpret_cast<float4 *>(d_rgba32f));
}

int arctic_shade_hits(ArcticRenderer *r, const ArcticScene *scene, const ArcticRay *rays, const ArcticHit *hits, uint64_t n, uint32_t flags, float *rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = shade_checks(r, scene, rays, hits, n, flags, rgba32f, "shade_hits");
    if (rc) return rc;
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::HitScene &H = r->hit;
    if (n) {
        HIPCHECK(r, H.d_rays.ensure(n * sizeof(ArcticRay)));
        HIPCHECK(r, H.d_hits.ensure(n * sizeof(ArcticHit)));
        HIPCHECK(r, H.d_color.ensure(n * 16));
        HIPCHECK(r, hipMemcpyAsync(H.d_rays.p, rays, n * sizeof(ArcticRay), hipMemcpyHostToDevice, r->stream));
        HIPCHECK(r, hipMemcpyAsync(H.d_hits.p, hits, n * sizeof(ArcticHit), hipMemcpyHostToDevice, r->stream));
    }
    if ((rc = shade_hits(r, scene, H.d_rays.p, H.d_hits.p, n, H.d_color.as<float4>())) != ARCTIC_OK || n == 0) return rc;
    return read_back(r, rgba32f, H.d_color, n * 16);
}

namespace {
// the checks, the G-buffer and the three launches of both reflection calls; d_out: the caller's device memory, or null = the handle's own
int trace_reflections(ArcticRenderer *r, const ArcticScene *scene, float bias, float4 *d_out, const char *who) {
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (!std::isfinite(bias)) return r->fail(ARCTIC_E_INVALID, "%s: the bias is not finite", who);
    const uint64_t n = (uint64_t)r->rows() * r->width;
    int rc = gbuffer_refusal(r, who);
    if (rc || (rc = sun_map_ready(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    if ((rc = gbuffer_in_place(r)) != ARCTIC_OK || (rc = ensure_ray_scene(r, scene)) != ARCTIC_OK) return rc;
    ArcticRenderer::HitScene &H = r->hit;
    HIPCHECK(r, H.d_rays.ensure(std::max<uint64_t>(n, 1) * sizeof(ArcticRay)));
    HIPCHECK(r, H.d_hits.ensure(std::max<uint64_t>(n, 1) * sizeof(ArcticHit)));
    if (!d_out) { HIPCHECK(r, H.d_color.ensure(std::max<uint64_t>(n, 1) * 16)); d_out = H.d_color.as<float4>(); }
    const GBuffer g = r->gbuffer();
    HIPCHECK(r, launch_reflect_rays(g.b, g.c, g.e, r->tiles_x, r->tiles_y, r->width, r->rows(), r->row0_in_tile, scene->camera.eye, bias, H.d_rays.p, r->stream));
    HIPCHECK(r, launch_trace(H.d_rays.p, n, r->ray.d_nodes.p, r->ray.d_tris.p, (uint32_t)r->ray.n_nodes, 0, H.d_hits.p, r->stream));
    return shade_hits(r, scene, H.d_rays.p, H.d_hits.p, n, d_out);
}
}  // namespace

int arctic_trace_reflections(ArcticRenderer *r, const ArcticScene *scene, float bias, float *rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = trace_reflections(r, scene, bias, nullptr, "trace_reflections");
    if (rc || !rgba32f) return rc;
    return read_back(r, rgba32f, r->hit.d_color, (size_t)r->rows() * r->width * 16, FROM_FRAME);
}

int arctic_trace_reflections_device(ArcticRenderer *r, const ArcticScene *scene, float bias, float *d_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_rgba32f || ((uintptr_t)d_rgba32f & 15u)) return r->fail(ARCTIC_E_INVALID, "trace_reflections_device: the output is null or not 16-byte aligned");
    return trace_reflections(r, scene, bias, reinterpret_cast<float4 *>(d_rgba32f), "trace_reflections_device");
}

int arctic_hit_shading_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "hit_shading_info: null");
    out4[0] = r->hit.device_bytes(); out4[1] = r->hit.pinned_bytes(); out4[2] = r->hit.n_prims; out4[3] = r->hit.tables_made;
    return ARCTIC_OK;
}

// ---- the composition (the definition: include/arctic_hip.h; the arithmetic: compose.h; the kernel: compose.hip) -----------------------------------
namespace {
// what both calls refuse with ARCTIC_E_INVALID for the composition's own sake; ao, refl: the planes k_compose will read
int compose_checks(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, const ArcticRayCompose *c, const void *ao, const void *refl, ComposeDesc &d, const char *who) {
    if (!valid_scene(sc) || !st) return r->fail(ARCTIC_E_INVALID, "%s: null scene or settings", who);
    if (c) std::memcpy(&d, c, sizeof d);
    const char *why = compose_refusal(c ? &d : nullptr);
    if (why || (why = compose_plane_refusal(d, ao, refl, 16u)) != nullptr) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    return ARCTIC_OK;
}
// ... and with ARCTIC_E_STATE, in the header's order: no side effect
int compose_states(ArcticRenderer *r, const ComposeDesc &d, const char *who) {
    int rc = gbuffer_refusal(r, who);
    if (rc) return rc;
    if ((rc = source_refusal(r, {HdrSource::Shaded, ""}, who)) != ARCTIC_OK) return rc;   // (the float HDR plane of the latest shading: post_source.cpp)
    if (d.flags & COMPOSE_AO) {
        if (const char *why = ambient_term_refusal(r)) return r->fail(ARCTIC_E_STATE, "%s: ARCTIC_COMPOSE_AO: %s, so the frame's ambient term is not ambient * base_color at level 0", who, why);
    }
    return ARCTIC_OK;
}
// the G-buffer, the handle's buffers and the launch: device pointers throughout; d_out: the caller's RGBA8, or null = the handle's own
int compose_planes(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, const ComposeDesc &d, const uint8_t *d_ao, const float *d_refl, uint8_t *d_out) {
    int rc = gbuffer_in_place(r);
    if (rc) return rc;
    ArcticRenderer::Compose &K = r->compose;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    if (!d_out) HIPCHECK(r, K.d_rgba8.ensure(std::max<uint64_t>(n, 1) * 4));
    HIPCHECK(r, K.d_ldr.ensure(std::max<uint64_t>(n, 1) * 12));
    HIPCHECK(r, K.d_hdr.ensure(std::max<uint64_t>(n, 1) * 12));
    const GBuffer g = r->gbuffer();
    ComposeParams p = {};
    p.plane_a = g.a; p.plane_b = g.b; p.plane_c = g.c; p.plane_e = g.e;
    p.tex = r->d_tex.as<TexDesc>(); p.srgb_lut = r->d_lut.as<float>();
    p.hdr = r->d_hdr.as<float>();
    p.ao = (d.flags & COMPOSE_AO) ? d_ao : nullptr; p.refl = (d.flags & COMPOSE_REFLECTIONS) ? d_refl : nullptr;
    p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : K.d_rgba8.as<uint8_t>()); p.out_ldr = K.d_ldr.as<float>(); p.out_hdr = K.d_hdr.as<float>();
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows(); p.row0_in_tile = r->row0_in_tile;
    p.n_materials = (uint32_t)(r->tex.size() / 3); p.flags = d.flags;
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.ao_strength = d.ao_strength; p.reflection_strength = d.reflection_strength; p.ambient = sc->ambient;
    std::memcpy(p.eye, sc->camera.eye, sizeof p.eye);
    HIPCHECK(r, launch_compose(p, r->stream));
    K.pixels = n; K.own_rgba8 = d_out == nullptr; K.flags = d.flags; ++K.launches;
    return ARCTIC_OK;
}
}  // namespace

int arctic_compose_planes_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                 const uint8_t *d_ao_u8, const float *d_reflection_rgba32f, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    ComposeDesc d;
    int rc = compose_checks(r, scene, settings, compose, d_ao_u8, d_reflection_rgba32f, d, "compose_planes_device");
    if (rc) return rc;
    if (d_out_rgba8 && ((uintptr_t)d_out_rgba8 & 3u)) return r->fail(ARCTIC_E_INVALID, "compose_planes_device: the output is not 4-byte aligned");
    if ((rc = compose_states(r, d, "compose_planes_device")) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return compose_planes(r, scene, settings, d, d_ao_u8, d_reflection_rgba32f, d_out_rgba8);
}

int arctic_pass_ray_effects(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                            const ArcticAmbientOcclusion *ao, const float *dirs, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_ray_effects";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    ComposeDesc d;
    int rc = compose_checks(r, scene, settings, compose, own_plane, own_plane, d, who);
    if (rc) return rc;
    if (d_out_rgba8 && ((uintptr_t)d_out_rgba8 & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the output is not 4-byte aligned", who);
    // every refusal of the two tracing calls, in front of the first launch (the calls below make them again, in their own words, to no effect)
    AoDesc a = {};
    if (d.flags & COMPOSE_AO) {
        if (ao) std::memcpy(&a, ao, sizeof a);
        if (const char *why = ao_refusal(ao ? &a : nullptr, dirs)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    }
    if ((d.flags & COMPOSE_REFLECTIONS) && !std::isfinite(d.reflection_bias)) return r->fail(ARCTIC_E_INVALID, "%s: the reflection bias is not finite", who);
    if ((rc = compose_states(r, d, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_AO) && a.filter && r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the filter needs the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = sun_map_ready(r, who)) != ARCTIC_OK) return rc;
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_AO) && (rc = trace_ambient_occlusion(r, scene, ao, dirs, nullptr, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = trace_reflections(r, scene, d.reflection_bias, nullptr, who)) != ARCTIC_OK) return rc;
    if ((rc = compose_planes(r, scene, settings, d, r->ao.d_out.as<uint8_t>(), r->hit.d_color.as<float>(), d_out_rgba8)) != ARCTIC_OK) return rc;
    ++r->compose.passes;
    return ARCTIC_OK;
}

int arctic_read_composed(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Compose &K = r->compose;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    if (!K.pixels || K.pixels != n) return r->fail(ARCTIC_E_STATE, "read_composed: nothing composed yet, or not since the last resize");
    if (rgba8 && !K.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_composed: the latest composition wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, K.d_ldr.p, n * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, K.d_hdr.p, n * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, K.d_rgba8.p, n * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_compose_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "compose_info: null");
    out4[0] = r->compose.device_bytes(); out4[1] = r->compose.launches; out4[2] = r->compose.passes; out4[3] = 0;
    return ARCTIC_OK;
}

// ---- temporal accumulation of the occlusion plane (the definition: include/arctic_hip.h; the arithmetic: ao_history.h; the kernel: ao_history.hip) --
namespace {
// what the calls refuse with ARCTIC_E_INVALID for the accumulation's own sake; in, out: the planes k_ao_accumulate will read and write
int accumulate_checks(ArcticRenderer *r, const ArcticScene *sc, const ArcticAoHistory *hist, const void *in, const void *out, AoHistoryDesc &d, const char *who) {
    if (!valid_scene(sc)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (!hist || !in || !out) return r->fail(ARCTIC_E_INVALID, "%s: null parameters or plane", who);
    std::memcpy(&d, hist, sizeof d);
    if (const char *why = ao_history_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    return ARCTIC_OK;
}
// ... and with ARCTIC_E_STATE: no side effect
int accumulate_states(ArcticRenderer *r, const char *who) {
    int rc = gbuffer_refusal(r, who);
    if (rc) return rc;
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the history's taps need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return ARCTIC_OK;
}
// the G-buffer, the history sets and the launch: device pointers throughout.  The handle's state moves only behind a launch that was enqueued.
// d_prev_world4: the motion form (k_ao_accumulate_motion reads that plane); null: the plain one (k_ao_accumulate).  Both share the history
int accumulate_planes(ArcticRenderer *r, const ArcticScene *sc, const AoHistoryDesc &d, const uint8_t *d_in, uint8_t *d_out, const void *d_prev_world4 = nullptr) {
    int rc = gbuffer_in_place(r);
    if (rc) return rc;
    ArcticRenderer::AoHistory &A = r->ao_history;
    const size_t plane = std::max<size_t>(r->n_tiles(), 1) * TILE_PIXELS * 16;
    for (DevBuf *b : {&A.d_a[0], &A.d_a[1], &A.d_b[0], &A.d_b[1]})
        if (b->cap < plane) HIPCHECK(r, b->alloc_exact(plane));   // (no headroom: the four planes are 64 bytes per pixel as the header says, 531 MB at 4K)
    const bool have = A.valid && A.width == r->width && A.height == r->height;
    const int from = A.cur, to = A.cur ^ 1;
    const GBuffer g = r->gbuffer();
    AoHistoryParams p = {};
    p.plane_b = g.b; p.plane_c = g.c; p.plane_e = g.e;
    p.prev_a = have ? A.d_a[from].p : nullptr; p.prev_b = have ? A.d_b[from].p : nullptr;
    p.next_a = A.d_a[to].p; p.next_b = A.d_b[to].p;
    p.ao_in = d_in; p.ao_out = d_out;
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.d = d;
    if (have) std::memcpy(p.P, A.proj_view, sizeof p.P);
    HIPCHECK(r, d_prev_world4 ? launch_ao_accumulate_motion(p, d_prev_world4, r->stream) : launch_ao_accumulate(p, r->stream));
    const ArcticCamera &c = sc->camera;
    camera_proj_view(c.eye, c.rotation, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], A.proj_view);
    A.cur = to; A.valid = true; A.width = r->width; A.height = r->height;
    ++A.launches; ++A.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_accumulate_ambient_occlusion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const uint8_t *d_ao_in_u8, uint8_t *d_ao_out_u8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_ambient_occlusion_device";
    AoHistoryDesc d;
    int rc = accumulate_checks(r, scene, hist, d_ao_in_u8, d_ao_out_u8, d, who);
    if (rc || (rc = accumulate_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return accumulate_planes(r, scene, d, d_ao_in_u8, d_ao_out_u8);
}

int arctic_accumulate_ambient_occlusion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const uint8_t *ao_in, uint8_t *ao_out) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_ambient_occlusion";
    AoHistoryDesc d;
    int rc = accumulate_checks(r, scene, hist, ao_in, ao_out, d, who);
    if (rc || (rc = accumulate_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    const size_t bytes = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->d_stage.ensure(std::max<size_t>(bytes, 16)));
    HIPCHECK(r, hipMemcpyAsync(r->d_stage.p, ao_in, bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = accumulate_planes(r, scene, d, r->d_stage.as<uint8_t>(), r->d_stage.as<uint8_t>())) != ARCTIC_OK) return rc;
    return read_back(r, ao_out, r->d_stage, bytes, FROM_FRAME);
}

int arctic_ao_history_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->ao_history.valid = false;   // (the planes stay: a call in flight may still write them, and the next call reuses them)
    r->ao_history.calls = 0;
    return ARCTIC_OK;
}

int arctic_read_ao_history(ArcticRenderer *r, float *value, float *count, float *world3, float *normal3) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::AoHistory &A = r->ao_history;
    if (!A.valid || A.width != r->width || A.height != r->height || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_ao_history: the history is empty (no call yet, or none since the last reset or resize)");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t n = r->n_tiles() * TILE_PIXELS;
    std::vector<float> a(n * 4), b(n * 4);
    HIPCHECK(r, hipMemcpy(a.data(), A.d_a[A.cur].p, n * 16, hipMemcpyDeviceToHost));
    HIPCHECK(r, hipMemcpy(b.data(), A.d_b[A.cur].p, n * 16, hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < r->height; ++y)
        for (uint32_t x = 0; x < r->width; ++x) {
            const size_t q = ((size_t)(y / TILE) * r->tiles_x + x / TILE) * TILE_PIXELS + (y % TILE) * TILE + x % TILE, o = (size_t)y * r->width + x;
            if (value) value[o] = a[4 * q + 3];
            if (count) count[o] = b[4 * q + 3];
            for (int i = 0; i < 3; ++i) {
                if (world3) world3[3 * o + i] = a[4 * q + i];
                if (normal3) normal3[3 * o + i] = b[4 * q + i];
            }
        }
    return ARCTIC_OK;
}

int arctic_ao_history_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "ao_history_info: null");
    out4[0] = r->ao_history.device_bytes(); out4[1] = r->ao_history.launches; out4[2] = r->ao_history.calls; out4[3] = 0;
    return ARCTIC_OK;
}

int arctic_pass_ray_effects_temporal(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                     const ArcticAmbientOcclusion *ao, const float *dirs, const ArcticAoHistory *hist, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_ray_effects_temporal";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    ComposeDesc d;
    int rc = compose_checks(r, scene, settings, compose, own_plane, own_plane, d, who);
    if (rc) return rc;
    if (!(d.flags & COMPOSE_AO)) return r->fail(ARCTIC_E_INVALID, "%s: ARCTIC_COMPOSE_AO is not set: there is nothing to accumulate (arctic_pass_ray_effects)", who);
    if (d_out_rgba8 && ((uintptr_t)d_out_rgba8 & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the output is not 4-byte aligned", who);
    // every refusal of the calls below, in front of the first launch (they make them again, in their own words, to no effect)
    AoDesc a = {};
    if (ao) std::memcpy(&a, ao, sizeof a);
    if (const char *why = ao_refusal(ao ? &a : nullptr, dirs)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    AoHistoryDesc h;
    if ((rc = accumulate_checks(r, scene, hist, own_plane, own_plane, h, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && !std::isfinite(d.reflection_bias)) return r->fail(ARCTIC_E_INVALID, "%s: the reflection bias is not finite", who);
    if ((rc = compose_states(r, d, who)) != ARCTIC_OK || (rc = accumulate_states(r, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = sun_map_ready(r, who)) != ARCTIC_OK) return rc;
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    if ((rc = trace_ambient_occlusion(r, scene, ao, dirs, nullptr, who)) != ARCTIC_OK) return rc;
    if ((rc = accumulate_planes(r, scene, h, r->ao.d_out.as<uint8_t>(), r->ao.d_out.as<uint8_t>())) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = trace_reflections(r, scene, d.reflection_bias, nullptr, who)) != ARCTIC_OK) return rc;
    if ((rc = compose_planes(r, scene, settings, d, r->ao.d_out.as<uint8_t>(), r->hit.d_color.as<float>(), d_out_rgba8)) != ARCTIC_OK) return rc;
    ++r->compose.passes;
    return ARCTIC_OK;
}

// ---- motion vectors and the accumulation that uses them (the definition: include/arctic_hip.h; the arithmetic: motion.h; the kernels: motion.hip) ---
}  // extern "C"
namespace arctic {   // (renderer_state.h: arctic_pass_taa and arctic_pass_motion_blur call these)
// what the motion calls refuse, in the header's order: no side effect
int motion_refusal(ArcticRenderer *r, const ArcticScene *sc, const void *prev_world4, const char *who) {
    if (!valid_scene(sc) || !prev_world4) return r->fail(ARCTIC_E_INVALID, "%s: null scene or prev_world4 plane", who);
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    return ARCTIC_OK;
}
// The table, k_motion, the snapshots, then M becomes this call's scene: device pointers throughout, everything enqueued on the handle's stream.
// Whatever can fail is done in front of the first launch; the handle's state moves only behind the launches
int motion_planes(ArcticRenderer *r, const ArcticScene *sc, float4 *d_pw, float2 *d_vel, float *d_bary, uint4 *d_src) {
    ArcticRenderer::Motion &M = r->motion;
    const bool have = M.valid && M.width == r->width && M.height == r->height;
    if (M.shapes.size() < r->meshes.size()) M.shapes.resize(r->meshes.size());
    HIPCHECK(r, M.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, M.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    // the table, in the prepass's order: the scene's objects whose mesh exists
    size_t n_tab = 0;
    for (uint64_t i = 0; i < sc->n_objects; ++i) n_tab += sc->objects[i].mesh_idx < r->meshes.size() ? 1 : 0;
    const size_t bytes = std::max<size_t>(n_tab, 1) * sizeof(MotionObject);
    MotionObject *h_objs = nullptr;
    HIPCHECK(r, M.objs_ring.stage(bytes, &h_objs));
    HIPCHECK(r, M.d_objs.ensure(bytes));
    std::vector<uint64_t> to_snap;   // the meshes whose snapshot this call writes: deformed, and not stamped with the shape they have
    size_t k = 0;
    for (uint64_t i = 0; i < sc->n_objects; ++i) {
        const ArcticObject &o = sc->objects[i];
        if (o.mesh_idx >= r->meshes.size()) continue;
        const Mesh &m = r->meshes[o.mesh_idx];
        ArcticRenderer::Motion::Shape &S = M.shapes[o.mesh_idx];
        MotionObject &d = h_objs[k++];
        d = MotionObject{};
        d.n_vertices = m.n_vertices; d.scene_object = (uint32_t)std::min<uint64_t>(i, 0xFFFFFFFEull);
        // step 3: M is not empty, the previous call's list had this entry, and it named the same mesh (which that call therefore saw)
        if (have && i < M.objects.size() && M.objects[i].mesh == o.mesh_idx && S.seen_call == M.call_id) {
            std::memcpy(d.prev_trs, M.objects[i].trs, sizeof d.prev_trs);
            if (S.seq_at_call == m.shape_seq) { d.prev = m.vertices_in_use(); d.stride = 14; }             // the shape has not moved since
            else if (S.rigid_at_call) { d.prev = m.d_vertices.as<float>(); d.stride = 14; }               // it was the mesh's own buffer then
            else if (S.d_snap && S.stamp == S.seq_at_call && S.n_vertices == m.n_vertices) { d.prev = S.d_snap.as<float>(); d.stride = 4; }
            d.has_prev = d.prev != nullptr;
        }
        if (m.deformed() && !(S.d_snap && S.stamp == m.shape_seq && S.n_vertices == m.n_vertices) && std::find(to_snap.begin(), to_snap.end(), o.mesh_idx) == to_snap.end())
            to_snap.push_back(o.mesh_idx);
    }
    for (uint64_t mi : to_snap) {   // (a snapshot is made once per mesh: its size never changes, so the buffer a table entry above points at stays)
        ArcticRenderer::Motion::Shape &S = M.shapes[mi];
        const Mesh &m = r->meshes[mi];
        if (!S.d_snap || S.n_vertices != m.n_vertices) {
            S.stamp = ~0ull;
            HIPCHECK(r, S.d_snap.alloc_exact(std::max<size_t>(m.n_vertices, 1) * 16));
            S.n_vertices = m.n_vertices;
        }
    }
    HIPCHECK(r, M.objs_ring.send(M.d_objs.p, n_tab * sizeof(MotionObject), r->stream));
    const int f = r->fwd();
    MotionParams p = {};
    p.vis = r->d_vis().as<unsigned long long>();
    p.recs = r->geo[f].d_recs.as<SetupRec>(); p.rrecs = r->geo[f].d_rrecs.as<RasterRec>(); p.rec_of = r->geo[f].d_rec_of.as<uint32_t>();
    p.objs = r->tables[f].objs; p.mobjs = M.d_objs.as<MotionObject>();
    p.n_objs = (uint32_t)n_tab; p.n_tiles = (uint32_t)r->n_tiles(); p.width = r->width; p.height = r->height; p.rows = r->rows(); p.row0_in_tile = r->row0_in_tile;
    p.gp = r->tables[f].gp;
    if (have) std::memcpy(p.P, M.proj_view, sizeof p.P);
    p.prev_world4 = d_pw; p.velocity2 = d_vel; p.bary3 = d_bary; p.source4 = d_src;
    HIPCHECK(r, launch_motion(p, r->stream));
    ++M.launches;
    M.valid = false;   // (until the snapshots below are enqueued too: a failure between leaves M empty, never half this call's)
    for (uint64_t mi : to_snap) {
        ArcticRenderer::Motion::Shape &S = M.shapes[mi];
        const Mesh &m = r->meshes[mi];
        HIPCHECK(r, launch_motion_snapshot(m.vertices_in_use(), m.n_vertices, S.d_snap.p, r->stream));
        S.stamp = m.shape_seq;
        ++M.snapshot_launches;
    }
    HIPCHECK(r, M.written.record(r->stream));
    // M becomes this call's scene
    ++M.call_id;
    M.objects.resize((size_t)sc->n_objects);
    for (uint64_t i = 0; i < sc->n_objects; ++i) {
        const ArcticObject &o = sc->objects[i];
        M.objects[(size_t)i].mesh = o.mesh_idx;
        std::memcpy(M.objects[(size_t)i].trs, o.trs, sizeof o.trs);
        if (o.mesh_idx >= r->meshes.size()) continue;
        const Mesh &m = r->meshes[o.mesh_idx];
        ArcticRenderer::Motion::Shape &S = M.shapes[o.mesh_idx];
        S.seq_at_call = m.shape_seq; S.rigid_at_call = !m.deformed(); S.seen_call = M.call_id;
    }
    const ArcticCamera &c = sc->camera;
    camera_proj_view(c.eye, c.rotation, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], M.proj_view);
    M.width = r->width; M.height = r->height; M.valid = true;
    ++M.calls;
    return ARCTIC_OK;
}
}  // namespace arctic
extern "C" {

int arctic_motion_vectors_device(ArcticRenderer *r, const ArcticScene *scene, float *d_prev_world4, float *d_velocity2) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "motion_vectors_device";
    if (((uintptr_t)d_prev_world4 & 15u) || ((uintptr_t)d_velocity2 & 7u)) return r->fail(ARCTIC_E_INVALID, "%s: prev_world4 must be 16-byte aligned, velocity2 8-byte aligned", who);
    int rc = motion_refusal(r, scene, d_prev_world4, who);
    if (rc || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return motion_planes(r, scene, reinterpret_cast<float4 *>(d_prev_world4), reinterpret_cast<float2 *>(d_velocity2), nullptr, nullptr);
}

int arctic_motion_vectors(ArcticRenderer *r, const ArcticScene *scene, float *prev_world4, float *velocity2, float *bary3, uint32_t *source4) {
    if (!r) return ARCTIC_E_INVALID;
    alignas(16) static const char own_plane[16] = {};   // (the plane k_motion writes is the handle's own: never null)
    int rc = motion_refusal(r, scene, own_plane, "motion_vectors");
    if (rc || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Motion &M = r->motion;
    const size_t n = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, M.d_pw.ensure(n * 16));
    if (velocity2) HIPCHECK(r, M.d_vel.ensure(n * 8));
    if (bary3) HIPCHECK(r, M.d_bary.ensure(n * 12));
    if (source4) HIPCHECK(r, M.d_src.ensure(n * 16));
    if ((rc = motion_planes(r, scene, M.d_pw.as<float4>(), velocity2 ? M.d_vel.as<float2>() : nullptr, bary3 ? M.d_bary.as<float>() : nullptr,
                            source4 ? M.d_src.as<uint4>() : nullptr)) != ARCTIC_OK) return rc;
    const size_t px = (size_t)r->rows() * r->width;
    if (prev_world4) HIPCHECK(r, hipMemcpyAsync(prev_world4, M.d_pw.p, px * 16, hipMemcpyDeviceToHost, r->stream));
    if (velocity2) HIPCHECK(r, hipMemcpyAsync(velocity2, M.d_vel.p, px * 8, hipMemcpyDeviceToHost, r->stream));
    if (bary3) HIPCHECK(r, hipMemcpyAsync(bary3, M.d_bary.p, px * 12, hipMemcpyDeviceToHost, r->stream));
    if (source4) HIPCHECK(r, hipMemcpyAsync(source4, M.d_src.p, px * 16, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return check_item_overflow(r);
}

int arctic_motion_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->motion.valid = false;   // (the snapshots and the table stay: a call in flight may still read them, and the next call reuses them)
    r->motion.calls = 0;
    return ARCTIC_OK;
}

int arctic_motion_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "motion_info: null");
    out4[0] = r->motion.device_bytes(); out4[1] = r->motion.launches; out4[2] = r->motion.snapshot_launches; out4[3] = r->motion.calls;
    return ARCTIC_OK;
}

int arctic_accumulate_ambient_occlusion_motion_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const float *d_prev_world4,
                                                      const uint8_t *d_ao_in_u8, uint8_t *d_ao_out_u8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_ambient_occlusion_motion_device";
    AoHistoryDesc d;
    int rc = accumulate_checks(r, scene, hist, d_ao_in_u8, d_ao_out_u8, d, who);
    if (rc) return rc;
    if (!d_prev_world4 || ((uintptr_t)d_prev_world4 & 15u)) return r->fail(ARCTIC_E_INVALID, "%s: the prev_world4 plane is null or not 16-byte aligned", who);
    if ((rc = accumulate_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return accumulate_planes(r, scene, d, d_ao_in_u8, d_ao_out_u8, d_prev_world4);
}

int arctic_accumulate_ambient_occlusion_motion(ArcticRenderer *r, const ArcticScene *scene, const ArcticAoHistory *hist, const float *prev_world4, const uint8_t *ao_in,
                                               uint8_t *ao_out) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_ambient_occlusion_motion";
    AoHistoryDesc d;
    int rc = accumulate_checks(r, scene, hist, ao_in, ao_out, d, who);
    if (rc) return rc;
    if (!prev_world4) return r->fail(ARCTIC_E_INVALID, "%s: null prev_world4 plane", who);
    if ((rc = accumulate_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    const size_t px = (size_t)r->rows() * r->width;
    HIPCHECK(r, r->d_stage.ensure(std::max<size_t>(px, 16)));
    HIPCHECK(r, r->motion.d_plane.ensure(std::max<size_t>(px, 1) * 16));
    HIPCHECK(r, hipMemcpyAsync(r->d_stage.p, ao_in, px, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(r, hipMemcpyAsync(r->motion.d_plane.p, prev_world4, px * 16, hipMemcpyHostToDevice, r->stream));
    if ((rc = accumulate_planes(r, scene, d, r->d_stage.as<uint8_t>(), r->d_stage.as<uint8_t>(), r->motion.d_plane.p)) != ARCTIC_OK) return rc;
    return read_back(r, ao_out, r->d_stage, px, FROM_FRAME);
}

int arctic_pass_ray_effects_motion(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticRayCompose *compose,
                                   const ArcticAmbientOcclusion *ao, const float *dirs, const ArcticAoHistory *hist, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_ray_effects_motion";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    ComposeDesc d;
    int rc = compose_checks(r, scene, settings, compose, own_plane, own_plane, d, who);
    if (rc) return rc;
    if (!(d.flags & COMPOSE_AO)) return r->fail(ARCTIC_E_INVALID, "%s: ARCTIC_COMPOSE_AO is not set: there is nothing to accumulate (arctic_pass_ray_effects)", who);
    if (d_out_rgba8 && ((uintptr_t)d_out_rgba8 & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the output is not 4-byte aligned", who);
    // every refusal of the calls below, in front of the first launch (they make them again, in their own words, to no effect)
    AoDesc a = {};
    if (ao) std::memcpy(&a, ao, sizeof a);
    if (const char *why = ao_refusal(ao ? &a : nullptr, dirs)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    AoHistoryDesc h;
    if ((rc = accumulate_checks(r, scene, hist, own_plane, own_plane, h, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && !std::isfinite(d.reflection_bias)) return r->fail(ARCTIC_E_INVALID, "%s: the reflection bias is not finite", who);
    if ((rc = motion_refusal(r, scene, own_plane, who)) != ARCTIC_OK) return rc;
    if ((rc = compose_states(r, d, who)) != ARCTIC_OK || (rc = accumulate_states(r, who)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = sun_map_ready(r, who)) != ARCTIC_OK) return rc;
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Motion &M = r->motion;
    HIPCHECK(r, M.d_plane.ensure(std::max<size_t>((size_t)r->rows() * r->width, 1) * 16));
    if ((rc = motion_planes(r, scene, M.d_plane.as<float4>(), nullptr, nullptr, nullptr)) != ARCTIC_OK) return rc;
    if ((rc = trace_ambient_occlusion(r, scene, ao, dirs, nullptr, who)) != ARCTIC_OK) return rc;
    if ((rc = accumulate_planes(r, scene, h, r->ao.d_out.as<uint8_t>(), r->ao.d_out.as<uint8_t>(), M.d_plane.p)) != ARCTIC_OK) return rc;
    if ((d.flags & COMPOSE_REFLECTIONS) && (rc = trace_reflections(r, scene, d.reflection_bias, nullptr, who)) != ARCTIC_OK) return rc;
    if ((rc = compose_planes(r, scene, settings, d, r->ao.d_out.as<uint8_t>(), r->hit.d_color.as<float>(), d_out_rgba8)) != ARCTIC_OK) return rc;
    ++r->compose.passes;
    return ARCTIC_OK;
}

}  // extern "C"
