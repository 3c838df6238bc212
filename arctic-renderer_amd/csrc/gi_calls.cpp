// gi_calls.cpp -- the indirect diffuse light's calls of the C-ABI (include/arctic_hip.h: arctic_trace_gi and the definition in front of it; the
// arithmetic: gi.h; the kernels: gi.hip; the arbiters: gi.cpp).  Of the handle (renderer_state.h) it owns ArcticRenderer::Gi, writes the
// reflection plane's rays, hits and colours (HitScene::d_rays, d_hits, d_color: a round's scratch) and reads the G-buffer planes, the material
// table and -- the composition -- the float HDR plane of the latest shading or composition (post_source.cpp); the walk and the radiance are the
// ray family's own steps (ensure_ray_scene, launch_trace, shade_hits), unchanged.  Enqueues on r->stream only.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "gi.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order
int gi_checks(ArcticRenderer *r, const ArcticGi *gi, const float *dirs, GiDesc &d, const char *who) {
    if (gi) std::memcpy(&d, gi, sizeof d);
    if (const char *why = gi_refusal(gi ? &d : nullptr, dirs)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    return ARCTIC_OK;
}
// ... and with ARCTIC_E_STATE: no side effect.  shaded: the call goes on to k_shade_hits, which needs the sun's map
int gi_states(ArcticRenderer *r, const GiDesc &d, bool shaded, const char *who) {
    int rc = gbuffer_refusal(r, who);
    if (rc || (shaded && (rc = sun_map_ready(r, who)) != ARCTIC_OK)) return rc;
    if (shaded && d.filter && r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the filter needs the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return ARCTIC_OK;
}
// the table on the device: sent again only when its bytes changed (the occlusion's rule, with a table and a ring of this stage's own)
int gi_table(ArcticRenderer *r, const GiDesc &d, const float *dirs) {
    ArcticRenderer::Gi &G = r->gi;
    const size_t n_floats = (size_t)d.pattern * d.pattern * d.n_rays * 3;
    const size_t table_bytes = 16 * GI_MAX_RAYS * 3 * sizeof(float);   // the largest table: the slot and d_dirs are made once
    if (G.n_floats != n_floats || std::memcmp(G.dirs_ring.slot[0].h.p, dirs, n_floats * sizeof(float)) != 0) {   // (n_floats != 0: an empty G holds no table)
        float *h_dirs = nullptr;
        HIPCHECK(r, G.dirs_ring.stage(table_bytes, &h_dirs));
        HIPCHECK(r, G.d_dirs.ensure(table_bytes));
        G.n_floats = 0;
        std::memcpy(h_dirs, dirs, n_floats * sizeof(float));
        HIPCHECK(r, G.dirs_ring.send(G.d_dirs.p, n_floats * sizeof(float), r->stream));
        G.n_floats = n_floats;
    }
    return ARCTIC_OK;
}
// round k's records into the reflection plane's ray buffer
int gi_round_rays(ArcticRenderer *r, const GiDesc &d, uint32_t round) {
    const GBuffer g = r->gbuffer();
    // (a band's first row is a multiple of 8 in the frame and in the shard alike, so the shard's row and the frame's agree modulo the pattern)
    const uint32_t frame_row0 = r->band_rows ? 0u : r->row_begin;
    HIPCHECK(r, launch_gi_rays(g.b, g.c, g.e, r->tiles_x, r->tiles_y, r->width, r->rows(), r->row0_in_tile, frame_row0, d, round, r->gi.d_dirs.as<float>(), r->hit.d_rays.p, r->stream));
    ++r->gi.launches;
    return ARCTIC_OK;
}
// the G-buffer, the structure, the table and the launches of both tracing calls; d_out: the caller's device plane, or null = the handle's own
int trace_gi(ArcticRenderer *r, const ArcticScene *scene, const GiDesc &d, const float *dirs, float *d_out) {
    int rc;
    if ((rc = gbuffer_in_place(r)) != ARCTIC_OK || (rc = ensure_ray_scene(r, scene)) != ARCTIC_OK || (rc = gi_table(r, d, dirs)) != ARCTIC_OK) return rc;
    ArcticRenderer::Gi &G = r->gi;
    ArcticRenderer::HitScene &H = r->hit;
    const uint64_t n = (uint64_t)r->rows() * r->width, cap = std::max<uint64_t>(n, 1);
    HIPCHECK(r, H.d_rays.ensure(cap * sizeof(ArcticRay)));
    HIPCHECK(r, H.d_hits.ensure(cap * sizeof(ArcticHit)));
    HIPCHECK(r, H.d_color.ensure(cap * 16));
    HIPCHECK(r, G.d_sum.ensure(cap * 16));
    if (!d_out) { HIPCHECK(r, G.d_estimate.ensure(cap * 16)); d_out = G.d_estimate.as<float>(); }
    G.pixels = 0;   // (until the estimate is enqueued: a failure leaves nothing to read)
    for (uint32_t k = 0; k < d.n_rays; ++k) {
        if ((rc = gi_round_rays(r, d, k)) != ARCTIC_OK) return rc;
        HIPCHECK(r, launch_trace(H.d_rays.p, n, r->ray.d_nodes.p, r->ray.d_tris.p, (uint32_t)r->ray.n_nodes, 0, H.d_hits.p, r->stream));
        if ((rc = shade_hits(r, scene, H.d_rays.p, H.d_hits.p, n, H.d_color.as<float4>())) != ARCTIC_OK) return rc;
        HIPCHECK(r, launch_gi_add(H.d_rays.p, H.d_color.p, n, d.clamp_max, k, G.d_sum.p, r->stream));
        ++G.launches;
    }
    const GBuffer g = r->gbuffer();
    HIPCHECK(r, launch_gi_estimate(g.b, g.c, g.e, r->tiles_x, r->tiles_y, r->width, r->rows(), d, G.d_sum.p, d_out, r->stream));
    ++G.launches; ++G.calls;
    G.pixels = n; G.own_estimate = d_out == G.d_estimate.as<float>();
    return ARCTIC_OK;
}
// both tracing calls up to the launches
int trace_gi_call(ArcticRenderer *r, const ArcticScene *scene, const ArcticGi *gi, const float *dirs, float *d_out, const char *who) {
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    GiDesc d;
    int rc = gi_checks(r, gi, dirs, d, who);
    if (rc || (rc = gi_states(r, d, true, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return trace_gi(r, scene, d, dirs, d_out);
}
}  // namespace

int arctic_trace_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticGi *gi, const float *dirs, float *rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    int rc = trace_gi_call(r, scene, gi, dirs, nullptr, "trace_gi");
    if (rc || !rgba32f) return rc;
    return read_back(r, rgba32f, r->gi.d_estimate, (size_t)r->rows() * r->width * 16, FROM_FRAME);
}

int arctic_trace_gi_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticGi *gi, const float *dirs, float *d_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_rgba32f || ((uintptr_t)d_rgba32f & 15u)) return r->fail(ARCTIC_E_INVALID, "trace_gi_device: the output is null or not 16-byte aligned");
    return trace_gi_call(r, scene, gi, dirs, d_rgba32f, "trace_gi_device");
}

int arctic_gi_rays(ArcticRenderer *r, const ArcticGi *gi, const float *dirs, uint32_t round, ArcticRay *rays) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "gi_rays";
    GiDesc d;
    int rc = gi_checks(r, gi, dirs, d, who);
    if (rc) return rc;
    if (round >= d.n_rays || !rays) return r->fail(ARCTIC_E_INVALID, "%s: round %u of %u, or a null output", who, round, d.n_rays);
    if ((rc = gi_states(r, d, false, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    if ((rc = gbuffer_in_place(r)) != ARCTIC_OK || (rc = gi_table(r, d, dirs)) != ARCTIC_OK) return rc;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    HIPCHECK(r, r->hit.d_rays.ensure(std::max<uint64_t>(n, 1) * sizeof(ArcticRay)));
    if ((rc = gi_round_rays(r, d, round)) != ARCTIC_OK) return rc;
    return read_back(r, rays, r->hit.d_rays, n * sizeof(ArcticRay), FROM_FRAME);
}

int arctic_read_gi_estimate(ArcticRenderer *r, float *sum_rgba32f, float *estimate_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Gi &G = r->gi;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    if (!G.pixels || G.pixels != n) return r->fail(ARCTIC_E_STATE, "read_gi_estimate: nothing traced yet, or not since the last resize");
    if (estimate_rgba32f && !G.own_estimate) return r->fail(ARCTIC_E_STATE, "read_gi_estimate: the latest call wrote the caller's plane, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (sum_rgba32f) HIPCHECK(r, hipMemcpy(sum_rgba32f, G.d_sum.p, n * 16, hipMemcpyDeviceToHost));
    if (estimate_rgba32f) HIPCHECK(r, hipMemcpy(estimate_rgba32f, G.d_estimate.p, n * 16, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_gi_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "gi_info: null");
    out4[0] = r->gi.device_bytes(); out4[1] = r->gi.launches; out4[2] = r->gi.calls; out4[3] = r->gi.history_bytes();
    return ARCTIC_OK;
}

// ---- stage 5: the temporal accumulation ---------------------------------------------------------------------------------------------------------
namespace {
// what the calls refuse with ARCTIC_E_INVALID for the accumulation's own sake; in, out: the planes k_gi_accumulate will read and write
int gi_history_checks(ArcticRenderer *r, const ArcticScene *sc, const ArcticGiHistory *hist, const void *in, const void *out, GiHistoryDesc &d, const char *who) {
    if (!valid_scene(sc)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (!hist || !in || !out) return r->fail(ARCTIC_E_INVALID, "%s: null parameters or plane", who);
    if (((uintptr_t)in | (uintptr_t)out) & 15u) return r->fail(ARCTIC_E_INVALID, "%s: the planes must be 16-byte aligned", who);
    std::memcpy(&d, hist, sizeof d);
    if (const char *why = ao_history_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    return ARCTIC_OK;
}
// ... and with ARCTIC_E_STATE: no side effect
int gi_history_states(ArcticRenderer *r, const char *who) {
    int rc = gbuffer_refusal(r, who);
    if (rc) return rc;
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the history's taps need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return ARCTIC_OK;
}
// the G-buffer, the history sets and the launch: device pointers throughout.  The handle's state moves only behind a launch that was enqueued
int gi_accumulate_planes(ArcticRenderer *r, const ArcticScene *sc, const GiHistoryDesc &d, const float *d_in, float *d_out) {
    int rc = gbuffer_in_place(r);
    if (rc) return rc;
    ArcticRenderer::Gi &G = r->gi;
    const size_t plane = std::max<size_t>(r->n_tiles(), 1) * TILE_PIXELS * 16;
    for (auto &set : G.d_hist)
        for (DevBuf &b : set)
            if (b.cap < plane) HIPCHECK(r, b.alloc_exact(plane));   // (no headroom: the six planes are 96 bytes per pixel as the header says)
    const bool have = G.hist_valid && G.hist_width == r->width && G.hist_height == r->height;
    const int from = G.hist_cur, to = G.hist_cur ^ 1;
    const GBuffer g = r->gbuffer();
    GiHistoryParams p = {};
    p.plane_b = g.b; p.plane_c = g.c; p.plane_e = g.e;
    for (int k = 0; k < 3; ++k) { p.prev[k] = have ? G.d_hist[from][k].p : nullptr; p.next[k] = G.d_hist[to][k].p; }
    p.gi_in = d_in; p.gi_out = d_out;
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.d = d;
    if (have) std::memcpy(p.P, G.proj_view, sizeof p.P);
    HIPCHECK(r, launch_gi_accumulate(p, r->stream));
    const ArcticCamera &c = sc->camera;
    camera_proj_view(c.eye, c.rotation, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], G.proj_view);
    G.hist_cur = to; G.hist_valid = true; G.hist_width = r->width; G.hist_height = r->height;
    ++G.launches; ++G.hist_calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_accumulate_gi_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticGiHistory *hist, const float *d_gi_in_rgba32f, float *d_gi_out_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_gi_device";
    GiHistoryDesc d;
    int rc = gi_history_checks(r, scene, hist, d_gi_in_rgba32f, d_gi_out_rgba32f, d, who);
    if (rc || (rc = gi_history_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return gi_accumulate_planes(r, scene, d, d_gi_in_rgba32f, d_gi_out_rgba32f);
}

int arctic_accumulate_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticGiHistory *hist, const float *gi_in_rgba32f, float *gi_out_rgba32f) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "accumulate_gi";
    alignas(16) static const char own_plane[16] = {};   // (the device plane is the handle's own: aligned)
    GiHistoryDesc d;
    int rc = gi_history_checks(r, scene, hist, gi_in_rgba32f ? own_plane : nullptr, gi_out_rgba32f ? own_plane : nullptr, d, who);
    if (rc || (rc = gi_history_states(r, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    const size_t bytes = (size_t)r->rows() * r->width * 16;
    HIPCHECK(r, r->d_stage.ensure(std::max<size_t>(bytes, 16)));
    HIPCHECK(r, hipMemcpyAsync(r->d_stage.p, gi_in_rgba32f, bytes, hipMemcpyHostToDevice, r->stream));
    if ((rc = gi_accumulate_planes(r, scene, d, r->d_stage.as<float>(), r->d_stage.as<float>())) != ARCTIC_OK) return rc;
    return read_back(r, gi_out_rgba32f, r->d_stage, bytes, FROM_FRAME);
}

int arctic_gi_history_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->gi.hist_valid = false;   // (the planes stay: a call in flight may still write them, and the next call reuses them)
    r->gi.hist_calls = 0;
    return ARCTIC_OK;
}

int arctic_read_gi_history(ArcticRenderer *r, float *acc3, float *count, float *world3, float *normal3) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Gi &G = r->gi;
    if (!G.hist_valid || G.hist_width != r->width || G.hist_height != r->height || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_gi_history: the history is empty (no call yet, or none since the last reset or resize)");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t n = r->n_tiles() * TILE_PIXELS;
    std::vector<float> plane[3];
    for (int k = 0; k < 3; ++k) {
        plane[k].resize(n * 4);
        HIPCHECK(r, hipMemcpy(plane[k].data(), G.d_hist[G.hist_cur][k].p, n * 16, hipMemcpyDeviceToHost));
    }
    for (uint32_t y = 0; y < r->height; ++y)
        for (uint32_t x = 0; x < r->width; ++x) {
            const size_t q = ((size_t)(y / TILE) * r->tiles_x + x / TILE) * TILE_PIXELS + (y % TILE) * TILE + x % TILE, o = (size_t)y * r->width + x;
            if (count) count[o] = plane[0][4 * q + 3];
            for (int i = 0; i < 3; ++i) {
                if (world3) world3[3 * o + i] = plane[0][4 * q + i];
                if (normal3) normal3[3 * o + i] = plane[1][4 * q + i];
                if (acc3) acc3[3 * o + i] = plane[2][4 * q + i];
            }
        }
    return ARCTIC_OK;
}

// ---- stage 6: the composition ------------------------------------------------------------------------------------------------------------------
namespace {
// which plane a NULL colour means under the record's flags
SourceFlag gi_source(uint32_t flags) { return {(flags & GI_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_GI_SOURCE_COMPOSED"}; }
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, gi, out_hdr, out: the planes k_gi_compose will read and write (null
// colour, gi and outputs: the handle's own)
int gi_compose_checks(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, const ArcticGiCompose *c, const void *color, const void *gi, const void *out_hdr,
                      const void *out, GiComposeDesc &d, const char *who) {
    if (!valid_scene(sc) || !st) return r->fail(ARCTIC_E_INVALID, "%s: null scene or settings", who);
    if (c) std::memcpy(&d, c, sizeof d);
    if (const char *why = gi_compose_refusal(c ? &d : nullptr)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if ((((uintptr_t)color | (uintptr_t)out_hdr | (uintptr_t)out) & 3u) || ((uintptr_t)gi & 15u))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane and the outputs must be 4-byte aligned, the indirect light's plane 16-byte aligned", who);
    return ARCTIC_OK;
}
// ... and with ARCTIC_E_STATE, in the header's order: no side effect.  own_color, own_gi: the planes are the handle's
int gi_compose_states(ArcticRenderer *r, const GiComposeDesc &d, bool own_color, bool own_gi, const char *who) {
    int rc = gbuffer_refusal(r, who);
    if (rc) return rc;
    if (own_color && (rc = source_refusal(r, gi_source(d.flags), who)) != ARCTIC_OK) return rc;
    if (own_gi && (!r->gi.pixels || r->gi.pixels != (uint64_t)r->rows() * r->width || !r->gi.own_estimate))
        return r->fail(ARCTIC_E_STATE, "%s: the handle holds no indirect light (arctic_trace_gi first; none since the last resize, or the latest call wrote the caller's plane)", who);
    if (d.ambient_scale != 1.0f) {
        if (const char *why = ambient_term_refusal(r))
            return r->fail(ARCTIC_E_STATE, "%s: ambient_scale != 1: %s, so the frame's ambient term is not ambient * base_color at level 0", who, why);
        if (own_color && (d.flags & GI_SOURCE_COMPOSED) && (r->compose.flags & ARCTIC_COMPOSE_AO))
            return r->fail(ARCTIC_E_STATE, "%s: ambient_scale != 1 with ARCTIC_GI_SOURCE_COMPOSED: the latest composition had ARCTIC_COMPOSE_AO and has scaled the ambient term already", who);
    }
    return ARCTIC_OK;
}
// the handle's buffers and the launch: device pointers throughout
int gi_compose_planes(ArcticRenderer *r, const ArcticScene *sc, const ArcticSettings *st, const GiComposeDesc &d, const float *d_color, const float *d_gi, float *d_out_hdr,
                      uint8_t *d_out) {
    int rc = gbuffer_in_place(r);
    if (rc) return rc;
    ArcticRenderer::Gi &G = r->gi;
    const uint64_t n = (uint64_t)r->rows() * r->width, cap = std::max<uint64_t>(n, 1);
    if (!d_out_hdr) HIPCHECK(r, G.d_hdr.ensure(cap * 12));
    if (!d_out) HIPCHECK(r, G.d_rgba8.ensure(cap * 4));
    HIPCHECK(r, G.d_ldr.ensure(cap * 12));
    SourcePlane source = {d_color, false};
    if (!d_color && (rc = source_plane(r, gi_source(d.flags).source, source)) != ARCTIC_OK) return rc;
    const GBuffer g = r->gbuffer();
    GiComposeParams p = {};
    p.plane_a = g.a; p.plane_b = g.b;
    p.tex = r->d_tex.as<TexDesc>(); p.srgb_lut = r->d_lut.as<float>();
    p.hdr = static_cast<const float *>(source.color); p.gi = d_gi ? d_gi : G.d_estimate.as<float>();
    p.out_hdr = d_out_hdr ? d_out_hdr : G.d_hdr.as<float>(); p.out_ldr = G.d_ldr.as<float>();
    p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : G.d_rgba8.as<uint8_t>());
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows(); p.row0_in_tile = r->row0_in_tile;
    p.n_materials = (uint32_t)(r->tex.size() / 3);
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.gi_strength = d.gi_strength; p.ambient_scale = d.ambient_scale; p.ambient = sc->ambient;
    G.composed = 0;   // (until the launch is enqueued: a failure leaves nothing to read)
    HIPCHECK(r, launch_gi_compose(p, r->stream));
    G.composed = n; G.own_hdr = d_out_hdr == nullptr; G.own_rgba8 = d_out == nullptr;
    ++G.launches;
    return ARCTIC_OK;
}
}  // namespace

int arctic_gi_compose_device(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticGiCompose *compose, const float *d_hdr_rgb32f,
                             const float *d_gi_rgba32f, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "gi_compose_device";
    GiComposeDesc d;
    int rc = gi_compose_checks(r, scene, settings, compose, d_hdr_rgb32f, d_gi_rgba32f, d_out_hdr_rgb32f, d_out_rgba8, d, who);
    if (rc || (rc = gi_compose_states(r, d, d_hdr_rgb32f == nullptr, d_gi_rgba32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return gi_compose_planes(r, scene, settings, d, d_hdr_rgb32f, d_gi_rgba32f, d_out_hdr_rgb32f, d_out_rgba8);
}

int arctic_read_gi(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Gi &G = r->gi;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    if (!G.composed || G.composed != n) return r->fail(ARCTIC_E_STATE, "read_gi: nothing composed yet, or not since the last resize");
    if (hdr_rgb && !G.own_hdr) return r->fail(ARCTIC_E_STATE, "read_gi: the latest composition wrote the caller's HDR plane, not the handle's");
    if (rgba8 && !G.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_gi: the latest composition wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    if (int ov = check_item_overflow(r)) return ov;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, G.d_ldr.p, n * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, G.d_hdr.p, n * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, G.d_rgba8.p, n * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

// ---- the one call: trace, accumulate when hist is given, compose -- byte for byte the calls above made by hand, on the handle's own planes ----------
int arctic_pass_gi(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticGi *gi, const float *dirs, const ArcticGiHistory *hist,
                   const ArcticGiCompose *compose, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_gi";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    // every refusal of the calls below, in front of the first launch
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    GiDesc g;
    GiHistoryDesc h;
    GiComposeDesc c;
    int rc = gi_checks(r, gi, dirs, g, who);
    if (rc || (hist && (rc = gi_history_checks(r, scene, hist, own_plane, own_plane, h, who)) != ARCTIC_OK)) return rc;
    if ((rc = gi_compose_checks(r, scene, settings, compose, nullptr, nullptr, nullptr, d_out_rgba8, c, who)) != ARCTIC_OK) return rc;
    if ((rc = gi_states(r, g, true, who)) != ARCTIC_OK || (hist && (rc = gi_history_states(r, who)) != ARCTIC_OK)) return rc;
    if ((rc = gi_compose_states(r, c, true, false, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    if ((rc = trace_gi(r, scene, g, dirs, nullptr)) != ARCTIC_OK) return rc;
    ArcticRenderer::Gi &G = r->gi;
    if (hist && (rc = gi_accumulate_planes(r, scene, h, G.d_estimate.as<float>(), G.d_estimate.as<float>())) != ARCTIC_OK) return rc;
    if ((rc = gi_compose_planes(r, scene, settings, c, nullptr, nullptr, nullptr, d_out_rgba8)) != ARCTIC_OK) return rc;
    ++G.passes;
    return ARCTIC_OK;
}

}  // extern "C"
