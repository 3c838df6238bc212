// fog_calls.cpp -- volumetric fog's calls of the C-ABI (include/arctic_hip.h: arctic_fog_device and the definition in front of it; the
// arithmetic: fog.h; the kernel: fog.hip; the arbiter and the view record's construction: fog.cpp).  Of the handle (renderer_state.h) it owns
// ArcticRenderer::Fog and reads the sun's map, the float HDR plane of the latest shading or composition and, through
// arctic_depth_plane_device, the visibility plane.  Enqueues on r->stream only.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "fog.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; view: null only for arctic_pass_fog, which builds it; the planes the kernel
// will read and write (null colour, outputs: the handle's own); align: whether they are device planes, whose alignment the loads and stores need
int fog_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticFog *fog, const ArcticFogView *view, bool need_view, const float *offsets16, const void *color,
               const void *depth, const void *out_hdr, const void *out, bool align, FogDesc &d, FogView &v, const char *who) {
    if (!st || !fog || (need_view && !view)) return r->fail(ARCTIC_E_INVALID, "%s: null settings, parameters or view", who);
    std::memcpy(&d, fog, sizeof d);
    if (const char *why = fog_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (need_view) {
        std::memcpy(&v, view, sizeof v);
        if (const char *why = fog_view_refusal(&v)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    }
    if (const char *why = fog_offsets_refusal(offsets16)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && (((uintptr_t)color | (uintptr_t)depth | (uintptr_t)out_hdr | (uintptr_t)out) & 3u))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane, the depth and the outputs must be 4-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags
SourceFlag fog_source(uint32_t flags) { return {(flags & FOG_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_FOG_SOURCE_COMPOSED"}; }
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which).  The sun's map under the rule of
// arctic_shade_hits: whole, and drawn or written at least once
int fog_states(ArcticRenderer *r, const FogDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: whole frames only, this handle owns %u of %u rows (the others are on other shards)", who, r->rows(), r->height);
    if (own_color) { if (int rc = source_refusal(r, fog_source(d.flags), who)) return rc; }
    if (r->shadow_size && r->shadow_sharded)
        return r->fail(ARCTIC_E_STATE, "%s: the sun's map is sharded (ARCTIC_OPT_SHADOW_SHARDED): a sample may lie in rows this handle never draws", who);
    if (r->shadow_size && !r->shadow_written_set[r->scur])
        return r->fail(ARCTIC_E_STATE, "%s: the sun's map was never drawn or written (arctic_pass_shadow_map, arctic_write_shadow_map or a frame first)", who);
    return ARCTIC_OK;
}
// the handle's buffers, the offset table and the launch: device pointers throughout but offsets16.  d_color: null = the handle's own plane, per
// d.flags; d_depth: null = every depth 1.0; d_out_hdr, d_out: the caller's planes, or null = the handle's own.  The handle's state moves only
// behind a launch that was enqueued
int fog_planes(ArcticRenderer *r, const ArcticSettings *st, const FogDesc &d, const FogView &v, const float *offsets16, const float *d_color, const float *d_depth,
               float *d_out_hdr, uint8_t *d_out) {
    ArcticRenderer::Fog &F = r->fog;
    const uint64_t n = std::max<uint64_t>((uint64_t)r->rows() * r->width, 1);
    const size_t table_bytes = FOG_OFFSETS * sizeof(float);
    if (!d_out_hdr) HIPCHECK(r, F.d_hdr.ensure(n * 12));
    if (!d_out) HIPCHECK(r, F.d_rgba8.ensure(n * 4));
    HIPCHECK(r, F.d_ldr.ensure(n * 12));
    HIPCHECK(r, F.d_offsets.ensure(table_bytes));
    HIPCHECK(r, F.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, F.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    float table[FOG_OFFSETS];
    for (uint32_t i = 0; i < FOG_OFFSETS; ++i) table[i] = offsets16 ? offsets16[i] : 0.5f;
    if (!F.have_offsets || std::memcmp(F.offsets_ring.slot[0].h.p, table, table_bytes) != 0) {
        float *h = nullptr;
        HIPCHECK(r, F.offsets_ring.stage(table_bytes, &h));
        F.have_offsets = false;
        std::memcpy(h, table, table_bytes);
        HIPCHECK(r, F.offsets_ring.send(F.d_offsets.p, table_bytes, r->stream));
        F.have_offsets = true;
        ++F.uploads;
    }
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, fog_source(d.flags).source, source)) return rc; }
    FogParams p = {};
    p.color = static_cast<const float *>(source.color);
    p.depth = d_depth;
    p.map = r->shadow_size ? r->d_shadow().as<float>() : nullptr; p.S = r->shadow_size;
    p.offsets = F.d_offsets.as<float>();
#if defined(ARCTIC_FOG_TABLE_VARIANT)
    // the measured alternative of DESIGN.md 6x (set by tools/fog_time.py alone).  1: a table of the map as it is at this library's first call,
    // built once -- the measurement marches a map that does not change, and leaves the table's upkeep out of the figure; 2: built again in
    // front of every march, which is what a stage that cannot know whether the map has changed would have to do
    static DevBuf blocks, bounds;
    const uint32_t nb = shadow_bounds_pitch(r->shadow_size);
    if (nb && (!blocks.p || ARCTIC_FOG_TABLE_VARIANT == 2)) {
        HIPCHECK(r, blocks.ensure((size_t)nb * nb * 8));
        HIPCHECK(r, bounds.ensure((size_t)nb * nb * 8));
        HIPCHECK(r, launch_shadow_bounds(p.map, r->shadow_size, blocks.as<float2>(), bounds.as<float2>(), r->stream));
    }
    p.blocks = nb ? blocks.as<float2>() : nullptr; p.nb = nb;
#endif
    p.out_hdr = d_out_hdr ? d_out_hdr : F.d_hdr.as<float>();
    p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : F.d_rgba8.as<uint8_t>());
    p.out_ldr = F.d_ldr.as<float>();
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d; p.v = v;
    F.valid = false;   // (until the launch is enqueued: a failure leaves nothing to read)
    HIPCHECK(r, launch_fog_march(p, r->stream));
    HIPCHECK(r, F.written.record(r->stream));
    F.valid = true; F.width = r->width; F.height = r->height; F.own_hdr = d_out_hdr == nullptr; F.own_rgba8 = d_out == nullptr;
    ++F.launches; ++F.calls;
    return ARCTIC_OK;
}
// the view record of a scene; false: the scene's camera or sun gives no finite record
bool fog_scene_view(const ArcticScene *scene, uint32_t width, uint32_t height, FogView &v) {
    const ArcticCamera &c = scene->camera;
    float fc[3], fs[3];
    dir_from_rot(c.rotation, fc);
    dir_from_rot(scene->sun.rotation, fs);
    fog_view_build(fc, fs, c.eye, c.aspect, c.fov_y, c.z_near_far[0], c.z_near_far[1], scene->sun.position, width, height, &v);
    return fog_view_refusal(&v) == nullptr;
}
}  // namespace

int arctic_fog_view(const ArcticScene *scene, uint32_t width, uint32_t height, ArcticFogView *out) {
    if (!scene || !out || width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    FogView v;
    if (!fog_scene_view(scene, width, height, v)) return ARCTIC_E_INVALID;
    std::memcpy(out, &v, sizeof v);
    return ARCTIC_OK;
}

int arctic_fog_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, const float *d_hdr_rgb32f,
                      const float *d_depth, float *d_out_hdr_rgb32f, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "fog_device";
    FogDesc d;
    FogView v;
    int rc = fog_checks(r, settings, fog, view, true, offsets16, d_hdr_rgb32f, d_depth, d_out_hdr_rgb32f, d_out_rgba8, true, d, v, who);
    if (rc || (rc = fog_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return fog_planes(r, settings, d, v, offsets16, d_hdr_rgb32f, d_depth, d_out_hdr_rgb32f, d_out_rgba8);
}

int arctic_fog(ArcticRenderer *r, const ArcticSettings *settings, const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, const float *hdr_rgb32f,
               const float *depth, float *out_hdr_rgb32f, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "fog";
    FogDesc d;
    FogView v;
    int rc = fog_checks(r, settings, fog, view, true, offsets16, hdr_rgb32f, depth, out_hdr_rgb32f, out_rgba8, false, d, v, who);
    if (rc || (rc = fog_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Fog &F = r->fog;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, F.written, F.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if (depth && (rc = upload_plane(r, F.written, F.d_depth, depth, px, 4)) != ARCTIC_OK) return rc;
    if ((rc = fog_planes(r, settings, d, v, offsets16, hdr_rgb32f ? F.d_color.as<float>() : nullptr, depth ? F.d_depth.as<float>() : nullptr, nullptr, nullptr)) != ARCTIC_OK) return rc;
    if (out_hdr_rgb32f) HIPCHECK(r, hipMemcpyAsync(out_hdr_rgb32f, F.d_hdr.p, px * 12, hipMemcpyDeviceToHost, r->stream));
    return read_back(r, out_rgba8, F.d_rgba8, px * 4, hdr_rgb32f == nullptr);
}

int arctic_pass_fog(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticFog *fog, const float *offsets16, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_fog";
    FogDesc d;
    FogView v;
    int rc = fog_checks(r, settings, fog, nullptr, false, offsets16, nullptr, nullptr, nullptr, d_out_rgba8, true, d, v, who);
    if (rc) return rc;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (!fog_scene_view(scene, r->width, std::max(r->height, 1u), v)) return r->fail(ARCTIC_E_INVALID, "%s: the scene's camera and sun give no finite view record with 0 < z_near < z_far", who);
    // the depth plane's refusal, in front of the first launch
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    if ((rc = fog_states(r, d, true, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Fog &F = r->fog;
    const size_t px = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, F.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, F.written.wait(r->stream));   // (the depth below overwrites a plane the previous call read)
    HIPCHECK(r, F.d_depth.ensure(px * 4));
    if ((rc = arctic_depth_plane_device(r, F.d_depth.as<float>())) != ARCTIC_OK) return rc;
    return fog_planes(r, settings, d, v, offsets16, nullptr, F.d_depth.as<float>(), nullptr, d_out_rgba8);
}

int arctic_read_fog(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Fog &F = r->fog;
    if (!F.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_fog: no fog yet, or not since the last resize");
    if (hdr_rgb && !F.own_hdr) return r->fail(ARCTIC_E_STATE, "read_fog: the latest call wrote the caller's HDR plane, not the handle's");
    if (rgba8 && !F.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_fog: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, F.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, F.d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, F.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_fog_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "fog_info: null");
    out4[0] = r->fog.device_bytes(); out4[1] = r->fog.launches; out4[2] = r->fog.calls; out4[3] = r->fog.uploads;
    return ARCTIC_OK;
}

}  // extern "C"
