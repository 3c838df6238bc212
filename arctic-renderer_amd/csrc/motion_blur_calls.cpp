// motion_blur_calls.cpp -- the motion blur's calls of the C-ABI (include/arctic_hip.h: arctic_motion_blur_device and the definition in front of
// it, arctic_depth_plane_device; the arithmetic: motion_blur.h; the kernels: motion_blur.hip; the arbiters: motion_blur.cpp).  Of the handle
// (renderer_state.h) it owns ArcticRenderer::MotionBlur and reads the visibility plane (the depth), and through post_source.cpp the float HDR
// plane of the latest shading or composition or the anti-aliasing's history; the one call makes the motion call of ray_calls.cpp into
// Motion::d_plane and its own velocity plane, or under ARCTIC_MB_SOURCE_TAA reads the velocity arctic_pass_taa left in Taa::d_vel.  Enqueues on
// r->stream only.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "motion_blur.h"

namespace arctic {   // (renderer_state.h: arctic_pass_dof calls it)
// arctic_depth_plane_device behind its refusals
int mb_depth_plane(ArcticRenderer *r, float *d_depth) {
    HIPCHECK(r, launch_mb_depth(r->d_vis().as<unsigned long long>(), d_depth, r->tiles_x, r->tiles_y, r->width, r->rows(), r->row0_in_tile, r->stream));
    return ARCTIC_OK;
}
}  // namespace arctic

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, vel, depth, out: the planes the kernels will read and write (null
// colour, depth, output: the handle's own, zero, the handle's own); align: whether they are device planes, whose alignment the loads and stores need
int mb_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticMotionBlur *mb, const void *color, const void *vel, const void *depth, const void *out, bool align,
              MotionBlurDesc &d, const char *who) {
    if (!st || !mb) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, mb, sizeof d);
    if (const char *why = motion_blur_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (!vel) return r->fail(ARCTIC_E_INVALID, "%s: null velocity2", who);
    if (align && ((((uintptr_t)color | (uintptr_t)depth | (uintptr_t)out) & 3u) || ((uintptr_t)vel & 7u)))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane, the depth and the output must be 4-byte aligned, velocity2 8-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags, and the public name of the flag that says so.  (The composition is refused under the
// anti-aliasing's name: this stage used to ask that stage's function, and the text is part of the ABI now)
SourceFlag mb_source(uint32_t flags) {
    if (flags & MB_SOURCE_TAA) return {HdrSource::Taa, "ARCTIC_MB_SOURCE_TAA"};
    return {(flags & MB_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_TAA_SOURCE_COMPOSED"};
}
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int mb_states(ArcticRenderer *r, const MotionBlurDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the gather's taps need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return own_color ? source_refusal(r, mb_source(d.flags), who) : ARCTIC_OK;
}
// the handle's buffers and the three launches: device pointers throughout.  d_color: null = the handle's own plane, per d.flags; d_depth: null =
// zero; d_out: the caller's RGBA8, or null = the handle's own.  The handle's state moves only behind launches that were enqueued
int mb_planes(ArcticRenderer *r, const ArcticSettings *st, const MotionBlurDesc &d, const float *d_color, const void *d_vel, const float *d_depth, uint8_t *d_out) {
    ArcticRenderer::MotionBlur &B = r->motion_blur;
    const uint64_t n = std::max<uint64_t>((uint64_t)r->rows() * r->width, 1), tiles = std::max<uint64_t>(r->n_tiles(), 1);
    HIPCHECK(r, B.d_prep.ensure(n * 8));
    HIPCHECK(r, B.d_tile.ensure(tiles * 8));
    HIPCHECK(r, B.d_neighbour.ensure(tiles * 8));
    HIPCHECK(r, B.d_hdr.ensure(n * 12));
    if (!d_out) HIPCHECK(r, B.d_rgba8.ensure(n * 4));
    HIPCHECK(r, B.d_ldr.ensure(n * 12));
    HIPCHECK(r, B.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, B.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, mb_source(d.flags).source, source)) return rc; }
    MotionBlurParams p = {};
    p.color = source.color; p.color_taa = source.color_taa;
    p.velocity = d_vel; p.depth = d_depth;
    p.prep = B.d_prep.p; p.tile_max = B.d_tile.p; p.neighbour_max = B.d_neighbour.p;
    p.out_hdr = B.d_hdr.as<float>(); p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : B.d_rgba8.as<uint8_t>()); p.out_ldr = B.d_ldr.as<float>();
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    B.valid = false;   // (until all three are enqueued: a failure between leaves nothing to read, never half this call's)
    HIPCHECK(r, launch_mb_tile_max(p, r->stream));
    HIPCHECK(r, launch_mb_neighbour_max(p, r->stream));
    HIPCHECK(r, launch_motion_blur(p, r->stream));
    HIPCHECK(r, B.written.record(r->stream));
    B.valid = true; B.width = r->width; B.height = r->height; B.own_rgba8 = d_out == nullptr;
    ++B.launches; ++B.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_motion_blur_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticMotionBlur *mb, const float *d_hdr_rgb32f, const float *d_velocity2,
                              const float *d_depth, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "motion_blur_device";
    MotionBlurDesc d;
    int rc = mb_checks(r, settings, mb, d_hdr_rgb32f, d_velocity2, d_depth, d_out_rgba8, true, d, who);
    if (rc || (rc = mb_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return mb_planes(r, settings, d, d_hdr_rgb32f, d_velocity2, d_depth, d_out_rgba8);
}

int arctic_motion_blur(ArcticRenderer *r, const ArcticSettings *settings, const ArcticMotionBlur *mb, const float *hdr_rgb32f, const float *velocity2, const float *depth,
                       uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "motion_blur";
    MotionBlurDesc d;
    int rc = mb_checks(r, settings, mb, hdr_rgb32f, velocity2, depth, out_rgba8, false, d, who);
    if (rc || (rc = mb_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::MotionBlur &B = r->motion_blur;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, B.written, B.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if ((rc = upload_plane(r, B.written, B.d_vel, velocity2, px, 8)) != ARCTIC_OK) return rc;
    if (depth && (rc = upload_plane(r, B.written, B.d_depth, depth, px, 4)) != ARCTIC_OK) return rc;
    if ((rc = mb_planes(r, settings, d, hdr_rgb32f ? B.d_color.as<float>() : nullptr, B.d_vel.p, depth ? B.d_depth.as<float>() : nullptr, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, out_rgba8, B.d_rgba8, px * 4, hdr_rgb32f == nullptr);
}

int arctic_depth_plane_device(ArcticRenderer *r, float *d_depth) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "depth_plane_device";
    if (!d_depth || ((uintptr_t)d_depth & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the plane is null or not 4-byte aligned", who);
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    int rc = select_device(r);
    if (rc) return rc;
    return mb_depth_plane(r, d_depth);
}

int arctic_pass_motion_blur(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticMotionBlur *mb, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_motion_blur";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    MotionBlurDesc d;
    int rc = mb_checks(r, settings, mb, nullptr, own_plane, nullptr, d_out_rgba8, true, d, who);
    // every refusal of the motion call and of the depth plane, in front of the first launch
    if (rc || (rc = motion_refusal(r, scene, own_plane, who)) != ARCTIC_OK || (rc = mb_states(r, d, true, who)) != ARCTIC_OK) return rc;
    const bool from_taa = (d.flags & MB_SOURCE_TAA) != 0;
    if (from_taa && !r->taa.by_pass)
        return r->fail(ARCTIC_E_STATE, "%s: ARCTIC_MB_SOURCE_TAA: the handle's latest anti-aliasing call was not arctic_pass_taa, so it holds no velocity2 of this frame", who);
    if ((rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::MotionBlur &B = r->motion_blur;
    const size_t px = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, B.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, B.written.wait(r->stream));   // (the motion call and the depth below overwrite planes the previous call read)
    HIPCHECK(r, B.d_depth.ensure(px * 4));
    const void *d_vel = r->taa.d_vel.p;
    if (!from_taa) {
        HIPCHECK(r, r->motion.d_plane.ensure(px * 16));
        HIPCHECK(r, B.d_vel.ensure(px * 8));
        if ((rc = motion_planes(r, scene, r->motion.d_plane.as<float4>(), B.d_vel.as<float2>(), nullptr, nullptr)) != ARCTIC_OK) return rc;
        d_vel = B.d_vel.p;
    }
    if ((rc = mb_depth_plane(r, B.d_depth.as<float>())) != ARCTIC_OK) return rc;
    return mb_planes(r, settings, d, nullptr, d_vel, B.d_depth.as<float>(), d_out_rgba8);
}

int arctic_read_motion_blur(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max2, float *neighbour_max2, float *prepared2) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::MotionBlur &B = r->motion_blur;
    if (!B.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_motion_blur: nothing blurred yet, or not since the last resize");
    if (rgba8 && !B.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_motion_blur: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width, tiles = r->n_tiles();
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, B.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, B.d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, B.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (tile_max2) HIPCHECK(r, hipMemcpy(tile_max2, B.d_tile.p, tiles * 8, hipMemcpyDeviceToHost));
    if (neighbour_max2) HIPCHECK(r, hipMemcpy(neighbour_max2, B.d_neighbour.p, tiles * 8, hipMemcpyDeviceToHost));
    if (prepared2) HIPCHECK(r, hipMemcpy(prepared2, B.d_prep.p, px * 8, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_motion_blur_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "motion_blur_info: null");
    out4[0] = r->motion_blur.device_bytes(); out4[1] = r->motion_blur.launches; out4[2] = r->motion_blur.calls; out4[3] = 0;
    return ARCTIC_OK;
}

}  // extern "C"
