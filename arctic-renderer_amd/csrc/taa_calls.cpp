// taa_calls.cpp -- the temporal anti-aliasing's calls of the C-ABI (include/arctic_hip.h: arctic_taa_resolve_device and the definition in front of
// it, arctic_set_camera_jitter; the arithmetic: taa.h; the kernel: taa.hip; the arbiter and the jittered matrix: taa.cpp).  Of the handle
// (renderer_state.h) it owns ArcticRenderer::Taa -- run_geometry reads Taa::jitter, a resize empties the history, the motion blur's one call reads
// Taa::d_vel and by_pass -- and reads the float HDR plane of the latest shading or composition (post_source.cpp); the one call makes the motion
// call of ray_calls.cpp into Motion::d_plane and its own velocity plane.  Enqueues on r->stream only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "renderer_state.h"
#include "taa.h"

extern "C" {

int arctic_set_camera_jitter(ArcticRenderer *r, float jx, float jy) {
    if (!r) return ARCTIC_E_INVALID;
    if (!(jx >= -1.0f && jx <= 1.0f && jy >= -1.0f && jy <= 1.0f)) return r->fail(ARCTIC_E_INVALID, "set_camera_jitter: both offsets must be finite and in [-1, 1] pixels");
    r->taa.jitter[0] = jx; r->taa.jitter[1] = jy;
    return ARCTIC_OK;
}

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, vel, out: the planes k_taa_resolve will read and write (null: the
// handle's own, zero, the handle's own); align: whether they are device planes, whose alignment the kernel's loads and stores need
int taa_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticTaa *taa, const void *color, const void *vel, const void *out, bool align, TaaDesc &d, const char *who) {
    if (!st || !taa) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, taa, sizeof d);
    if (const char *why = taa_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && ((((uintptr_t)color | (uintptr_t)out) & 3u) || ((uintptr_t)vel & 7u)))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane and the output must be 4-byte aligned, velocity2 8-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags
SourceFlag taa_source(uint32_t flags) { return {(flags & TAA_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_TAA_SOURCE_COMPOSED"}; }
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int taa_states(ArcticRenderer *r, const TaaDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the history's taps need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return own_color ? source_refusal(r, taa_source(d.flags), who) : ARCTIC_OK;
}
// the two sets of T, the handle's buffers and the launch: device pointers throughout.  d_color: null = the handle's own plane, per d.flags;
// d_vel: null = zero; d_out: the caller's RGBA8, or null = the handle's own.  The handle's state moves only behind a launch that was enqueued
int taa_planes(ArcticRenderer *r, const ArcticSettings *st, const TaaDesc &d, const float *d_color, const void *d_vel, uint8_t *d_out) {
    ArcticRenderer::Taa &T = r->taa;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    const size_t plane = std::max<size_t>(r->n_tiles(), 1) * TILE_PIXELS * 16;
    for (DevBuf *b : {&T.d_t[0], &T.d_t[1]})
        if (b->cap < plane) HIPCHECK(r, b->alloc_exact(plane));   // (no headroom: the two sets are 32 bytes per pixel as the header says)
    if (!d_out) HIPCHECK(r, T.d_rgba8.ensure(std::max<uint64_t>(n, 1) * 4));
    HIPCHECK(r, T.d_ldr.ensure(std::max<uint64_t>(n, 1) * 12));
    HIPCHECK(r, T.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, T.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    const bool have = T.holds(*r);
    const int from = T.cur, to = T.cur ^ 1;
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, taa_source(d.flags).source, source)) return rc; }
    TaaParams p = {};
    p.color = static_cast<const float *>(source.color);
    p.velocity = d_vel;
    p.prev = have ? T.d_t[from].p : nullptr; p.next = T.d_t[to].p;
    p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : T.d_rgba8.as<uint8_t>()); p.out_ldr = T.d_ldr.as<float>();
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    HIPCHECK(r, launch_taa_resolve(p, r->stream));
    HIPCHECK(r, T.written.record(r->stream));
    T.cur = to; T.valid = true; T.width = r->width; T.height = r->height; T.own_rgba8 = d_out == nullptr;
    T.by_pass = false;   // (arctic_pass_taa sets it behind this)
    ++T.launches; ++T.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_taa_resolve_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaa *taa, const float *d_hdr_rgb32f, const float *d_velocity2, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "taa_resolve_device";
    TaaDesc d;
    int rc = taa_checks(r, settings, taa, d_hdr_rgb32f, d_velocity2, d_out_rgba8, true, d, who);
    if (rc || (rc = taa_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return taa_planes(r, settings, d, d_hdr_rgb32f, d_velocity2, d_out_rgba8);
}

int arctic_taa_resolve(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaa *taa, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "taa_resolve";
    TaaDesc d;
    int rc = taa_checks(r, settings, taa, hdr_rgb32f, velocity2, out_rgba8, false, d, who);
    if (rc || (rc = taa_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Taa &T = r->taa;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, T.written, T.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if (velocity2 && (rc = upload_plane(r, T.written, T.d_vel, velocity2, px, 8)) != ARCTIC_OK) return rc;
    if ((rc = taa_planes(r, settings, d, hdr_rgb32f ? T.d_color.as<float>() : nullptr, velocity2 ? T.d_vel.p : nullptr, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, out_rgba8, T.d_rgba8, px * 4, hdr_rgb32f == nullptr);
}

int arctic_pass_taa(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticTaa *taa, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_taa";
    alignas(16) static const char own_plane[16] = {};   // (the planes are the handle's own: never null, always aligned)
    TaaDesc d;
    int rc = taa_checks(r, settings, taa, nullptr, nullptr, d_out_rgba8, true, d, who);
    // every refusal of the motion call, in front of the first launch (the call below makes them again, to no effect)
    if (rc || (rc = motion_refusal(r, scene, own_plane, who)) != ARCTIC_OK || (rc = taa_states(r, d, true, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    const size_t px = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, r->motion.d_plane.ensure(px * 16));
    HIPCHECK(r, r->taa.d_vel.ensure(px * 8));
    if ((rc = motion_planes(r, scene, r->motion.d_plane.as<float4>(), r->taa.d_vel.as<float2>(), nullptr, nullptr)) != ARCTIC_OK) return rc;
    if ((rc = taa_planes(r, settings, d, nullptr, r->taa.d_vel.p, d_out_rgba8)) != ARCTIC_OK) return rc;
    r->taa.by_pass = true;   // (Taa::d_vel is this frame's velocity2: arctic_pass_motion_blur under ARCTIC_MB_SOURCE_TAA reads it)
    return ARCTIC_OK;
}

int arctic_taa_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->taa.valid = false;   // (the planes stay: a call in flight may still write them, and the next call reuses them)
    r->taa.calls = 0;
    return ARCTIC_OK;
}

int arctic_read_taa(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Taa &T = r->taa;
    if (!T.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_taa: T is empty (no call yet, or none since the last reset or resize)");
    if (rgba8 && !T.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_taa: the latest resolve wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, T.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, T.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (hdr_rgb || count) {
        const size_t n = r->n_tiles() * TILE_PIXELS;
        std::vector<float> t(n * 4);
        HIPCHECK(r, hipMemcpy(t.data(), T.d_t[T.cur].p, n * 16, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < r->height; ++y)
            for (uint32_t x = 0; x < r->width; ++x) {
                const size_t q = ((size_t)(y / TILE) * r->tiles_x + x / TILE) * TILE_PIXELS + (y % TILE) * TILE + x % TILE, o = (size_t)y * r->width + x;
                if (count) count[o] = t[4 * q + 3];
                if (hdr_rgb) for (int i = 0; i < 3; ++i) hdr_rgb[3 * o + i] = t[4 * q + i];
            }
    }
    return ARCTIC_OK;
}

int arctic_taa_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "taa_info: null");
    out4[0] = r->taa.device_bytes(); out4[1] = r->taa.launches; out4[2] = r->taa.calls; out4[3] = 0;
    return ARCTIC_OK;
}

}  // extern "C"
