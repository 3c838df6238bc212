// taa_upscale_calls.cpp -- the temporal upscaler's calls of the C-ABI (include/arctic_hip.h: arctic_taa_upscale_device and the definition in
// front of it; the arithmetic: taa_upscale.h; the kernel: taa_upscale.hip; the arbiter and the jitter: taa_upscale.cpp).  Of the handle
// (renderer_state.h) it owns ArcticRenderer::TaaUpscale and reads the float HDR plane of the latest shading or composition; the one call goes
// through the public arctic_motion_vectors_device, into Motion::d_plane and its own velocity plane.  Enqueues on r->stream only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "renderer_state.h"
#include "taa_upscale.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, vel, out: the planes k_taa_upscale will read and write (null: the
// handle's own, zero, the handle's own); align: whether they are device planes, whose alignment the kernel's loads and stores need
int upscale_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticTaaUpscale *up, const void *color, const void *vel, const void *out, bool align, TaaUpscaleDesc &d,
                   const char *who) {
    if (!st || !up) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, up, sizeof d);
    if (const char *why = taa_upscale_refusal(&d, r->width, std::max(r->height, 1u))) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && ((((uintptr_t)color | (uintptr_t)out) & 3u) || ((uintptr_t)vel & 7u)))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane and the output must be 4-byte aligned, velocity2 8-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags
SourceFlag upscale_source(uint32_t flags) { return {(flags & TAA_UPSCALE_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED"}; }
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int upscale_states(ArcticRenderer *r, const TaaUpscaleDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the samples' boxes need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return own_color ? source_refusal(r, upscale_source(d.flags), who) : ARCTIC_OK;
}
// the two sets of U, the handle's buffers and the launch: device pointers throughout.  d_color: null = the handle's own plane, per d.flags;
// d_vel: null = zero; d_out: the caller's RGBA8, or null = the handle's own.  The handle's state moves only behind a launch that was enqueued
int upscale_planes(ArcticRenderer *r, const ArcticSettings *st, const TaaUpscaleDesc &d, const float *d_color, const void *d_vel, uint8_t *d_out) {
    ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    const uint32_t tiles_x = (d.out_width + TILE - 1) / TILE, tiles_y = (d.out_height + TILE - 1) / TILE;
    const uint64_t n = (uint64_t)d.out_width * d.out_height;
    const size_t plane = (size_t)tiles_x * tiles_y * TILE_PIXELS * 16;
    for (DevBuf *b : {&U.d_u[0], &U.d_u[1]})
        if (b->cap != plane) {   // (no headroom: the two sets are 32 bytes per output pixel as the header says, at any output size)
            U.valid = false;
            HIPCHECK(r, b->alloc_exact(plane));
        }
    if (!d_out) HIPCHECK(r, U.d_rgba8.ensure(n * 4));
    HIPCHECK(r, U.d_ldr.ensure(n * 12));
    HIPCHECK(r, U.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, U.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    const bool have = U.holds(*r) && U.out_width == d.out_width && U.out_height == d.out_height;
    const int from = U.cur, to = U.cur ^ 1;
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, upscale_source(d.flags).source, source)) return rc; }
    TaaUpscaleParams p = {};
    p.color = static_cast<const float *>(source.color);
    p.velocity = d_vel;
    p.prev = have ? U.d_u[from].p : nullptr; p.next = U.d_u[to].p;
    p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : U.d_rgba8.as<uint8_t>()); p.out_ldr = U.d_ldr.as<float>();
    p.width = r->width; p.height = r->height; p.tiles_x = tiles_x; p.tiles_y = tiles_y;
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    HIPCHECK(r, launch_taa_upscale(p, r->stream));
    HIPCHECK(r, U.written.record(r->stream));
    U.cur = to; U.valid = true; U.in_width = r->width; U.in_height = r->height; U.out_width = d.out_width; U.out_height = d.out_height; U.own_rgba8 = d_out == nullptr;
    ++U.launches; ++U.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_taa_upscale_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, const float *d_hdr_rgb32f, const float *d_velocity2,
                              uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "taa_upscale_device";
    TaaUpscaleDesc d;
    int rc = upscale_checks(r, settings, upscale, d_hdr_rgb32f, d_velocity2, d_out_rgba8, true, d, who);
    if (rc || (rc = upscale_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return upscale_planes(r, settings, d, d_hdr_rgb32f, d_velocity2, d_out_rgba8);
}

int arctic_taa_upscale(ArcticRenderer *r, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, const float *hdr_rgb32f, const float *velocity2, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "taa_upscale";
    TaaUpscaleDesc d;
    int rc = upscale_checks(r, settings, upscale, hdr_rgb32f, velocity2, out_rgba8, false, d, who);
    if (rc || (rc = upscale_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, U.written, U.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if (velocity2 && (rc = upload_plane(r, U.written, U.d_vel, velocity2, px, 8)) != ARCTIC_OK) return rc;
    if ((rc = upscale_planes(r, settings, d, hdr_rgb32f ? U.d_color.as<float>() : nullptr, velocity2 ? U.d_vel.p : nullptr, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, out_rgba8, U.d_rgba8, (size_t)d.out_width * d.out_height * 4, hdr_rgb32f == nullptr);
}

int arctic_pass_taa_upscale(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticTaaUpscale *upscale, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_taa_upscale";
    TaaUpscaleDesc d;
    int rc = upscale_checks(r, settings, upscale, nullptr, nullptr, d_out_rgba8, true, d, who);
    if (rc) return rc;
    // every refusal of the motion call, in front of the first launch (the call below makes them again, in its own words, to no effect)
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    if ((rc = upscale_states(r, d, true, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    const size_t px = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, U.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, U.written.wait(r->stream));   // (the velocity below overwrites a plane the previous call read)
    HIPCHECK(r, r->motion.d_plane.ensure(px * 16));
    HIPCHECK(r, U.d_vel.ensure(px * 8));
    if ((rc = arctic_motion_vectors_device(r, scene, r->motion.d_plane.as<float>(), U.d_vel.as<float>())) != ARCTIC_OK) return rc;
    return upscale_planes(r, settings, d, nullptr, U.d_vel.p, d_out_rgba8);
}

int arctic_taa_upscale_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->taa_upscale.valid = false;   // (the planes stay: a call in flight may still write them, and the next call reuses them)
    r->taa_upscale.calls = 0;
    return ARCTIC_OK;
}

int arctic_read_taa_upscale(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, float *count, uint8_t *rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    if (!U.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_taa_upscale: U is empty (no call yet, or none since the last reset or resize)");
    if (rgba8 && !U.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_taa_upscale: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const uint32_t W = U.out_width, H = U.out_height, tiles_x = (W + TILE - 1) / TILE, tiles_y = (H + TILE - 1) / TILE;
    const size_t px = (size_t)W * H;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, U.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, U.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (hdr_rgb || count) {
        const size_t n = (size_t)tiles_x * tiles_y * TILE_PIXELS;
        std::vector<float> t(n * 4);
        HIPCHECK(r, hipMemcpy(t.data(), U.d_u[U.cur].p, n * 16, hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const size_t q = ((size_t)(y / TILE) * tiles_x + x / TILE) * TILE_PIXELS + (y % TILE) * TILE + x % TILE, o = (size_t)y * W + x;
                if (count) count[o] = t[4 * q + 3];
                if (hdr_rgb) for (int i = 0; i < 3; ++i) hdr_rgb[3 * o + i] = t[4 * q + i];
            }
    }
    return ARCTIC_OK;
}

int arctic_taa_upscale_hdr_device(ArcticRenderer *r, float *d_hdr_rgb32f) {
    if (!r) return ARCTIC_E_INVALID;
    if (!d_hdr_rgb32f || ((uintptr_t)d_hdr_rgb32f & 3u)) return r->fail(ARCTIC_E_INVALID, "taa_upscale_hdr_device: the plane is null or not 4-byte aligned");
    ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    if (!U.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "taa_upscale_hdr_device: U is empty (no call yet, or none since the last reset or resize)");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, U.written.wait(r->stream));   // (the call that wrote U, if the stream has changed since)
    HIPCHECK(r, launch_taa_upscale_hdr(U.d_u[U.cur].p, d_hdr_rgb32f, U.out_width, U.out_height, (U.out_width + TILE - 1) / TILE, (U.out_height + TILE - 1) / TILE, r->stream));
    HIPCHECK(r, U.written.record(r->stream));   // (the next call overwrites the other set only; a reallocation waits for the device)
    return ARCTIC_OK;
}

int arctic_taa_upscale_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "taa_upscale_info: null");
    const ArcticRenderer::TaaUpscale &U = r->taa_upscale;
    out4[0] = U.device_bytes(); out4[1] = U.launches; out4[2] = U.calls; out4[3] = (uint64_t)U.out_width | ((uint64_t)U.out_height << 32);
    return ARCTIC_OK;
}

}  // extern "C"
