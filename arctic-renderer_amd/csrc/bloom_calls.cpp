// bloom_calls.cpp -- bloom's calls of the C-ABI (include/arctic_hip.h: arctic_bloom_device and the definition in front of it; the arithmetic:
// bloom.h; the kernels: bloom.hip; the arbiters and the layout: bloom.cpp).  Of the handle (renderer_state.h) it owns ArcticRenderer::Bloom and
// reads its colour plane through post_source.cpp, which knows the stages in front of it.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "bloom.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, out: the planes the kernels will read and write (null: the handle's
// own); align: whether they are device planes, whose alignment the loads and stores need
int bloom_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticBloom *bloom, const void *color, const void *out, bool align, BloomDesc &d, const char *who) {
    if (!st || !bloom) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, bloom, sizeof d);
    if (const char *why = bloom_refusal(&d)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && (((uintptr_t)color | (uintptr_t)out) & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the colour plane and the output must be 4-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags (they exclude each other), and the public name of the flag that says so
SourceFlag bloom_source(uint32_t flags) {
    if (flags & BLOOM_SOURCE_DOF) return {HdrSource::Dof, "ARCTIC_BLOOM_SOURCE_DOF"};
    if (flags & BLOOM_SOURCE_MOTION_BLUR) return {HdrSource::MotionBlur, "ARCTIC_BLOOM_SOURCE_MOTION_BLUR"};
    if (flags & BLOOM_SOURCE_TAA) return {HdrSource::Taa, "ARCTIC_BLOOM_SOURCE_TAA"};
    return {(flags & BLOOM_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_BLOOM_SOURCE_COMPOSED"};
}
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int bloom_states(ArcticRenderer *r, const BloomDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the pyramid's footprints need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return own_color ? source_refusal(r, bloom_source(d.flags), who) : ARCTIC_OK;
}
// the handle's buffers and the 2 L launches: device pointers throughout.  d_color: null = the handle's own plane, per d.flags; d_out: the caller's
// RGBA8, or null = the handle's own.  The pyramids are sized for 8 levels, so a record with other levels allocates nothing.  The handle's state
// moves only behind launches that were enqueued
int bloom_planes(ArcticRenderer *r, const ArcticSettings *st, const BloomDesc &d, const float *d_color, uint8_t *d_out) {
    ArcticRenderer::Bloom &B = r->bloom;
    const uint64_t n = std::max<uint64_t>((uint64_t)r->rows() * r->width, 1);
    const BloomLayout most = bloom_layout(r->width, r->rows(), BLOOM_MAX_LEVELS);
    HIPCHECK(r, B.d_down.ensure(std::max<uint64_t>(most.down_floats, 1) * 4));
    HIPCHECK(r, B.d_up.ensure(std::max<uint64_t>(most.up_floats, 1) * 4));
    HIPCHECK(r, B.d_hdr.ensure(n * 12));
    if (!d_out) HIPCHECK(r, B.d_rgba8.ensure(n * 4));
    HIPCHECK(r, B.d_ldr.ensure(n * 12));
    HIPCHECK(r, B.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, B.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, bloom_source(d.flags).source, source)) return rc; }
    BloomParams p = {};
    p.color = source.color; p.color_taa = source.color_taa;
    p.down = B.d_down.as<float>(); p.up = B.d_up.as<float>();
    p.out_hdr = B.d_hdr.as<float>(); p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : B.d_rgba8.as<uint8_t>()); p.out_ldr = B.d_ldr.as<float>();
    p.tiles_x = r->tiles_x; p.width = r->width; p.rows = r->rows();
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    p.layout = bloom_layout(r->width, r->rows(), d.levels);
    B.valid = false;   // (until all are enqueued: a failure between leaves nothing to read, never half this call's)
    HIPCHECK(r, launch_bloom_down_first(p, r->stream));
    for (uint32_t level = 2; level <= d.levels; ++level) HIPCHECK(r, launch_bloom_down(p, level, r->stream));
    for (uint32_t level = d.levels - 1; level >= 1; --level) HIPCHECK(r, launch_bloom_up(p, level, r->stream));
    HIPCHECK(r, launch_bloom_composite(p, r->stream));
    HIPCHECK(r, B.written.record(r->stream));
    B.valid = true; B.width = r->width; B.height = r->height; B.levels = d.levels; B.own_rgba8 = d_out == nullptr;
    ++B.launches; ++B.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_bloom_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticBloom *bloom, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "bloom_device";
    BloomDesc d;
    int rc = bloom_checks(r, settings, bloom, d_hdr_rgb32f, d_out_rgba8, true, d, who);
    if (rc || (rc = bloom_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return bloom_planes(r, settings, d, d_hdr_rgb32f, d_out_rgba8);
}

int arctic_bloom(ArcticRenderer *r, const ArcticSettings *settings, const ArcticBloom *bloom, const float *hdr_rgb32f, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "bloom";
    BloomDesc d;
    int rc = bloom_checks(r, settings, bloom, hdr_rgb32f, out_rgba8, false, d, who);
    if (rc || (rc = bloom_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Bloom &B = r->bloom;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, B.written, B.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if ((rc = bloom_planes(r, settings, d, hdr_rgb32f ? B.d_color.as<float>() : nullptr, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, out_rgba8, B.d_rgba8, px * 4, hdr_rgb32f == nullptr);
}

int arctic_read_bloom(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *down, float *up) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Bloom &B = r->bloom;
    if (!B.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_bloom: no bloom yet, or not since the last resize");
    if (rgba8 && !B.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_bloom: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width;
    const BloomLayout l = bloom_layout(r->width, r->rows(), B.levels);
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, B.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, B.d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, B.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (down) HIPCHECK(r, hipMemcpy(down, B.d_down.p, l.down_floats * 4, hipMemcpyDeviceToHost));
    if (up && l.up_floats) HIPCHECK(r, hipMemcpy(up, B.d_up.p, l.up_floats * 4, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_bloom_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "bloom_info: null");
    out4[0] = r->bloom.device_bytes(); out4[1] = r->bloom.launches; out4[2] = r->bloom.calls; out4[3] = 0;
    return ARCTIC_OK;
}

}  // extern "C"
