// exposure_calls.cpp -- auto-exposure's calls of the C-ABI (include/arctic_hip.h: arctic_exposure_device and the definition in front of it; the
// arithmetic: exposure.h; the kernels: exposure.hip; the arbiters and the layout: exposure.cpp).  Of the handle (renderer_state.h) it owns
// ArcticRenderer::Exposure and reads its colour plane through post_source.cpp, which knows the stages in front of it.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "exposure.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, out: the planes the kernels will read and write (null: the handle's
// own); align: whether they are device planes, whose alignment the loads and stores need
int exposure_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticExposure *exposure, const void *color, const void *out, bool align, ExposureDesc &d, const char *who) {
    if (!st || !exposure) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, exposure, sizeof d);
    if (const char *why = exposure_refusal(&d, r->width, r->height)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && (((uintptr_t)color | (uintptr_t)out) & 3u)) return r->fail(ARCTIC_E_INVALID, "%s: the colour plane and the output must be 4-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags (the sources exclude each other), and the public name of the flag that says so
SourceFlag exposure_source(uint32_t flags) {
    if (flags & EXPOSURE_SOURCE_BLOOM) return {HdrSource::Bloom, "ARCTIC_EXPOSURE_SOURCE_BLOOM"};
    if (flags & EXPOSURE_SOURCE_DOF) return {HdrSource::Dof, "ARCTIC_EXPOSURE_SOURCE_DOF"};
    if (flags & EXPOSURE_SOURCE_MOTION_BLUR) return {HdrSource::MotionBlur, "ARCTIC_EXPOSURE_SOURCE_MOTION_BLUR"};
    if (flags & EXPOSURE_SOURCE_TAA) return {HdrSource::Taa, "ARCTIC_EXPOSURE_SOURCE_TAA"};
    return {(flags & EXPOSURE_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_EXPOSURE_SOURCE_COMPOSED"};
}
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int exposure_states(ArcticRenderer *r, const ExposureDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the meter needs the whole frame, this handle owns %u of %u rows (the others are on other shards)", who, r->rows(), r->height);
    if (own_color) { if (int rc = source_refusal(r, exposure_source(d.flags), who)) return rc; }
    if ((d.flags & EXPOSURE_HOLD) && !r->exposure.holds(*r))
        return r->fail(ARCTIC_E_STATE, "%s: ARCTIC_EXPOSURE_HOLD: no exposure is held (no metering call yet, or none since arctic_exposure_reset or the last resize)", who);
    return ARCTIC_OK;
}
// the handle's buffers and the launches: device pointers throughout.  d_color: null = the handle's own plane, per d.flags; d_out: the caller's
// RGBA8, or null = the handle's own.  The handle's state moves only behind launches that were enqueued
int exposure_planes(ArcticRenderer *r, const ArcticSettings *st, const ExposureDesc &d, const float *d_color, uint8_t *d_out) {
    ArcticRenderer::Exposure &X = r->exposure;
    const uint64_t n = (uint64_t)r->rows() * r->width;
    const ExposureLayout layout = exposure_layout(r->width, r->rows());
    const bool meter = !(d.flags & EXPOSURE_HOLD), apply = !(d.flags & EXPOSURE_METER_ONLY);
    HIPCHECK(r, X.d_partials.ensure(layout.table_bytes));
    HIPCHECK(r, X.d_hist.ensure(EXPOSURE_BINS * 4));
    HIPCHECK(r, X.d_state.ensure(sizeof(ExposureState)));
    if (apply) {
        HIPCHECK(r, X.d_hdr.ensure(n * 12));
        if (!d_out) HIPCHECK(r, X.d_rgba8.ensure(n * 4));
        HIPCHECK(r, X.d_ldr.ensure(n * 12));
    }
    HIPCHECK(r, X.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, X.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, exposure_source(d.flags).source, source)) return rc; }
    ExposureParams p = {};
    p.color = source.color; p.color_taa = source.color_taa;
    p.partials = X.d_partials.as<uint32_t>(); p.hist = X.d_hist.as<uint32_t>(); p.state = X.d_state.as<ExposureState>();
    if (apply) { p.out_hdr = X.d_hdr.as<float>(); p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : X.d_rgba8.as<uint8_t>()); p.out_ldr = X.d_ldr.as<float>(); }
    p.tiles_x = r->tiles_x; p.width = r->width; p.rows = r->rows();
    exposure_window(d, r->width, r->rows(), p.window);
    p.groups = layout.groups;
    p.fresh = !X.valid;   // (what the record holds does not count: nothing of it is read)
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    if (meter) X.valid = false;   // (until all are enqueued: a failure between leaves nothing to read, never half this call's)
    if (apply) X.planes = false;
    if (meter) {
        HIPCHECK(r, launch_exposure_meter(p, r->stream));
        HIPCHECK(r, launch_exposure_resolve(p, r->stream));
    }
    if (apply) HIPCHECK(r, launch_exposure_apply(p, r->stream));
    HIPCHECK(r, X.written.record(r->stream));
    X.width = r->width; X.height = r->height;   // (a resize has cleared valid and planes: neither outlives its size)
    if (meter) { X.valid = true; ++X.meters; }
    if (apply) { X.planes = true; X.own_rgba8 = d_out == nullptr; ++X.launches; }
    ++X.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_exposure_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticExposure *exposure, const float *d_hdr_rgb32f, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "exposure_device";
    ExposureDesc d;
    int rc = exposure_checks(r, settings, exposure, d_hdr_rgb32f, d_out_rgba8, true, d, who);
    if (rc || (rc = exposure_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return exposure_planes(r, settings, d, d_hdr_rgb32f, d_out_rgba8);
}

int arctic_exposure(ArcticRenderer *r, const ArcticSettings *settings, const ArcticExposure *exposure, const float *hdr_rgb32f, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "exposure";
    ExposureDesc d;
    int rc = exposure_checks(r, settings, exposure, hdr_rgb32f, out_rgba8, false, d, who);
    if (rc || (rc = exposure_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Exposure &X = r->exposure;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, X.written, X.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if ((rc = exposure_planes(r, settings, d, hdr_rgb32f ? X.d_color.as<float>() : nullptr, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, (d.flags & EXPOSURE_METER_ONLY) ? nullptr : out_rgba8, X.d_rgba8, px * 4, hdr_rgb32f == nullptr);   // (a metering call has no planes)
}

int arctic_read_exposure(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, uint32_t *hist256, ArcticExposureState *state) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Exposure &X = r->exposure;
    const bool whole = r->rows() == r->height, size = X.width == r->width && X.height == r->height && whole;
    if ((hist256 || state) && !(X.holds(*r) && whole)) return r->fail(ARCTIC_E_STATE, "read_exposure: nothing metered yet, or not since arctic_exposure_reset or the last resize");
    if ((ldr_rgb || hdr_rgb || rgba8) && !(X.planes && size)) return r->fail(ARCTIC_E_STATE, "read_exposure: no exposed frame yet, or not since the last resize");
    if (rgba8 && !X.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_exposure: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width;
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, X.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, X.d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, X.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (hist256) HIPCHECK(r, hipMemcpy(hist256, X.d_hist.p, EXPOSURE_BINS * 4, hipMemcpyDeviceToHost));
    if (state) HIPCHECK(r, hipMemcpy(state, X.d_state.p, sizeof(ExposureState), hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_exposure_reset(ArcticRenderer *r) {
    if (!r) return ARCTIC_E_INVALID;
    r->exposure.valid = false;
    return ARCTIC_OK;
}

int arctic_exposure_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "exposure_info: null");
    out4[0] = r->exposure.device_bytes(); out4[1] = r->exposure.launches; out4[2] = r->exposure.calls; out4[3] = r->exposure.meters;
    return ARCTIC_OK;
}

}  // extern "C"
