// exposure.h -- auto-exposure (include/arctic_hip.h: arctic_exposure_device and the text in front of it, which is the definition; nothing here
// restates it, it only carries it out).  ONE copy of the luminance key, the bin, the percentile band's share of a bin, the binary64 tail of the
// resolve and the exposed pixel, compiled for the host (exposure.cpp: the arbiters arctic_exposure_histogram, arctic_exposure_resolve and
// arctic_exposure_pixels) and for the device (exposure.hip), both with contraction off.  Plain C++ like bloom.h; rq_min and rq_max are ray_query.h's.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticExposure (static_assert in exposure.cpp)
struct ExposureDesc {
    uint32_t flags, low_q16, high_q16;
    float key_value, min_exposure, max_exposure, rate_up, rate_down, fallback_exposure;
    uint32_t window[4], reserved;
};
// == ArcticExposureState
struct ExposureState {
    double adapted_key;
    float exposure, luminance;
    uint32_t metered, valid, frames, reserved;
};
constexpr uint32_t EXPOSURE_SOURCE_COMPOSED = 1u, EXPOSURE_SOURCE_TAA = 2u, EXPOSURE_SOURCE_MOTION_BLUR = 4u, EXPOSURE_SOURCE_DOF = 8u, EXPOSURE_SOURCE_BLOOM = 16u,
                   EXPOSURE_SKIP_BLACK = 32u, EXPOSURE_RESET = 64u, EXPOSURE_HOLD = 128u, EXPOSURE_METER_ONLY = 256u;   // ARCTIC_EXPOSURE_*
constexpr uint32_t EXPOSURE_SOURCES = EXPOSURE_SOURCE_COMPOSED | EXPOSURE_SOURCE_TAA | EXPOSURE_SOURCE_MOTION_BLUR | EXPOSURE_SOURCE_DOF | EXPOSURE_SOURCE_BLOOM;
constexpr uint32_t EXPOSURE_BINS = 256, EXPOSURE_THREADS = 256;
constexpr uint32_t EXPOSURE_PER_THREAD = 4, EXPOSURE_TRIP = EXPOSURE_THREADS * EXPOSURE_PER_THREAD;   // a workgroup's pixels per trip of the meter's loop
constexpr uint32_t EXPOSURE_MAX_SIDE = 16384;
constexpr int32_t EXPOSURE_KEY_BASE = 888;   // (127 - 16) * 8: the key of 2^-16

// The meter's launch geometry.  The cap on the workgroups is the measured choice of DESIGN.md 6w; tools/exposure_time.py alone builds libraries
// with another (the Makefile never sets it)
#if !defined(ARCTIC_EXPOSURE_MAX_GROUPS)
#define ARCTIC_EXPOSURE_MAX_GROUPS 256
#endif
struct ExposureLayout { uint32_t groups, pixels_per_trip; uint64_t table_bytes; };
RQ_HD ExposureLayout exposure_layout(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    uint64_t g = (n + EXPOSURE_TRIP - 1) / EXPOSURE_TRIP;
    if (g < 1) g = 1;
    if (g > ARCTIC_EXPOSURE_MAX_GROUPS) g = ARCTIC_EXPOSURE_MAX_GROUPS;
    return ExposureLayout{(uint32_t)g, EXPOSURE_TRIP, g * EXPOSURE_BINS * 4};
}

RQ_HD uint32_t exposure_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
RQ_HD float exposure_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }

// step 1: the bin of the colour c
RQ_HD uint32_t exposure_bin(const float *c) {
    const float x0 = c[0] > 0.0f ? rq_min(c[0], 65504.0f) : 0.0f;   // (a NaN fails the test)
    const float x1 = c[1] > 0.0f ? rq_min(c[1], 65504.0f) : 0.0f;
    const float x2 = c[2] > 0.0f ? rq_min(c[2], 65504.0f) : 0.0f;
    const float l = (0.2126f * x0 + 0.7152f * x1) + 0.0722f * x2;
    const int32_t key = (int32_t)(exposure_bits(l) >> 20) - EXPOSURE_KEY_BASE;
    return (uint32_t)(key < 0 ? 0 : (key > 255 ? 255 : key));
}

// step 2: H'[b] of H[b]
RQ_HD uint32_t exposure_counted(const ExposureDesc &d, uint32_t b, uint32_t h) { return (d.flags & EXPOSURE_SKIP_BLACK) && b == 0u ? 0u : h; }
// ... lo and hi of N
RQ_HD void exposure_band(const ExposureDesc &d, uint64_t n, uint64_t &lo, uint64_t &hi) { lo = (n * d.low_q16) >> 16; hi = (n * d.high_q16) >> 16; }
// ... c_b of P_b, P_{b+1}
RQ_HD uint64_t exposure_share(uint64_t p0, uint64_t p1, uint64_t lo, uint64_t hi) {
    const uint64_t top = p1 < hi ? p1 : hi, bottom = p0 > lo ? p0 : lo;
    return top > bottom ? top - bottom : 0u;
}
RQ_HD float exposure_clamp(const ExposureDesc &d, float e) { return rq_min(rq_max(e, d.min_exposure), d.max_exposure); }
// ... and everything behind M and S: prev is the state in front of this call (prev_valid: whether it counts), out the state behind it
RQ_HD void exposure_adapt(const ExposureDesc &d, uint64_t M, uint64_t S, const ExposureState &prev, bool prev_valid, ExposureState &out) {
    out.reserved = 0u;
    if (M == 0u) {   // no measurement: the adaptation stays where it is, this call's exposure is the fallback's
        out.adapted_key = prev_valid ? prev.adapted_key : 0.0;
        out.luminance = prev_valid ? prev.luminance : 0.0f;
        out.valid = prev_valid ? 1u : 0u;
        out.frames = prev_valid ? prev.frames : 0u;
        out.metered = 0u;
        out.exposure = exposure_clamp(d, d.fallback_exposure);
        return;
    }
    const double m = (double)S / (double)M;
    const double a_t = m + 888.5;
    double a = a_t;
    if (prev_valid && !(d.flags & EXPOSURE_RESET)) {
        const float rate = a_t > prev.adapted_key ? d.rate_up : d.rate_down;
        const double step = (a_t - prev.adapted_key) * (double)rate;
        a = prev.adapted_key + step;
    }
    const float L = exposure_float((uint32_t)(a * 1048576.0));
    out.adapted_key = a;
    out.luminance = L;
    out.exposure = exposure_clamp(d, d.key_value / L);
    out.metered = M > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)M;
    out.valid = 1u;
    out.frames = (prev_valid && !(d.flags & EXPOSURE_RESET) ? prev.frames : 0u) + 1u;
}

// step 3 of one pixel
RQ_HD void exposure_apply(const float *c, float e, float *out) { out[0] = c[0] * e; out[1] = c[1] * e; out[2] = c[2] * e; }

// ---- host side (exposure.cpp) ------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the record's sake, in the header's order: null = nothing; else the reason.  width and
// height: the frame the window must lie in
const char *exposure_refusal(const ExposureDesc *d, uint32_t width, uint32_t height);
// the window of the record as x0, y0, x1, y1 (all zero: the whole frame)
RQ_HD void exposure_window(const ExposureDesc &d, uint32_t width, uint32_t height, uint32_t *w) {
    if ((d.window[0] | d.window[1] | d.window[2] | d.window[3]) == 0u) { w[0] = 0; w[1] = 0; w[2] = width; w[3] = height; }
    else { w[0] = d.window[0]; w[1] = d.window[1]; w[2] = d.window[2]; w[3] = d.window[3]; }
}

#if defined(__HIPCC__)
// exposure.hip.  The planes of a handle that owns the whole frame (width x rows pixels).  color: row-major float3, or -- color_taa -- the
// anti-aliasing's tile-major float4 history (tiles_x tiles a row).  partials: T[groups][256]; hist: H[256]; state: the record.  fresh: the state in
// memory does not count (the first call, or the first behind a reset or a resize).  out_hdr, out_ldr (3 floats) and out_rgba8, row-major.
struct ExposureParams {
    const void *color; bool color_taa;
    uint32_t *partials, *hist;
    ExposureState *state;
    float *out_hdr; uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, width, rows;
    uint32_t window[4];
    uint32_t groups;
    bool fresh;
    int32_t tm;
    float inv_gamma, exposure;
    ExposureDesc d;
};
// each enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_exposure_meter(const ExposureParams &p, hipStream_t s);
hipError_t launch_exposure_resolve(const ExposureParams &p, hipStream_t s);
hipError_t launch_exposure_apply(const ExposureParams &p, hipStream_t s);
#endif

}  // namespace arctic
