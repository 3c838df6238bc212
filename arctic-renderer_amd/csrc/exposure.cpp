// exposure.cpp -- the host side of auto-exposure (include/arctic_hip.h: arctic_exposure_device): what the entry points refuse before a device is
// touched, the meter's launch geometry (arctic_exposure_layout), the caller's convenience arctic_exposure_rate, and the arbiters
// arctic_exposure_histogram, arctic_exposure_resolve and arctic_exposure_pixels -- the functions of exposure.h that exposure.hip runs, on the
// CPU.  No device type: it also compiles with a host compiler alone (tests/cpp/exposure_sanitize.cpp).
#include "exposure.h"
#include "../../include/arctic_hip.h"

#include <cmath>
#include <cstddef>
#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticExposure) == 56 && sizeof(ExposureDesc) == 56, "ArcticExposure");
static_assert(offsetof(ArcticExposure, low_q16) == offsetof(ExposureDesc, low_q16) && offsetof(ArcticExposure, high_q16) == offsetof(ExposureDesc, high_q16) &&
              offsetof(ArcticExposure, key_value) == offsetof(ExposureDesc, key_value) && offsetof(ArcticExposure, min_exposure) == offsetof(ExposureDesc, min_exposure) &&
              offsetof(ArcticExposure, max_exposure) == offsetof(ExposureDesc, max_exposure) && offsetof(ArcticExposure, rate_up) == offsetof(ExposureDesc, rate_up) &&
              offsetof(ArcticExposure, rate_down) == offsetof(ExposureDesc, rate_down) && offsetof(ArcticExposure, fallback_exposure) == offsetof(ExposureDesc, fallback_exposure) &&
              offsetof(ArcticExposure, window) == offsetof(ExposureDesc, window) && offsetof(ArcticExposure, reserved) == offsetof(ExposureDesc, reserved),
              "the public record is the internal one");
static_assert(sizeof(ArcticExposureState) == 32 && sizeof(ExposureState) == 32, "ArcticExposureState");
static_assert(offsetof(ArcticExposureState, exposure) == offsetof(ExposureState, exposure) && offsetof(ArcticExposureState, luminance) == offsetof(ExposureState, luminance) &&
              offsetof(ArcticExposureState, metered) == offsetof(ExposureState, metered) && offsetof(ArcticExposureState, valid) == offsetof(ExposureState, valid) &&
              offsetof(ArcticExposureState, frames) == offsetof(ExposureState, frames), "the public state is the internal one");
static_assert(ARCTIC_EXPOSURE_SOURCE_COMPOSED == EXPOSURE_SOURCE_COMPOSED && ARCTIC_EXPOSURE_SOURCE_TAA == EXPOSURE_SOURCE_TAA &&
              ARCTIC_EXPOSURE_SOURCE_MOTION_BLUR == EXPOSURE_SOURCE_MOTION_BLUR && ARCTIC_EXPOSURE_SOURCE_DOF == EXPOSURE_SOURCE_DOF &&
              ARCTIC_EXPOSURE_SOURCE_BLOOM == EXPOSURE_SOURCE_BLOOM && ARCTIC_EXPOSURE_SKIP_BLACK == EXPOSURE_SKIP_BLACK && ARCTIC_EXPOSURE_RESET == EXPOSURE_RESET &&
              ARCTIC_EXPOSURE_HOLD == EXPOSURE_HOLD && ARCTIC_EXPOSURE_METER_ONLY == EXPOSURE_METER_ONLY, "the flags");

const char *exposure_refusal(const ExposureDesc *d, uint32_t width, uint32_t height) {
    if (!d) return "null parameters";
    if (d->flags & ~(EXPOSURE_SOURCES | EXPOSURE_SKIP_BLACK | EXPOSURE_RESET | EXPOSURE_HOLD | EXPOSURE_METER_ONLY)) return "flags have unknown bits";
    const uint32_t source = d->flags & EXPOSURE_SOURCES;
    if (source & (source - 1u)) return "the ARCTIC_EXPOSURE_SOURCE_* flags exclude each other";
    if ((d->flags & EXPOSURE_HOLD) && (d->flags & (EXPOSURE_METER_ONLY | EXPOSURE_RESET))) return "ARCTIC_EXPOSURE_HOLD excludes ARCTIC_EXPOSURE_METER_ONLY and ARCTIC_EXPOSURE_RESET";
    if (!(d->low_q16 < d->high_q16 && d->high_q16 <= 65536u)) return "the percentile band is not 0 <= low < high <= 65536";
    if (!(d->key_value > 0.0f && d->key_value <= 65504.0f)) return "key_value outside (0, 65504]";   // (a NaN fails every comparison)
    if (!(d->min_exposure > 0.0f && d->min_exposure <= d->max_exposure && d->max_exposure <= 65504.0f)) return "not 0 < min_exposure <= max_exposure <= 65504";
    if (!(d->rate_up >= 0.0f && d->rate_up <= 1.0f)) return "rate_up outside [0, 1]";
    if (!(d->rate_down >= 0.0f && d->rate_down <= 1.0f)) return "rate_down outside [0, 1]";
    if (!(d->fallback_exposure > 0.0f && d->fallback_exposure <= 65504.0f)) return "fallback_exposure outside (0, 65504]";
    if ((d->window[0] | d->window[1] | d->window[2] | d->window[3]) != 0u &&
        !(d->window[0] < d->window[2] && d->window[2] <= width && d->window[1] < d->window[3] && d->window[3] <= height))
        return "the window is neither all zero nor x0 < x1 <= width, y0 < y1 <= height";
    if (d->reserved != 0u) return "reserved is not 0";
    return nullptr;
}

namespace {
bool bad_side(uint32_t n) { return n == 0 || n > EXPOSURE_MAX_SIDE; }
}  // namespace

}  // namespace arctic

extern "C" int arctic_exposure_layout(uint32_t width, uint32_t height, uint64_t *out3) {
    using namespace arctic;
    if (!out3 || bad_side(width) || bad_side(height)) return ARCTIC_E_INVALID;
    const ExposureLayout l = exposure_layout(width, height);
    out3[0] = l.groups; out3[1] = l.pixels_per_trip; out3[2] = l.table_bytes;
    return ARCTIC_OK;
}

extern "C" float arctic_exposure_rate(float dt, float speed) {
    const float r = (float)(1.0 - std::exp(-(double)dt * (double)speed));
    return r >= 0.0f ? (r <= 1.0f ? r : 1.0f) : 0.0f;   // (a NaN or a negative product: no adaptation)
}

extern "C" int arctic_exposure_histogram(const ArcticExposure *exposure, uint32_t width, uint32_t height, const float *rgb, uint32_t *hist256) {
    using namespace arctic;
    if (bad_side(width) || bad_side(height)) return ARCTIC_E_INVALID;
    ExposureDesc d;
    if (exposure) std::memcpy(&d, exposure, sizeof d);
    if (exposure_refusal(exposure ? &d : nullptr, width, height)) return ARCTIC_E_INVALID;
    if (!rgb || !hist256) return ARCTIC_E_INVALID;
    uint32_t w[4];
    exposure_window(d, width, height, w);
    for (uint32_t b = 0; b < EXPOSURE_BINS; ++b) hist256[b] = 0u;
    for (uint32_t y = w[1]; y < w[3]; ++y)
        for (uint32_t x = w[0]; x < w[2]; ++x) ++hist256[exposure_bin(rgb + ((size_t)y * width + x) * 3)];
    return ARCTIC_OK;
}

extern "C" int arctic_exposure_resolve(const ArcticExposure *exposure, const uint32_t *hist256, const ArcticExposureState *previous, ArcticExposureState *state) {
    using namespace arctic;
    ExposureDesc d;
    if (exposure) std::memcpy(&d, exposure, sizeof d);
    if (exposure_refusal(exposure ? &d : nullptr, EXPOSURE_MAX_SIDE, EXPOSURE_MAX_SIDE)) return ARCTIC_E_INVALID;
    if (!hist256 || !state) return ARCTIC_E_INVALID;
    uint64_t total = 0;
    for (uint32_t b = 0; b < EXPOSURE_BINS; ++b) total += exposure_counted(d, b, hist256[b]);
    uint64_t lo, hi, at = 0, M = 0, S = 0;
    exposure_band(d, total, lo, hi);
    for (uint32_t b = 0; b < EXPOSURE_BINS; ++b) {
        const uint64_t next = at + exposure_counted(d, b, hist256[b]), share = exposure_share(at, next, lo, hi);
        M += share; S += share * b;
        at = next;
    }
    ExposureState prev = {}, out;
    if (previous) std::memcpy(&prev, previous, sizeof prev);
    exposure_adapt(d, M, S, prev, previous && prev.valid != 0u, out);
    std::memcpy(state, &out, sizeof out);
    return ARCTIC_OK;
}

extern "C" int arctic_exposure_pixels(uint64_t n, const float *rgb, float exposure, float *out_rgb) {
    using namespace arctic;
    if (n && (!rgb || !out_rgb)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k) exposure_apply(rgb + 3 * k, exposure, out_rgb + 3 * k);
    return ARCTIC_OK;
}
