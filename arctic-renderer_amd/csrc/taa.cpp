// taa.cpp -- the host side of the temporal anti-aliasing (include/arctic_hip.h: arctic_taa_resolve_device, arctic_set_camera_jitter): what the
// entry points refuse before a device is touched, the pure host function arctic_jitter_proj_view, and the arbiter arctic_taa_pixels -- the
// functions of taa.h that taa.hip runs, on the CPU.  No HIP type: it also compiles with a host compiler alone (tests/cpp/taa_sanitize.cpp).
#include "taa.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticTaa) == 32 && sizeof(TaaDesc) == 32, "ArcticTaa");
static_assert(offsetof(ArcticTaa, max_history) == offsetof(TaaDesc, max_history) && offsetof(ArcticTaa, min_weight) == offsetof(TaaDesc, min_weight) &&
              offsetof(ArcticTaa, jitter) == offsetof(TaaDesc, jitter) && offsetof(ArcticTaa, reserved) == offsetof(TaaDesc, reserved), "the public record is the internal one");
static_assert(ARCTIC_TAA_LUMA_WEIGHT == TAA_LUMA_WEIGHT && ARCTIC_TAA_SOURCE_COMPOSED == TAA_SOURCE_COMPOSED, "the flags");

const char *taa_refusal(const TaaDesc *d) {
    if (!d) return "null parameters";
    if (d->flags & ~(TAA_LUMA_WEIGHT | TAA_SOURCE_COMPOSED)) return "flags have unknown bits";
    if (!(d->max_history >= 1.0f && d->max_history <= 65536.0f)) return "max_history outside [1, 65536]";   // (a NaN fails every comparison)
    if (!(d->min_weight >= 0.0f && d->min_weight < 1.0f)) return "min_weight outside [0, 1)";
    for (int i = 0; i < 2; ++i)
        if (!(d->jitter[i] >= -1.0f && d->jitter[i] <= 1.0f)) return "jitter outside [-1, 1]";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return "reserved not 0";
    return nullptr;
}

void taa_jitter_matrix(float *m, uint32_t width, uint32_t height, float jx, float jy) {
    const float kx = (2.0f * jx) / (float)width, ky = (2.0f * jy) / (float)height;
    for (int c = 0; c < 4; ++c) {
        m[4 * c + 0] = m[4 * c + 0] + kx * m[4 * c + 3];
        m[4 * c + 1] = m[4 * c + 1] - ky * m[4 * c + 3];
    }
}

}  // namespace arctic

extern "C" int arctic_jitter_proj_view(float *proj_view16, uint32_t width, uint32_t height, float jx, float jy) {
    using namespace arctic;
    if (!proj_view16 || width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (!(jx >= -1.0f && jx <= 1.0f && jy >= -1.0f && jy <= 1.0f)) return ARCTIC_E_INVALID;
    taa_jitter_matrix(proj_view16, width, height, jx, jy);
    return ARCTIC_OK;
}

extern "C" int arctic_taa_pixels(const ArcticTaa *taa, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb, const float *velocity2,
                                 const float *prev_rgbn, float *out_rgbn) {
    using namespace arctic;
    TaaDesc d;
    if (taa) std::memcpy(&d, taa, sizeof d);
    if (taa_refusal(taa ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (n && (!pixel_xy || !cur_rgb || !out_rgbn)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= width || (uint32_t)pixel_xy[2 * k + 1] >= height) return ARCTIC_E_INVALID;
    const auto color = [&](uint32_t qx, uint32_t qy, float *c) {
        const float *s = cur_rgb + ((size_t)qy * width + qx) * 3;
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    };
    const auto history = [&](uint32_t qx, uint32_t qy, float *e) {
        const float *s = prev_rgbn + ((size_t)qy * width + qx) * 4;
        e[0] = s[0]; e[1] = s[1]; e[2] = s[2]; e[3] = s[3];
    };
    for (uint64_t k = 0; k < n; ++k) {
        const float v[2] = {velocity2 ? velocity2[2 * k] : 0.0f, velocity2 ? velocity2[2 * k + 1] : 0.0f};
        taa_pixel((uint32_t)pixel_xy[2 * k], (uint32_t)pixel_xy[2 * k + 1], width, height, d, color, v, prev_rgbn != nullptr, history, out_rgbn + 4 * k);
    }
    return ARCTIC_OK;
}
