// taa_upscale.cpp -- the host side of the temporal upscaler (include/arctic_hip.h: arctic_taa_upscale_device and the definition in front of it):
// what the entry points refuse before a device is touched, the pure host function arctic_taa_upscale_jitter, and the arbiter
// arctic_taa_upscale_pixels -- the function of taa_upscale.h that taa_upscale.hip runs, on the CPU.  No HIP type: it also compiles with a host
// compiler alone (tests/cpp/taa_upscale_sanitize.cpp).
#include "taa_upscale.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticTaaUpscale) == 48 && sizeof(TaaUpscaleDesc) == 48, "ArcticTaaUpscale");
static_assert(offsetof(ArcticTaaUpscale, max_history) == offsetof(TaaUpscaleDesc, max_history) && offsetof(ArcticTaaUpscale, min_weight) == offsetof(TaaUpscaleDesc, min_weight) &&
              offsetof(ArcticTaaUpscale, jitter) == offsetof(TaaUpscaleDesc, jitter) && offsetof(ArcticTaaUpscale, sharpness) == offsetof(TaaUpscaleDesc, sharpness) &&
              offsetof(ArcticTaaUpscale, confidence_floor) == offsetof(TaaUpscaleDesc, confidence_floor) && offsetof(ArcticTaaUpscale, out_width) == offsetof(TaaUpscaleDesc, out_width) &&
              offsetof(ArcticTaaUpscale, out_height) == offsetof(TaaUpscaleDesc, out_height) && offsetof(ArcticTaaUpscale, reserved) == offsetof(TaaUpscaleDesc, reserved),
              "the public record is the internal one");
static_assert(ARCTIC_TAA_UPSCALE_LUMA_WEIGHT == TAA_UPSCALE_LUMA_WEIGHT && ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED == TAA_UPSCALE_SOURCE_COMPOSED &&
              ARCTIC_TAA_UPSCALE_NO_CLAMP == TAA_UPSCALE_NO_CLAMP && ARCTIC_TAA_UPSCALE_JITTER_EXACT == TAA_UPSCALE_JITTER_EXACT, "the flags");

namespace {
// the sizes the upscaler takes along one axis: in <= out <= 4 * in, both in 1..16384
bool sizes_ok(uint32_t in, uint32_t out) { return in >= 1 && in <= 16384u && out >= in && out <= 16384u && out <= TAA_UPSCALE_MAX_RATIO * in; }
}  // namespace

const char *taa_upscale_refusal(const TaaUpscaleDesc *d, uint32_t w, uint32_t h) {
    if (!d) return "null parameters";
    if (d->flags & ~(TAA_UPSCALE_LUMA_WEIGHT | TAA_UPSCALE_SOURCE_COMPOSED | TAA_UPSCALE_NO_CLAMP)) return "flags have unknown bits";
    if (!(d->max_history >= 1.0f && d->max_history <= 65536.0f)) return "max_history outside [1, 65536]";   // (a NaN fails every comparison)
    if (!(d->min_weight >= 0.0f && d->min_weight < 1.0f)) return "min_weight outside [0, 1)";
    for (int i = 0; i < 2; ++i)
        if (!(d->jitter[i] >= -1.0f && d->jitter[i] <= 1.0f)) return "jitter outside [-1, 1]";
    if (!(d->sharpness >= 0.0f && d->sharpness <= 65536.0f)) return "sharpness outside [0, 65536]";
    if (!(d->confidence_floor > 0.0f && d->confidence_floor <= 1.0f)) return "confidence_floor outside (0, 1]";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return "reserved not 0";
    if (!sizes_ok(w, d->out_width) || !sizes_ok(h, d->out_height)) return "the output size must lie in 1..16384, at or above the input's and at most four times it";
    return nullptr;
}

namespace {
// halton(i, base) of the header, in fp32
float halton(uint32_t i, uint32_t base) {
    float f = 1.0f, x = 0.0f;
    const float b = (float)base;
    while (i > 0) {
        f = f / b;
        x = x + f * (float)(i % base);
        i = i / base;
    }
    return x;
}
}  // namespace

}  // namespace arctic

extern "C" int arctic_taa_upscale_jitter(uint32_t index, uint32_t w, uint32_t W, uint32_t h, uint32_t H, float *out2) {
    using namespace arctic;
    if (!out2 || !sizes_ok(w, W) || !sizes_ok(h, H)) return ARCTIC_E_INVALID;
    if (index & TAA_UPSCALE_JITTER_EXACT) {
        const uint32_t s = W / w;
        if (W != s * w || H != s * h || !(s == 1 || s == 2 || s == 4)) return ARCTIC_E_INVALID;
        const uint32_t i = (index & ~TAA_UPSCALE_JITTER_EXACT) % (s * s);
        out2[0] = 0.5f - ((float)(i % s) + 0.5f) / (float)s;
        out2[1] = 0.5f - ((float)(i / s) + 0.5f) / (float)s;
        return ARCTIC_OK;
    }
    const uint32_t L = 8u * ((W + w - 1) / w) * ((H + h - 1) / h), i = index % L + 1;
    out2[0] = halton(i, 2) - 0.5f;
    out2[1] = halton(i, 3) - 0.5f;
    return ARCTIC_OK;
}

extern "C" int arctic_taa_upscale_pixels(const ArcticTaaUpscale *upscale, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *cur_rgb,
                                         const float *velocity2, const float *prev_rgbn, float *out_rgbn) {
    using namespace arctic;
    TaaUpscaleDesc d;
    if (upscale) std::memcpy(&d, upscale, sizeof d);
    if (taa_upscale_refusal(upscale ? &d : nullptr, width, height)) return ARCTIC_E_INVALID;
    if (n && (!pixel_xy || !cur_rgb || !out_rgbn)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the output frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= d.out_width || (uint32_t)pixel_xy[2 * k + 1] >= d.out_height) return ARCTIC_E_INVALID;
    const auto color = [&](uint32_t qx, uint32_t qy, float *c) {
        const float *s = cur_rgb + ((size_t)qy * width + qx) * 3;
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    };
    const auto velocity = [&](uint32_t qx, uint32_t qy, float *v) {
        const float *s = velocity2 ? velocity2 + ((size_t)qy * width + qx) * 2 : nullptr;
        v[0] = s ? s[0] : 0.0f; v[1] = s ? s[1] : 0.0f;
    };
    const auto history = [&](uint32_t qx, uint32_t qy, float *e) {
        const float *s = prev_rgbn + ((size_t)qy * d.out_width + qx) * 4;
        e[0] = s[0]; e[1] = s[1]; e[2] = s[2]; e[3] = s[3];
    };
    for (uint64_t k = 0; k < n; ++k)
        taa_upscale_pixel((uint32_t)pixel_xy[2 * k], (uint32_t)pixel_xy[2 * k + 1], width, height, d, color, velocity, prev_rgbn != nullptr, history, out_rgbn + 4 * k);
    return ARCTIC_OK;
}
