// bloom.cpp -- the host side of bloom (include/arctic_hip.h: arctic_bloom_device): what the entry points refuse before a device is touched, the
// layout of the pyramid (arctic_bloom_layout) and the arbiters arctic_bloom_pyramid and arctic_bloom_pixels -- the functions of bloom.h that
// bloom.hip runs, on the CPU.  No HIP type: it also compiles with a host compiler alone (tests/cpp/bloom_sanitize.cpp).
#include "bloom.h"
#include "../../include/arctic_hip.h"

#include <cstddef>
#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticBloom) == 32 && sizeof(BloomDesc) == 32, "ArcticBloom");
static_assert(offsetof(ArcticBloom, threshold) == offsetof(BloomDesc, threshold) && offsetof(ArcticBloom, soft_knee) == offsetof(BloomDesc, soft_knee) &&
              offsetof(ArcticBloom, clamp_max) == offsetof(BloomDesc, clamp_max) && offsetof(ArcticBloom, intensity) == offsetof(BloomDesc, intensity) &&
              offsetof(ArcticBloom, spread) == offsetof(BloomDesc, spread) && offsetof(ArcticBloom, levels) == offsetof(BloomDesc, levels) &&
              offsetof(ArcticBloom, reserved) == offsetof(BloomDesc, reserved), "the public record is the internal one");
static_assert(ARCTIC_BLOOM_SOURCE_COMPOSED == BLOOM_SOURCE_COMPOSED && ARCTIC_BLOOM_SOURCE_TAA == BLOOM_SOURCE_TAA && ARCTIC_BLOOM_SOURCE_MOTION_BLUR == BLOOM_SOURCE_MOTION_BLUR &&
              ARCTIC_BLOOM_SOURCE_DOF == BLOOM_SOURCE_DOF && ARCTIC_BLOOM_MAX_LEVELS == BLOOM_MAX_LEVELS, "the flags");

const char *bloom_refusal(const BloomDesc *d) {
    if (!d) return "null parameters";
    if (d->flags & ~(BLOOM_SOURCE_COMPOSED | BLOOM_SOURCE_TAA | BLOOM_SOURCE_MOTION_BLUR | BLOOM_SOURCE_DOF)) return "flags have unknown bits";
    if (d->flags & (d->flags - 1u)) return "the ARCTIC_BLOOM_SOURCE_* flags exclude each other";
    if (!(d->threshold >= 0.0f && d->threshold <= 65504.0f)) return "threshold outside [0, 65504]";   // (a NaN fails every comparison)
    if (!(d->soft_knee >= 0.0f && d->soft_knee <= 1.0f)) return "soft_knee outside [0, 1]";
    if (!(d->clamp_max > 0.0f && d->clamp_max <= 65504.0f)) return "clamp_max outside (0, 65504]";
    if (!(d->intensity >= 0.0f && d->intensity <= 16.0f)) return "intensity outside [0, 16]";
    if (!(d->spread >= 0.0f && d->spread <= 1.0f)) return "spread outside [0, 1]";
    if (!(d->levels >= 1u && d->levels <= BLOOM_MAX_LEVELS)) return "levels outside 1..8";
    if (d->reserved != 0u) return "reserved is not 0";
    return nullptr;
}

namespace {
// a row-major float3 plane as bloom_up's texel
struct PlaneTexel {
    const float *t;
    uint32_t w;
    void operator()(uint32_t x, uint32_t y, float *c) const {
        const float *s = t + ((size_t)y * w + x) * 3;
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    }
};
bool bad_side(uint32_t n) { return n == 0 || n > BLOOM_MAX_SIDE; }
}  // namespace

}  // namespace arctic

extern "C" int arctic_bloom_layout(uint32_t width, uint32_t height, uint32_t levels, uint64_t *out) {
    using namespace arctic;
    if (!out || bad_side(width) || bad_side(height) || levels < 1u || levels > BLOOM_MAX_LEVELS) return ARCTIC_E_INVALID;
    const BloomLayout l = bloom_layout(width, height, levels);
    for (uint32_t k = 0; k < levels; ++k) { out[3 * k] = l.w[k]; out[3 * k + 1] = l.h[k]; out[3 * k + 2] = l.offset[k]; }
    out[3 * levels] = l.down_floats; out[3 * levels + 1] = l.up_floats;
    return ARCTIC_OK;
}

extern "C" int arctic_bloom_pyramid(const ArcticBloom *bloom, uint32_t width, uint32_t height, const float *rgb, float *down, float *up) {
    using namespace arctic;
    BloomDesc d;
    if (bloom) std::memcpy(&d, bloom, sizeof d);
    if (bloom_refusal(bloom ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (bad_side(width) || bad_side(height)) return ARCTIC_E_INVALID;
    if (!rgb || !down || (!up && d.levels > 1u)) return ARCTIC_E_INVALID;
    const BloomLayout l = bloom_layout(width, height, d.levels);
    // D_1: the prefilter is evaluated where the footprint reads it (the kernel evaluates it once per source pixel: the same function of the same colour)
    for (uint32_t y = 0; y < l.h[0]; ++y)
        for (uint32_t x = 0; x < l.w[0]; ++x) {
            const auto texel = [&](uint32_t i, uint32_t j, float *c) {
                const uint32_t qx = bloom_clamp((int32_t)(2 * x + i) - 2, width), qy = bloom_clamp((int32_t)(2 * y + j) - 2, height);
                bloom_prefilter(d, rgb + ((size_t)qy * width + qx) * 3, c);
            };
            bloom_down<true>(texel, down + ((size_t)y * l.w[0] + x) * 3);
        }
    for (uint32_t k = 1; k < d.levels; ++k) {
        const float *src = down + l.offset[k - 1];
        float *dst = down + l.offset[k];
        const uint32_t ws = l.w[k - 1], hs = l.h[k - 1];
        for (uint32_t y = 0; y < l.h[k]; ++y)
            for (uint32_t x = 0; x < l.w[k]; ++x) {
                const auto texel = [&](uint32_t i, uint32_t j, float *c) {
                    PlaneTexel{src, ws}(bloom_clamp((int32_t)(2 * x + i) - 2, ws), bloom_clamp((int32_t)(2 * y + j) - 2, hs), c);
                };
                bloom_down<false>(texel, dst + ((size_t)y * l.w[k] + x) * 3);
            }
    }
    for (uint32_t k = d.levels - 1; k >= 1; --k) {   // level k (index k - 1) from level k + 1
        const float *coarse = (k + 1 == d.levels ? down : up) + l.offset[k];
        const PlaneTexel texel = {coarse, l.w[k]};
        for (uint32_t y = 0; y < l.h[k - 1]; ++y)
            for (uint32_t x = 0; x < l.w[k - 1]; ++x) {
                const size_t o = l.offset[k - 1] + ((size_t)y * l.w[k - 1] + x) * 3;
                float t[3];
                bloom_up(x, y, l.w[k], l.h[k], texel, t);
                bloom_up_add(d, down + o, t, up + o);
            }
    }
    return ARCTIC_OK;
}

extern "C" int arctic_bloom_pixels(const ArcticBloom *bloom, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb, const float *up1,
                                   float *out_rgb) {
    using namespace arctic;
    BloomDesc d;
    if (bloom) std::memcpy(&d, bloom, sizeof d);
    if (bloom_refusal(bloom ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (bad_side(width) || bad_side(height)) return ARCTIC_E_INVALID;
    if (n && (!pixel_xy || !rgb || !up1 || !out_rgb)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= width || (uint32_t)pixel_xy[2 * k + 1] >= height) return ARCTIC_E_INVALID;
    const uint32_t w1 = bloom_half(width), h1 = bloom_half(height);
    const PlaneTexel texel = {up1, w1};
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t px = (uint32_t)pixel_xy[2 * k], py = (uint32_t)pixel_xy[2 * k + 1];
        float t[3];
        bloom_up(px, py, w1, h1, texel, t);
        bloom_composite(d, rgb + ((size_t)py * width + px) * 3, t, out_rgb + 3 * k);
    }
    return ARCTIC_OK;
}
