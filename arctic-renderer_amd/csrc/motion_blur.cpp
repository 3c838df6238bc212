// motion_blur.cpp -- the host side of the motion blur (include/arctic_hip.h: arctic_motion_blur_device): what the entry points refuse before a
// device is touched, and the arbiters arctic_motion_blur_prepare and arctic_motion_blur_pixels -- the functions of motion_blur.h that
// motion_blur.hip runs, on the CPU.  No HIP type: it also compiles with a host compiler alone (tests/cpp/motion_blur_sanitize.cpp).
#include "motion_blur.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticMotionBlur) == 32 && sizeof(MotionBlurDesc) == 32, "ArcticMotionBlur");
static_assert(offsetof(ArcticMotionBlur, shutter) == offsetof(MotionBlurDesc, shutter) && offsetof(ArcticMotionBlur, max_radius) == offsetof(MotionBlurDesc, max_radius) &&
              offsetof(ArcticMotionBlur, samples) == offsetof(MotionBlurDesc, samples) && offsetof(ArcticMotionBlur, depth_extent) == offsetof(MotionBlurDesc, depth_extent) &&
              offsetof(ArcticMotionBlur, reserved) == offsetof(MotionBlurDesc, reserved), "the public record is the internal one");
static_assert(ARCTIC_MB_DITHER == MB_DITHER && ARCTIC_MB_SOURCE_COMPOSED == MB_SOURCE_COMPOSED && ARCTIC_MB_SOURCE_TAA == MB_SOURCE_TAA, "the flags");

const char *motion_blur_refusal(const MotionBlurDesc *d) {
    if (!d) return "null parameters";
    if (d->flags & ~(MB_DITHER | MB_SOURCE_COMPOSED | MB_SOURCE_TAA)) return "flags have unknown bits";
    if ((d->flags & MB_SOURCE_COMPOSED) && (d->flags & MB_SOURCE_TAA)) return "ARCTIC_MB_SOURCE_COMPOSED and ARCTIC_MB_SOURCE_TAA exclude each other";
    if (!(d->shutter >= 0.0f && d->shutter <= 4.0f)) return "shutter outside [0, 4]";   // (a NaN fails every comparison)
    if (!(d->max_radius >= 1.0f && d->max_radius <= 64.0f)) return "max_radius outside [1, 64]";
    if (!(d->samples >= 1u && d->samples <= 64u)) return "samples outside 1..64";
    if (!(d->depth_extent > 0.0f && rq_finite(d->depth_extent))) return "depth_extent not finite and above 0";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2]) return "reserved not 0";
    return nullptr;
}

}  // namespace arctic

extern "C" int arctic_motion_blur_prepare(const ArcticMotionBlur *mb, uint32_t width, uint32_t height, const float *velocity2, const float *depth, float *tile_max2,
                                          float *neighbour_max2, float *prepared2) {
    using namespace arctic;
    MotionBlurDesc d;
    if (mb) std::memcpy(&d, mb, sizeof d);
    if (motion_blur_refusal(mb ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (!velocity2 || !tile_max2 || !neighbour_max2 || !prepared2) return ARCTIC_E_INVALID;
    const uint32_t tiles_x = (width + MB_TILE - 1) / MB_TILE, tiles_y = (height + MB_TILE - 1) / MB_TILE;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t o = (size_t)y * width + x;
            float h[2], l2, l;
            mb_half_velocity(d, velocity2[2 * o], velocity2[2 * o + 1], h, l2, l);
            prepared2[2 * o] = l; prepared2[2 * o + 1] = depth ? depth[o] : 0.0f;
        }
    const auto half = [&](uint32_t x, uint32_t y, float *h, float &l2) {
        const size_t o = (size_t)y * width + x;
        float l;
        mb_half_velocity(d, velocity2[2 * o], velocity2[2 * o + 1], h, l2, l);
    };
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) mb_tile_max(tx, ty, width, height, half, tile_max2 + 2 * ((size_t)ty * tiles_x + tx));
    const auto tile = [&](uint32_t tx, uint32_t ty, float *h) {
        const float *s = tile_max2 + 2 * ((size_t)ty * tiles_x + tx);
        h[0] = s[0]; h[1] = s[1];
    };
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) mb_neighbour_max(tx, ty, tiles_x, tiles_y, mb_window(d), tile, neighbour_max2 + 2 * ((size_t)ty * tiles_x + tx));
    return ARCTIC_OK;
}

extern "C" int arctic_motion_blur_pixels(const ArcticMotionBlur *mb, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                                         const float *prepared2, const float *neighbour_max2, float *out_rgb) {
    using namespace arctic;
    MotionBlurDesc d;
    if (mb) std::memcpy(&d, mb, sizeof d);
    if (motion_blur_refusal(mb ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (n && (!pixel_xy || !rgb || !prepared2 || !neighbour_max2 || !out_rgb)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= width || (uint32_t)pixel_xy[2 * k + 1] >= height) return ARCTIC_E_INVALID;
    const uint32_t tiles_x = (width + MB_TILE - 1) / MB_TILE;
    const auto color = [&](uint32_t qx, uint32_t qy, float *c) {
        const float *s = rgb + ((size_t)qy * width + qx) * 3;
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    };
    const auto prep = [&](uint32_t qx, uint32_t qy, float &l, float &z) {
        const float *s = prepared2 + ((size_t)qy * width + qx) * 2;
        l = s[0]; z = s[1];
    };
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t px = (uint32_t)pixel_xy[2 * k], py = (uint32_t)pixel_xy[2 * k + 1];
        const float *nm = neighbour_max2 + 2 * ((size_t)(py / MB_TILE) * tiles_x + px / MB_TILE);
        mb_pixel(px, py, width, height, d, nm[0], nm[1], color, prep, out_rgb + 3 * k);
    }
    return ARCTIC_OK;
}
