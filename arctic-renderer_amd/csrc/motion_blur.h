// motion_blur.h -- the motion blur (include/arctic_hip.h: arctic_motion_blur_device and the text in front of it, which is the definition; nothing
// here restates it, it only carries it out).  ONE copy of the half velocity, the two tile maxima and the depth-aware gather, compiled for the
// host (motion_blur.cpp: the arbiters arctic_motion_blur_prepare and arctic_motion_blur_pixels) and for the device (motion_blur.hip), both with
// contraction off.  Plain C++ like taa.h; rq_min, rq_max and rq_finite are ray_query.h's.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticMotionBlur (static_assert in motion_blur.cpp)
struct MotionBlurDesc { uint32_t flags; float shutter, max_radius; uint32_t samples; float depth_extent; uint32_t reserved[3]; };
constexpr uint32_t MB_DITHER = 1u, MB_SOURCE_COMPOSED = 2u, MB_SOURCE_TAA = 4u;   // ARCTIC_MB_*
constexpr uint32_t MB_TILE = 8;   // a tile of the two maxima is the G-buffer's: 8 x 8 pixels

RQ_HD float mb_clamp01(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }
// step 3's window, in tiles: ceil(max_radius / 8), 1 .. 8 for a max_radius the calls accept
RQ_HD uint32_t mb_window(const MotionBlurDesc &d) { return (uint32_t)__builtin_ceilf(d.max_radius / 8.0f); }

// step 1: the half velocity h of a pixel whose velocity is v, its squared length l2 (what the tile maximum compares) and its length l, floored
RQ_HD void mb_half_velocity(const MotionBlurDesc &d, float vx, float vy, float *h, float &l2, float &l) {
    const float k = 0.5f * d.shutter;
    float hx = vx * k, hy = vy * k;
    if (!(rq_finite(hx) && rq_finite(hy))) { hx = 0.0f; hy = 0.0f; }
    const float len = __builtin_sqrtf(hx * hx + hy * hy);
    if (len > d.max_radius) {
        const float s = d.max_radius / len;
        hx = hx * s; hy = hy * s;
    }
    l2 = hx * hx + hy * hy;
    l = rq_max(__builtin_sqrtf(l2), 0.5f);
    h[0] = hx; h[1] = hy;
}

// step 2 on the host: tile (tx, ty)'s winner among its pixels inside the frame, in lane order, the first among equals.  half(x, y, h, l2)
template <class Half>
RQ_HD void mb_tile_max(uint32_t tx, uint32_t ty, uint32_t width, uint32_t height, Half half, float *out) {
    float best = -1.0f;
    for (uint32_t lane = 0; lane < MB_TILE * MB_TILE; ++lane) {
        const uint32_t x = tx * MB_TILE + (lane & 7u), y = ty * MB_TILE + (lane >> 3);
        if (x >= width || y >= height) continue;
        float h[2], l2;
        half(x, y, h, l2);
        if (l2 > best) { best = l2; out[0] = h[0]; out[1] = h[1]; }
    }
}

// step 3: tile (tx, ty)'s winner among the tiles of its window inside the grid, row-major, the first among equals.  tile(x, y, h) loads tile_max2
template <class Tile>
RQ_HD void mb_neighbour_max(uint32_t tx, uint32_t ty, uint32_t tiles_x, uint32_t tiles_y, uint32_t window, Tile tile, float *out) {
    float best = -1.0f;
    const int32_t R = (int32_t)window;
    for (int32_t dy = -R; dy <= R; ++dy)
        for (int32_t dx = -R; dx <= R; ++dx) {
            const int32_t x = (int32_t)tx + dx, y = (int32_t)ty + dy;
            if (x < 0 || y < 0 || x >= (int32_t)tiles_x || y >= (int32_t)tiles_y) continue;
            float h[2];
            tile((uint32_t)x, (uint32_t)y, h);
            const float l2 = h[0] * h[0] + h[1] * h[1];
            if (l2 > best) { best = l2; out[0] = h[0]; out[1] = h[1]; }
        }
}

// the 4 x 4 Bayer matrix of step 4, rows {0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}: four bits per entry, entry [y][x] at 4 * (4y + x)
RQ_HD float mb_bayer(uint32_t px, uint32_t py) { return (float)((0x5D7F91B36E4CA280ull >> (((py & 3u) * 4u + (px & 3u)) * 4u)) & 15ull); }

RQ_HD float mb_cone(float dist, float l) { return mb_clamp01(1.0f - dist / l); }
RQ_HD float mb_cylinder(float dist, float l) {
    const float s = mb_clamp01((dist - 0.95f * l) / (0.1f * l));
    return 1.0f - (s * s) * (3.0f - 2.0f * s);
}

// Step 4 for pixel (px, py) of a width x height frame; (dx, dy): neighbour_max2 of the pixel's tile.  color(qx, qy, c) loads C and
// prep(qx, qy, l, z) loads P of a pixel inside the frame -- both are called only for such pixels, the colour of a tap only when its weight enters
template <class Color, class Prep>
RQ_HD void mb_pixel(uint32_t px, uint32_t py, uint32_t width, uint32_t height, const MotionBlurDesc &d, float dx, float dy, Color color, Prep prep, float *out) {
    float c[3];
    color(px, py, c);
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    const float dl = __builtin_sqrtf(dx * dx + dy * dy);
    if (!(dl > 0.5f)) return;   // nothing fast reaches this tile: a copy
    float lp, zp;
    prep(px, py, lp, zp);
    float w = 1.0f / lp;
    float acc[3] = {c[0] * w, c[1] * w, c[2] * w};
    const float o = (d.flags & MB_DITHER) ? ((mb_bayer(px, py) + 0.5f) / 16.0f) - 0.5f : 0.0f;
    const float n = (float)d.samples, cx = (float)px + 0.5f, cy = (float)py + 0.5f, xmax = (float)(width - 1u), ymax = (float)(height - 1u);
    for (uint32_t i = 0; i < d.samples; ++i) {
        const float t = ((((float)i + 0.5f) + o) / n) * 2.0f - 1.0f;
        const float qx = __builtin_floorf(cx + t * dx), qy = __builtin_floorf(cy + t * dy);
        if (!(qx >= 0.0f && qx <= xmax && qy >= 0.0f && qy <= ymax)) continue;   // outside the frame (a NaN fails): weight 0, nothing read
        const uint32_t ux = (uint32_t)qx, uy = (uint32_t)qy;
        const float dist = __builtin_fabsf(t) * dl;
        float lq, zq;
        prep(ux, uy, lq, zq);
        const float f = mb_clamp01(1.0f - (zq - zp) / d.depth_extent);
        const float b = mb_clamp01(1.0f - (zp - zq) / d.depth_extent);
        const float a = (f * mb_cone(dist, lq) + b * mb_cone(dist, lp)) + (mb_cylinder(dist, lq) * mb_cylinder(dist, lp)) * 2.0f;
        if (!(a > 0.0f)) continue;   // a select: the colour does not enter
        float s[3];
        color(ux, uy, s);
        w = w + a;
        acc[0] = acc[0] + s[0] * a; acc[1] = acc[1] + s[1] * a; acc[2] = acc[2] + s[2] * a;
    }
    out[0] = acc[0] / w; out[1] = acc[1] / w; out[2] = acc[2] / w;
}

// ---- host side (motion_blur.cpp) -------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the block's sake, in the header's order: null = nothing; else the reason
const char *motion_blur_refusal(const MotionBlurDesc *d);

#if defined(__HIPCC__)
// motion_blur.hip.  The planes of a handle that owns the whole frame (width x rows pixels).  velocity: float2 per pixel, row-major, 8-byte
// aligned; depth: one float per pixel, row-major, or null = 0 everywhere; prep: P, float2 {l, z} per pixel, row-major; tile_max, neighbour_max:
// float2 per tile.  color: row-major float3, or -- color_taa -- the anti-aliasing's tile-major float4 history.  out_hdr (3 floats), out_ldr (3
// floats) and out_rgba8, row-major.  No plane that is written may alias another
struct MotionBlurParams {
    const void *velocity; const float *depth;
    void *prep, *tile_max, *neighbour_max;
    const void *color; bool color_taa;
    float *out_hdr; uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, tiles_y, width, rows;
    int32_t tm;
    float inv_gamma, exposure;
    MotionBlurDesc d;
};
// each enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_mb_tile_max(const MotionBlurParams &p, hipStream_t s);
hipError_t launch_mb_neighbour_max(const MotionBlurParams &p, hipStream_t s);
hipError_t launch_motion_blur(const MotionBlurParams &p, hipStream_t s);
// the depth word of the visibility plane `vis` (tile-major keys, depth bits << 32 | order id; ~0 = nothing drawn = 1.0) of the handle's rows
// (row0_in_tile: the first row's offset in its tile row) as a row-major float plane
hipError_t launch_mb_depth(const unsigned long long *vis, float *depth, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows, uint32_t row0_in_tile, hipStream_t s);
#endif

}  // namespace arctic
