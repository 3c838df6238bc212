// dof.h -- depth of field (include/arctic_hip.h: arctic_dof_device and the text in front of it, which is the definition; nothing here restates
// it, it only carries it out).  ONE copy of the view distance and signed radius, the two tile maxima and the disc gather, compiled for the
// host (dof.cpp: the arbiters arctic_dof_prepare and arctic_dof_pixels) and for the device (dof.hip), both with contraction off.  Plain C++
// like motion_blur.h; rq_min, rq_max and rq_finite are ray_query.h's.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticDof (static_assert in dof.cpp)
struct DofDesc { uint32_t flags; float focus_distance, coc_scale, max_radius; uint32_t samples; float depth_extent, z_near, z_far; };
constexpr uint32_t DOF_SOURCE_COMPOSED = 1u, DOF_SOURCE_TAA = 2u, DOF_SOURCE_MOTION_BLUR = 4u;   // ARCTIC_DOF_*
constexpr uint32_t DOF_TILE = 8;          // a tile of the two maxima is the G-buffer's: 8 x 8 pixels
constexpr uint32_t DOF_MAX_SAMPLES = 64;
constexpr float DOF_A0 = 0.5641896f;      // 1 / sqrt(pi): a sharp pixel's disc has the area of one pixel
constexpr float DOF_INV_PI = 0.31830987f;

RQ_HD float dof_clamp01(float x) { return !(x > 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x); }
// step 3's window, in tiles: ceil(max_radius / 8), 1 .. 8 for a max_radius the calls accept
RQ_HD uint32_t dof_window(const DofDesc &d) { return (uint32_t)__builtin_ceilf(d.max_radius / 8.0f); }

// step 1's view distance of a pixel whose prepass depth is `depth` (arctic_dof_focus_at returns it)
RQ_HD float dof_view_distance(float z_near, float z_far, float depth) {
    const float den = z_far - depth * (z_far - z_near);
    return den > 0.0f ? (z_near * z_far) / den : z_far;   // (a NaN fails the test)
}

// step 1: the signed radius s and the view distance zv of a pixel
RQ_HD void dof_signed_radius(const DofDesc &d, float depth, float &s, float &zv) {
    zv = dof_view_distance(d.z_near, d.z_far, depth);
    s = d.coc_scale * (1.0f - d.focus_distance / zv);
    if (!rq_finite(s)) s = 0.0f;
    s = rq_min(rq_max(s, -d.max_radius), d.max_radius);
}
// a_p of a signed radius
RQ_HD float dof_disc(float s) { return rq_max(__builtin_fabsf(s), DOF_A0); }

// step 2 on the host: the largest |s| among tile (tx, ty)'s pixels inside the frame.  radius(x, y) gives |s|
template <class Radius>
RQ_HD float dof_tile_max(uint32_t tx, uint32_t ty, uint32_t width, uint32_t height, Radius radius) {
    float best = 0.0f;
    for (uint32_t lane = 0; lane < DOF_TILE * DOF_TILE; ++lane) {
        const uint32_t x = tx * DOF_TILE + (lane & 7u), y = ty * DOF_TILE + (lane >> 3);
        if (x >= width || y >= height) continue;
        best = rq_max(best, radius(x, y));
    }
    return best;
}

// step 3: the largest tile_max among the tiles of (tx, ty)'s window inside the grid.  tile(x, y) loads tile_max
template <class Tile>
RQ_HD float dof_neighbour_max(uint32_t tx, uint32_t ty, uint32_t tiles_x, uint32_t tiles_y, uint32_t window, Tile tile) {
    float best = 0.0f;
    const int32_t R = (int32_t)window;
    for (int32_t dy = -R; dy <= R; ++dy)
        for (int32_t dx = -R; dx <= R; ++dx) {
            const int32_t x = (int32_t)tx + dx, y = (int32_t)ty + dy;
            if (x < 0 || y < 0 || x >= (int32_t)tiles_x || y >= (int32_t)tiles_y) continue;
            best = rq_max(best, tile((uint32_t)x, (uint32_t)y));
        }
    return best;
}

// Step 4 for pixel (px, py) of a width x height frame; R: neighbour_max of the pixel's tile; taps2: d.samples float2.  color(qx, qy, c) loads C
// and prep(qx, qy, s, z) loads P of a pixel inside the frame -- both are called only for such pixels, the colour of a tap only when its weight enters
template <class Color, class Prep>
RQ_HD void dof_pixel(uint32_t px, uint32_t py, uint32_t width, uint32_t height, const DofDesc &d, float R, const float *taps2, Color color, Prep prep, float *out) {
    float c[3];
    color(px, py, c);
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    if (!(R > 0.5f)) return;   // nothing out of focus reaches this tile: a copy
    float sp, zp;
    prep(px, py, sp, zp);
    const float ap = dof_disc(sp);
    const float k = (R * R) / (float)d.samples;
    float w = DOF_INV_PI / (ap * ap);
    float acc[3] = {c[0] * w, c[1] * w, c[2] * w};
    bool entered = false;
    const float cx = (float)px + 0.5f, cy = (float)py + 0.5f, xmax = (float)(width - 1u), ymax = (float)(height - 1u);
    for (uint32_t i = 0; i < d.samples; ++i) {
        const float ox = taps2[2 * i] * R, oy = taps2[2 * i + 1] * R;
        const float qx = __builtin_floorf(cx + ox), qy = __builtin_floorf(cy + oy);
        if (!(qx >= 0.0f && qx <= xmax && qy >= 0.0f && qy <= ymax)) continue;   // outside the frame (a NaN fails): nothing read
        const uint32_t ux = (uint32_t)qx, uy = (uint32_t)qy;
        const float dist = __builtin_sqrtf(ox * ox + oy * oy);
        float sq, zq;
        prep(ux, uy, sq, zq);
        const float aq = dof_disc(sq);
        const float behind = dof_clamp01((zq - zp) / d.depth_extent);
        const float e = aq - behind * (aq - rq_min(aq, ap));
        const float cover = dof_clamp01(e - dist);
        const float a = (cover * k) / (aq * aq);
        if (!(a > 0.0f)) continue;   // a select: the colour does not enter
        float s[3];
        color(ux, uy, s);
        w = w + a;
        acc[0] = acc[0] + s[0] * a; acc[1] = acc[1] + s[1] * a; acc[2] = acc[2] + s[2] * a;
        entered = true;
    }
    if (!entered) return;      // a pixel that nothing covers keeps its bits
    out[0] = acc[0] / w; out[1] = acc[1] / w; out[2] = acc[2] / w;
}

// ---- host side (dof.cpp) -----------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the block's sake, in the header's order: null = nothing; else the reason.
// zero_planes: z_near == z_far == 0 is accepted (arctic_pass_dof, which takes the scene's camera planes)
const char *dof_refusal(const DofDesc *d, bool zero_planes);
// ... and for the tap table's: d->samples float2, every component finite, inside the unit disc
const char *dof_taps_refusal(const DofDesc *d, const float *taps2);
// dof_view_distance as dof.cpp compiles it, with contraction off: for a unit that is not compiled so (arctic_dof_focus_at)
float dof_view_distance_host(float z_near, float z_far, float depth);

#if defined(__HIPCC__)
// dof.hip.  The planes of a handle that owns the whole frame (width x rows pixels).  depth: one float per pixel, row-major; prep: P, float2
// {s, zv} per pixel, row-major; tile_max, neighbour_max: one float per tile; taps: d.samples float2 on the device.  color: row-major float3,
// or -- color_taa -- the anti-aliasing's tile-major float4 history.  out_hdr (3 floats), out_ldr (3 floats) and out_rgba8, row-major.  No
// plane that is written may alias another
struct DofParams {
    const float *depth;
    void *prep; float *tile_max, *neighbour_max;
    const void *color; bool color_taa;
    const float *taps;
    float *out_hdr; uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, tiles_y, width, rows;
    int32_t tm;
    float inv_gamma, exposure;
    DofDesc d;
};
// each enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_dof_prepare(const DofParams &p, hipStream_t s);
hipError_t launch_dof_neighbour_max(const DofParams &p, hipStream_t s);
hipError_t launch_dof_gather(const DofParams &p, hipStream_t s);
#endif

}  // namespace arctic
