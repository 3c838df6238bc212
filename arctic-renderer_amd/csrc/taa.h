// taa.h -- the temporal anti-aliasing resolve (include/arctic_hip.h: arctic_taa_resolve_device and the text in front of it, which is the definition;
// nothing here restates it, it only carries it out).  ONE copy of the neighbourhood box, the four history taps, the clamp and the two blends,
// compiled for the host (taa.cpp: the arbiter arctic_taa_pixels) and for the device (taa.hip: k_taa_resolve), both with contraction off.  Plain
// C++ like ao_history.h, whose tap scheme it shares; rq_min, rq_max and rq_finite are ray_query.h's.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticTaa (static_assert in taa.cpp)
struct TaaDesc { uint32_t flags; float max_history, min_weight, jitter[2]; uint32_t reserved[3]; };
constexpr uint32_t TAA_LUMA_WEIGHT = 1u, TAA_SOURCE_COMPOSED = 2u;   // ARCTIC_TAA_*

// step 6's weight of a colour under ARCTIC_TAA_LUMA_WEIGHT
RQ_HD float taa_luma_weight(const float *c) { return 1.0f / (1.0f + rq_max(rq_max(rq_max(c[0], c[1]), c[2]), 0.0f)); }

// Steps 1 to 6 for pixel (px, py) of a width x height frame.  color(qx, qy, c) loads C of a pixel inside the frame; v: the pixel's velocity;
// have: T is not empty; history(qx, qy, e) loads the previous T's {r, g, b, N} of a pixel inside the frame -- it is called only for such taps,
// and what it loads is used only under the selects below.  out: {r, g, b, N}, the entry to store
template <class Color, class History>
RQ_HD void taa_pixel(uint32_t px, uint32_t py, uint32_t width, uint32_t height, const TaaDesc &d, Color color, const float *v, bool have, History history, float *out) {
    const float W = (float)width, H = (float)height;
    // step 1: the pixel and its 3x3 box, clamped at the frame's edge
    float c[3], lo[3], hi[3];
    color(px, py, c);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t x = (int32_t)px + dx, y = (int32_t)py + dy;
            const uint32_t qx = (uint32_t)(x < 0 ? 0 : x > (int32_t)width - 1 ? (int32_t)width - 1 : x);
            const uint32_t qy = (uint32_t)(y < 0 ? 0 : y > (int32_t)height - 1 ? (int32_t)height - 1 : y);
            float n[3];
            color(qx, qy, n);
            for (int i = 0; i < 3; ++i) {
                if (dy == -1 && dx == -1) { lo[i] = n[i]; hi[i] = n[i]; }
                lo[i] = (n[i] < lo[i]) ? n[i] : lo[i];
                hi[i] = (n[i] > hi[i]) ? n[i] : hi[i];
            }
        }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = 1.0f;   // steps 2, 3 and 4's rejections
    if (!have) return;
    // step 3: where the history is fetched
    const float hx = (((float)px + 0.5f) + v[0]) + d.jitter[0], hy = (((float)py + 0.5f) + v[1]) + d.jitter[1];
    const float gx = hx - 0.5f, gy = hy - 0.5f;
    const float ix = __builtin_floorf(gx), iy = __builtin_floorf(gy);
    const float ax = gx - ix, ay = gy - iy;
    if (!(rq_finite(hx) && rq_finite(hy) && ix >= -1.0f && ix <= W - 1.0f && iy >= -1.0f && iy <= H - 1.0f)) return;   // (a NaN fails every comparison)
    // step 4: the four taps
    const int32_t x0 = (int32_t)ix, y0 = (int32_t)iy;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float weight[4] = {bx * by, ax * by, bx * ay, ax * ay};
    float k[4], kr[4], kg[4], kb[4], kn[4];
    for (int t = 0; t < 4; ++t) {
        const int32_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
        bool accepted = false;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (qx >= 0 && qy >= 0 && qx < (int32_t)width && qy < (int32_t)height) {
            history((uint32_t)qx, (uint32_t)qy, e);
            accepted = e[3] > 0.0f;
        }
        k[t] = accepted ? weight[t] : 0.0f;
        kr[t] = accepted ? weight[t] * e[0] : 0.0f;
        kg[t] = accepted ? weight[t] * e[1] : 0.0f;
        kb[t] = accepted ? weight[t] * e[2] : 0.0f;
        kn[t] = accepted ? weight[t] * e[3] : 0.0f;
    }
    const float S = ((k[0] + k[1]) + k[2]) + k[3];
    if (!(S > d.min_weight)) return;
    // step 5: the history's colour, clamped to the box
    float h[3] = {(((kr[0] + kr[1]) + kr[2]) + kr[3]) / S, (((kg[0] + kg[1]) + kg[2]) + kg[3]) / S, (((kb[0] + kb[1]) + kb[2]) + kb[3]) / S};
    const float hn = (((kn[0] + kn[1]) + kn[2]) + kn[3]) / S;
    for (int i = 0; i < 3; ++i) {
        h[i] = (h[i] < lo[i]) ? lo[i] : h[i];
        h[i] = (h[i] > hi[i]) ? hi[i] : h[i];
    }
    // step 6: the blend
    const float N = rq_min(hn + 1.0f, d.max_history);
    const float a = 1.0f / N;
    if (d.flags & TAA_LUMA_WEIGHT) {
        const float wc = taa_luma_weight(c), wh = taa_luma_weight(h);
        const float kc = a * wc, kh = (1.0f - a) * wh;
        const float sum = kc + kh;
        for (int i = 0; i < 3; ++i) out[i] = (c[i] * kc + h[i] * kh) / sum;
    } else {
        for (int i = 0; i < 3; ++i) out[i] = h[i] + (c[i] - h[i]) * a;
    }
    out[3] = N;
}

// ---- host side (taa.cpp) ---------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the block's sake, in the header's order: null = nothing; else the reason
const char *taa_refusal(const TaaDesc *d);
// arctic_jitter_proj_view's arithmetic (the caller has checked the arguments)
void taa_jitter_matrix(float *m, uint32_t width, uint32_t height, float jx, float jy);

#if defined(__HIPCC__)
// taa.hip.  What k_taa_resolve reads and writes, for a handle that owns the whole frame (width x rows pixels): the row-major planes color (3 floats
// per pixel; a wave reads its tile and an apron of one pixel into LDS) and velocity (2 floats, 8-byte aligned; null = zero) in; the previous T
// (prev: float4 per pixel, tile-major like the G-buffer; null = T is empty) and the one it writes (next: never the previous one); RGBA8 and
// float LDR (3 floats), row-major, out.  No plane may alias another.
struct TaaParams {
    const float *color; const void *velocity;
    const void *prev; void *next;
    uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, tiles_y, width, rows;
    int32_t tm;
    float inv_gamma, exposure;
    TaaDesc d;
};
// enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_taa_resolve(const TaaParams &p, hipStream_t s);
#endif

}  // namespace arctic
