// taa_upscale.h -- the temporal upscaler (include/arctic_hip.h: arctic_taa_upscale_device and the text in front of it, which is the definition;
// nothing here restates it, it only carries it out).  ONE copy of the nearest sample, its confidence, the box, the four history taps on the
// output grid and the blends, compiled for the host (taa_upscale.cpp: the arbiter arctic_taa_upscale_pixels) and for the device
// (taa_upscale.hip: k_taa_upscale), both with contraction off.  The flags' values and the luma weight are taa.h's: the two stages share them.
#pragma once
#include "taa.h"

namespace arctic {

// == ArcticTaaUpscale (static_assert in taa_upscale.cpp); the first five fields lie where TaaDesc's do
struct TaaUpscaleDesc { uint32_t flags; float max_history, min_weight, jitter[2], sharpness, confidence_floor; uint32_t out_width, out_height, reserved[3]; };
constexpr uint32_t TAA_UPSCALE_LUMA_WEIGHT = TAA_LUMA_WEIGHT, TAA_UPSCALE_SOURCE_COMPOSED = TAA_SOURCE_COMPOSED, TAA_UPSCALE_NO_CLAMP = 4u;   // ARCTIC_TAA_UPSCALE_*
constexpr uint32_t TAA_UPSCALE_MAX_RATIO = 4, TAA_UPSCALE_JITTER_EXACT = 0x80000000u;

// The input pixels one 8 x 8 output tile can name.  Along an axis the tile's pixels px0 .. px0+7 have centres u = (px + 0.5) * r with r <= 1, so
// their u + j span at most 7 before rounding; a product and a sum of values below 2^15 each round by less than 2^-9, so the rounded sums span
// less than 8, their floors differ by at most 8, and clamping only narrows that: at most 9 values of q.  The box adds one pixel on either side
constexpr uint32_t TAA_UPSCALE_SPAN = 8 /* TILE */ - 1 + 2, TAA_UPSCALE_FOOTPRINT = TAA_UPSCALE_SPAN + 2;
static_assert(TAA_UPSCALE_FOOTPRINT == 11, "an output tile reads at most 11 x 11 input pixels, the box's apron included");

// step 1 along one axis for output pixel p: in is the input's extent, r the ratio, j the jitter.  Returns q and writes D
RQ_HD uint32_t taa_upscale_nearest(uint32_t p, uint32_t in, float r, float j, float *D) {
    const float u = ((float)p + 0.5f) * r;
    const float f = __builtin_floorf(u + j), top = (float)in - 1.0f;
    const float qf = f < 0.0f ? 0.0f : f > top ? top : f;   // (u + j is finite: |j| <= 1)
    *D = (((qf + 0.5f) - j) - u) / r;
    return (uint32_t)qf;
}

// Steps 1 to 6 for output pixel (px, py): w x h is the input frame, d.out_width x d.out_height the output.  color(qx, qy, c) loads C of an input
// pixel inside the input frame; velocity(qx, qy, v) loads its velocity2 (zero where there is no plane); have: U is not empty; history(qx, qy, e)
// loads the previous U's {r, g, b, N} of a pixel inside the OUTPUT frame -- it is called only for such taps, and what it loads is used only
// under the selects below.  out: {r, g, b, N}, the entry to store
template <class Color, class Velocity, class History>
RQ_HD void taa_upscale_pixel(uint32_t px, uint32_t py, uint32_t w, uint32_t h, const TaaUpscaleDesc &d, Color color, Velocity velocity, bool have, History history, float *out) {
    const float W = (float)d.out_width, H = (float)d.out_height;
    const float rx = (float)w / W, ry = (float)h / H;
    // step 1: the nearest sample and its offset in output pixels
    float Dx, Dy;
    const uint32_t qx = taa_upscale_nearest(px, w, rx, d.jitter[0], &Dx), qy = taa_upscale_nearest(py, h, ry, d.jitter[1], &Dy);
    // step 2: its colour and the box of the 3 x 3 input pixels around it, clamped at the input frame's edge
    float c[3], lo[3], hi[3];
    color(qx, qy, c);
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int32_t x = (int32_t)qx + dx, y = (int32_t)qy + dy;
            const uint32_t nx = (uint32_t)(x < 0 ? 0 : x > (int32_t)w - 1 ? (int32_t)w - 1 : x);
            const uint32_t ny = (uint32_t)(y < 0 ? 0 : y > (int32_t)h - 1 ? (int32_t)h - 1 : y);
            float n[3];
            color(nx, ny, n);
            for (int i = 0; i < 3; ++i) {
                if (dy == -1 && dx == -1) { lo[i] = n[i]; hi[i] = n[i]; }
                lo[i] = (n[i] < lo[i]) ? n[i] : lo[i];
                hi[i] = (n[i] > hi[i]) ? n[i] : hi[i];
            }
        }
    // step 3: the confidence
    const float beta = rq_max(0.0f, 1.0f - d.sharpness * (Dx * Dx + Dy * Dy));
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = rq_max(beta, d.confidence_floor);   // step 4, and every rejection of step 5
    if (!have) return;
    // step 5: where the history is fetched, on the output grid
    float v[2];
    velocity(qx, qy, v);
    const float hx = (((float)px + 0.5f) + v[0] / rx) + d.jitter[0] / rx, hy = (((float)py + 0.5f) + v[1] / ry) + d.jitter[1] / ry;
    const float gx = hx - 0.5f, gy = hy - 0.5f;
    const float ix = __builtin_floorf(gx), iy = __builtin_floorf(gy);
    const float ax = gx - ix, ay = gy - iy;
    if (!(rq_finite(hx) && rq_finite(hy) && ix >= -1.0f && ix <= W - 1.0f && iy >= -1.0f && iy <= H - 1.0f)) return;   // (a NaN fails every comparison)
    const int32_t x0 = (int32_t)ix, y0 = (int32_t)iy;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float weight[4] = {bx * by, ax * by, bx * ay, ax * ay};
    float k[4], kr[4], kg[4], kb[4], kn[4];
    for (int t = 0; t < 4; ++t) {
        const int32_t tx = x0 + (t & 1), ty = y0 + (t >> 1);
        bool accepted = false;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (tx >= 0 && ty >= 0 && tx < (int32_t)d.out_width && ty < (int32_t)d.out_height) {
            history((uint32_t)tx, (uint32_t)ty, e);
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
    float hc[3] = {(((kr[0] + kr[1]) + kr[2]) + kr[3]) / S, (((kg[0] + kg[1]) + kg[2]) + kg[3]) / S, (((kb[0] + kb[1]) + kb[2]) + kb[3]) / S};
    const float hn = (((kn[0] + kn[1]) + kn[2]) + kn[3]) / S;
    if (!(d.flags & TAA_UPSCALE_NO_CLAMP))
        for (int i = 0; i < 3; ++i) {
            hc[i] = (hc[i] < lo[i]) ? lo[i] : hc[i];
            hc[i] = (hc[i] > hi[i]) ? hi[i] : hc[i];
        }
    // step 6: the blend
    const float sum_n = hn + beta;
    const float N = rq_min(sum_n, d.max_history);
    const float a = beta / N;
    out[3] = N;
    if (beta == 0.0f) {
        for (int i = 0; i < 3; ++i) out[i] = hc[i];
    } else if (sum_n == beta) {
        // (out = c, which it is already)
    } else if (d.flags & TAA_UPSCALE_LUMA_WEIGHT) {
        const float wc = taa_luma_weight(c), wh = taa_luma_weight(hc);
        const float kc = a * wc, kh = (1.0f - a) * wh;
        const float sum = kc + kh;
        for (int i = 0; i < 3; ++i) out[i] = (c[i] * kc + hc[i] * kh) / sum;
    } else {
        for (int i = 0; i < 3; ++i) out[i] = hc[i] + (c[i] - hc[i]) * a;
    }
}

// ---- host side (taa_upscale.cpp) -------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the record's sake and for the sizes', in the header's order: null = nothing; else the
// reason.  w, h: the input frame
const char *taa_upscale_refusal(const TaaUpscaleDesc *d, uint32_t w, uint32_t h);

#if defined(__HIPCC__)
// taa_upscale.hip.  What k_taa_upscale reads and writes, for a handle that owns the whole frame: the row-major input planes color (3 floats per
// input pixel; a wave reads its tile's footprint into LDS) and velocity (2 floats, 8-byte aligned; null = zero); the previous U (prev: float4 per
// OUTPUT pixel, tile-major in 8 x 8 output tiles; null = U is empty) and the one it writes (next: never the previous one); RGBA8 and float LDR
// (3 floats), row-major at the output size.  No plane may alias another.
struct TaaUpscaleParams {
    const float *color; const void *velocity;
    const void *prev; void *next;
    uint32_t *out_rgba8; float *out_ldr;
    uint32_t width, height;          // the input frame
    uint32_t tiles_x, tiles_y;       // of the output frame
    int32_t tm;
    float inv_gamma, exposure;
    TaaUpscaleDesc d;
};
// enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_taa_upscale(const TaaUpscaleParams &p, hipStream_t s);
// u: a set of U of tiles_x x tiles_y output tiles; out: width x height x 3 floats, row-major.  Likewise
hipError_t launch_taa_upscale_hdr(const void *u, float *out, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s);
#endif

}  // namespace arctic
