// ao_history.h -- temporal accumulation of the ambient occlusion's byte plane (include/arctic_hip.h: arctic_accumulate_ambient_occlusion_device and
// the text in front of it, which is the definition; nothing here restates it, it only carries it out).  ONE copy of the reprojection, the four taps
// and the blend, compiled for the host (ao_history.cpp: the arbiter arctic_accumulate_pixels) and for the device (ao_history.hip: k_ao_accumulate),
// both with contraction off.  Plain C++ like compose.h; the normalisation (ao_normal) and the acceptance test (ao_accepts) are ray_ao.h's, unchanged.
#pragma once
#include "ray_ao.h"

namespace arctic {

// == ArcticAoHistory (static_assert in ao_history.cpp)
struct AoHistoryDesc { float max_history, normal_cos, plane_dist, min_weight; uint32_t reserved[4]; };

// one entry of the history: what step 7 writes and a later call's tap reads.  All zero: a pixel without geometry or NOT COVERED (count 0: never a tap)
struct AoHistoryEntry { float world[3], value, m[3], count; };

// step 3: where `w` lay in the previous call's frame.  P: that call's proj_view ([col][row], arctic_frame_constants' layout); W, H: the frame's size
// as floats.  false: reject everything.  ix, iy: the first tap's position, in [-1, W-1] x [-1, H-1] (tested in float: a conversion of them is defined)
RQ_HD bool aoh_reproject(const float *P, const float *w, float W, float H, float &ix, float &iy, float &ax, float &ay) {
    float c[4];
    for (int i = 0; i < 4; ++i) c[i] = ((P[i] * w[0] + P[4 + i] * w[1]) + P[8 + i] * w[2]) + P[12 + i];
    if (!(c[3] > 0.0f && rq_finite(c[0]) && rq_finite(c[1]) && rq_finite(c[3]))) return false;
    const float iw = 1.0f / c[3];
    const float nx = c[0] * iw, ny = c[1] * iw;
    const float sx = (nx + 1.0f) * (0.5f * W), sy = (1.0f - ny) * (0.5f * H);
    const float gx = sx - 0.5f, gy = sy - 0.5f;
    ix = __builtin_floorf(gx); iy = __builtin_floorf(gy);
    ax = gx - ix; ay = gy - iy;
    return ix >= -1.0f && ix <= W - 1.0f && iy >= -1.0f && iy <= H - 1.0f;   // (a NaN fails every comparison)
}

// step 7's byte
RQ_HD uint32_t aoh_byte(float value) { return (uint32_t)rq_min(rq_max(__builtin_floorf(value + 0.5f), 0.0f), 255.0f); }

// Steps 1 to 7 for one pixel.  geometry: the pixel has a material; n: its G-buffer normal (not normalised); w: its world position; cur: its current
// byte as a float; P: the previous call's matrix, or null = the history is empty; width x height: the frame.  fetch(qx, qy, e) loads the previous
// call's entry of the pixel at (qx, qy), which lies inside the frame; it is called only for such taps, and what it loads is used only under the
// selects below.  Returns the byte; `out`: the entry to write
template <class Fetch>
RQ_HD uint32_t aoh_pixel(bool geometry, const float *n, const float *w, float cur, const float *P, uint32_t width, uint32_t height, const AoHistoryDesc &d, Fetch fetch,
                         AoHistoryEntry &out) {
    float m[3];
    if (!(ao_normal(n[0], n[1], n[2], m) && geometry)) {
        out = AoHistoryEntry{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
        return 255u;
    }
    float N = 1.0f, value = cur;
    float ix, iy, ax, ay;
    if (P && aoh_reproject(P, w, (float)width, (float)height, ix, iy, ax, ay)) {
        const int32_t x0 = (int32_t)ix, y0 = (int32_t)iy;
        const float bx = 1.0f - ax, by = 1.0f - ay;
        const float weight[4] = {bx * by, ax * by, bx * ay, ax * ay};
        float k[4], kv[4], kc[4];
        for (int t = 0; t < 4; ++t) {
            const int32_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
            bool accepted = false;
            AoHistoryEntry e = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
            if (qx >= 0 && qy >= 0 && qx < (int32_t)width && qy < (int32_t)height) {
                fetch((uint32_t)qx, (uint32_t)qy, e);
                accepted = e.count > 0.0f && ao_accepts(m, w, e.m, e.world, d.normal_cos, d.plane_dist);
            }
            k[t] = accepted ? weight[t] : 0.0f;
            kv[t] = accepted ? weight[t] * e.value : 0.0f;
            kc[t] = accepted ? weight[t] * e.count : 0.0f;
        }
        const float S = ((k[0] + k[1]) + k[2]) + k[3];
        if (S > d.min_weight) {
            const float V = ((kv[0] + kv[1]) + kv[2]) + kv[3], C = ((kc[0] + kc[1]) + kc[2]) + kc[3];
            const float hv = V / S, hn = C / S;
            N = rq_min(hn + 1.0f, d.max_history);
            const float a = 1.0f / N;
            value = hv + (cur - hv) * a;
        }
    }
    out = AoHistoryEntry{{w[0], w[1], w[2]}, value, {m[0], m[1], m[2]}, N};
    return aoh_byte(value);
}

// ---- host side (ao_history.cpp) --------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the block's sake, in the header's order: null = nothing; else the reason
const char *ao_history_refusal(const AoHistoryDesc *d);

#if defined(__HIPCC__)
// ao_history.hip.  What k_ao_accumulate reads and writes: G-buffer planes b, c, e (common.h) of tiles_x x tiles_y tiles of a handle that owns the whole
// frame (width x rows pixels from row 0 of the first tile row); the previous call's history (prev_a = {world3, value}, prev_b = {m3, count}: float4
// per pixel, tile-major like the G-buffer; both null = the history is empty) and the one it writes (next_a, next_b: never the previous ones); the
// row-major byte planes ao_in and ao_out, which may be the same plane; P: the previous call's matrix
struct AoHistoryParams {
    const float *plane_b; const void *plane_c, *plane_e;
    const void *prev_a, *prev_b;
    void *next_a, *next_b;
    const uint8_t *ao_in; uint8_t *ao_out;
    uint32_t tiles_x, tiles_y, width, rows;
    AoHistoryDesc d;
    float P[16];
};
// enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_ao_accumulate(const AoHistoryParams &p, hipStream_t s);
#endif

}  // namespace arctic
