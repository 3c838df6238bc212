// bloom.h -- bloom (include/arctic_hip.h: arctic_bloom_device and the text in front of it, which is the definition; nothing here restates it, it
// only carries it out).  ONE copy of the prefilter, the two downsamples, the tent and the composite, compiled for the host (bloom.cpp: the
// arbiters arctic_bloom_pyramid and arctic_bloom_pixels) and for the device (bloom.hip), both with contraction off.  Plain C++ like dof.h;
// rq_min and rq_max are ray_query.h's.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticBloom (static_assert in bloom.cpp)
struct BloomDesc { uint32_t flags; float threshold, soft_knee, clamp_max, intensity, spread; uint32_t levels, reserved; };
constexpr uint32_t BLOOM_SOURCE_COMPOSED = 1u, BLOOM_SOURCE_TAA = 2u, BLOOM_SOURCE_MOTION_BLUR = 4u, BLOOM_SOURCE_DOF = 8u;   // ARCTIC_BLOOM_*
constexpr uint32_t BLOOM_MAX_LEVELS = 8;
constexpr uint32_t BLOOM_MAX_SIDE = 16384;

// the integer clamp of an index to 0 .. n - 1 (n >= 1)
RQ_HD uint32_t bloom_clamp(int32_t i, uint32_t n) { return i < 0 ? 0u : ((uint32_t)i > n - 1u ? n - 1u : (uint32_t)i); }
// a level's side from the level above it
RQ_HD uint32_t bloom_half(uint32_t n) { return (n + 1u) / 2u; }

// the pyramid of a width x height frame: w, h and the float offset of levels 1 .. levels (index 0 .. levels - 1), and the two totals
struct BloomLayout {
    uint32_t levels, w[BLOOM_MAX_LEVELS], h[BLOOM_MAX_LEVELS];
    uint64_t offset[BLOOM_MAX_LEVELS], down_floats, up_floats;
};
RQ_HD BloomLayout bloom_layout(uint32_t width, uint32_t height, uint32_t levels) {
    BloomLayout l = {};
    l.levels = levels;
    uint64_t at = 0;
    for (uint32_t k = 0; k < levels && k < BLOOM_MAX_LEVELS; ++k) {
        width = bloom_half(width); height = bloom_half(height);
        l.w[k] = width; l.h[k] = height; l.offset[k] = at;
        if (k + 1 == levels) l.up_floats = at;   // (U_L is D_L: `up` ends in front of it)
        at += (uint64_t)width * height * 3;
    }
    l.down_floats = at;
    return l;
}

// step 1: b[q] of the colour c
RQ_HD void bloom_prefilter(const BloomDesc &d, const float *c, float *b) {
    const float x0 = c[0] > 0.0f ? rq_min(c[0], d.clamp_max) : 0.0f;   // (a NaN fails the test)
    const float x1 = c[1] > 0.0f ? rq_min(c[1], d.clamp_max) : 0.0f;
    const float x2 = c[2] > 0.0f ? rq_min(c[2], d.clamp_max) : 0.0f;
    const float br = rq_max(x0, rq_max(x1, x2));
    const float knee = d.threshold * d.soft_knee;
    float t = br - (d.threshold - knee);
    t = rq_min(rq_max(t, 0.0f), 2.0f * knee);
    const float soft = (t * t) / (4.0f * knee + 1e-5f);
    const float m = rq_max(soft, br - d.threshold);
    const float contrib = rq_min(m / rq_max(br, 1e-5f), 1.0f);
    b[0] = x0 * contrib; b[1] = x1 * contrib; b[2] = x2 * contrib;
}

struct Bloom3 { float r, g, b; };
RQ_HD Bloom3 bloom_add(Bloom3 a, Bloom3 b) { return Bloom3{a.r + b.r, a.g + b.g, a.b + b.b}; }
RQ_HD Bloom3 bloom_mul(Bloom3 a, float s) { return Bloom3{a.r * s, a.g * s, a.b * s}; }

// step 2 at one destination pixel.  texel(i, j, c) loads S~(i, j), i, j = 0 .. 5: the caller clamps (bloom_clamp(2x - 2 + i, Ws), ...) or has
// clamped already.  KARIS: the first level's form
template <bool KARIS, class Texel>
RQ_HD void bloom_down(Texel texel, float *out) {
    const auto at = [&](uint32_t i, uint32_t j) { float c[3]; texel(i, j, c); return Bloom3{c[0], c[1], c[2]}; };
    const auto box = [&](uint32_t a, uint32_t b) { return bloom_mul(bloom_add(bloom_add(at(a, b), at(a + 1, b)), bloom_add(at(a, b + 1), at(a + 1, b + 1))), 0.25f); };
    const auto group = [&](uint32_t a, uint32_t b) { return bloom_mul(bloom_add(bloom_add(box(a, b), box(a + 2, b)), bloom_add(box(a, b + 2), box(a + 2, b + 2))), 0.25f); };
    const Bloom3 g0 = group(1, 1), g1 = group(0, 0), g2 = group(2, 0), g3 = group(0, 2), g4 = group(2, 2);
    if (KARIS) {
        const auto luma = [](Bloom3 g) { return (0.2126f * g.r + 0.7152f * g.g) + 0.0722f * g.b; };
        const float w0 = 0.5f / (1.0f + luma(g0)), w1 = 0.125f / (1.0f + luma(g1)), w2 = 0.125f / (1.0f + luma(g2)), w3 = 0.125f / (1.0f + luma(g3)),
                    w4 = 0.125f / (1.0f + luma(g4));
        const Bloom3 num = bloom_add(bloom_mul(g0, w0), bloom_add(bloom_add(bloom_mul(g1, w1), bloom_mul(g2, w2)), bloom_add(bloom_mul(g3, w3), bloom_mul(g4, w4))));
        const float den = w0 + ((w1 + w2) + (w3 + w4));
        out[0] = num.r / den; out[1] = num.g / den; out[2] = num.b / den;
    } else {
        const Bloom3 o = bloom_add(bloom_mul(g0, 0.5f), bloom_mul(bloom_add(bloom_add(g1, g2), bloom_add(g3, g4)), 0.125f));
        out[0] = o.r; out[1] = o.g; out[2] = o.b;
    }
}

// step 3's base and weights along one axis for destination coordinate x
RQ_HD void bloom_up_axis(uint32_t x, int32_t &base, float *w) {
    const int32_t h = (int32_t)(x >> 1);
    if (x & 1u) { base = h - 1; w[0] = 0.1875f; w[1] = 0.4375f; w[2] = 0.3125f; w[3] = 0.0625f; }
    else { base = h - 2; w[0] = 0.0625f; w[1] = 0.3125f; w[2] = 0.4375f; w[3] = 0.1875f; }
}
// step 3: UP(T, wt, ht) at destination pixel (x, y).  texel(tx, ty, c) loads T at a texel inside wt x ht
template <class Texel>
RQ_HD void bloom_up(uint32_t x, uint32_t y, uint32_t wt, uint32_t ht, Texel texel, float *out) {
    int32_t bx, by;
    float wx[4], wy[4];
    bloom_up_axis(x, bx, wx);
    bloom_up_axis(y, by, wy);
    Bloom3 row[4];
    for (int32_t j = 0; j < 4; ++j) {
        const uint32_t ty = bloom_clamp(by + j, ht);
        Bloom3 t[4];
        for (int32_t i = 0; i < 4; ++i) {
            float c[3];
            texel(bloom_clamp(bx + i, wt), ty, c);
            t[i] = Bloom3{c[0], c[1], c[2]};
        }
        row[j] = bloom_add(bloom_add(bloom_mul(t[0], wx[0]), bloom_mul(t[1], wx[1])), bloom_add(bloom_mul(t[2], wx[2]), bloom_mul(t[3], wx[3])));
    }
    const Bloom3 o = bloom_add(bloom_add(bloom_mul(row[0], wy[0]), bloom_mul(row[1], wy[1])), bloom_add(bloom_mul(row[2], wy[2]), bloom_mul(row[3], wy[3])));
    out[0] = o.r; out[1] = o.g; out[2] = o.b;
}
// ... and U_k = D_k + spread * UP(U_{k+1}) of one pixel: dk is D_k's, up is UP's
RQ_HD void bloom_up_add(const BloomDesc &d, const float *dk, const float *up, float *out) {
    out[0] = dk[0] + d.spread * up[0]; out[1] = dk[1] + d.spread * up[1]; out[2] = dk[2] + d.spread * up[2];
}

// step 4 of one pixel: c is C[p], up is UP(U_1) there
RQ_HD void bloom_composite(const BloomDesc &d, const float *c, const float *up, float *out) {
    for (int k = 0; k < 3; ++k) {
        const float a = d.intensity * up[k];
        out[k] = a > 0.0f ? c[k] + a : c[k];   // a select: a pixel that no bloom reaches keeps its bits
    }
}

// ---- host side (bloom.cpp) ---------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the record's sake, in the header's order: null = nothing; else the reason
const char *bloom_refusal(const BloomDesc *d);

#if defined(__HIPCC__)
// bloom.hip.  The planes of a handle that owns the whole frame (width x rows pixels).  color: row-major float3, or -- color_taa -- the
// anti-aliasing's tile-major float4 history (tiles_x tiles a row).  down, up: the two pyramids as `layout` packs them.  out_hdr (3 floats),
// out_ldr (3 floats) and out_rgba8, row-major.  No plane that is written may alias another
struct BloomParams {
    const void *color; bool color_taa;
    float *down, *up;
    float *out_hdr; uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, width, rows;
    int32_t tm;
    float inv_gamma, exposure;
    BloomDesc d;
    BloomLayout layout;
};
// each enqueues on `s` and returns the launch error, never synchronises.  level: 2 .. L for the downsample (writes D_level), L-1 .. 1 for the tent
// (writes U_level)
hipError_t launch_bloom_down_first(const BloomParams &p, hipStream_t s);
hipError_t launch_bloom_down(const BloomParams &p, uint32_t level, hipStream_t s);
hipError_t launch_bloom_up(const BloomParams &p, uint32_t level, hipStream_t s);
hipError_t launch_bloom_composite(const BloomParams &p, hipStream_t s);
#endif

}  // namespace arctic
