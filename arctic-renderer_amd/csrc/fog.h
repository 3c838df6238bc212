// fog.h -- volumetric fog (include/arctic_hip.h: arctic_fog_device and the text in front of it, which is the definition; nothing here restates
// it, it only carries it out).  ONE copy of the ray, the extinction step, fog_exp2, the march through the sun's map and the phase function,
// compiled for the host (fog.cpp: the arbiter arctic_fog_pixels) and for the device (fog.hip), both with contraction off.  Plain C++ like
// dof.h; rq_min, rq_max, rq_bits and rq_finite are ray_query.h's, dof_view_distance is dof.h's.
#pragma once
#include "ray_query.h"
#include "dof.h"

namespace arctic {

// == ArcticFog, ArcticFogView (static_assert in fog.cpp)
struct FogDesc { uint32_t flags; float density, anisotropy, max_distance; uint32_t steps; float bias; float scatter_color[3], ambient_color[3]; uint32_t reserved; };
struct FogView { float eye[3], z_near, ray00[3], z_far, ray_dx[3], pad0, ray_dy[3], pad1, sun_dir[3], pad2, light[3][4]; };
constexpr uint32_t FOG_SOURCE_COMPOSED = 1u;   // ARCTIC_FOG_SOURCE_COMPOSED
constexpr uint32_t FOG_MAX_STEPS = 128;
constexpr uint32_t FOG_OFFSETS = 16;           // the offset table: 4 x 4 pixels
constexpr uint32_t FOG_BATCH = 8;              // samples whose V_k are found, one after the other, in front of their part of the T chain
constexpr float FOG_LOG2E = 1.442695f;
constexpr float FOG_INV_4PI = 0.07957747f;

// step 2's polynomial: p of f in [0, 1], Horner from the top, a multiply and an add per coefficient
RQ_HD float fog_exp2_poly(float f) {
    float p = 0x1.ca8f0ap-13f;
    p = p * f; p = p + 0x1.44d4d2p-10f;
    p = p * f; p = p + 0x1.3d54d8p-7f;
    p = p * f; p = p + 0x1.c67f5p-5f;
    p = p * f; p = p + 0x1.ebfdf2p-3f;
    p = p * f; p = p + 0x1.62e428p-1f;
    p = p * f; p = p + 0x1p+0f;
    return p;
}
// step 2's 2^x for x <= 0
RQ_HD float fog_exp2(float x) {
    x = x > -126.0f ? x : -126.0f;   // (a NaN fails the test)
    const float n = __builtin_floorf(x);
    const float p = fog_exp2_poly(x - n);
    const uint32_t bits = rq_bits(p) + ((uint32_t)(int32_t)n << 23);
    return rq_min(__builtin_bit_cast(float, bits), 1.0f);
}

RQ_HD float fog_row(const float *row, const float *P) { return ((row[0] * P[0] + row[1] * P[1]) + row[2] * P[2]) + row[3]; }

// step 3's V_k of the sample at view distance z along D: true = lit.  map(tu, tv) loads one texel and is called only for a texel inside the map
template <class Map>
RQ_HD bool fog_visible(const FogView &v, const float *D, float z, float bias, uint32_t S, Map map) {
    if (S == 0u) return true;
    const float P[3] = {v.eye[0] + D[0] * z, v.eye[1] + D[1] * z, v.eye[2] + D[2] * z};
    const float u = fog_row(v.light[0], P), t = fog_row(v.light[1], P), w = fog_row(v.light[2], P);
    const float tu = __builtin_floorf(u * (float)S), tv = __builtin_floorf(t * (float)S), last = (float)(S - 1u);
    if (!(tu >= 0.0f && tu <= last && tv >= 0.0f && tv <= last && !(w > 1.0f))) return true;   // outside (a NaN fails): nothing read
#if defined(ARCTIC_FOG_TABLE_VARIANT) && defined(__HIP_DEVICE_COMPILE__)
    // a measured alternative of DESIGN.md 6x (set by tools/fog_time.py alone): a min/max table of 4 x 4 texel blocks decides the sample first
    bool lit;
    if (map.decided((uint32_t)tu, (uint32_t)tv, w - bias, lit)) return lit;
#endif
    return !(w - bias > map((uint32_t)tu, (uint32_t)tv));
}

// Steps 1 to 4 for pixel (px, py): c = C of the pixel, depth its prepass depth, offset its entry of the table; out: 3 floats; terms2: {T, I} or null
template <class Map>
RQ_HD void fog_pixel(uint32_t px, uint32_t py, const FogDesc &d, const FogView &v, float offset, const float *c, float depth, uint32_t S, Map map, float *out, float *terms2) {
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    float D[3];
    for (int a = 0; a < 3; ++a) D[a] = (v.ray00[a] + fx * v.ray_dx[a]) + fy * v.ray_dy[a];
    const float len = __builtin_sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    const float zv = dof_view_distance(v.z_near, v.z_far, depth);
    const float z_end = rq_min(zv, d.max_distance);
    const float dz = z_end / (float)d.steps;
    const float x = -((d.density * FOG_LOG2E) * len) * dz;
    const float a = fog_exp2(x);
    float T = 1.0f, I = 0.0f;
    // The samples FOG_BATCH at a time: their V_k, which do not depend on T -- each sample tests, loads and compares in turn -- then the batch's part
    // of the T chain, the only loop-carried values
    for (uint32_t k0 = 0; k0 < d.steps; k0 += FOG_BATCH) {
        bool lit[FOG_BATCH];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < FOG_BATCH; ++j) {
            const uint32_t k = k0 + j;
            lit[j] = k < d.steps ? fog_visible(v, D, ((float)k + offset) * dz, d.bias, S, map) : false;
        }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < FOG_BATCH; ++j) {   // the chain, in order of k
            if (k0 + j >= d.steps) break;
            const float Tn = T * a;
            const float term = T - Tn;
            I = lit[j] ? I + term : I;
            T = Tn;
        }
    }
    if (terms2) { terms2[0] = T; terms2[1] = I; }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
    if (!(T < 1.0f)) return;   // zero density, zero length, a NaN: the pixel keeps its bits
    const float g = d.anisotropy;
    const float cos_t = -((D[0] * v.sun_dir[0] + D[1] * v.sun_dir[1]) + D[2] * v.sun_dir[2]) / len;
    const float q = (1.0f + g * g) - (2.0f * g) * cos_t;
    const float ph = ((1.0f - g * g) * FOG_INV_4PI) / (q * __builtin_sqrtf(q));
    const float rest = 1.0f - T;
    for (int ch = 0; ch < 3; ++ch) out[ch] = (c[ch] * T + (d.scatter_color[ch] * ph) * I) + d.ambient_color[ch] * rest;
}

// the table entry of pixel (px, py)
RQ_HD uint32_t fog_offset_index(uint32_t px, uint32_t py) { return (py & 3u) * 4u + (px & 3u); }

// ---- host side (fog.cpp) -----------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID for the records' sake, in the header's order: null = nothing; else the reason
const char *fog_refusal(const FogDesc *d);
const char *fog_view_refusal(const FogView *v);
// ... and for the offset table's (null = every entry 0.5)
const char *fog_offsets_refusal(const float *offsets16);
// arctic_fog_view behind its checks: fwd_cam and fwd_sun are dir_from_rot's fp32 output for the camera's and the sun's rotation; everything else in
// binary64, rounded once.  cam: eye[3], aspect, fov_y (degrees), z_near, z_far; sun_pos[3]
void fog_view_build(const float *fwd_cam, const float *fwd_sun, const float *eye, float aspect, float fov_y, float z_near, float z_far, const float *sun_pos, uint32_t width,
                    uint32_t height, FogView *out);

#if defined(__HIPCC__)
// fog.hip.  The planes of a handle that owns the whole frame (width x rows pixels).  color: row-major float3; depth: one float per pixel,
// row-major, or null (every depth 1.0); map: S x S floats, row-major, or S = 0; offsets: 16 floats on the device.  out_hdr (3 floats), out_ldr
// (3 floats) and out_rgba8, row-major.  No plane that is written may alias another
struct FogParams {
    const float *color, *depth, *map, *offsets;
#if defined(ARCTIC_FOG_TABLE_VARIANT)
    const float2 *blocks; uint32_t nb;   // the variant's table: min/max per 4 x 4 texel block, nb blocks per row; null: none
#endif
    float *out_hdr; uint32_t *out_rgba8; float *out_ldr;
    uint32_t tiles_x, tiles_y, width, rows, S;
    int32_t tm;
    float inv_gamma, exposure;
    FogDesc d;
    FogView v;
};
// enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_fog_march(const FogParams &p, hipStream_t s);
#endif

}  // namespace arctic
