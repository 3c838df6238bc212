// ray_ao.h -- ambient occlusion from the resident G-buffer (include/arctic_hip.h: arctic_trace_ambient_occlusion and the text in front of it, which
// is the definition; nothing here restates it, it only carries it out).  ONE copy of the normalisation, the frame, the ray and the result formula,
// compiled for the host (ray_ao.cpp: the arbiter arctic_ambient_occlusion_points) and for the device (ray_ao.hip: k_trace_ao, k_ao_filter), both
// with contraction off.  Plain C++ like ray_query.h, whose rays and walk it uses unchanged.
#pragma once
#include "ray_query.h"

namespace arctic {

// == ArcticAmbientOcclusion (static_assert in ray_ao.cpp)
struct AoDesc { uint32_t n_rays, pattern; float radius, bias; uint32_t filter; float normal_cos, plane_dist; uint32_t reserved; };
constexpr uint32_t AO_MAX_RAYS = 64;

// step 1: m = n / len.  false: the pixel is NOT COVERED (len zero or not finite, or an m[i] that is not finite)
RQ_HD bool ao_normal(float n0, float n1, float n2, float *m) {
    const float len = __builtin_sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
    m[0] = n0 / len; m[1] = n1 / len; m[2] = n2 / len;
    return len != 0.0f && rq_finite(len) && rq_finite(m[0]) && rq_finite(m[1]) && rq_finite(m[2]);
}
// step 2: the frame from m alone
RQ_HD void ao_frame(const float *m, float *t, float *bt) {
    const float s = __builtin_copysignf(1.0f, m[2]);
    const float a = -1.0f / (s + m[2]);
    const float b = (m[0] * m[1]) * a;
    t[0] = 1.0f + ((s * m[0]) * m[0]) * a; t[1] = s * b; t[2] = (-s) * m[0];
    bt[0] = b; bt[1] = s + (m[1] * m[1]) * a; bt[2] = -m[1];
}
// the origin every ray of a pixel starts from, and step 3: ray k from its local direction l
RQ_HD void ao_origin(const float *world, const float *m, float bias, float *o) {
    for (int i = 0; i < 3; ++i) o[i] = world[i] + bias * m[i];
}
RQ_HD RayIn ao_ray(const float *o, const float *m, const float *t, const float *bt, const float *l, float radius) {
    RayIn r;
    for (int i = 0; i < 3; ++i) { r.o[i] = o[i]; r.d[i] = (t[i] * l[0] + bt[i] * l[1]) + m[i] * l[2]; }
    r.t_min = 0.0f; r.t_max = radius;
    return r;
}
// both results: V = rays that saw nothing, T = rays cast (unfiltered: of the pixel; filtered: of the accepted pixels).  T <= 64 * 16
RQ_HD uint32_t ao_result(uint32_t V, uint32_t T) { return (510u * V + T) / (2u * T); }
// the direction set of the pixel at (x, y) OF THE FRAME
RQ_HD uint32_t ao_set(uint32_t x, uint32_t y, uint32_t P) { return (y % P) * P + x % P; }
// the filter's test of another pixel q of the window against p (both covered, q inside the frame)
RQ_HD bool ao_accepts(const float *mp, const float *wp, const float *mq, const float *wq, float normal_cos, float plane_dist) {
    const float dx = wq[0] - wp[0], dy = wq[1] - wp[1], dz = wq[2] - wp[2];
    return (mp[0] * mq[0] + mp[1] * mq[1]) + mp[2] * mq[2] >= normal_cos && __builtin_fabsf((mp[0] * dx + mp[1] * dy) + mp[2] * dz) <= plane_dist;
}

// ---- host side (ray_ao.cpp) ----------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID, in the header's order: null = nothing; else the reason.  dirs: P * P * n_rays * 3 floats
const char *ao_refusal(const AoDesc *ao, const float *dirs);

#if defined(__HIPCC__)
// ray_ao.hip.  G-buffer planes b, c, e (common.h) of tiles_x x tiles_y tiles; the handle's rows x width pixels start at row row0_in_tile of the first
// tile row and at row frame_row0 of the frame.  d_dirs: the table on the device.  launch_trace_ao writes one byte per pixel, row-major: the hits, or
// (as_result) the unfiltered result.  launch_ao_filter (whole frames only: rows = the frame's height) turns the hits plane into the filtered result
hipError_t launch_trace_ao(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                           uint32_t row0_in_tile, uint32_t frame_row0, const AoDesc &ao, const float *d_dirs, const void *nodes, const void *tris, uint32_t n_nodes,
                           int as_result, uint8_t *out, hipStream_t s);
hipError_t launch_ao_filter(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                            const AoDesc &ao, const uint8_t *hits, uint8_t *out, hipStream_t s);
#endif

}  // namespace arctic
