// gi.h -- one bounce of indirect diffuse light from the resident G-buffer (include/arctic_hip.h: arctic_trace_gi and the text in front of it,
// which is the definition; nothing here restates it, it only carries it out).  ONE copy of the ray of a round, of the sanitised sum and of the
// estimate, compiled for the host (gi.cpp: the arbiters arctic_gi_points and arctic_gi_estimate_pixels) and for the device (gi.hip: k_gi_rays,
// k_gi_add, k_gi_estimate, k_gi_accumulate, k_gi_compose), both with contraction off.  Plain C++ like ray_ao.h, whose normal, frame, origin, ray,
// set and acceptance it uses unchanged, as it does the reprojection of ao_history.h.
#pragma once
#include "ao_history.h"

namespace arctic {

// == ArcticGi (static_assert in gi.cpp)
struct GiDesc { uint32_t n_rays, pattern; float max_distance, bias, clamp_max; uint32_t filter; float normal_cos, plane_dist; uint32_t reserved[4]; };
constexpr uint32_t GI_MAX_RAYS = 16;
// a plane entry of S and of E: {r, g, b, rays}
struct alignas(16) GiSum { float r, g, b, cnt; };

// stage 1: round k's ray of one pixel from its world position, its normal and the local direction l of its set; false (and the all-zero record)
// where the pixel has no geometry or is NOT COVERED by the occlusion's step 1
RQ_HD bool gi_ray(const float *world, const float *n, bool geometry, const float *l, float bias, float max_distance, RayIn &r) {
    float m[3], t[3], bt[3], o[3];
    const bool covered = ao_normal(n[0], n[1], n[2], m) && geometry;
    ao_frame(m, t, bt);
    ao_origin(world, m, bias, o);
    r = ao_ray(o, m, t, bt, l, max_distance);
    if (!covered) r = RayIn{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};   // (a select per word: no branch around the arithmetic)
    return covered;
}
// a pixel HAD A RAY in a round iff its record is not the all-zero one: a ray that was cast carries t_max = max_distance > 0
RQ_HD bool gi_had_ray(float t_max) { return t_max > 0.0f; }
// stage 3: one channel, by selects (a NaN fails both compares)
RQ_HD float gi_sanitise(float l, float clamp_max) { return l > clamp_max ? clamp_max : (l > 0.0f ? l : 0.0f); }
// ... and the sum of a round: round 0 stores, the later rounds add; a pixel without a ray adds nothing
RQ_HD GiSum gi_add(GiSum S, bool first, bool had, float lr, float lg, float lb, float clamp_max) {
    if (first) S = GiSum{0.0f, 0.0f, 0.0f, 0.0f};
    if (!had) return S;
    return GiSum{S.r + gi_sanitise(lr, clamp_max), S.g + gi_sanitise(lg, clamp_max), S.b + gi_sanitise(lb, clamp_max), S.cnt + 1.0f};
}
// stage 4: the mean of a sum (the pixel's own, or the window's)
RQ_HD GiSum gi_estimate(GiSum S) { return S.cnt > 0.0f ? GiSum{S.r / S.cnt, S.g / S.cnt, S.b / S.cnt, S.cnt} : GiSum{0.0f, 0.0f, 0.0f, 0.0f}; }
// the window of the filter: offsets lo .. lo + P - 1 on both axes (the occlusion filter's)
RQ_HD int32_t gi_window_lo(uint32_t P) { return -(int32_t)(P / 2); }

// ---- stage 5: the temporal accumulation of E (the occlusion history's steps with a three-channel value) ------------------------------------------
// == ArcticGiHistory: ArcticAoHistory's fields and refusals (ao_history_refusal)
typedef AoHistoryDesc GiHistoryDesc;
// one entry of the history, three float4 planes: {world, N}, {m, 0}, {acc, 0}.  All zero: a pixel that is not covered (count 0: never a tap)
struct GiHistoryEntry { float world[3], count, m[3], acc[3]; };

// Steps 1 to 7 for one pixel, aoh_pixel's with `value` a colour.  cur: the pixel's E; a pixel whose E.a is 0 is treated as not covered.  fetch(qx,
// qy, e) loads the previous call's entry of a pixel inside the frame.  Returns {acc.rgb, N}; `out`: the entry to write
template <class Fetch>
RQ_HD GiSum gih_pixel(bool geometry, const float *n, const float *w, const GiSum &cur, const float *P, uint32_t width, uint32_t height, const GiHistoryDesc &d, Fetch fetch,
                      GiHistoryEntry &out) {
    float m[3];
    if (!(ao_normal(n[0], n[1], n[2], m) && geometry && cur.cnt > 0.0f)) {
        out = GiHistoryEntry{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
        return GiSum{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const float c[3] = {cur.r, cur.g, cur.b};
    float N = 1.0f, acc[3] = {c[0], c[1], c[2]};
    float ix, iy, ax, ay;
    if (P && aoh_reproject(P, w, (float)width, (float)height, ix, iy, ax, ay)) {
        const int32_t x0 = (int32_t)ix, y0 = (int32_t)iy;
        const float bx = 1.0f - ax, by = 1.0f - ay;
        const float weight[4] = {bx * by, ax * by, bx * ay, ax * ay};
        float k[4], kc[4], kv[3][4];
        for (int t = 0; t < 4; ++t) {
            const int32_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
            bool accepted = false;
            GiHistoryEntry e = {{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
            if (qx >= 0 && qy >= 0 && qx < (int32_t)width && qy < (int32_t)height) {
                fetch((uint32_t)qx, (uint32_t)qy, e);
                accepted = e.count > 0.0f && ao_accepts(m, w, e.m, e.world, d.normal_cos, d.plane_dist);
            }
            k[t] = accepted ? weight[t] : 0.0f;
            kc[t] = accepted ? weight[t] * e.count : 0.0f;
            for (int i = 0; i < 3; ++i) kv[i][t] = accepted ? weight[t] * e.acc[i] : 0.0f;
        }
        const float S = ((k[0] + k[1]) + k[2]) + k[3];
        if (S > d.min_weight) {
            const float C = ((kc[0] + kc[1]) + kc[2]) + kc[3];
            const float hn = C / S;
            N = rq_min(hn + 1.0f, d.max_history);
            const float a = 1.0f / N;
            for (int i = 0; i < 3; ++i) {
                const float V = ((kv[i][0] + kv[i][1]) + kv[i][2]) + kv[i][3];
                const float hv = V / S;
                acc[i] = hv + (c[i] - hv) * a;
            }
        }
    }
    out = GiHistoryEntry{{w[0], w[1], w[2]}, N, {m[0], m[1], m[2]}, {acc[0], acc[1], acc[2]}};
    return GiSum{acc[0], acc[1], acc[2], N};
}

// ---- stage 6: the composition's two terms ---------------------------------------------------------------------------------------------------------
// == ArcticGiCompose (static_assert in gi.cpp)
struct GiComposeDesc { uint32_t flags; float gi_strength, ambient_scale; uint32_t reserved[5]; };
constexpr uint32_t GI_SOURCE_COMPOSED = 1u;   // ARCTIC_GI_SOURCE_COMPOSED
// the ambient correction: compose_occlusion's form with ka = ambient_scale.  ambient_scale = 1: k is +0
RQ_HD void gi_compose_ambient(float *C, const float *base, float ambient, float ambient_scale) {
    const float k = ambient_scale - 1.0f;
    for (int i = 0; i < 3; ++i) C[i] = C[i] + (ambient * base[i]) * k;
}
// is there indirect light to add?  (a select: where this is false nothing of E.rgb is looked at; a NaN E.a is false)
RQ_HD bool gi_compose_lit(float e_a) { return e_a > 0.0f; }
RQ_HD void gi_compose_indirect(float *C, const float *base, float metal, float gi_strength, const float *E) {
    const float s = gi_strength * (1.0f - metal);
    for (int i = 0; i < 3; ++i) C[i] = C[i] + s * (base[i] * E[i]);
}

// ---- host side (gi.cpp) --------------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID, in the header's order: null = nothing; else the reason.  dirs: P * P * n_rays * 3 floats
const char *gi_refusal(const GiDesc *gi, const float *dirs);
const char *gi_compose_refusal(const GiComposeDesc *d);

#if defined(__HIPCC__)
// gi.hip.  G-buffer planes b, c, e (common.h) of tiles_x x tiles_y tiles; the handle's rows x width pixels start at row row0_in_tile of the first
// tile row and at row frame_row0 of the frame.  d_dirs: the table on the device.  Every launcher enqueues on `s` and returns the launch error.
// launch_gi_rays: round k's record of every pixel of the handle's rows, row-major (rows * width records of 32 bytes)
hipError_t launch_gi_rays(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                          uint32_t row0_in_tile, uint32_t frame_row0, const GiDesc &gi, uint32_t round, const float *d_dirs, void *rays, hipStream_t s);
// launch_gi_add: S[p] from round `round`'s records and colours (n of each, 16-byte aligned)
hipError_t launch_gi_add(const void *rays, const void *colors, uint64_t n, float clamp_max, uint32_t round, void *S, hipStream_t s);
// launch_gi_estimate: E from S, both row-major float4 planes of rows * width entries; with gi.filter (whole frames only: rows = the frame's height)
// over the window of the pattern
hipError_t launch_gi_estimate(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                              const GiDesc &gi, const void *S, void *E, hipStream_t s);
// What k_gi_accumulate reads and writes, on a handle that owns the whole frame: the previous call's history (prev[0..2] = {world3, N}, {m3, 0},
// {acc3, 0}: float4 per pixel, tile-major like the G-buffer; prev[0] null = the history is empty) and the one it writes (next[0..2]: never the
// previous ones); the row-major float4 planes gi_in (E) and gi_out ({acc, N}), which may be the same plane; P: the previous call's matrix
struct GiHistoryParams {
    const float *plane_b; const void *plane_c, *plane_e;
    const void *prev[3];
    void *next[3];
    const void *gi_in; void *gi_out;
    uint32_t tiles_x, tiles_y, width, rows;
    GiHistoryDesc d;
    float P[16];
};
hipError_t launch_gi_accumulate(const GiHistoryParams &p, hipStream_t s);
struct TexDesc;
// What k_gi_compose reads and writes: G-buffer planes a, b of the handle's rows, the material table, and the row-major planes of those rows x
// width pixels: hdr (3 floats) and gi (4 floats, 16-byte aligned) in; RGBA8, float LDR and the composed HDR (3 floats each) out
struct GiComposeParams {
    const void *plane_a; const float *plane_b;
    const TexDesc *tex; const float *srgb_lut;
    const float *hdr; const void *gi;
    uint32_t *out_rgba8; float *out_ldr, *out_hdr;
    uint32_t tiles_x, tiles_y, width, rows, row0_in_tile, n_materials;
    int32_t tm;
    float gi_strength, ambient_scale, ambient, inv_gamma, exposure;
};
hipError_t launch_gi_compose(const GiComposeParams &p, hipStream_t s);
#endif

}  // namespace arctic
