// motion.h -- per-pixel motion vectors and the accumulation that uses them (include/arctic_hip.h: arctic_motion_vectors_device,
// arctic_accumulate_ambient_occlusion_motion_device and the text in front of them, which is the definition; nothing here restates it, it only
// carries it out).  ONE copy of "where was this surface point in the previous call", of its velocity and of the accumulation's motion form,
// compiled for the host (motion.cpp: the arbiters arctic_motion_pixels and arctic_accumulate_pixels_motion) and for the device (motion.hip:
// k_motion, k_ao_accumulate_motion), both with contraction off.  Plain C++ like ao_history.h; the vertex product is hit_attributes.h's (k_vertex's),
// the projection's operations are aoh_reproject's up to sx, sy (restated: ao_history.h stays what it is), and the accumulation stands on
// aoh_reproject, ao_accepts, ao_normal and aoh_byte, unchanged.
#pragma once
#include "ao_history.h"
#include "hit_attributes.h"
#if defined(__HIPCC__)
#include "common.h"   // (the prepass's records, for MotionParams below)
#endif

namespace arctic {

constexpr uint32_t MOTION_NO_OBJECT = 0xFFFFFFFFu;   // source4's object where a pixel has no geometry
// prev_world4's w: nothing known about the previous call / the previous point alone / the point and its velocity
constexpr float MOTION_NONE = 0.0f, MOTION_POINT = 1.0f, MOTION_VELOCITY = 2.0f;

// What a call uploads per object of the prepass's table (the scene's objects whose mesh exists, in order -- SetupRec::object counts those): the
// PREVIOUS call's trs of the same entry of the scene, where the mesh's vertices lay at that call (`stride` floats apart: 14 in a vertex buffer, 4
// in a snapshot), the mesh's vertex count, the entry's index in the scene's object list, and whether the entry HAS A PREVIOUS at all
struct alignas(16) MotionObject {
    float prev_trs[16];
    const float *prev;
    uint32_t stride, n_vertices, scene_object, has_prev;
    uint32_t pad[2];
};
static_assert(sizeof(MotionObject) == 96, "MotionObject");

// step 4: the three vertices through the previous trs (ha_mat_vec, rows 0..2), then interpolate_attr's order
RQ_HD void mo_prev_world(const float *prev_trs, const float *p0, const float *p1, const float *p2, const float *B, float *pw) {
    float X0[4], X1[4], X2[4];
    ha_mat_vec(prev_trs, p0[0], p0[1], p0[2], 1.0f, X0);
    ha_mat_vec(prev_trs, p1[0], p1[1], p1[2], 1.0f, X1);
    ha_mat_vec(prev_trs, p2[0], p2[1], p2[2], 1.0f, X2);
    for (int j = 0; j < 3; ++j) pw[j] = (B[0] * X0[j] + B[1] * X1[j]) + B[2] * X2[j];
}

// step 5: aoh_reproject's operations up to sx, sy, through the PREVIOUS call's matrix.  false: c3 <= 0 or a c that is not finite -- no velocity
RQ_HD bool mo_velocity(const float *P, const float *pw, float W, float H, float cx, float cy, float *vel) {
    float c[4];
    for (int i = 0; i < 4; ++i) c[i] = ((P[i] * pw[0] + P[4 + i] * pw[1]) + P[8 + i] * pw[2]) + P[12 + i];
    vel[0] = 0.0f; vel[1] = 0.0f;
    if (!(c[3] > 0.0f && rq_finite(c[0]) && rq_finite(c[1]) && rq_finite(c[3]))) return false;
    const float iw = 1.0f / c[3];
    const float nx = c[0] * iw, ny = c[1] * iw;
    const float sx = (nx + 1.0f) * (0.5f * W), sy = (1.0f - ny) * (0.5f * H);
    vel[0] = sx - cx; vel[1] = sy - cy;
    return true;
}

// Steps 3 to 5 for one pixel with geometry.  has_prev: step 3's three conditions hold; prev_trs, p0..p2: the previous trs and the three previous
// object-space positions (read only under has_prev); B: the pixel's barycentrics; P: the previous call's matrix; (px, py): the pixel in the frame
RQ_HD void mo_pixel(bool has_prev, const float *prev_trs, const float *p0, const float *p1, const float *p2, const float *B, const float *P, uint32_t width, uint32_t height,
                    int32_t px, int32_t py, float *pw4, float *vel) {
    pw4[0] = pw4[1] = pw4[2] = 0.0f; pw4[3] = MOTION_NONE;
    vel[0] = vel[1] = 0.0f;
    if (!has_prev) return;
    mo_prev_world(prev_trs, p0, p1, p2, B, pw4);
    pw4[3] = mo_velocity(P, pw4, (float)width, (float)height, (float)px + 0.5f, (float)py + 0.5f, vel) ? MOTION_VELOCITY : MOTION_POINT;
}

// The accumulation's motion form: aoh_pixel (ao_history.h) with two changes -- step 3 reprojects pw4's point and rejects everything unless its flag
// is at least 1; step 4's plane test is taken from that point, in the previous frame.  Everything else, the entry written included, is aoh_pixel's
template <class Fetch>
RQ_HD uint32_t aoh_pixel_motion(bool geometry, const float *n, const float *w, const float *pw4, float cur, const float *P, uint32_t width, uint32_t height, const AoHistoryDesc &d,
                                Fetch fetch, AoHistoryEntry &out) {
    float m[3];
    if (!(ao_normal(n[0], n[1], n[2], m) && geometry)) {
        out = AoHistoryEntry{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f};
        return 255u;
    }
    float N = 1.0f, value = cur;
    float ix, iy, ax, ay;
    if (P && pw4[3] >= MOTION_POINT && aoh_reproject(P, pw4, (float)width, (float)height, ix, iy, ax, ay)) {
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
                accepted = e.count > 0.0f && ao_accepts(m, pw4, e.m, e.world, d.normal_cos, d.plane_dist);
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

#if defined(__HIPCC__)
// motion.hip.  What k_motion reads: the visibility plane and the records of the forward prepass in place (what k_resolve reads), the prepass's own
// object table (for the index buffers) and this call's MotionObject table beside it (n_objs entries).  What it writes: the row-major planes of the
// handle's rows -- prev_world4 always; velocity2, bary3 and source4 where they are not null.  have_prev: M is not empty; P: the previous call's matrix
struct MotionParams {
    const unsigned long long *vis;
    const SetupRec *recs; const RasterRec *rrecs; const uint32_t *rec_of;
    const ObjectRec *objs; const MotionObject *mobjs;
    uint32_t n_objs, n_tiles, width, height, rows, row0_in_tile;
    GeomParams gp;
    float P[16];
    float4 *prev_world4; float2 *velocity2; float *bary3; uint4 *source4;
};
// all three enqueue on `s` and return the launch error, never synchronise
hipError_t launch_motion(const MotionParams &p, hipStream_t s);
// positions of `n` vertices (14 floats apart) -> float4 {x, y, z, 0} each
hipError_t launch_motion_snapshot(const float *vertices, uint32_t n, void *snapshot, hipStream_t s);
// k_ao_accumulate's arguments and the row-major prev_world4 plane of the whole frame
hipError_t launch_ao_accumulate_motion(const AoHistoryParams &p, const void *prev_world4, hipStream_t s);
#endif

}  // namespace arctic
