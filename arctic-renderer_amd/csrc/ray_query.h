// ray_query.h -- ray queries against the scene's triangles (include/arctic_hip.h: arctic_trace_rays and the text in front of it, which is the
// definition; nothing here restates it, it only carries it out).  ONE copy of the intersection arithmetic and of the walk, compiled for the host
// (bvh.cpp: the builder, arctic_trace_triangles) and for the device (trace.hip: k_trace, k_trace_sun), both with contraction off.  Plain C++: no
// HIP type appears here, so the builder and the host walk also compile with a host compiler alone (tests/cpp/bvh_sanitize.cpp).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RQ_HD __host__ __device__ __forceinline__
#else
#define RQ_HD inline
#endif

namespace arctic {

// ---- the structure on the device and on the host ------------------------------------------------------------------------------------------
// Nodes in DEPTH-FIRST order with a SKIP LINK: node i's first child is node i + 1, `skip` is the node behind i's subtree (n_nodes behind the last),
// so a walk is  i = descend ? i + 1 : skip  -- the index strictly increases, no stack.  leaf = first << 3 | count: count = 0 an interior node,
// 1..4 a leaf whose triangles are records first .. first + count - 1 (and whose skip is i + 1).  Boxes are exact fp32 unions, no padding.
struct alignas(16) RayNode { float bmin[3]; uint32_t skip; float bmax[3]; uint32_t leaf; };          // 32 bytes: two 16-byte loads
struct alignas(16) RayTri { float p0[3], p1[3], p2[3]; uint32_t prim; uint32_t pad[2]; };             // 48 bytes: three 16-byte loads
static_assert(sizeof(RayNode) == 32 && sizeof(RayTri) == 48, "ray query records");
struct alignas(16) RayIn { float o[3], t_min, d[3], t_max; };                                         // == ArcticRay
struct alignas(16) RayOut { float t, u, v; uint32_t prim; };                                          // == ArcticHit
constexpr uint32_t RAY_NO_PRIM = 0xFFFFFFFFu;
constexpr uint32_t RAY_LEAF_MAX = 4;
constexpr uint64_t RAY_MAX_STORED = (1ull << 29) - 1;   // `first` has 29 bits

// the records are READ as whole 16-byte pieces (one vector load each on the device), whatever part of them a path of the walk uses
typedef float rq_f4 __attribute__((vector_size(16), may_alias));
RQ_HD uint32_t rq_bits(float x) { return __builtin_bit_cast(uint32_t, x); }

constexpr uint32_t RQ_INF_BITS = 0x7F800000u;
RQ_HD float rq_inf() { return __builtin_huge_valf(); }
// min / max as the header defines them: of two equal operands (zeros of either sign included) the FIRST; never applied to a NaN
RQ_HD float rq_min(float a, float b) { return b < a ? b : a; }
RQ_HD float rq_max(float a, float b) { return a < b ? b : a; }
RQ_HD bool rq_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & RQ_INF_BITS) != RQ_INF_BITS; }

// a ray as the walk uses it: the reciprocals are taken once (1.0f / d is the same float wherever it is taken)
struct RayPrep {
    float o0, o1, o2, d0, d1, d2;
    float i0, i1, i2;      // 1.0f / d (unused where d == 0)
    float n0, n1, n2;      // the same for the NODE test, +inf where d == 0 (see rq_node)
    float t_min, t_max;
    bool valid;            // finite origin and direction, direction not zero
    bool odd;              // some d == 0 or some reciprocal not finite: the node test has to watch for 0 * inf
};
RQ_HD RayPrep rq_prepare(const RayIn &r) {
    RayPrep p;
    p.o0 = r.o[0]; p.o1 = r.o[1]; p.o2 = r.o[2]; p.d0 = r.d[0]; p.d1 = r.d[1]; p.d2 = r.d[2];
    p.t_min = r.t_min; p.t_max = r.t_max;
    p.valid = rq_finite(p.o0) && rq_finite(p.o1) && rq_finite(p.o2) && rq_finite(p.d0) && rq_finite(p.d1) && rq_finite(p.d2) &&
              !(p.d0 == 0.0f && p.d1 == 0.0f && p.d2 == 0.0f);
    p.i0 = 1.0f / p.d0; p.i1 = 1.0f / p.d1; p.i2 = 1.0f / p.d2;
    p.n0 = p.d0 == 0.0f ? rq_inf() : p.i0; p.n1 = p.d1 == 0.0f ? rq_inf() : p.i1; p.n2 = p.d2 == 0.0f ? rq_inf() : p.i2;
    p.odd = !(rq_finite(p.n0) && rq_finite(p.n1) && rq_finite(p.n2));
    return p;
}

// one axis of "ray against box", exactly as defined: false = the box is missed on this axis
RQ_HD bool rq_axis(float o, float d, float inv, float bmin, float bmax, float &lo, float &hi) {
    lo = -rq_inf(); hi = rq_inf();
    if (d == 0.0f) return bmin <= o && o <= bmax;
    const float l = (bmin - o) * inv, h = (bmax - o) * inv;
    if (l != l || h != h) return true;   // 0 * inf: a direction component whose reciprocal overflows and an origin in the plane: no constraint
    lo = rq_min(l, h); hi = rq_max(l, h);
    return true;
}
RQ_HD bool rq_box(const RayPrep &r, float bx0, float by0, float bz0, float bx1, float by1, float bz1, float &tn, float &tf) {
    float l0, h0, l1, h1, l2, h2;
    const bool a = rq_axis(r.o0, r.d0, r.i0, bx0, bx1, l0, h0), b = rq_axis(r.o1, r.d1, r.i1, by0, by1, l1, h1), c = rq_axis(r.o2, r.d2, r.i2, bz0, bz1, l2, h2);
    tn = rq_max(rq_max(l0, l1), l2);
    tf = rq_min(rq_min(h0, h1), h2);
    return a && b && c && tn <= tf;
}

// "ray against triangle", exactly as defined (the caller has excluded triangles with a vertex that is not finite)
RQ_HD bool rq_triangle(const RayPrep &r, const float *p0, const float *p1, const float *p2, float &t, float &u, float &v) {
    float tn, tf;
    if (!rq_box(r, rq_min(rq_min(p0[0], p1[0]), p2[0]), rq_min(rq_min(p0[1], p1[1]), p2[1]), rq_min(rq_min(p0[2], p1[2]), p2[2]),
                rq_max(rq_max(p0[0], p1[0]), p2[0]), rq_max(rq_max(p0[1], p1[1]), p2[1]), rq_max(rq_max(p0[2], p1[2]), p2[2]), tn, tf)) return false;
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const float pvx = r.d1 * e2z - r.d2 * e2y, pvy = r.d2 * e2x - r.d0 * e2z, pvz = r.d0 * e2y - r.d1 * e2x;
    const float det = (e1x * pvx + e1y * pvy) + e1z * pvz;
    const float inv = 1.0f / det;
    const float tvx = r.o0 - p0[0], tvy = r.o1 - p0[1], tvz = r.o2 - p0[2];
    u = ((tvx * pvx + tvy * pvy) + tvz * pvz) * inv;
    const float qvx = tvy * e1z - tvz * e1y, qvy = tvz * e1x - tvx * e1z, qvz = tvx * e1y - tvy * e1x;
    v = ((r.d0 * qvx + r.d1 * qvy) + r.d2 * qvz) * inv;
    const float tm = ((e2x * qvx + e2y * qvy) + e2z * qvz) * inv;
    if (!(det != 0.0f && u >= 0.0f && u <= 1.0f && v >= 0.0f && u + v <= 1.0f) || tm != tm) return false;
    t = rq_min(rq_max(tm, tn), tf);
    return r.t_min <= t && t <= r.t_max;
}
RQ_HD bool rq_finite9(const float *p) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && rq_finite(p[k]);
    return ok;
}

// A world vertex, exactly as defined (and as geometry.hip's mat_vec writes attributes 11..13): m holds the matrix's columns `col` floats apart
// (an object's trs: 4; the refit's per-object record, which keeps the 12 floats in use: 3), s = the vertex's position
RQ_HD void rq_world_vertex(const float *m, int col, const float *s, float *out) {
    for (int k = 0; k < 3; ++k) out[k] = ((m[k] * s[0] + m[col + k] * s[1]) + m[2 * col + k] * s[2]) + m[3 * col + k] * 1.0f;
}

// ---- refit (include/arctic_hip.h: "a refitted structure") ------------------------------------------------------------------------------------
// A DEAD slot: nine quiet NaNs.  rq_triangle never reports it, whatever the ray:
//   some d[a] == 0: rq_axis compares bmin <= o && o <= bmax with bmin = bmax = NaN -- false, the box is missed;
//   every d[a] != 0: l and h are NaN on every axis, which rq_axis reads as "no constraint", so the box IS met with (-inf, +inf) -- but then
//     e1 = e2 = NaN, det = NaN, u = NaN, and `det != 0 && u >= 0 && ...` is false because u >= 0 is false for a NaN: a miss.
constexpr uint32_t RQ_DEAD_BITS = 0x7FC00000u;
RQ_HD float rq_dead() { return __builtin_bit_cast(float, RQ_DEAD_BITS); }
// The EMPTY box {+inf, -inf} is the identity of the union below (rq_min(+inf, x) = x, rq_max(-inf, x) = x for every finite x).  Under rq_node it is
// never pruned: lo - o = +inf and hi - o = -inf, times a factor that is never zero (a valid ray has no infinite d) and never NaN, give {+inf, -inf}
// in some order on every axis -- also for d == 0, whose factor is +inf --, so every axis contributes (-inf, +inf).  The walk then descends into a
// subtree that holds dead slots only: time, never a result.
struct RayBox { float lo[3], hi[3]; };
RQ_HD RayBox rq_empty_box() { RayBox b; for (int a = 0; a < 3; ++a) { b.lo[a] = rq_inf(); b.hi[a] = -rq_inf(); } return b; }
RQ_HD void rq_grow(RayBox &b, const RayBox &c) { for (int a = 0; a < 3; ++a) { b.lo[a] = rq_min(b.lo[a], c.lo[a]); b.hi[a] = rq_max(b.hi[a], c.hi[a]); } }
RQ_HD RayBox rq_triangle_box(const float *p) {   // p: nine finite floats
    RayBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = rq_min(rq_min(p[a], p[3 + a]), p[6 + a]); b.hi[a] = rq_max(rq_max(p[a], p[3 + a]), p[6 + a]); }
    return b;
}
// The refit's SCHEDULE: tasks of one wave each, in stages; a stage reads only what earlier stages (earlier launches) wrote.  A task owns up to 64
// INPUT nodes -- stage 0: leaves, whose boxes it forms from their slots; later stages: the roots earlier tasks wrote -- and the up to 63 interior
// nodes that join them under one root.  Inside the task a node is a local number: input l is l, interior k is n_in + k.  Lane l takes input l,
// lane k interior k, in the round of its height (1 + the larger of its children's; inputs have height 0).
constexpr uint32_t REFIT_WAVE = 64;
struct RefitInterior { uint32_t node; uint32_t link; };   // link = local number of child 0 | child 1 << 8 | height << 16
struct RefitSchedule {
    std::vector<uint32_t> head;          // per task: n_in | n_int << 8 | heights << 16
    std::vector<uint32_t> inputs;        // REFIT_WAVE per task (unused entries: 0)
    std::vector<RefitInterior> interior; // REFIT_WAVE per task
    std::vector<uint32_t> stage_first;   // task index where each stage begins, and the task count behind the last
    uint32_t stages() const { return stage_first.empty() ? 0u : (uint32_t)stage_first.size() - 1; }
};
// where a stored slot's vertices come from: the object (the scene's objects order) and the three vertex indices of its mesh
struct RefitSource { uint32_t object, i0, i1, i2; };

// The NODE test.  It only has to be CONSERVATIVE: true whenever the node's box, by the definition, is met with
// max(tn, t_min) <= min(tf, t_max, t_best) -- a needless visit costs time, never a result.  So it may use the hardware's min / max (which differ
// from the defined ones in the sign of a zero only), takes d == 0 as a reciprocal of +inf (a box the origin is outside of then gives an
// interval at +-inf, one it is strictly inside of (-inf, +inf)), and folds the ray's own interval in.  ODD rays (RayPrep::odd) can produce
// 0 * inf = NaN -- origin in a box's plane -- which the definition reads as "no constraint": they take the variant that checks for it.
template <bool ODD>
RQ_HD bool rq_node(const RayPrep &r, const rq_f4 &lo, const rq_f4 &hi, float cap) {
    float l0 = (lo[0] - r.o0) * r.n0, h0 = (hi[0] - r.o0) * r.n0;
    float l1 = (lo[1] - r.o1) * r.n1, h1 = (hi[1] - r.o1) * r.n1;
    float l2 = (lo[2] - r.o2) * r.n2, h2 = (hi[2] - r.o2) * r.n2;
    if (ODD) {
        if (__builtin_isunordered(l0, h0)) { l0 = -rq_inf(); h0 = rq_inf(); }
        if (__builtin_isunordered(l1, h1)) { l1 = -rq_inf(); h1 = rq_inf(); }
        if (__builtin_isunordered(l2, h2)) { l2 = -rq_inf(); h2 = rq_inf(); }
    }
    // (fminf / fmaxf drop a NaN operand: a NaN t_min or t_max constrains nothing here, and the triangle test then refuses every hit)
    const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l0, h0), __builtin_fminf(l1, h1)), __builtin_fmaxf(__builtin_fminf(l2, h2), r.t_min));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l0, h0), __builtin_fmaxf(l1, h1)), __builtin_fminf(__builtin_fmaxf(l2, h2), cap));
    return !(tn > tf);   // strict: a tie must still be found
}

// The walk: closest hit (ANY = false) or any hit.  `visits`, where given, counts {nodes fetched, triangles tested} (host measurements).
// Terminates whatever the arrays hold: the index grows by at least one per turn and a leaf has at most 7 turns.
template <bool ANY, bool ODD>
RQ_HD RayOut rq_walk(const RayPrep &r, const RayNode *nodes, const RayTri *tris, uint32_t n_nodes, uint64_t *visits = nullptr) {
    RayOut best = {0.0f, 0.0f, 0.0f, RAY_NO_PRIM};
    float best_t = rq_inf();
    uint32_t i = 0;
    while (i < n_nodes) {
        const rq_f4 *np = reinterpret_cast<const rq_f4 *>(nodes + i);
        const rq_f4 lo = np[0], hi = np[1];                    // {bmin.xyz, skip} {bmax.xyz, first << 3 | count}
        uint32_t next = rq_bits(lo[3]);
        if (visits) ++visits[0];
        const float cap = ANY ? r.t_max : __builtin_fminf(r.t_max, best_t);
        if (rq_node<ODD>(r, lo, hi, cap)) {
            next = i + 1;
            const uint32_t leaf = rq_bits(hi[3]), count = leaf & 7u, first = leaf >> 3;
            for (uint32_t k = 0; k < count; ++k) {
                const rq_f4 *tp = reinterpret_cast<const rq_f4 *>(tris + first + k);
                const rq_f4 a = tp[0], b = tp[1], c = tp[2];   // {p0.xyz, p1.x} {p1.yz, p2.xy} {p2.z, prim, -, -}
                const float p0[3] = {a[0], a[1], a[2]}, p1[3] = {a[3], b[0], b[1]}, p2[3] = {b[2], b[3], c[0]};
                const uint32_t prim = rq_bits(c[1]);
                float t, u, v;
                if (visits) ++visits[1];
                if (rq_triangle(r, p0, p1, p2, t, u, v)) {
                    if (ANY) { best.prim = 0u; next = n_nodes; }
                    else if (t < best_t || (t == best_t && prim < best.prim)) { best_t = t; best.t = t; best.u = u; best.v = v; best.prim = prim; }
                }
            }
        }
        i = next > i ? next : i + 1;   // (next > i always, in a structure that passed bvh_validate)
    }
    return best;
}

// ---- re-split (include/arctic_hip.h: "a re-split structure") -----------------------------------------------------------------------------------
// The builder halves [lo, hi) at lo + (hi - lo) / 2 and stops at hi - lo <= RAY_LEAF_MAX, so the segment that holds slot position p after `level`
// splits follows from the slot count alone.  A segment that has become a leaf stays as it is at every deeper level.
RQ_HD void rq_segment(uint32_t n, uint32_t level, uint32_t p, uint32_t &lo, uint32_t &hi) {
    lo = 0; hi = n;
    for (uint32_t l = 0; l < level && l < 32u && hi - lo > RAY_LEAF_MAX; ++l) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p < mid) hi = mid; else lo = mid;
    }
}
// levels at which some segment of n slots is still split (0: the root is a leaf); the halves differ by at most one, so the largest decides
RQ_HD uint32_t rq_split_levels(uint32_t n) {
    uint32_t levels = 0;
    for (uint32_t widest = n; widest > RAY_LEAF_MAX; widest = widest - widest / 2) ++levels;
    return levels;
}
// A finite float as a 32-bit key whose unsigned order is the floats' order under <: -0 counts as +0, so equal floats have equal keys.  Every
// finite key lies below RQ_KEY_DEAD, which a dead triangle takes on every axis.  rq_key_float: the float a finite key stands for
constexpr uint32_t RQ_KEY_DEAD = 0xFFFFFFFFu;
RQ_HD uint32_t rq_float_key(float x) {
    const uint32_t b = x == 0.0f ? 0u : __builtin_bit_cast(uint32_t, x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RQ_HD float rq_key_float(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// the axis of a segment whose live centroids span [cmin[a], cmax[a]]: the widest fp32 extent under a strict >, the lowest axis on a tie
RQ_HD int rq_split_axis(const float *cmin, const float *cmax) {
    int axis = 0;
    float widest = cmax[0] - cmin[0];
    for (int a = 1; a < 3; ++a) if (cmax[a] - cmin[a] > widest) { widest = cmax[a] - cmin[a]; axis = a; }
    return axis;
}
// the centroid of a finite triangle: of its box, halves first (the sum of two finite halves is finite)
RQ_HD void rq_centroid(const float *p, float *c) {
    const RayBox b = rq_triangle_box(p);
    for (int a = 0; a < 3; ++a) c[a] = 0.5f * b.lo[a] + 0.5f * b.hi[a];
}

// what a refit uploads per object: the 12 floats of its trs in use (column c at m[3 c]) and the mesh's vertices in use (14 floats per vertex)
struct alignas(16) RefitObject { float m[12]; const float *vertices; uint32_t n_vertices, pad; };
static_assert(sizeof(RefitObject) == 64, "refit object record");
#if defined(__HIPCC__)
// ray_refit.hip.  T: the device copies of a RefitSchedule's tables and of the slots' sources; stage_first: the HOST's array of n_stages + 1 task
// indices.  One launch per stage that has a task, in stream order on s; *launches: how many
struct RefitTablesDev { const uint32_t *head, *inputs; const RefitInterior *interior; const RefitSource *src; };
hipError_t launch_ray_refit(const RefitTablesDev &T, const uint32_t *stage_first, uint32_t n_stages, void *nodes, uint32_t n_nodes, void *tris, uint32_t n_slots,
                            const RefitObject *objs, uint32_t n_objs, hipStream_t s, uint32_t *launches);
// ray_resplit.hip.  The slot order of a fresh build of the pose NOW, written into the slots' prims and into src (the device copy of the build's
// source records), in stream order on s; launch_ray_refit then fills slots and boxes.  ws: ray_resplit_workspace(n_slots) bytes of device memory,
// 256-byte aligned, the handle's for as long as the structure stands.  *launches: the kernels and fills enqueued here, a radix sort counted as one
hipError_t ray_resplit_workspace(uint32_t n_slots, size_t *bytes);
hipError_t launch_ray_resplit(void *ws, size_t ws_bytes, void *tris, uint32_t n_slots, RefitSource *src, const RefitObject *objs, uint32_t n_objs, hipStream_t s,
                              uint32_t *launches);
#endif

// ---- host side (bvh.cpp) ---------------------------------------------------------------------------------------------------------------------
struct Bvh {
    std::vector<RayNode> nodes;
    std::vector<RayTri> tris;     // reordered by leaf; triangles with a vertex that is not finite are left out
    uint32_t depth = 0;           // nodes on the longest path from the root (0: no node)
};
// tris9: n triangles of 9 floats (world space); prims: their numbers, or null = the array index.  Deterministic: median split on the widest centroid
// axis, ties by prim.  false: more than RAY_MAX_STORED triangles to store
bool bvh_build(const float *tris9, uint64_t n, const uint32_t *prims, Bvh &out);
// every node: index < skip <= n_nodes, first + count <= n_tris, a child's box inside its parent's (what the device walk relies on)
bool bvh_validate(const Bvh &b);
// the scene's triangles of one object: p = mat_vec(trs, vertex, 1) exactly as k_vertex writes attr[11..13]; triangles with an index out of range
// are skipped but numbered.  Appends 9 floats + one prim per kept triangle; returns the next prim
uint64_t ray_world_triangles(const float *trs, const float *vertices14, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, uint64_t first_prim,
                             std::vector<float> &tris9, std::vector<uint32_t> &prims);
void bvh_trace_host(const Bvh &b, const RayIn *rays, uint64_t n, bool any, RayOut *hits, uint64_t *visits /* 2, or null */);
void brute_trace_host(const float *tris9, uint64_t n_tris, const RayIn *rays, uint64_t n, bool any, RayOut *hits);
// ray_world_triangles' bookkeeping for a refit: the source of every triangle it kept, in its order
void ray_triangle_sources(uint32_t object, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, std::vector<RefitSource> &out);
// The definition of a refitted structure, on the host, for a tree whose prims are array indices: slot k takes the triangle tris9_now[9 * prim]
// (dead when not finite), leaf boxes the union of their live slots, interior boxes the union of their children, topology untouched.
// false (nothing written): a prim at or above n_now, or a tree that fails the topology part of bvh_validate
bool bvh_refit(Bvh &b, const float *tris9_now, uint64_t n_now);
// The definition of a re-split structure, on the host, for a tree bvh_build made whose prims are array indices: the slots' prims are reordered by
// the builder's own recursion applied to tris9_now (a triangle that is not finite now orders behind every live one on every axis), then bvh_refit.
// false (nothing written): what bvh_refit refuses, or a topology that is not the builder's for this slot count
bool bvh_resplit(Bvh &b, const float *tris9_now, uint64_t n_now);
// the schedule for b's topology and its check: every node written exactly once, every input written in an earlier stage, every number in range
void refit_schedule(const Bvh &b, RefitSchedule &out);
bool refit_schedule_validate(const Bvh &b, const RefitSchedule &s);

}  // namespace arctic
