// bvh.cpp -- the host side of the ray queries (include/arctic_hip.h: arctic_trace_rays and the definition in front of it): the scene's
// triangles in world space, the acceleration structure the device walks (ray_query.h: RayNode / RayTri), its validation, and the host arbiter
// arctic_trace_triangles -- the same walk and the same intersection functions as trace.hip, or a loop over every triangle.
// Compiled with contraction off like host_math.cpp: every operation of the definition rounds once.  No HIP call: builds with a host compiler alone.
#include "ray_query.h"
#include "../../include/arctic_hip.h"

#include <algorithm>
#include <cstring>

namespace arctic {

namespace {

struct Ref { float c[3]; uint32_t prim; uint64_t src; };   // centroid of the triangle's box, its number, its index in the input

struct Builder {
    const float *tris9;
    std::vector<Ref> refs;
    Bvh *out;

    static void tri_box(const float *p, float lo[3], float hi[3]) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(std::min(p[a], p[3 + a]), p[6 + a]);
            hi[a] = std::max(std::max(p[a], p[3 + a]), p[6 + a]);
        }
    }
    void build(size_t lo, size_t hi, uint32_t depth) {
        const size_t idx = out->nodes.size();
        out->nodes.push_back(RayNode{});
        out->depth = std::max(out->depth, depth);
        float bmin[3], bmax[3], cmin[3], cmax[3];
        for (int a = 0; a < 3; ++a) { bmin[a] = cmin[a] = rq_inf(); bmax[a] = cmax[a] = -rq_inf(); }
        for (size_t k = lo; k < hi; ++k) {
            float l[3], h[3];
            tri_box(tris9 + 9 * refs[k].src, l, h);
            for (int a = 0; a < 3; ++a) {
                bmin[a] = std::min(bmin[a], l[a]); bmax[a] = std::max(bmax[a], h[a]);
                cmin[a] = std::min(cmin[a], refs[k].c[a]); cmax[a] = std::max(cmax[a], refs[k].c[a]);
            }
        }
        uint32_t leaf = 0;
        if (hi - lo <= RAY_LEAF_MAX) {
            std::sort(refs.begin() + lo, refs.begin() + hi, [](const Ref &x, const Ref &y) { return x.prim < y.prim; });
            leaf = (uint32_t)(out->tris.size() << 3) | (uint32_t)(hi - lo);
            for (size_t k = lo; k < hi; ++k) {
                RayTri t = {};
                const float *p = tris9 + 9 * refs[k].src;
                std::memcpy(t.p0, p, 12); std::memcpy(t.p1, p + 3, 12); std::memcpy(t.p2, p + 6, 12);
                t.prim = refs[k].prim;
                out->tris.push_back(t);
            }
        } else {
            int axis = 0;   // the widest centroid axis, the lowest on a tie (an extent may overflow to +inf: still ordered)
            float widest = cmax[0] - cmin[0];
            for (int a = 1; a < 3; ++a) if (cmax[a] - cmin[a] > widest) { widest = cmax[a] - cmin[a]; axis = a; }
            const size_t mid = lo + (hi - lo) / 2;
            // a strict total order (the numbers are distinct), so the two halves are the same SETS whatever nth_element does inside
            std::nth_element(refs.begin() + lo, refs.begin() + mid, refs.begin() + hi, [axis](const Ref &x, const Ref &y) {
                return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.prim < y.prim);
            });
            build(lo, mid, depth + 1);
            build(mid, hi, depth + 1);
        }
        RayNode &n = out->nodes[idx];
        for (int a = 0; a < 3; ++a) { n.bmin[a] = bmin[a]; n.bmax[a] = bmax[a]; }
        n.skip = (uint32_t)out->nodes.size();
        n.leaf = leaf;
    }
};

inline bool inside(const RayNode &c, const RayNode &p) {
    for (int a = 0; a < 3; ++a) if (!(p.bmin[a] <= c.bmin[a] && c.bmax[a] <= p.bmax[a])) return false;
    return true;
}

}  // namespace

bool bvh_build(const float *tris9, uint64_t n, const uint32_t *prims, Bvh &out) {
    out.nodes.clear(); out.tris.clear(); out.depth = 0;
    Builder b{tris9, {}, &out};
    for (uint64_t k = 0; k < n; ++k) {
        const float *p = tris9 + 9 * k;
        if (!rq_finite9(p)) continue;   // never hit
        float lo[3], hi[3];
        Builder::tri_box(p, lo, hi);
        Ref r;
        for (int a = 0; a < 3; ++a) r.c[a] = 0.5f * lo[a] + 0.5f * hi[a];   // (halves first: the sum of two finite halves is finite)
        r.prim = prims ? prims[k] : (uint32_t)k;
        r.src = k;
        b.refs.push_back(r);
    }
    if (b.refs.size() > RAY_MAX_STORED) return false;
    if (b.refs.empty()) return true;
    out.nodes.reserve(b.refs.size());
    out.tris.reserve(b.refs.size());
    b.build(0, b.refs.size(), 1);   // (the depth of the recursion is at most 1 + log2 of the count: every split halves it)
    return true;
}

bool bvh_validate(const Bvh &b) {
    const uint64_t n = b.nodes.size(), n_tris = b.tris.size();
    if (n > 0xFFFFFFFFull || n_tris > RAY_MAX_STORED) return false;
    for (uint64_t i = 0; i < n; ++i) {
        const RayNode &x = b.nodes[i];
        if (!(i < x.skip && x.skip <= n)) return false;
        for (int a = 0; a < 3; ++a) if (!(x.bmin[a] <= x.bmax[a])) return false;   // (also refuses a NaN)
        const uint64_t count = x.leaf & 7u, first = x.leaf >> 3;
        if (count) {
            if (count > RAY_LEAF_MAX || first + count > n_tris || x.skip != i + 1) return false;
            for (uint64_t k = first; k < first + count; ++k) {
                const RayTri &t = b.tris[k];
                for (int a = 0; a < 3; ++a)
                    for (const float *p : {t.p0, t.p1, t.p2}) if (!(x.bmin[a] <= p[a] && p[a] <= x.bmax[a])) return false;
            }
        } else {
            const uint64_t c0 = i + 1;
            if (c0 >= x.skip) return false;
            const uint64_t c1 = b.nodes[c0].skip;
            if (!(c0 < c1 && c1 < x.skip) || b.nodes[c1].skip != x.skip) return false;
            if (!inside(b.nodes[c0], x) || !inside(b.nodes[c1], x)) return false;
        }
    }
    return true;
}

uint64_t ray_world_triangles(const float *trs, const float *vertices14, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, uint64_t first_prim,
                             std::vector<float> &tris9, std::vector<uint32_t> &prims) {
    for (uint32_t t = 0; t < n_triangles; ++t) {
        const uint32_t i[3] = {indices[3 * t], indices[3 * t + 1], indices[3 * t + 2]};
        if (!(i[0] < n_vertices && i[1] < n_vertices && i[2] < n_vertices)) continue;   // geometry.hip: load_indices
        for (int j = 0; j < 3; ++j) {
            const float *s = vertices14 + (size_t)i[j] * 14;
            for (int k = 0; k < 3; ++k) tris9.push_back(((trs[k] * s[0] + trs[4 + k] * s[1]) + trs[8 + k] * s[2]) + trs[12 + k] * 1.0f);   // geometry.hip: mat_vec
        }
        prims.push_back((uint32_t)(first_prim + t));
    }
    return first_prim + n_triangles;
}

void bvh_trace_host(const Bvh &b, const RayIn *rays, uint64_t n, bool any, RayOut *hits, uint64_t *visits) {
    const uint32_t n_nodes = (uint32_t)b.nodes.size();
    for (uint64_t k = 0; k < n; ++k) {
        const RayPrep r = rq_prepare(rays[k]);
        RayOut h = {0.0f, 0.0f, 0.0f, RAY_NO_PRIM};
        if (r.valid) {
            if (any) h = r.odd ? rq_walk<true, true>(r, b.nodes.data(), b.tris.data(), n_nodes, visits) : rq_walk<true, false>(r, b.nodes.data(), b.tris.data(), n_nodes, visits);
            else h = r.odd ? rq_walk<false, true>(r, b.nodes.data(), b.tris.data(), n_nodes, visits) : rq_walk<false, false>(r, b.nodes.data(), b.tris.data(), n_nodes, visits);
        }
        hits[k] = h;
    }
}

void brute_trace_host(const float *tris9, uint64_t n_tris, const RayIn *rays, uint64_t n, bool any, RayOut *hits) {
    for (uint64_t k = 0; k < n; ++k) {
        const RayPrep r = rq_prepare(rays[k]);
        RayOut best = {0.0f, 0.0f, 0.0f, RAY_NO_PRIM};
        bool found = false;
        for (uint64_t j = 0; r.valid && j < n_tris; ++j) {
            const float *p = tris9 + 9 * j;
            float t, u, v;
            if (!rq_finite9(p) || !rq_triangle(r, p, p + 3, p + 6, t, u, v)) continue;
            if (any) { best.prim = 0u; break; }
            if (!found || t < best.t) { best.t = t; best.u = u; best.v = v; best.prim = (uint32_t)j; found = true; }   // ascending j: a tie keeps the smaller prim
        }
        hits[k] = best;
    }
}

}  // namespace arctic

extern "C" int arctic_trace_triangles(const float *tris9, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits) {
    using namespace arctic;
    static_assert(sizeof(ArcticRay) == sizeof(RayIn) && sizeof(ArcticHit) == sizeof(RayOut), "the public records are the internal ones");
    if ((flags & ~(ARCTIC_TRACE_ANY | ARCTIC_TRACE_BRUTE)) || (n_tris && !tris9) || (n && (!rays || !hits))) return ARCTIC_E_INVALID;
    if (n_tris > 0xFFFFFFFEull) return ARCTIC_E_CAPACITY;
    const bool any = (flags & ARCTIC_TRACE_ANY) != 0;
    // (memcpy in and out: the caller's records need not be 16-byte aligned)
    std::vector<RayIn> in(n);
    std::vector<RayOut> out(n);
    if (n) std::memcpy(static_cast<void *>(in.data()), rays, n * sizeof(RayIn));
    if (flags & ARCTIC_TRACE_BRUTE) brute_trace_host(tris9, n_tris, in.data(), n, any, out.data());
    else {
        Bvh b;
        if (!bvh_build(tris9, n_tris, nullptr, b)) return ARCTIC_E_CAPACITY;
        if (!bvh_validate(b)) return ARCTIC_E_INVALID;
        bvh_trace_host(b, in.data(), n, any, out.data(), nullptr);
    }
    if (n) std::memcpy(static_cast<void *>(hits), out.data(), n * sizeof(RayOut));
    return ARCTIC_OK;
}
