// bvh.cpp -- the host side of the ray queries (include/arctic_hip.h: arctic_trace_rays and the definition in front of it): the scene's
// triangles in world space, the acceleration structure the device walks (ray_query.h: RayNode / RayTri), its validation, and the host arbiter
// arctic_trace_triangles -- the same walk and the same intersection functions as trace.hip, or a loop over every triangle.
// Compiled with contraction off like host_math.cpp: every operation of the definition rounds once.  No HIP call: builds with a host compiler alone.
#include "ray_query.h"
#include "../../include/arctic_hip.h"

#include <algorithm>
#include <cstddef>
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
            float w[3];
            rq_world_vertex(trs, 4, vertices14 + (size_t)i[j] * 14, w);   // geometry.hip: mat_vec
            tris9.insert(tris9.end(), w, w + 3);
        }
        prims.push_back((uint32_t)(first_prim + t));
    }
    return first_prim + n_triangles;
}

void ray_triangle_sources(uint32_t object, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, std::vector<RefitSource> &out) {
    for (uint32_t t = 0; t < n_triangles; ++t) {
        const uint32_t i[3] = {indices[3 * t], indices[3 * t + 1], indices[3 * t + 2]};
        if (!(i[0] < n_vertices && i[1] < n_vertices && i[2] < n_vertices)) continue;   // (ray_world_triangles' rule)
        out.push_back(RefitSource{object, i[0], i[1], i[2]});
    }
}

namespace {
// the part of bvh_validate that a refit relies on: indices only, no box (a refitted tree has empty boxes and dead slots)
bool topology_ok(const Bvh &b) {
    const uint64_t n = b.nodes.size(), n_tris = b.tris.size();
    if (n > 0xFFFFFFFFull || n_tris > RAY_MAX_STORED) return false;
    for (uint64_t i = 0; i < n; ++i) {
        const RayNode &x = b.nodes[i];
        if (!(i < x.skip && x.skip <= n)) return false;
        const uint64_t count = x.leaf & 7u, first = x.leaf >> 3;
        if (count) {
            if (count > RAY_LEAF_MAX || first + count > n_tris || x.skip != i + 1) return false;
        } else {
            const uint64_t c0 = i + 1;
            if (c0 >= x.skip) return false;
            const uint64_t c1 = b.nodes[c0].skip;
            if (!(c0 < c1 && c1 < x.skip) || b.nodes[c1].skip != x.skip) return false;
        }
    }
    return true;
}
void put_box(RayNode &n, const RayBox &x) { for (int a = 0; a < 3; ++a) { n.bmin[a] = x.lo[a]; n.bmax[a] = x.hi[a]; } }
RayBox get_box(const RayNode &n) { RayBox x; for (int a = 0; a < 3; ++a) { x.lo[a] = n.bmin[a]; x.hi[a] = n.bmax[a]; } return x; }
}  // namespace

bool bvh_refit(Bvh &b, const float *tris9_now, uint64_t n_now) {
    if (!topology_ok(b)) return false;
    for (const RayTri &t : b.tris) if (t.prim >= n_now) return false;
    for (RayTri &t : b.tris) {
        float p[9];
        std::memcpy(p, tris9_now + 9 * (size_t)t.prim, sizeof p);
        if (!rq_finite9(p)) for (float &x : p) x = rq_dead();
        std::memcpy(t.p0, p, 12); std::memcpy(t.p1, p + 3, 12); std::memcpy(t.p2, p + 6, 12);
    }
    for (size_t i = b.nodes.size(); i-- > 0;) {   // depth-first order: a node's children stand behind it
        RayNode &n = b.nodes[i];
        RayBox box = rq_empty_box();
        const uint32_t count = n.leaf & 7u, first = n.leaf >> 3;
        if (count) {
            for (uint32_t k = first; k < first + count; ++k) {
                float p[9];
                std::memcpy(p, b.tris[k].p0, 12); std::memcpy(p + 3, b.tris[k].p1, 12); std::memcpy(p + 6, b.tris[k].p2, 12);
                if (rq_finite9(p)) rq_grow(box, rq_triangle_box(p));
            }
        } else {
            rq_grow(box, get_box(b.nodes[i + 1]));
            rq_grow(box, get_box(b.nodes[b.nodes[i + 1].skip]));
        }
        put_box(n, box);
    }
    return true;
}

namespace {
// is the tree the one Builder::build makes for its slot count?  Node i must cover slots [lo, hi): a leaf of exactly those when hi - lo <= 4, else
// an interior node whose children cover the two halves.  Iterative, and every index is checked (topology_ok has passed)
bool builder_topology(const Bvh &b) {
    struct Item { uint64_t node, lo, hi; };
    if (b.tris.empty()) return b.nodes.empty();
    std::vector<Item> todo{{0, 0, b.tris.size()}};
    uint64_t seen = 0;
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        if (it.node >= b.nodes.size()) return false;
        const RayNode &x = b.nodes[it.node];
        ++seen;
        if (it.hi - it.lo <= RAY_LEAF_MAX) {
            if ((x.leaf & 7u) != it.hi - it.lo || (x.leaf >> 3) != it.lo) return false;
        } else {
            if (x.leaf & 7u) return false;
            const uint64_t mid = it.lo + (it.hi - it.lo) / 2;
            todo.push_back({b.nodes[it.node + 1].skip, mid, it.hi});
            todo.push_back({it.node + 1, it.lo, mid});
        }
    }
    return seen == b.nodes.size();
}

struct SplitRef { float c[3]; uint32_t prim; bool dead; };
}  // namespace

bool bvh_resplit(Bvh &b, const float *tris9_now, uint64_t n_now) {
    if (!topology_ok(b) || !builder_topology(b)) return false;
    for (const RayTri &t : b.tris) if (t.prim >= n_now) return false;
    std::vector<SplitRef> refs(b.tris.size());
    for (size_t k = 0; k < refs.size(); ++k) {
        SplitRef &r = refs[k];
        r.prim = b.tris[k].prim;
        const float *p = tris9_now + 9 * (size_t)r.prim;
        r.dead = !rq_finite9(p);
        if (r.dead) r.c[0] = r.c[1] = r.c[2] = 0.0f; else rq_centroid(p, r.c);
    }
    struct Seg { size_t lo, hi; };
    std::vector<Seg> todo;
    if (!refs.empty()) todo.push_back({0, refs.size()});
    while (!todo.empty()) {
        const Seg s = todo.back();
        todo.pop_back();
        if (s.hi - s.lo <= RAY_LEAF_MAX) {
            std::sort(refs.begin() + s.lo, refs.begin() + s.hi, [](const SplitRef &x, const SplitRef &y) { return x.prim < y.prim; });
            continue;
        }
        float cmin[3] = {0.0f, 0.0f, 0.0f}, cmax[3] = {0.0f, 0.0f, 0.0f};
        bool any = false;
        for (size_t k = s.lo; k < s.hi; ++k) {
            if (refs[k].dead) continue;
            for (int a = 0; a < 3; ++a) {
                cmin[a] = any ? rq_min(cmin[a], refs[k].c[a]) : refs[k].c[a];
                cmax[a] = any ? rq_max(cmax[a], refs[k].c[a]) : refs[k].c[a];
            }
            any = true;
        }
        const int axis = any ? rq_split_axis(cmin, cmax) : 0;
        // the whole segment in the definition's order: live before dead, then the centroid under < (-0 == +0), then the prim
        std::sort(refs.begin() + s.lo, refs.begin() + s.hi, [axis](const SplitRef &x, const SplitRef &y) {
            if (x.dead != y.dead) return y.dead;
            if (!x.dead && x.c[axis] != y.c[axis]) return x.c[axis] < y.c[axis];
            return x.prim < y.prim;
        });
        const size_t mid = s.lo + (s.hi - s.lo) / 2;
        todo.push_back({s.lo, mid});
        todo.push_back({mid, s.hi});
    }
    for (size_t k = 0; k < refs.size(); ++k) b.tris[k].prim = refs[k].prim;
    return bvh_refit(b, tris9_now, n_now);
}

// Stage 0 cuts the depth-first array into the maximal subtrees of at most 64 leaves; every later stage does the same to the tree that is left
// when the roots written so far count as its leaves.  A task's nodes need not be contiguous (they are in stage 0), so they are listed.
void refit_schedule(const Bvh &b, RefitSchedule &out) {
    out = RefitSchedule{};
    const uint32_t n = (uint32_t)b.nodes.size();
    out.stage_first.push_back(0);
    if (n == 0) return;
    std::vector<char> is_input(n, 0);      // a leaf of the tree this stage looks at
    for (uint32_t i = 0; i < n; ++i) is_input[i] = (b.nodes[i].leaf & 7u) != 0;
    std::vector<uint32_t> width(n), local(n), height(n);
    bool stage0 = true;
    for (;;) {
        // inputs below every node of the stage's tree (nodes behind an input's subtree root are never looked at)
        for (uint32_t i = n; i-- > 0;) width[i] = is_input[i] ? 1u : (b.nodes[i].leaf & 7u) ? 0u : width[i + 1] + width[b.nodes[i + 1].skip];
        std::vector<uint32_t> roots;
        for (uint32_t i = 0; i < n;) {
            if (width[i] > REFIT_WAVE) { ++i; continue; }
            roots.push_back(i);
            if (stage0 || !is_input[i]) {   // (an input that stands alone has been written already: no task)
                const size_t base = out.head.size() * REFIT_WAVE;
                out.inputs.resize(base + REFIT_WAVE, 0u);
                out.interior.resize(base + REFIT_WAVE, RefitInterior{0u, 0u});
                uint32_t n_in = 0, n_int = 0, heights = 0;
                std::vector<uint32_t> inner;
                for (uint32_t j = i; j < b.nodes[i].skip;) {
                    if (is_input[j]) { local[j] = n_in; height[j] = 0; out.inputs[base + n_in++] = j; j = b.nodes[j].skip; }
                    else { inner.push_back(j); ++j; }
                }
                for (uint32_t j : inner) local[j] = n_in + n_int++;
                for (size_t k = inner.size(); k-- > 0;) {   // children first
                    const uint32_t j = inner[k], c0 = j + 1, c1 = b.nodes[c0].skip;
                    height[j] = 1 + std::max(height[c0], height[c1]);
                    heights = std::max(heights, height[j]);
                    out.interior[base + (local[j] - n_in)] = RefitInterior{j, local[c0] | local[c1] << 8 | height[j] << 16};
                }
                out.head.push_back(n_in | n_int << 8 | heights << 16);
            }
            i = b.nodes[i].skip;
        }
        out.stage_first.push_back((uint32_t)out.head.size());
        if (roots.size() == 1 && roots[0] == 0) break;
        std::fill(is_input.begin(), is_input.end(), 0);
        for (uint32_t r : roots) is_input[r] = 1;
        stage0 = false;
    }
}

bool refit_schedule_validate(const Bvh &b, const RefitSchedule &s) {
    const uint32_t n = (uint32_t)b.nodes.size();
    if (s.stage_first.empty() || s.stage_first[0] != 0 || s.stage_first.back() != s.head.size()) return false;
    if (s.inputs.size() != s.head.size() * REFIT_WAVE || s.interior.size() != s.inputs.size()) return false;
    if (n == 0) return s.head.empty();
    std::vector<uint32_t> written(n, 0xFFFFFFFFu);   // the stage that writes each node
    for (uint32_t st = 0; st + 1 < s.stage_first.size(); ++st) {
        if (s.stage_first[st] > s.stage_first[st + 1]) return false;
        for (uint32_t t = s.stage_first[st]; t < s.stage_first[st + 1]; ++t) {
            const uint32_t n_in = s.head[t] & 255u, n_int = s.head[t] >> 8 & 255u, heights = s.head[t] >> 16;
            if (n_in == 0 || n_in > REFIT_WAVE || n_int >= REFIT_WAVE || n_int + 1 != n_in || heights >= REFIT_WAVE) return false;
            for (uint32_t l = 0; l < n_in; ++l) {
                const uint32_t j = s.inputs[(size_t)t * REFIT_WAVE + l];
                if (j >= n) return false;
                if (st == 0) { if (!(b.nodes[j].leaf & 7u) || written[j] != 0xFFFFFFFFu) return false; written[j] = 0; }
                else if (written[j] >= st) return false;   // (also: never written)
            }
            // interiors by height, so that a child's height is known before its parent's is checked
            for (uint32_t h = 1; h <= heights; ++h)
                for (uint32_t k = 0; k < n_int; ++k) {
                    const RefitInterior &e = s.interior[(size_t)t * REFIT_WAVE + k];
                    if ((e.link >> 16) != h) continue;
                    const uint32_t a = e.link & 255u, c = e.link >> 8 & 255u;
                    if (e.node >= n || (b.nodes[e.node].leaf & 7u) || written[e.node] != 0xFFFFFFFFu) return false;
                    if (a >= n_in + n_int || c >= n_in + n_int || a == n_in + k || c == n_in + k) return false;
                    // the children named are the node's children, and both are ready in an earlier round
                    const uint32_t c0 = e.node + 1, c1 = b.nodes[c0].skip;
                    const uint32_t node_a = a < n_in ? s.inputs[(size_t)t * REFIT_WAVE + a] : s.interior[(size_t)t * REFIT_WAVE + a - n_in].node;
                    const uint32_t node_c = c < n_in ? s.inputs[(size_t)t * REFIT_WAVE + c] : s.interior[(size_t)t * REFIT_WAVE + c - n_in].node;
                    if (node_a != c0 || node_c != c1) return false;
                    const uint32_t ha = a < n_in ? 0u : s.interior[(size_t)t * REFIT_WAVE + a - n_in].link >> 16;
                    const uint32_t hc = c < n_in ? 0u : s.interior[(size_t)t * REFIT_WAVE + c - n_in].link >> 16;
                    if (ha >= h || hc >= h) return false;
                    written[e.node] = st;
                }
            for (uint32_t k = 0; k < n_int; ++k) {
                const uint32_t h = s.interior[(size_t)t * REFIT_WAVE + k].link >> 16;
                if (h == 0 || h > heights) return false;   // an interior outside every round would never be written
            }
        }
    }
    for (uint32_t i = 0; i < n; ++i) if (written[i] == 0xFFFFFFFFu) return false;
    return true;
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

extern "C" int arctic_refit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                                      ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2) {
    using namespace arctic;
    static_assert(sizeof(ArcticRayNode) == sizeof(RayNode) && sizeof(ArcticRayTri) == sizeof(RayTri), "the public records are the internal ones");
    static_assert(offsetof(ArcticRayNode, skip) == offsetof(RayNode, skip) && offsetof(ArcticRayNode, bmax) == offsetof(RayNode, bmax) && offsetof(ArcticRayNode, leaf) == offsetof(RayNode, leaf), "node layout");
    static_assert(offsetof(ArcticRayTri, p1) == offsetof(RayTri, p1) && offsetof(ArcticRayTri, p2) == offsetof(RayTri, p2) && offsetof(ArcticRayTri, prim) == offsetof(RayTri, prim), "triangle layout");
    if ((flags & ~(ARCTIC_TRACE_ANY | ARCTIC_TRACE_BRUTE)) || (n_tris && (!tris9_build || !tris9_now)) || (n && (!rays || !hits))) return ARCTIC_E_INVALID;
    if (n_tris > 0xFFFFFFFEull) return ARCTIC_E_CAPACITY;
    Bvh b;
    if (!bvh_build(tris9_build, n_tris, nullptr, b)) return ARCTIC_E_CAPACITY;
    if (!bvh_validate(b)) return ARCTIC_E_INVALID;
    // the schedule decides nothing about the result; it is made and checked here so that the host arbiter exercises what the device relies on
    RefitSchedule sched;
    refit_schedule(b, sched);
    if (!refit_schedule_validate(b, sched)) return ARCTIC_E_INVALID;
    if ((nodes && node_cap < b.nodes.size()) || (tris && tri_cap < b.tris.size())) return ARCTIC_E_CAPACITY;
    if (!bvh_refit(b, tris9_now, n_tris)) return ARCTIC_E_INVALID;
    std::vector<RayIn> in(n);
    std::vector<RayOut> out(n);
    if (n) std::memcpy(static_cast<void *>(in.data()), rays, n * sizeof(RayIn));
    if (flags & ARCTIC_TRACE_BRUTE) brute_trace_host(tris9_now, n_tris, in.data(), n, (flags & ARCTIC_TRACE_ANY) != 0, out.data());
    else bvh_trace_host(b, in.data(), n, (flags & ARCTIC_TRACE_ANY) != 0, out.data(), nullptr);
    if (n) std::memcpy(static_cast<void *>(hits), out.data(), n * sizeof(RayOut));
    if (nodes && !b.nodes.empty()) std::memcpy(static_cast<void *>(nodes), b.nodes.data(), b.nodes.size() * sizeof(RayNode));
    if (tris && !b.tris.empty()) std::memcpy(static_cast<void *>(tris), b.tris.data(), b.tris.size() * sizeof(RayTri));
    if (counts2) { counts2[0] = b.nodes.size(); counts2[1] = b.tris.size(); }
    return ARCTIC_OK;
}

extern "C" int arctic_resplit_triangles(const float *tris9_build, const float *tris9_now, uint64_t n_tris, const ArcticRay *rays, uint64_t n, uint32_t flags, ArcticHit *hits,
                                        ArcticRayNode *nodes, uint64_t node_cap, ArcticRayTri *tris, uint64_t tri_cap, uint64_t *counts2) {
    using namespace arctic;
    if ((flags & ~(ARCTIC_TRACE_ANY | ARCTIC_TRACE_BRUTE)) || (n_tris && (!tris9_build || !tris9_now)) || (n && (!rays || !hits))) return ARCTIC_E_INVALID;
    if (n_tris > 0xFFFFFFFEull) return ARCTIC_E_CAPACITY;
    Bvh b;
    if (!bvh_build(tris9_build, n_tris, nullptr, b)) return ARCTIC_E_CAPACITY;
    if (!bvh_validate(b)) return ARCTIC_E_INVALID;
    RefitSchedule sched;   // (as in arctic_refit_triangles: what the device's refit behind the re-split relies on)
    refit_schedule(b, sched);
    if (!refit_schedule_validate(b, sched)) return ARCTIC_E_INVALID;
    if ((nodes && node_cap < b.nodes.size()) || (tris && tri_cap < b.tris.size())) return ARCTIC_E_CAPACITY;
    if (!bvh_resplit(b, tris9_now, n_tris)) return ARCTIC_E_INVALID;
    std::vector<RayIn> in(n);
    std::vector<RayOut> out(n);
    if (n) std::memcpy(static_cast<void *>(in.data()), rays, n * sizeof(RayIn));
    if (flags & ARCTIC_TRACE_BRUTE) brute_trace_host(tris9_now, n_tris, in.data(), n, (flags & ARCTIC_TRACE_ANY) != 0, out.data());
    else bvh_trace_host(b, in.data(), n, (flags & ARCTIC_TRACE_ANY) != 0, out.data(), nullptr);
    if (n) std::memcpy(static_cast<void *>(hits), out.data(), n * sizeof(RayOut));
    if (nodes && !b.nodes.empty()) std::memcpy(static_cast<void *>(nodes), b.nodes.data(), b.nodes.size() * sizeof(RayNode));
    if (tris && !b.tris.empty()) std::memcpy(static_cast<void *>(tris), b.tris.data(), b.tris.size() * sizeof(RayTri));
    if (counts2) { counts2[0] = b.nodes.size(); counts2[1] = b.tris.size(); }
    return ARCTIC_OK;
}

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
