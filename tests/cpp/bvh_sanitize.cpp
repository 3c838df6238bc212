// bvh_sanitize.cpp -- the builder and the host walk of the ray queries (arctic-renderer_amd/csrc/bvh.cpp, ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_ray_query_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/bvh_sanitize.cpp arctic-renderer_amd/csrc/bvh.cpp
// Degenerate inputs -- no triangle, one, all identical, NaN and infinite vertices, coordinates of 1e30, slivers on one line -- each built, validated,
// walked (closest and any hit) and compared with the loop over every triangle, and through arctic_trace_triangles with its refusals.
// Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/ray_query.h"
#include "../../include/arctic_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

using namespace arctic;

static int failures = 0;
static void bad(const std::string &name, const char *why) { std::printf("BAD %s: %s\n", name.c_str(), why); ++failures; }

static std::vector<RayIn> rays_for(std::mt19937 &g, size_t n, float span) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<RayIn> r(n);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) { r[k].o[a] = span * u(g); r[k].d[a] = u(g); }
        r[k].t_min = 0.0f; r[k].t_max = inf;
        switch (k % 16) {
        case 1: r[k].d[0] = 0.0f; break;
        case 2: r[k].d[0] = r[k].d[1] = 0.0f; break;
        case 3: r[k].d[0] = r[k].d[1] = r[k].d[2] = 0.0f; break;
        case 4: r[k].o[1] = nan; break;
        case 5: r[k].d[2] = inf; break;
        case 6: r[k].t_min = -inf; break;
        case 7: r[k].t_max = nan; break;
        case 8: r[k].d[1] = 1e-45f; r[k].o[1] = 0.0f; break;
        case 9: r[k].o[0] = r[k].o[1] = r[k].o[2] = 0.0f; break;
        case 10: r[k].d[0] = 1e30f; r[k].d[1] = -1e30f; break;
        default: break;
        }
    }
    return r;
}

static void run(const std::string &name, const std::vector<float> &tris9, float span) {
    std::mt19937 g(1234);
    const uint64_t n_tris = tris9.size() / 9;
    const std::vector<RayIn> rays = rays_for(g, 257, span);
    Bvh b;
    if (!bvh_build(tris9.data(), n_tris, nullptr, b)) return bad(name, "bvh_build refused");
    if (!bvh_validate(b)) return bad(name, "bvh_validate refused the builder's own tree");
    if (b.tris.size() > n_tris || (b.nodes.empty() != b.tris.empty())) return bad(name, "counts");
    for (int any = 0; any < 2; ++any) {
        std::vector<RayOut> w(rays.size()), f(rays.size()), c(rays.size());
        uint64_t visits[2] = {0, 0};
        bvh_trace_host(b, rays.data(), rays.size(), any != 0, w.data(), visits);
        brute_trace_host(tris9.data(), n_tris, rays.data(), rays.size(), any != 0, f.data());
        if (std::memcmp(w.data(), f.data(), w.size() * sizeof(RayOut)) != 0) return bad(name, "the walk differs from the loop over every triangle");
        if (visits[0] > (uint64_t)rays.size() * b.nodes.size()) return bad(name, "more node visits than nodes");
        for (uint32_t flags : {0u, (uint32_t)ARCTIC_TRACE_BRUTE}) {
            // (the public entry point copies: records that are NOT 16-byte aligned)
            std::vector<char> in(rays.size() * sizeof(ArcticRay) + 4), out(rays.size() * sizeof(ArcticHit) + 4);
            std::memcpy(in.data() + 4, rays.data(), rays.size() * sizeof(ArcticRay));
            const int rc = arctic_trace_triangles(tris9.data(), n_tris, reinterpret_cast<const ArcticRay *>(in.data() + 4), rays.size(), flags | (any ? ARCTIC_TRACE_ANY : 0u),
                                                  reinterpret_cast<ArcticHit *>(out.data() + 4));
            if (rc != ARCTIC_OK) return bad(name, "arctic_trace_triangles failed");
            if (std::memcmp(out.data() + 4, f.data(), f.size() * sizeof(RayOut)) != 0) return bad(name, "arctic_trace_triangles differs");
        }
    }
    std::printf("ok %s: %zu triangles kept, %zu nodes, depth %u\n", name.c_str(), b.tris.size(), b.nodes.size(), b.depth);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::mt19937 g(99);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    auto random_tris = [&](size_t n, float scale) { std::vector<float> t(9 * n); for (float &x : t) x = scale * u(g); return t; };

    run("empty", {}, 1.0f);
    run("one", random_tris(1, 1.0f), 1.0f);
    run("five", random_tris(5, 1.0f), 1.0f);
    run("random-1000", random_tris(1000, 1.0f), 1.0f);
    { std::vector<float> t; const float one[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}; for (int k = 0; k < 1000; ++k) t.insert(t.end(), one, one + 9); run("identical-1000", t, 1.0f); }
    { std::vector<float> t(9 * 300, 0.0f); run("all-zero-300", t, 1.0f); }
    { std::vector<float> t = random_tris(200, 1.0f); for (size_t k = 0; k < t.size(); k += 31) t[k] = (k % 2) ? nan : inf; run("nan-and-inf-vertices", t, 1.0f); }
    { std::vector<float> t(9 * 64, nan); run("all-nan", t, 1.0f); }
    run("huge-1e30", random_tris(500, 1e30f), 1e30f);
    run("huge-3e38", random_tris(100, 3e38f), 3e38f);
    run("tiny-1e-40", random_tris(100, 1e-40f), 1e-40f);
    { std::vector<float> t(9 * 400); for (size_t k = 0; k < t.size(); ++k) t[k] = (k % 3 == 0) ? u(g) : 0.0f; run("slivers-on-a-line", t, 1.0f); }

    // refusals of the entry point
    ArcticRay r = {{0, 0, 0}, 0, {0, 0, 1}, inf};
    ArcticHit h;
    const float tri[9] = {0, 0, 1, 1, 0, 1, 0, 1, 1};
    if (arctic_trace_triangles(nullptr, 1, &r, 1, 0, &h) != ARCTIC_E_INVALID || arctic_trace_triangles(tri, 1, nullptr, 1, 0, &h) != ARCTIC_E_INVALID ||
        arctic_trace_triangles(tri, 1, &r, 1, 0, nullptr) != ARCTIC_E_INVALID || arctic_trace_triangles(tri, 1, &r, 1, 4, &h) != ARCTIC_E_INVALID ||
        arctic_trace_triangles(tri, 0xFFFFFFFFull, &r, 1, 0, &h) != ARCTIC_E_CAPACITY || arctic_trace_triangles(nullptr, 0, nullptr, 0, 0, nullptr) != ARCTIC_OK)
        bad("refusals", "a refusal is missing");
    else std::printf("ok refusals\n");

    // a tree that is NOT the builder's: the validation has to refuse it
    {
        Bvh b;
        const std::vector<float> t = random_tris(40, 1.0f);
        (void)bvh_build(t.data(), 40, nullptr, b);
        int refused = 0, tried = 0;
        { Bvh c = b; c.nodes[0].skip = 0; ++tried; refused += !bvh_validate(c); }
        { Bvh c = b; c.nodes[1].skip = (uint32_t)c.nodes.size() + 1; ++tried; refused += !bvh_validate(c); }
        { Bvh c = b; c.nodes.back().leaf = (uint32_t)(c.tris.size() << 3) | 1u; ++tried; refused += !bvh_validate(c); }
        { Bvh c = b; c.nodes[1].bmin[0] = -9.0f; ++tried; refused += !bvh_validate(c); }
        { Bvh c = b; c.nodes[0].bmax[2] = nan; ++tried; refused += !bvh_validate(c); }
        { Bvh c = b; c.nodes[2].skip = 1; ++tried; refused += !bvh_validate(c); }
        if (refused != tried) bad("validation", "a broken tree passed");
        else std::printf("ok validation\n");
        // ... and the walk ends on a broken tree all the same (the index grows every turn)
        Bvh c = b;
        for (RayNode &n : c.nodes) n.skip = 0;
        std::vector<RayIn> rays = rays_for(g, 16, 1.0f);
        std::vector<RayOut> out(rays.size());
        bvh_trace_host(c, rays.data(), rays.size(), false, out.data(), nullptr);
        std::printf("ok walk-ends-on-a-broken-tree\n");
    }
    return failures ? 1 : 0;
}
