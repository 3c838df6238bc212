// bvh_refit_sanitize.cpp -- the host side of the refit (arctic-renderer_amd/csrc/bvh.cpp: bvh_refit, refit_schedule and its validation,
// arctic_refit_triangles) under -fsanitize=address,undefined, in a program of its own (tests/test_ray_refit_abi.py builds and runs it; it is never
// loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/bvh_refit_sanitize.cpp arctic-renderer_amd/csrc/bvh.cpp
// A tree built on A is refitted to B and must answer as the loop over every triangle of B: no triangle, one, random moves, every triangle dead,
// coordinates of 1e30, and a B shorter than the tables, which has to be refused.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/ray_query.h"
#include "../../include/arctic_hip.h"

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
    const float inf = std::numeric_limits<float>::infinity();
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) { r[k].o[a] = span * u(g); r[k].d[a] = u(g); }
        r[k].t_min = k % 5 == 0 ? -inf : 0.0f; r[k].t_max = inf;
        if (k % 7 == 1) r[k].d[0] = 0.0f;
        if (k % 7 == 2) r[k].d[1] = r[k].d[2] = 0.0f;
        if (k % 7 == 3) r[k].d[2] = 1e-45f;
    }
    return r;
}

static void run(const std::string &name, const std::vector<float> &a, const std::vector<float> &b, float span) {
    std::mt19937 g(4321);
    const uint64_t n_tris = a.size() / 9;
    const std::vector<RayIn> rays = rays_for(g, 257, span);
    Bvh t;
    if (!bvh_build(a.data(), n_tris, nullptr, t) || !bvh_validate(t)) return bad(name, "the build");
    RefitSchedule s;
    refit_schedule(t, s);
    if (!refit_schedule_validate(t, s)) return bad(name, "the schedule failed its own validation");
    size_t written = 0;
    for (uint32_t k = 0; k < s.head.size(); ++k) written += (s.head[k] >> 8 & 255u) + (k < s.stage_first[1] ? (s.head[k] & 255u) : 0u);
    if (written != t.nodes.size()) return bad(name, "the schedule does not write every node once");
    const Bvh before = t;
    if (!bvh_refit(t, b.data(), n_tris)) return bad(name, "bvh_refit refused");
    for (size_t i = 0; i < t.nodes.size(); ++i) if (t.nodes[i].skip != before.nodes[i].skip || t.nodes[i].leaf != before.nodes[i].leaf) return bad(name, "topology changed");
    for (int any = 0; any < 2; ++any) {
        std::vector<RayOut> w(rays.size()), f(rays.size());
        bvh_trace_host(t, rays.data(), rays.size(), any != 0, w.data(), nullptr);
        brute_trace_host(b.data(), n_tris, rays.data(), rays.size(), any != 0, f.data());
        if (std::memcmp(w.data(), f.data(), w.size() * sizeof(RayOut)) != 0) return bad(name, "the refitted walk differs from the loop over every triangle");
        // the public entry point, with records that are NOT 16-byte aligned and a structure returned
        std::vector<char> in(rays.size() * sizeof(ArcticRay) + 4), out(rays.size() * sizeof(ArcticHit) + 4);
        std::memcpy(in.data() + 4, rays.data(), rays.size() * sizeof(ArcticRay));
        std::vector<ArcticRayNode> nodes(t.nodes.size());
        std::vector<ArcticRayTri> tris(t.tris.size());
        uint64_t counts[2] = {99, 99};
        const int rc = arctic_refit_triangles(a.data(), b.data(), n_tris, reinterpret_cast<const ArcticRay *>(in.data() + 4), rays.size(), any ? ARCTIC_TRACE_ANY : 0u,
                                              reinterpret_cast<ArcticHit *>(out.data() + 4), nodes.data(), nodes.size(), tris.data(), tris.size(), counts);
        if (rc != ARCTIC_OK || counts[0] != t.nodes.size() || counts[1] != t.tris.size()) return bad(name, "arctic_refit_triangles failed");
        if (std::memcmp(out.data() + 4, f.data(), f.size() * sizeof(RayOut)) != 0) return bad(name, "arctic_refit_triangles differs");
        if (!tris.empty() && std::memcmp(tris.data(), t.tris.data(), tris.size() * sizeof(RayTri)) != 0) return bad(name, "the returned slots differ");
    }
    std::printf("ok %s: %zu slots, %zu nodes, %u stages, %zu tasks\n", name.c_str(), t.tris.size(), t.nodes.size(), s.stages(), s.head.size());
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::mt19937 g(77);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    auto random_tris = [&](size_t n, float scale) { std::vector<float> t(9 * n); for (float &x : t) x = scale * u(g); return t; };
    auto moved = [&](std::vector<float> t, float by) { for (float &x : t) x += by * u(g); return t; };

    run("empty", {}, {}, 1.0f);
    { const std::vector<float> a = random_tris(1, 1.0f); run("one", a, moved(a, 0.5f), 1.0f); }
    { const std::vector<float> a = random_tris(5, 1.0f); run("five", a, moved(a, 0.5f), 1.0f); }
    { const std::vector<float> a = random_tris(257, 1.0f); run("moved-257", a, moved(a, 2.0f), 2.0f); }
    { const std::vector<float> a = random_tris(20000, 1.0f); run("moved-20000-three-stages", a, moved(a, 0.1f), 1.0f); }
    { const std::vector<float> a = random_tris(300, 1.0f); std::vector<float> b(a.size(), nan); for (size_t k = 0; k < b.size(); k += 5) b[k] = inf; run("all-dead", a, b, 1.0f); }
    { const std::vector<float> a = random_tris(300, 1.0f); std::vector<float> b = moved(a, 0.3f); for (size_t k = 0; k < b.size(); k += 53) b[k] = (k % 2) ? nan : -inf; run("some-dead", a, b, 1.0f); }
    { const std::vector<float> a = random_tris(500, 1.0f); run("to-1e30", a, random_tris(500, 1e30f), 1e30f); }
    { const std::vector<float> a = random_tris(500, 1e30f); run("from-1e30", a, random_tris(500, 1.0f), 1.0f); }
    { const std::vector<float> a = random_tris(100, 3e38f); run("huge-3e38", a, random_tris(100, 3e38f), 3e38f); }

    // a B shorter than the tables: refused, nothing written
    {
        const std::vector<float> a = random_tris(40, 1.0f), b = random_tris(39, 1.0f);
        Bvh t;
        (void)bvh_build(a.data(), 40, nullptr, t);
        const Bvh before = t;
        const bool refused = !bvh_refit(t, b.data(), 39);
        const bool untouched = std::memcmp(t.tris.data(), before.tris.data(), t.tris.size() * sizeof(RayTri)) == 0 && std::memcmp(t.nodes.data(), before.nodes.data(), t.nodes.size() * sizeof(RayNode)) == 0;
        // ... and a tree whose topology is broken
        Bvh c = before; c.nodes[0].skip = 0;
        Bvh d = before; d.nodes.back().leaf = (uint32_t)(d.tris.size() << 3) | 2u;
        if (!refused || !untouched || bvh_refit(c, a.data(), 40) || bvh_refit(d, a.data(), 40)) bad("shorter-b", "a refit that had to be refused ran");
        else std::printf("ok shorter-b-refused\n");
        // a schedule that is not the tree's: refused
        RefitSchedule s;
        refit_schedule(before, s);
        int tried = 0, caught = 0;
        { RefitSchedule x = s; x.inputs[0] = (uint32_t)before.nodes.size(); ++tried; caught += !refit_schedule_validate(before, x); }
        { RefitSchedule x = s; x.interior[0].node = 1u << 30; ++tried; caught += !refit_schedule_validate(before, x); }
        { RefitSchedule x = s; x.interior[0].link |= 255u; ++tried; caught += !refit_schedule_validate(before, x); }
        { RefitSchedule x = s; x.interior[1].node = x.interior[0].node; ++tried; caught += !refit_schedule_validate(before, x); }
        { RefitSchedule x = s; x.head[0] = (x.head[0] & ~0xFF00u) | ((x.head[0] >> 8 & 255u) - 1) << 8; ++tried; caught += !refit_schedule_validate(before, x); }
        { RefitSchedule x = s; x.interior[0].link += 1u << 16; ++tried; caught += !refit_schedule_validate(before, x); }
        if (caught != tried) bad("schedule-validation", "a broken schedule passed");
        else std::printf("ok schedule-validation\n");
    }

    // refusals of the entry point write nothing
    {
        ArcticRay r = {{0, 0, 0}, 0, {0, 0, 1}, inf};
        ArcticHit h = {77, 77, 77, 77};
        ArcticRayNode node[2]; ArcticRayTri tri[1]; uint64_t counts[2] = {5, 5};
        std::memset(node, 0x5A, sizeof node); std::memset(tri, 0x5A, sizeof tri);
        const float a[18] = {0, 0, 1, 1, 0, 1, 0, 1, 1, 0, 0, 2, 1, 0, 2, 0, 1, 2};
        bool ok = arctic_refit_triangles(nullptr, a, 2, &r, 1, 0, &h, node, 2, tri, 1, counts) == ARCTIC_E_INVALID && arctic_refit_triangles(a, nullptr, 2, &r, 1, 0, &h, node, 2, tri, 1, counts) == ARCTIC_E_INVALID &&
                  arctic_refit_triangles(a, a, 2, nullptr, 1, 0, &h, node, 2, tri, 1, counts) == ARCTIC_E_INVALID && arctic_refit_triangles(a, a, 2, &r, 1, 0, nullptr, node, 2, tri, 1, counts) == ARCTIC_E_INVALID &&
                  arctic_refit_triangles(a, a, 2, &r, 1, 4, &h, node, 2, tri, 1, counts) == ARCTIC_E_INVALID && arctic_refit_triangles(a, a, 0xFFFFFFFFull, &r, 1, 0, &h, node, 2, tri, 1, counts) == ARCTIC_E_CAPACITY &&
                  arctic_refit_triangles(a, a, 2, &r, 1, 0, &h, node, 0, tri, 1, counts) == ARCTIC_E_CAPACITY && arctic_refit_triangles(a, a, 2, &r, 1, 0, &h, node, 2, tri, 1, counts) == ARCTIC_E_CAPACITY;
        unsigned char *p = reinterpret_cast<unsigned char *>(node);
        for (size_t k = 0; k < sizeof node; ++k) ok = ok && p[k] == 0x5A;
        ok = ok && h.t == 77 && counts[0] == 5 && arctic_refit_triangles(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr) == ARCTIC_OK;
        if (!ok) bad("refusals", "a refusal is missing or wrote something");
        else std::printf("ok refusals\n");
    }
    return failures ? 1 : 0;
}
