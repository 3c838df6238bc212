// ao_sanitize.cpp -- the host arbiter of the ambient occlusion (arctic-renderer_amd/csrc/ray_ao.cpp, ray_ao.h, on bvh.cpp and ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_ambient_occlusion_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/ao_sanitize.cpp \
//       arctic-renderer_amd/csrc/ray_ao.cpp arctic-renderer_amd/csrc/bvh.cpp
// Empty, degenerate and large inputs -- no triangle, no point, NaN and infinite vertices, coordinates of 1e30, normals that are zero, overflow or
// are not finite, directions with zero components, every n_rays and pattern at its limits -- each through the structure and through the loop over
// every triangle, which have to agree; buffers are sized exactly, so a read or write past an end is caught.  Then the refusals, each of which must
// leave the output untouched.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/ray_ao.h"
#include "../../include/arctic_hip.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
static void bad(const std::string &name, const char *why) { std::printf("BAD %s: %s\n", name.c_str(), why); ++failures; }
static const float p_inf = std::numeric_limits<float>::infinity(), q_nan = std::numeric_limits<float>::quiet_NaN();

static void run(const std::string &name, const std::vector<float> &tris9, size_t n_points, uint32_t n_rays, uint32_t P, float radius, float span) {
    std::mt19937 g(4321);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> points(6 * n_points), dirs((size_t)P * P * n_rays * 3);
    std::vector<uint32_t> sets(n_points);
    for (size_t k = 0; k < n_points; ++k) {
        for (int a = 0; a < 3; ++a) { points[6 * k + a] = span * u(g); points[6 * k + 3 + a] = u(g); }
        sets[k] = (uint32_t)(k % (P * P));
        float *n = &points[6 * k + 3];
        switch (k % 16) {
        case 1: n[0] = n[1] = n[2] = 0.0f; break;
        case 2: n[0] = n[1] = 0.0f; n[2] = -0.0f; break;
        case 3: n[0] = 3e19f; n[1] = 3e19f; break;
        case 4: n[1] = q_nan; break;
        case 5: n[2] = p_inf; break;
        case 6: n[0] = n[1] = 0.0f; n[2] = 1.0f; break;
        case 7: n[0] = n[1] = 0.0f; n[2] = -1.0f; break;
        case 8: n[0] = 1e-30f; n[1] = 1e-30f; n[2] = 1e-30f; break;
        case 9: points[6 * k + 1] = q_nan; break;
        case 10: points[6 * k] = p_inf; break;
        case 11: n[0] = 1.0f; n[1] = 0.0f; n[2] = 0.0f; break;
        default: break;
        }
    }
    for (size_t k = 0; k < dirs.size(); ++k) dirs[k] = u(g);
    for (size_t k = 0; k + 2 < dirs.size(); k += 9) { dirs[k] = 0.0f; dirs[k + 1] = (k % 2) ? 0.0f : 1e-45f; }
    if (dirs.size() >= 6) dirs[3] = dirs[4] = dirs[5] = 0.0f;   // a zero direction: an invalid ray, a miss
    const ArcticAmbientOcclusion ao = {n_rays, P, radius, 1e-3f, 0, 0.0f, 0.0f, 0};
    const uint64_t n_tris = tris9.size() / 9;
    std::vector<uint8_t> walk(n_points), loop(n_points);
    if (arctic_ambient_occlusion_points(tris9.data(), n_tris, points.data(), sets.data(), n_points, &ao, dirs.data(), 0, walk.data()) != ARCTIC_OK ||
        arctic_ambient_occlusion_points(tris9.data(), n_tris, points.data(), sets.data(), n_points, &ao, dirs.data(), ARCTIC_TRACE_BRUTE, loop.data()) != ARCTIC_OK)
        return bad(name, "refused");
    if (walk != loop) return bad(name, "the walk differs from the loop over every triangle");
    size_t most = 0, total = 0;
    for (size_t k = 0; k < n_points; ++k) {
        if (walk[k] > n_rays) return bad(name, "more hits than rays");
        if (k % 16 >= 1 && k % 16 <= 5 && walk[k] != 0) return bad(name, "a point that is not covered has hits");
        most = walk[k] > most ? walk[k] : most; total += walk[k];
    }
    std::printf("ok %s: %zu points, %u rays, pattern %u: %zu hits, at most %zu\n", name.c_str(), n_points, n_rays, P, total, most);
}

int main() {
    std::mt19937 g(99);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    auto random_tris = [&](size_t n, float scale) { std::vector<float> t(9 * n); for (float &x : t) x = scale * u(g); return t; };

    run("empty", {}, 100, 4, 2, p_inf, 1.0f);
    run("no-points", random_tris(10, 1.0f), 0, 4, 2, p_inf, 1.0f);
    run("one-ray", random_tris(1, 1.0f), 64, 1, 1, p_inf, 1.0f);
    run("five", random_tris(5, 1.0f), 200, 5, 2, 0.5f, 1.0f);
    run("random-1000", random_tris(1000, 1.0f), 500, 16, 4, 0.25f, 1.0f);
    run("large-20000", random_tris(20000, 1.0f), 300, 64, 4, p_inf, 1.0f);
    { std::vector<float> t; const float one[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}; for (int k = 0; k < 1000; ++k) t.insert(t.end(), one, one + 9); run("identical-1000", t, 200, 4, 4, p_inf, 1.0f); }
    { std::vector<float> t = random_tris(200, 1.0f); for (size_t k = 0; k < t.size(); k += 31) t[k] = (k % 2) ? q_nan : p_inf; run("nan-and-inf-vertices", t, 200, 4, 2, p_inf, 1.0f); }
    { std::vector<float> t(9 * 64, q_nan); run("all-nan", t, 64, 4, 1, p_inf, 1.0f); }
    run("huge-1e30", random_tris(500, 1e30f), 200, 4, 2, 3e38f, 1e30f);
    run("tiny-1e-40", random_tris(100, 1e-40f), 100, 4, 2, 1e-38f, 1e-40f);

    // refusals: each leaves the output as it was
    const float tri[9] = {0, 0, 1, 1, 0, 1, 0, 1, 1}, point[6] = {0.2f, 0.2f, 0, 0, 0, 1};
    float dirs[16 * 2 * 3];
    for (int k = 0; k < 16 * 2; ++k) { dirs[3 * k] = 0.0f; dirs[3 * k + 1] = 0.0f; dirs[3 * k + 2] = 1.0f; }
    const uint32_t set0 = 0, set4 = 4;
    const ArcticAmbientOcclusion good = {2, 2, 2.0f, 1e-3f, 0, 0.0f, 0.0f, 0};
    uint8_t h = 77;
    int refused = 0, tried = 0;
    auto expect = [&](int rc, int want) { ++tried; refused += rc == want && h == 77; };
    if (arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &good, dirs, 0, &h) != ARCTIC_OK || h != 2) bad("refusals", "the good call");
    h = 77;
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, nullptr, dirs, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &good, nullptr, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(nullptr, 1, point, &set0, 1, &good, dirs, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, nullptr, &set0, 1, &good, dirs, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, point, nullptr, 1, &good, dirs, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &good, dirs, 0, nullptr), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &good, dirs, ARCTIC_TRACE_ANY, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set4, 1, &good, dirs, 0, &h), ARCTIC_E_INVALID);
    expect(arctic_ambient_occlusion_points(tri, 0xFFFFFFFFull, point, &set0, 1, &good, dirs, 0, &h), ARCTIC_E_CAPACITY);
    for (int k = 0; k < 12; ++k) {
        ArcticAmbientOcclusion a = good;
        switch (k) {
        case 0: a.n_rays = 0; break;
        case 1: a.n_rays = 65; break;
        case 2: a.pattern = 3; break;
        case 3: a.pattern = 0; break;
        case 4: a.radius = 0.0f; break;
        case 5: a.radius = q_nan; break;
        case 6: a.bias = p_inf; break;
        case 7: a.filter = 2; break;
        case 8: a.reserved = 1; break;
        case 9: a.filter = 1; a.normal_cos = q_nan; break;
        case 10: a.filter = 1; a.plane_dist = -1.0f; break;
        default: a.filter = 1; a.plane_dist = q_nan; break;
        }
        expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &a, dirs, 0, &h), ARCTIC_E_INVALID);
    }
    dirs[5] = p_inf;
    expect(arctic_ambient_occlusion_points(tri, 1, point, &set0, 1, &good, dirs, 0, &h), ARCTIC_E_INVALID);
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    if (arctic_ambient_occlusion_points(nullptr, 0, nullptr, nullptr, 0, &good, dirs + 6, 0, nullptr) != ARCTIC_OK) bad("nothing-to-do", "refused");
    else std::printf("ok nothing-to-do\n");
    return failures ? 1 : 0;
}
