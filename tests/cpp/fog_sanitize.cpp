// fog_sanitize.cpp -- the host arbiter of volumetric fog (arctic-renderer_amd/csrc/fog.cpp, fog.h, on dof.h and ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_fog_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/fog_sanitize.cpp \
//       arctic-renderer_amd/csrc/fog.cpp
// Frames of 1x1, 3x5, 13x11 and 64x40, maps of side 0, 1, 16 and 64, 1, 7 and 128 steps, under an ordinary view record and hostile ones: rows
// that send every sample off one side of the map, rows and rays of 3e38 whose products overflow, a view whose rays have length 0.  Every array
// is sized exactly -- the map, the colour, the depth, the outputs -- so a read or write past an end is caught, and a float that leaves the
// range of its integer cast is undefined behaviour the sanitizer reports.  Every pixel of the output must be written, T must lie in [0, 1] or
// be a NaN, I in [0, 1].  Then the refusals, each of which must leave the outputs untouched, and the view record's construction.  Prints one
// "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/fog.h"
#include "../../include/arctic_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
static void bad(const std::string &name, const char *why) { std::printf("BAD %s: %s\n", name.c_str(), why); ++failures; }
static const float p_inf = std::numeric_limits<float>::infinity(), q_nan = std::numeric_limits<float>::quiet_NaN();

static ArcticFog record(uint32_t steps) {
    ArcticFog f = {};
    f.density = 0.12f; f.anisotropy = 0.6f; f.max_distance = 45.0f; f.steps = steps; f.bias = 0.004f;
    for (int c = 0; c < 3; ++c) { f.scatter_color[c] = 3.0f - 0.5f * (float)c; f.ambient_color[c] = 0.05f; }
    return f;
}

static ArcticFogView view(int which) {
    ArcticFogView v = {};
    const float eye[3] = {0.0f, 1.0f, 0.0f}, r00[3] = {-0.5f, 0.4f, 1.0f}, dx[3] = {0.02f, 0.0f, 0.0f}, dy[3] = {0.0f, -0.02f, 0.0f}, sun[3] = {0.0f, -1.0f, 0.0f};
    const float light[3][4] = {{0.05f, 0.0f, 0.0f, 0.5f}, {0.0f, 0.0f, 0.05f, 0.25f}, {0.0f, -0.05f, 0.0f, 0.5f}};
    std::memcpy(v.eye, eye, sizeof eye); std::memcpy(v.ray00, r00, sizeof r00); std::memcpy(v.ray_dx, dx, sizeof dx); std::memcpy(v.ray_dy, dy, sizeof dy);
    std::memcpy(v.sun_dir, sun, sizeof sun); std::memcpy(v.light, light, sizeof light);
    v.z_near = 0.5f; v.z_far = 50.0f;
    if (which == 1) { v.light[0][3] = -3.0f; }                                                  // off the left
    if (which == 2) { v.light[0][3] = 3.0f; v.light[1][3] = 1.0f; }                             // off the right, and v = 1 exactly at the eye
    if (which == 3) { v.light[1][3] = -2.0f; v.light[2][3] = 5.0f; }                            // off the top, beyond depth 1
    if (which == 4) {                                                                            // overflow: products of 3e38, sums of opposite infinities
        for (int a = 0; a < 3; ++a) { v.eye[a] = 1e30f; v.ray00[a] = (a - 1) * 3e30f; v.ray_dx[a] = 1e29f; v.ray_dy[a] = -1e29f; }
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 4; ++a) v.light[k][a] = (a % 2 ? -3e38f : 3e38f);
    }
    if (which == 5) { for (int a = 0; a < 3; ++a) { v.ray00[a] = 0.0f; v.ray_dx[a] = 0.0f; v.ray_dy[a] = 0.0f; } }   // rays of length 0
    if (which == 6) { for (int a = 0; a < 3; ++a) v.light[0][a] = 1e-3f; v.light[0][3] = 0.999999f; v.light[1][3] = 0.999999f; v.light[1][2] = 0.0f; }   // the last texel
    return v;
}

static void run(const std::string &name, uint32_t W, uint32_t H, uint32_t S, uint32_t steps, int which, bool table, bool with_depth) {
    std::mt19937 g(977 + W + S);
    std::uniform_real_distribution<float> u(0.0f, 4.0f), d(0.9f, 1.0f), m(0.2f, 0.8f), o(0.0f, 0.999f);
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n), depth(n), map((size_t)S * S), out(3 * n, -7.0f), terms(2 * n, -7.0f);
    std::vector<int32_t> xy(2 * n);
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) rgb[3 * k + a] = u(g);
        depth[k] = d(g);
        xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W);
    }
    const float odd[6] = {q_nan, p_inf, -p_inf, -2.0f, 1e30f, -0.0f}, odd_depth[5] = {0.0f, 1.0f, 1.5f, q_nan, -p_inf};
    for (size_t k = 0; k < n; k += 3) { rgb[3 * k + k % 3] = odd[(k / 3) % 6]; depth[k] = odd_depth[(k / 3) % 5]; }
    for (float &t : map) t = m(g);
    if (S > 1) { map[1] = q_nan; map[S] = p_inf; map[(size_t)S * S - 1] = 0.0f; }
    float offsets[16];
    for (float &t : offsets) t = o(g);
    const ArcticFog f = record(steps);
    const ArcticFogView v = view(which);
    if (arctic_fog_pixels(&f, &v, table ? offsets : nullptr, n, xy.data(), W, H, rgb.data(), with_depth ? depth.data() : nullptr, S ? map.data() : nullptr, S, out.data(), terms.data()) !=
        ARCTIC_OK)
        return bad(name, "refused");
    size_t fogged = 0;
    for (size_t k = 0; k < n; ++k) {
        const float T = terms[2 * k], I = terms[2 * k + 1];
        if (T == -7.0f || I == -7.0f || out[3 * k] == -7.0f || out[3 * k + 1] == -7.0f || out[3 * k + 2] == -7.0f) return bad(name, "a pixel was not written");
        if (!std::isnan(T) && !(T >= 0.0f && T <= 1.0f)) return bad(name, "T outside [0, 1]");
        if (!(I >= 0.0f && I <= 1.0f + 1e-5f)) return bad(name, "I outside [0, 1]");
        fogged += T < 1.0f;
    }
    std::printf("ok %s: %ux%u, S %u, %u steps, view %d: %zu of %zu pixels fogged\n", name.c_str(), W, H, S, steps, which, fogged, n);
}

static void refusals() {
    const std::string name = "refusals";
    std::vector<float> rgb(3 * 4 * 4, 1.0f), out(3 * 4 * 4, -7.0f), terms(2 * 4 * 4, -7.0f), map(16, 0.5f);
    std::vector<int32_t> xy(2 * 16, 1);
    const ArcticFog good = record(8);
    const ArcticFogView gv = view(0);
    const auto call = [&](const ArcticFog *f, const ArcticFogView *v, const float *offsets) {
        return arctic_fog_pixels(f, v, offsets, 16, xy.data(), 4, 4, rgb.data(), nullptr, map.data(), 4, out.data(), terms.data());
    };
    std::vector<ArcticFog> bads;
    const auto with = [&](auto change) { ArcticFog f = good; change(f); bads.push_back(f); };
    with([](ArcticFog &f) { f.flags = 2u; });
    with([](ArcticFog &f) { f.flags = 0x80000001u; });
    with([](ArcticFog &f) { f.density = -0.1f; });
    with([](ArcticFog &f) { f.density = 64.5f; });
    with([](ArcticFog &f) { f.density = q_nan; });
    with([](ArcticFog &f) { f.anisotropy = 0.96f; });
    with([](ArcticFog &f) { f.anisotropy = -0.96f; });
    with([](ArcticFog &f) { f.anisotropy = q_nan; });
    with([](ArcticFog &f) { f.max_distance = 0.0f; });
    with([](ArcticFog &f) { f.max_distance = 65505.0f; });
    with([](ArcticFog &f) { f.max_distance = q_nan; });
    with([](ArcticFog &f) { f.steps = 0u; });
    with([](ArcticFog &f) { f.steps = 129u; });
    with([](ArcticFog &f) { f.bias = -0.1f; });
    with([](ArcticFog &f) { f.bias = 1.5f; });
    with([](ArcticFog &f) { f.bias = q_nan; });
    with([](ArcticFog &f) { f.scatter_color[1] = -1.0f; });
    with([](ArcticFog &f) { f.scatter_color[2] = p_inf; });
    with([](ArcticFog &f) { f.ambient_color[0] = q_nan; });
    with([](ArcticFog &f) { f.ambient_color[2] = 65505.0f; });
    with([](ArcticFog &f) { f.reserved = 1u; });
    for (const ArcticFog &f : bads)
        if (call(&f, &gv, nullptr) != ARCTIC_E_INVALID) return bad(name, "a bad record was taken");
    std::vector<ArcticFogView> bad_views;
    const auto with_view = [&](auto change) { ArcticFogView v = gv; change(v); bad_views.push_back(v); };
    with_view([](ArcticFogView &v) { v.pad0 = 1.0f; });
    with_view([](ArcticFogView &v) { v.pad1 = -0.0f; });
    with_view([](ArcticFogView &v) { v.pad2 = q_nan; });
    with_view([](ArcticFogView &v) { v.eye[1] = q_nan; });
    with_view([](ArcticFogView &v) { v.ray_dx[0] = p_inf; });
    with_view([](ArcticFogView &v) { v.light[2][3] = -p_inf; });
    with_view([](ArcticFogView &v) { v.sun_dir[2] = q_nan; });
    with_view([](ArcticFogView &v) { v.z_near = 0.0f; });
    with_view([](ArcticFogView &v) { v.z_near = v.z_far; });
    with_view([](ArcticFogView &v) { v.z_far = p_inf; });
    for (const ArcticFogView &v : bad_views)
        if (call(&good, &v, nullptr) != ARCTIC_E_INVALID) return bad(name, "a bad view record was taken");
    float offsets[16];
    const float bad_offsets[4] = {1.0f, -0.01f, q_nan, p_inf};
    for (float b : bad_offsets) {
        for (float &t : offsets) t = 0.25f;
        offsets[11] = b;
        if (call(&good, &gv, offsets) != ARCTIC_E_INVALID) return bad(name, "a bad offset was taken");
    }
    if (call(nullptr, &gv, nullptr) != ARCTIC_E_INVALID || call(&good, nullptr, nullptr) != ARCTIC_E_INVALID) return bad(name, "a null record was taken");
    const auto sized = [&](uint32_t W, uint32_t H, uint32_t S, const float *c, const float *m, float *o, const int32_t *p) {
        return arctic_fog_pixels(&good, &gv, nullptr, 16, p, W, H, c, nullptr, m, S, o, terms.data());
    };
    if (sized(0, 4, 4, rgb.data(), map.data(), out.data(), xy.data()) != ARCTIC_E_INVALID || sized(4, 16385, 4, rgb.data(), map.data(), out.data(), xy.data()) != ARCTIC_E_INVALID ||
        sized(4, 4, 16385, rgb.data(), map.data(), out.data(), xy.data()) != ARCTIC_E_INVALID || sized(4, 4, 4, nullptr, map.data(), out.data(), xy.data()) != ARCTIC_E_INVALID ||
        sized(4, 4, 4, rgb.data(), nullptr, out.data(), xy.data()) != ARCTIC_E_INVALID || sized(4, 4, 4, rgb.data(), map.data(), nullptr, xy.data()) != ARCTIC_E_INVALID ||
        sized(4, 4, 4, rgb.data(), map.data(), out.data(), nullptr) != ARCTIC_E_INVALID)
        return bad(name, "a null array or a bad size was taken");
    std::vector<int32_t> outside(xy);
    outside[31] = 4;
    if (sized(4, 4, 4, rgb.data(), map.data(), out.data(), outside.data()) != ARCTIC_E_INVALID) return bad(name, "a pixel outside the frame was taken");
    outside[31] = 1; outside[0] = -1;
    if (sized(4, 4, 4, rgb.data(), map.data(), out.data(), outside.data()) != ARCTIC_E_INVALID) return bad(name, "a negative pixel was taken");
    for (float t : out) if (t != -7.0f) return bad(name, "a refused call wrote the output");
    for (float t : terms) if (t != -7.0f) return bad(name, "a refused call wrote the terms");
    if (arctic_fog_pixels(&good, &gv, nullptr, 0, nullptr, 4, 4, nullptr, nullptr, nullptr, 0, nullptr, nullptr) != ARCTIC_OK) return bad(name, "n = 0");
    if (arctic_fog_exp2_poly(4, nullptr, out.data()) != ARCTIC_E_INVALID || arctic_fog_exp2_poly(0, nullptr, nullptr) != ARCTIC_OK) return bad(name, "the polynomial");
    std::printf("ok %s: %zu bad records, %zu bad views\n", name.c_str(), bads.size(), bad_views.size());
}

static void exp2_and_view() {
    const std::string name = "exp2-and-view";
    const float xs[10] = {0.0f, -0.0f, -1e-30f, -0.5f, -1.0f, -125.5f, -126.0f, -1e30f, -p_inf, q_nan};
    for (float x : xs) {
        const float a = arctic_fog_exp2(x);
        if (!(a > 0.0f && a <= 1.0f)) return bad(name, "fog_exp2 left (0, 1]");
    }
    if (arctic_fog_exp2(0.0f) != 1.0f || arctic_fog_exp2(-0.0f) != 1.0f || arctic_fog_exp2(-1.0f) != 0.5f) return bad(name, "fog_exp2 of 0 and -1");
    const float fc[3] = {0.6f, -0.3f, 0.74f}, fs[3] = {0.1f, -0.9f, 0.4f}, eye[3] = {1.0f, 2.0f, 3.0f}, sun[3] = {4.0f, 20.0f, -3.0f};
    arctic::FogView v;
    arctic::fog_view_build(fc, fs, eye, 16.0f / 9.0f, 60.0f, 0.1f, 100.0f, sun, 1920, 1080, &v);
    if (arctic::fog_view_refusal(&v)) return bad(name, "an ordinary scene gave a refused record");
    const float straight_up[3] = {0.0f, 1.0f, 0.0f};                              // lookAt degenerates: the record is not finite, and is refused
    arctic::fog_view_build(straight_up, fs, eye, 1.0f, 60.0f, 0.1f, 100.0f, sun, 64, 64, &v);
    if (!arctic::fog_view_refusal(&v)) return bad(name, "a degenerate camera gave an accepted record");
    std::printf("ok %s\n", name.c_str());
}

int main() {
    const uint32_t sizes[4][2] = {{1, 1}, {3, 5}, {13, 11}, {64, 40}}, maps[4] = {0, 1, 16, 64}, steps[3] = {1, 7, 128};
    int k = 0;
    for (const auto &s : sizes)
        for (uint32_t S : maps)
            for (int which = 0; which < 7; ++which, ++k) {
                const std::string f = std::to_string(s[0]) + "x" + std::to_string(s[1]) + "-" + std::to_string(S) + "-" + std::to_string(which);
                run((which ? "hostile-" : "ordinary-") + f, s[0], s[1], S, steps[k % 3], which, k % 2 == 0, k % 4 != 3);
            }
    refusals();
    exp2_and_view();
    return failures ? 1 : 0;
}
