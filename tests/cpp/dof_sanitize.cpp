// dof_sanitize.cpp -- the host arbiters of depth of field (arctic-renderer_amd/csrc/dof.cpp, dof.h, on ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_dof_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/dof_sanitize.cpp \
//       arctic-renderer_amd/csrc/dof.cpp
// Frames of 1x1, 8x8, 17x9, 40x24 and 72x40 with every pixel listed; depths that are ordinary, 0, 1, beyond 1, negative, NaN, infinite or 1e30
// (the float-to-int conversion of a tap position must never see a value outside the frame); NaN colours; taps on the rim of the disc; 1, 16
// and 64 taps -- buffers are sized exactly, so a read or write past an end is caught.  Then planes from elsewhere, then the refusals, each of
// which must leave the outputs untouched.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/dof.h"
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

// Vogel's spiral, or -- rim -- every tap on the unit circle's axes, where x*x + y*y is exactly 1
static std::vector<float> table(uint32_t samples, bool rim) {
    std::vector<float> t(2 * samples);
    for (uint32_t i = 0; i < samples; ++i) {
        const double r = std::sqrt((i + 0.5) / samples), phi = i * 2.399963229728653;
        t[2 * i] = rim ? (i % 2 ? 0.0f : (i % 4 ? -1.0f : 1.0f)) : (float)(r * std::cos(phi));
        t[2 * i + 1] = rim ? (i % 2 ? (i % 4 == 1 ? 1.0f : -1.0f) : 0.0f) : (float)(r * std::sin(phi));
    }
    return t;
}

// kind: 0 ordinary, 1 the planes and beyond, 2 NaN, 3 infinite, 4 1e30
static void run(const std::string &name, uint32_t W, uint32_t H, int kind, bool rim, float max_radius, uint32_t samples) {
    std::mt19937 g(1234);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const size_t n = (size_t)W * H, tiles = (size_t)((W + 7) / 8) * ((H + 7) / 8);
    std::vector<float> rgb(3 * n), z(n), tile(tiles, -7.0f), near(tiles, -7.0f), P(2 * n, -7.0f), out(3 * n, -7.0f);
    std::vector<int32_t> xy(2 * n);
    const float edge[6] = {0.0f, 1.0f, 1.5f, -2.0f, 0.999999f, 1.0000001f};
    for (size_t k = 0; k < n; ++k) {
        xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W);
        for (int a = 0; a < 3; ++a) rgb[3 * k + a] = 4.0f * u(g);
        if (k % 11 == 5) rgb[3 * k + 1] = q_nan;
        float d = 0.9f + 0.1f * u(g);
        if (kind == 1) d = edge[k % 6];
        if (kind == 2 && k % 3 == 0) d = q_nan;
        if (kind == 3 && k % 3 == 0) d = k % 2 ? p_inf : -p_inf;
        if (kind == 4 && k % 3 == 0) d = k % 2 ? 1e30f : -1e30f;
        z[k] = d;
    }
    const std::vector<float> taps = table(samples, rim);
    const ArcticDof dof = {0, 5.0f, 24.0f, max_radius, samples, 0.5f, 0.1f, 1000.0f};
    if (arctic_dof_prepare(&dof, W, H, z.data(), tile.data(), near.data(), P.data()) != ARCTIC_OK) return bad(name, "prepare refused");
    for (size_t k = 0; k < n; ++k)
        if (!(std::fabs(P[2 * k]) <= max_radius) || std::isnan(P[2 * k + 1])) return bad(name, "s outside [-max_radius, max_radius], or zv a NaN");
    for (size_t k = 0; k < tiles; ++k)
        if (!(tile[k] >= 0.0f && tile[k] <= max_radius && near[k] >= tile[k] && near[k] <= max_radius)) return bad(name, "a maximum outside [0, max_radius], or below its tile's");
    if (arctic_dof_pixels(&dof, taps.data(), n, xy.data(), W, H, rgb.data(), P.data(), near.data(), out.data()) != ARCTIC_OK) return bad(name, "pixels refused");
    size_t finite = 0;
    for (size_t k = 0; k < n; ++k) {
        if (out[3 * k] == -7.0f && out[3 * k + 2] == -7.0f) return bad(name, "a pixel was not written");
        finite += std::isfinite(out[3 * k]) && std::isfinite(out[3 * k + 1]) && std::isfinite(out[3 * k + 2]);
    }
    std::printf("ok %s: %ux%u, max_radius %g, %u taps: %zu of %zu pixels finite\n", name.c_str(), W, H, max_radius, samples, finite, n);
}

int main() {
    const uint32_t sizes[5][2] = {{1, 1}, {8, 8}, {17, 9}, {40, 24}, {72, 40}};
    for (const auto &s : sizes) {
        const std::string f = "-" + std::to_string(s[0]) + "x" + std::to_string(s[1]);
        run("ordinary" + f, s[0], s[1], 0, false, 16.0f, 16);
        run("rim" + f, s[0], s[1], 0, true, 64.0f, 16);
        run("one-tap" + f, s[0], s[1], 0, false, 16.0f, 1);
        run("64-taps" + f, s[0], s[1], 0, false, 64.0f, 64);
        run("planes" + f, s[0], s[1], 1, true, 6.5f, 16);
        run("nan" + f, s[0], s[1], 2, false, 16.0f, 16);
        run("inf" + f, s[0], s[1], 3, true, 16.0f, 16);
        run("1e30" + f, s[0], s[1], 4, false, 16.0f, 16);
    }

    // planes from elsewhere: a P whose s or zv is 0, NaN, negative, infinite or huge and a neighbour_max that is NaN, infinite, negative or 1e30
    // -- no tap may leave the frame
    {
        const uint32_t W = 17, H = 9;
        const size_t n = (size_t)W * H, tiles = 3 * 2;
        std::vector<float> rgb(3 * n, 1.0f), P(2 * n), near(tiles), out(3 * n, -7.0f);
        std::vector<int32_t> xy(2 * n);
        const float odd[6] = {0.0f, q_nan, 1e30f, -1.0f, p_inf, 0.5f};
        for (size_t k = 0; k < n; ++k) { xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W); P[2 * k] = odd[k % 6]; P[2 * k + 1] = odd[(k + 1) % 6]; }
        const float radii[6] = {q_nan, p_inf, 1e30f, -p_inf, 3e9f, -5e9f};
        for (size_t k = 0; k < tiles; ++k) near[k] = radii[k];
        const std::vector<float> taps = table(9, true);
        const ArcticDof dof = {0, 5.0f, 24.0f, 16.0f, 9, 0.5f, 0.1f, 1000.0f};
        if (arctic_dof_pixels(&dof, taps.data(), n, xy.data(), W, H, rgb.data(), P.data(), near.data(), out.data()) != ARCTIC_OK) bad("odd-planes", "refused");
        else std::printf("ok odd-planes\n");
    }

    // the thin lens: 50 mm at f/2 focused at 2 m on a 24 mm sensor, 1080 rows: c = 0.0025 / (2 * 1.95), radius = 0.5 c / 0.024 * 1080 = 14.42 pixels
    {
        float scale = 77.0f;
        if (arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, 2.0f, 1080, &scale) != ARCTIC_OK || !(std::fabs(scale - 14.4231f) < 1e-3f)) bad("thin-lens", "the worked figure");
        else std::printf("ok thin-lens: %.4f pixels\n", scale);
    }

    // refusals: each leaves the outputs as they were
    const float rgb[3] = {1, 2, 3}, z[1] = {0.5f}, P[2] = {2, 0.5f}, near[1] = {2}, taps[4] = {0, 0, 0.5f, 0.5f};
    const int32_t xy[2] = {0, 0}, outside[2] = {1, 0}, negative[2] = {0, -1};
    const ArcticDof good = {1, 5.0f, 8.0f, 16.0f, 2, 0.5f, 0.1f, 1000.0f};
    float out[3] = {77, 77, 77}, t1[1] = {77}, n1[1] = {77}, p2[2] = {77, 77}, scale = 77;
    int refused = 0, tried = 0;
    auto untouched = [&] { return out[0] == 77 && out[1] == 77 && out[2] == 77 && t1[0] == 77 && n1[0] == 77 && p2[0] == 77 && p2[1] == 77 && scale == 77; };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_dof_prepare(&good, 1, 1, z, t1, n1, p2) != ARCTIC_OK || t1[0] == 77 || n1[0] != t1[0] || p2[0] == 77 || p2[1] == 77) bad("refusals", "the good prepare");
    if (arctic_dof_pixels(&good, taps, 1, xy, 1, 1, rgb, P, near, out) != ARCTIC_OK || out[0] == 77) bad("refusals", "the good call");
    out[0] = out[1] = out[2] = t1[0] = n1[0] = p2[0] = p2[1] = 77;
    if (arctic_dof_pixels(&good, taps, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr) != ARCTIC_OK) bad("refusals", "no pixel");
    expect(arctic_dof_pixels(nullptr, taps, 1, xy, 1, 1, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, nullptr, 1, xy, 1, 1, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, nullptr, 1, 1, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 1, 1, nullptr, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 1, 1, rgb, nullptr, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 1, 1, rgb, P, nullptr, out));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 1, 1, rgb, P, near, nullptr));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 0, 1, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, xy, 1, 16385, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, outside, 1, 1, rgb, P, near, out));
    expect(arctic_dof_pixels(&good, taps, 1, negative, 1, 1, rgb, P, near, out));
    const float bad_taps[4][4] = {{0, 0, q_nan, 0}, {0, 0, 0, p_inf}, {0, 0, 0.8f, 0.8f}, {-1.0000001f, 0, 0, 0}};
    for (const auto &t : bad_taps) expect(arctic_dof_pixels(&good, t, 1, xy, 1, 1, rgb, P, near, out));
    expect(arctic_dof_prepare(nullptr, 1, 1, z, t1, n1, p2));
    expect(arctic_dof_prepare(&good, 1, 1, nullptr, t1, n1, p2));
    expect(arctic_dof_prepare(&good, 1, 1, z, nullptr, n1, p2));
    expect(arctic_dof_prepare(&good, 1, 1, z, t1, nullptr, p2));
    expect(arctic_dof_prepare(&good, 1, 1, z, t1, n1, nullptr));
    expect(arctic_dof_prepare(&good, 0, 1, z, t1, n1, p2));
    expect(arctic_dof_prepare(&good, 1, 16385, z, t1, n1, p2));
    for (int k = 0; k < 27; ++k) {
        ArcticDof c = good;
        switch (k) {
        case 0: c.flags = 8; break;
        case 1: c.flags = 0x80000001u; break;
        case 2: c.flags = ARCTIC_DOF_SOURCE_COMPOSED | ARCTIC_DOF_SOURCE_TAA; break;
        case 3: c.flags = ARCTIC_DOF_SOURCE_TAA | ARCTIC_DOF_SOURCE_MOTION_BLUR; break;
        case 4: c.flags = 7; break;
        case 5: c.focus_distance = 0.0f; break;
        case 6: c.focus_distance = -1.0f; break;
        case 7: c.focus_distance = q_nan; break;
        case 8: c.focus_distance = p_inf; break;
        case 9: c.coc_scale = -0.001f; break;
        case 10: c.coc_scale = 4096.5f; break;
        case 11: c.coc_scale = q_nan; break;
        case 12: c.max_radius = 0.999f; break;
        case 13: c.max_radius = 64.001f; break;
        case 14: c.max_radius = q_nan; break;
        case 15: c.samples = 0; break;
        case 16: c.samples = 65; break;
        case 17: c.depth_extent = 0.0f; break;
        case 18: c.depth_extent = q_nan; break;
        case 19: c.depth_extent = p_inf; break;
        case 20: c.z_near = 0.0f; break;
        case 21: c.z_near = q_nan; break;
        case 22: c.z_far = 0.1f; break;
        case 23: c.z_far = p_inf; break;
        case 24: c.z_far = q_nan; break;
        case 25: c.z_near = 0.0f; c.z_far = 0.0f; break;                 // (only arctic_pass_dof accepts the zeros)
        default: c.z_near = -1.0f; break;
        }
        if (k != 15 && k != 16) expect(arctic_dof_pixels(&c, taps, 1, xy, 1, 1, rgb, P, near, out));   // (taps has two entries)
        else expect(arctic_dof_pixels(&c, nullptr, 1, xy, 1, 1, rgb, P, near, out));
        expect(arctic_dof_prepare(&c, 1, 1, z, t1, n1, p2));
    }
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, 2.0f, 1080, nullptr));
    expect(arctic_dof_coc_scale(0.0f, 50.0f, 24.0f, 2.0f, 1080, &scale));
    expect(arctic_dof_coc_scale(q_nan, 50.0f, 24.0f, 2.0f, 1080, &scale));
    expect(arctic_dof_coc_scale(2.0f, -50.0f, 24.0f, 2.0f, 1080, &scale));
    expect(arctic_dof_coc_scale(2.0f, p_inf, 24.0f, 2.0f, 1080, &scale));
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 0.0f, 2.0f, 1080, &scale));
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, 0.05f, 1080, &scale));   // (focused at the focal length)
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, p_inf, 1080, &scale));
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, 2.0f, 0, &scale));
    expect(arctic_dof_coc_scale(2.0f, 50.0f, 24.0f, 2.0f, 16385, &scale));
    expect(arctic_dof_coc_scale(1e-30f, 3e5f, 1e-30f, 301.0f, 16384, &scale));   // (the result overflows)
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
