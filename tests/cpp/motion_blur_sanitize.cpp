// motion_blur_sanitize.cpp -- the host arbiters of the motion blur (arctic-renderer_amd/csrc/motion_blur.cpp, motion_blur.h, on ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_motion_blur_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/motion_blur_sanitize.cpp \
//       arctic-renderer_amd/csrc/motion_blur.cpp
// Frames of 1x1, 8x8, 17x9, 40x24 and 72x40 with every pixel listed; velocities that are ordinary, far beyond max_radius, NaN, infinite or 1e30
// (the float-to-int conversion of a tap position must never see a value outside the frame); NaN colours and depths; with and without the depth
// plane and the dither; 1, 7 and 64 taps -- buffers are sized exactly, so a read or write past an end is caught, and an absent plane is a null
// pointer, so a read of it is caught too.  Then the refusals, each of which must leave the outputs untouched.  Prints one "ok <case>" line per
// case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/motion_blur.h"
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

// kind: 0 ordinary, 1 far beyond max_radius, 2 NaN, 3 infinite, 4 1e30
static void run(const std::string &name, uint32_t W, uint32_t H, int kind, bool depth, uint32_t flags, uint32_t samples) {
    std::mt19937 g(1234);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const size_t n = (size_t)W * H, tiles = (size_t)((W + 7) / 8) * ((H + 7) / 8);
    std::vector<float> rgb(3 * n), vel(2 * n), z(n), tile(2 * tiles, -7.0f), near(2 * tiles, -7.0f), P(2 * n, -7.0f), out(3 * n, -7.0f);
    std::vector<int32_t> xy(2 * n);
    for (size_t k = 0; k < n; ++k) {
        xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W);
        for (int a = 0; a < 3; ++a) rgb[3 * k + a] = 4.0f * u(g);
        if (k % 11 == 5) rgb[3 * k + 1] = q_nan;
        z[k] = k % 13 == 7 ? q_nan : u(g);
        for (int a = 0; a < 2; ++a) {
            float v = 24.0f * u(g) - 12.0f;
            if (kind == 1) v = (k % 2 ? 1.0f : -1.0f) * (500.0f + 1000.0f * u(g));
            if (kind == 2 && k % 3 == (size_t)a) v = q_nan;
            if (kind == 3 && k % 3 == (size_t)a) v = k % 2 ? p_inf : -p_inf;
            if (kind == 4 && k % 3 == (size_t)a) v = k % 2 ? 1e30f : -1e30f;
            vel[2 * k + a] = v;
        }
    }
    const ArcticMotionBlur mb = {flags, 1.0f, 16.0f, samples, 0.05f, {0, 0, 0}};
    if (arctic_motion_blur_prepare(&mb, W, H, vel.data(), depth ? z.data() : nullptr, tile.data(), near.data(), P.data()) != ARCTIC_OK) return bad(name, "prepare refused");
    for (size_t k = 0; k < n; ++k)
        if (!(P[2 * k] >= 0.5f && P[2 * k] <= 16.001f)) return bad(name, "l outside [0.5, max_radius]");
    for (size_t k = 0; k < 2 * tiles; ++k)
        if (!(std::fabs(tile[k]) <= 16.001f && std::fabs(near[k]) <= 16.001f)) return bad(name, "a maximum beyond max_radius, or not finite");
    if (arctic_motion_blur_pixels(&mb, n, xy.data(), W, H, rgb.data(), P.data(), near.data(), out.data()) != ARCTIC_OK) return bad(name, "pixels refused");
    size_t finite = 0;
    for (size_t k = 0; k < n; ++k) {
        if (out[3 * k] == -7.0f && out[3 * k + 2] == -7.0f) return bad(name, "a pixel was not written");
        finite += std::isfinite(out[3 * k]) && std::isfinite(out[3 * k + 1]) && std::isfinite(out[3 * k + 2]);
    }
    std::printf("ok %s: %ux%u, flags %u, %u taps: %zu of %zu pixels finite\n", name.c_str(), W, H, flags, samples, finite, n);
}

int main() {
    const uint32_t sizes[5][2] = {{1, 1}, {8, 8}, {17, 9}, {40, 24}, {72, 40}};
    for (const auto &s : sizes) {
        const std::string f = "-" + std::to_string(s[0]) + "x" + std::to_string(s[1]);
        run("ordinary" + f, s[0], s[1], 0, true, 0, 7);
        run("no-depth" + f, s[0], s[1], 0, false, ARCTIC_MB_DITHER, 7);
        run("one-tap" + f, s[0], s[1], 0, true, 0, 1);
        run("64-taps" + f, s[0], s[1], 0, true, ARCTIC_MB_DITHER, 64);
        run("beyond" + f, s[0], s[1], 1, true, 0, 7);
        run("nan" + f, s[0], s[1], 2, true, ARCTIC_MB_DITHER, 7);
        run("inf" + f, s[0], s[1], 3, false, 0, 7);
        run("1e30" + f, s[0], s[1], 4, true, 0, 7);
    }

    // planes from elsewhere: a P whose l is 0, NaN or huge and a neighbour_max2 that is NaN, infinite or 1e30 -- no tap may leave the frame
    {
        const uint32_t W = 17, H = 9;
        const size_t n = (size_t)W * H, tiles = 3 * 2;
        std::vector<float> rgb(3 * n, 1.0f), P(2 * n), near(2 * tiles), out(3 * n, -7.0f);
        std::vector<int32_t> xy(2 * n);
        const float odd[6] = {0.0f, q_nan, 1e30f, -1.0f, p_inf, 0.5f};
        for (size_t k = 0; k < n; ++k) { xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W); P[2 * k] = odd[k % 6]; P[2 * k + 1] = odd[(k + 1) % 6]; }
        const float dirs[12] = {q_nan, 1.0f, p_inf, 0.0f, 1e30f, -1e30f, -p_inf, q_nan, 3e9f, 3e9f, -5e9f, 1.0f};
        for (size_t k = 0; k < 2 * tiles; ++k) near[k] = dirs[k];
        const ArcticMotionBlur mb = {ARCTIC_MB_DITHER, 1.0f, 16.0f, 9, 0.05f, {0, 0, 0}};
        if (arctic_motion_blur_pixels(&mb, n, xy.data(), W, H, rgb.data(), P.data(), near.data(), out.data()) != ARCTIC_OK) bad("odd-planes", "refused");
        else std::printf("ok odd-planes\n");
    }

    // refusals: each leaves the outputs as they were
    const float rgb[3] = {1, 2, 3}, vel[2] = {4, 0}, z[1] = {0.5f}, P[2] = {2, 0.5f}, near[2] = {2, 0};
    const int32_t xy[2] = {0, 0}, outside[2] = {1, 0}, negative[2] = {0, -1};
    const ArcticMotionBlur good = {1, 1.0f, 16.0f, 15, 0.05f, {0, 0, 0}};
    float out[3] = {77, 77, 77}, t2[2] = {77, 77}, n2[2] = {77, 77}, p2[2] = {77, 77};
    int refused = 0, tried = 0;
    auto untouched = [&] { return out[0] == 77 && out[1] == 77 && out[2] == 77 && t2[0] == 77 && t2[1] == 77 && n2[0] == 77 && n2[1] == 77 && p2[0] == 77 && p2[1] == 77; };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_motion_blur_prepare(&good, 1, 1, vel, z, t2, n2, p2) != ARCTIC_OK || t2[0] != 2 || n2[0] != 2 || p2[0] != 2 || p2[1] != 0.5f) bad("refusals", "the good prepare");
    if (arctic_motion_blur_pixels(&good, 1, xy, 1, 1, rgb, P, near, out) != ARCTIC_OK || out[0] == 77) bad("refusals", "the good call");
    out[0] = out[1] = out[2] = t2[0] = t2[1] = n2[0] = n2[1] = p2[0] = p2[1] = 77;
    if (arctic_motion_blur_pixels(&good, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr) != ARCTIC_OK) bad("refusals", "no pixel");
    expect(arctic_motion_blur_pixels(nullptr, 1, xy, 1, 1, rgb, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, nullptr, 1, 1, rgb, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 1, 1, nullptr, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 1, 1, rgb, nullptr, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 1, 1, rgb, P, nullptr, out));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 1, 1, rgb, P, near, nullptr));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 0, 1, rgb, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, xy, 1, 16385, rgb, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, outside, 1, 1, rgb, P, near, out));
    expect(arctic_motion_blur_pixels(&good, 1, negative, 1, 1, rgb, P, near, out));
    expect(arctic_motion_blur_prepare(nullptr, 1, 1, vel, z, t2, n2, p2));
    expect(arctic_motion_blur_prepare(&good, 1, 1, nullptr, z, t2, n2, p2));
    expect(arctic_motion_blur_prepare(&good, 1, 1, vel, z, nullptr, n2, p2));
    expect(arctic_motion_blur_prepare(&good, 1, 1, vel, z, t2, nullptr, p2));
    expect(arctic_motion_blur_prepare(&good, 1, 1, vel, z, t2, n2, nullptr));
    expect(arctic_motion_blur_prepare(&good, 0, 1, vel, z, t2, n2, p2));
    expect(arctic_motion_blur_prepare(&good, 1, 16385, vel, z, t2, n2, p2));
    for (int k = 0; k < 18; ++k) {
        ArcticMotionBlur c = good;
        switch (k) {
        case 0: c.flags = 8; break;
        case 1: c.flags = 0x80000001u; break;
        case 2: c.flags = ARCTIC_MB_SOURCE_COMPOSED | ARCTIC_MB_SOURCE_TAA; break;
        case 3: c.shutter = -0.001f; break;
        case 4: c.shutter = 4.001f; break;
        case 5: c.shutter = q_nan; break;
        case 6: c.shutter = p_inf; break;
        case 7: c.max_radius = 0.999f; break;
        case 8: c.max_radius = 64.001f; break;
        case 9: c.max_radius = q_nan; break;
        case 10: c.samples = 0; break;
        case 11: c.samples = 65; break;
        case 12: c.depth_extent = 0.0f; break;
        case 13: c.depth_extent = -0.05f; break;
        case 14: c.depth_extent = q_nan; break;
        case 15: c.depth_extent = p_inf; break;
        case 16: c.reserved[0] = 1; break;
        default: c.reserved[2] = 1; break;
        }
        expect(arctic_motion_blur_pixels(&c, 1, xy, 1, 1, rgb, P, near, out));
        expect(arctic_motion_blur_prepare(&c, 1, 1, vel, z, t2, n2, p2));
    }
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
