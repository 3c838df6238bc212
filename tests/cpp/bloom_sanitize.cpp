// bloom_sanitize.cpp -- the host arbiters of bloom (arctic-renderer_amd/csrc/bloom.cpp, bloom.h, on ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_bloom_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/bloom_sanitize.cpp \
//       arctic-renderer_amd/csrc/bloom.cpp
// Frames of 1x1, 3x5, 8x8, 17x9, 40x24 and 72x40 at 1, 2, 5 and 8 levels with every pixel listed; colours that are ordinary, NaN, infinite of
// either sign, negative or 1e30 -- the pyramids are sized exactly as arctic_bloom_layout says, so a read or write past an end is caught, and
// every element must be written, finite and >= 0.  Then the refusals, each of which must leave the outputs untouched.  Prints one "ok <case>"
// line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/bloom.h"
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

// kind: 0 ordinary, 1 with NaN, infinite, negative and huge colours
static void run(const std::string &name, uint32_t W, uint32_t H, uint32_t levels, int kind) {
    std::mt19937 g(4321);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const size_t n = (size_t)W * H;
    uint64_t lay[3 * 8 + 2];
    if (arctic_bloom_layout(W, H, levels, lay) != ARCTIC_OK) return bad(name, "layout refused");
    uint64_t at = 0;
    uint32_t w = W, h = H;
    for (uint32_t k = 0; k < levels; ++k) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (lay[3 * k] != w || lay[3 * k + 1] != h || lay[3 * k + 2] != at) return bad(name, "the layout");
        if (k + 1 == levels && lay[3 * levels + 1] != at) return bad(name, "the layout's floats of up");
        at += (uint64_t)w * h * 3;
    }
    if (lay[3 * levels] != at) return bad(name, "the layout's floats of down");
    const size_t n_down = lay[3 * levels], n_up = lay[3 * levels + 1];
    std::vector<float> rgb(3 * n), down(n_down, -7.0f), up(n_up, -7.0f), out(3 * n, -7.0f);
    std::vector<int32_t> xy(2 * n);
    const float odd[6] = {q_nan, p_inf, -p_inf, -2.0f, 1e30f, -0.0f};
    for (size_t k = 0; k < n; ++k) {
        xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W);
        for (int a = 0; a < 3; ++a) { const float v = u(g); rgb[3 * k + a] = 20.0f * v * v * v * v; }
        if (kind == 1 && k % 3 == 0) rgb[3 * k + k % 2] = odd[(k / 3) % 6];
    }
    const ArcticBloom bloom = {0, 0.7f, 0.25f, 50.0f, 1.5f, 0.75f, levels, 0};
    if (arctic_bloom_pyramid(&bloom, W, H, rgb.data(), down.data(), levels > 1 ? up.data() : nullptr) != ARCTIC_OK) return bad(name, "pyramid refused");
    for (const std::vector<float> *plane : {&down, &up})
        for (float v : *plane)
            if (!(v >= 0.0f && std::isfinite(v))) return bad(name, "an element of a pyramid is not finite and >= 0, or was not written");
    const float *u1 = levels > 1 ? up.data() : down.data();
    if (arctic_bloom_pixels(&bloom, n, xy.data(), W, H, rgb.data(), u1, out.data()) != ARCTIC_OK) return bad(name, "pixels refused");
    size_t finite = 0;
    for (size_t k = 0; k < 3 * n; ++k) {
        if (out[k] == -7.0f) return bad(name, "a pixel was not written");
        if (std::isnan(out[k]) != std::isnan(rgb[k])) return bad(name, "a NaN that is not the colour's own");
        finite += std::isfinite(out[k]);
    }
    std::printf("ok %s: %ux%u, %u levels: %zu of %zu values finite\n", name.c_str(), W, H, levels, finite, 3 * n);
}

int main() {
    const uint32_t sizes[6][2] = {{1, 1}, {3, 5}, {8, 8}, {17, 9}, {40, 24}, {72, 40}};
    const uint32_t levels[4] = {1, 2, 5, 8};
    for (const auto &s : sizes)
        for (uint32_t l : levels) {
            const std::string f = "-" + std::to_string(s[0]) + "x" + std::to_string(s[1]) + "-" + std::to_string(l);
            run("ordinary" + f, s[0], s[1], l, 0);
            run("odd" + f, s[0], s[1], l, 1);
        }

    // refusals: each leaves the outputs as they were
    const float rgb[3] = {4, 2, 1}, u1[3] = {1, 1, 1};
    const int32_t xy[2] = {0, 0}, outside[2] = {1, 0}, negative[2] = {0, -1};
    const ArcticBloom good = {ARCTIC_BLOOM_SOURCE_DOF, 1.0f, 0.5f, 65504.0f, 0.5f, 1.0f, 2, 0};
    float out[3] = {77, 77, 77}, down[6] = {77, 77, 77, 77, 77, 77}, up[3] = {77, 77, 77};
    uint64_t lay[26];
    for (uint64_t &v : lay) v = 77;
    int refused = 0, tried = 0;
    auto untouched = [&] {
        for (float v : out) if (v != 77) return false;
        for (float v : down) if (v != 77) return false;
        for (float v : up) if (v != 77) return false;
        for (uint64_t v : lay) if (v != 77) return false;
        return true;
    };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_bloom_pyramid(&good, 1, 1, rgb, down, up) != ARCTIC_OK || down[0] == 77 || down[5] == 77 || up[2] == 77) bad("refusals", "the good pyramid");
    if (arctic_bloom_pixels(&good, 1, xy, 1, 1, rgb, u1, out) != ARCTIC_OK || out[0] == 77) bad("refusals", "the good call");
    for (float &v : out) v = 77;
    for (float &v : down) v = 77;
    for (float &v : up) v = 77;
    if (arctic_bloom_pixels(&good, 0, nullptr, 1, 1, nullptr, nullptr, nullptr) != ARCTIC_OK) bad("refusals", "no pixel");
    ArcticBloom one = good;
    one.levels = 1;
    if (arctic_bloom_pyramid(&one, 1, 1, rgb, down, nullptr) != ARCTIC_OK || down[0] == 77 || down[3] != 77) bad("refusals", "one level needs no up");
    for (float &v : down) v = 77;
    expect(arctic_bloom_pixels(nullptr, 1, xy, 1, 1, rgb, u1, out));
    expect(arctic_bloom_pixels(&good, 1, nullptr, 1, 1, rgb, u1, out));
    expect(arctic_bloom_pixels(&good, 1, xy, 1, 1, nullptr, u1, out));
    expect(arctic_bloom_pixels(&good, 1, xy, 1, 1, rgb, nullptr, out));
    expect(arctic_bloom_pixels(&good, 1, xy, 1, 1, rgb, u1, nullptr));
    expect(arctic_bloom_pixels(&good, 1, xy, 0, 1, rgb, u1, out));
    expect(arctic_bloom_pixels(&good, 1, xy, 1, 16385, rgb, u1, out));
    expect(arctic_bloom_pixels(&good, 1, outside, 1, 1, rgb, u1, out));
    expect(arctic_bloom_pixels(&good, 1, negative, 1, 1, rgb, u1, out));
    expect(arctic_bloom_pyramid(nullptr, 1, 1, rgb, down, up));
    expect(arctic_bloom_pyramid(&good, 1, 1, nullptr, down, up));
    expect(arctic_bloom_pyramid(&good, 1, 1, rgb, nullptr, up));
    expect(arctic_bloom_pyramid(&good, 1, 1, rgb, down, nullptr));   // (two levels need it)
    expect(arctic_bloom_pyramid(&good, 0, 1, rgb, down, up));
    expect(arctic_bloom_pyramid(&good, 1, 16385, rgb, down, up));
    expect(arctic_bloom_layout(1, 1, 1, nullptr));
    expect(arctic_bloom_layout(0, 1, 1, lay));
    expect(arctic_bloom_layout(1, 16385, 1, lay));
    expect(arctic_bloom_layout(1, 1, 0, lay));
    expect(arctic_bloom_layout(1, 1, 9, lay));
    for (int k = 0; k < 25; ++k) {
        ArcticBloom c = good;
        switch (k) {
        case 0: c.flags = 16; break;
        case 1: c.flags = 0x80000001u; break;
        case 2: c.flags = ARCTIC_BLOOM_SOURCE_COMPOSED | ARCTIC_BLOOM_SOURCE_TAA; break;
        case 3: c.flags = ARCTIC_BLOOM_SOURCE_MOTION_BLUR | ARCTIC_BLOOM_SOURCE_DOF; break;
        case 4: c.flags = 15; break;
        case 5: c.threshold = -0.001f; break;
        case 6: c.threshold = 65505.0f; break;
        case 7: c.threshold = q_nan; break;
        case 8: c.threshold = p_inf; break;
        case 9: c.soft_knee = -0.001f; break;
        case 10: c.soft_knee = 1.001f; break;
        case 11: c.soft_knee = q_nan; break;
        case 12: c.clamp_max = 0.0f; break;
        case 13: c.clamp_max = 65505.0f; break;
        case 14: c.clamp_max = q_nan; break;
        case 15: c.intensity = -0.001f; break;
        case 16: c.intensity = 16.001f; break;
        case 17: c.intensity = q_nan; break;
        case 18: c.spread = -0.001f; break;
        case 19: c.spread = 1.001f; break;
        case 20: c.spread = q_nan; break;
        case 21: c.levels = 0; break;
        case 22: c.levels = 9; break;
        case 23: c.reserved = 1; break;
        default: c.clamp_max = -1.0f; break;
        }
        expect(arctic_bloom_pixels(&c, 1, xy, 1, 1, rgb, u1, out));
        expect(arctic_bloom_pyramid(&c, 1, 1, rgb, down, up));
    }
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
