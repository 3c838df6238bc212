// taa_upscale_sanitize.cpp -- the host arbiter of the temporal upscaler and arctic_taa_upscale_jitter (arctic-renderer_amd/csrc/taa_upscale.cpp,
// taa_upscale.h, on taa.h and ray_query.h) under -fsanitize=address,undefined, in a program of its own (tests/test_taa_upscale_sanitize.py builds
// and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/taa_upscale_sanitize.cpp \
//       arctic-renderer_amd/csrc/taa_upscale.cpp
// The size pairs 1x1 -> 1x1, 1x1 -> 4x4, 8x8 -> 16x16, 17x9 -> 29x14, 40x24 -> 64x40 and 37x23 -> 148x92 with every output pixel listed; an
// empty history and a full one; velocities that are ordinary, point far outside the frame, are NaN, infinite or 1e30 (the float-to-int
// conversion of the tap position must never see them); history entries with N = 0 and NaN colours; NaN colours in the current frame; every
// flag; and the record at the limits of its ranges: jitter -1 and +1, sharpness 0 and 65536, confidence_floor 1 and the smallest float,
// max_history 1 and 65536, min_weight just below 1.  Buffers are sized exactly, so a read or write past an end is caught, and an absent plane is a
// null pointer, so a read of it is caught too.  Then the jitter helper and the refusals, each of which must leave the output untouched.  Prints
// one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/taa_upscale.h"
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

static ArcticTaaUpscale record(uint32_t flags, uint32_t W, uint32_t H) {
    ArcticTaaUpscale t = {};
    t.flags = flags; t.max_history = 4.0f; t.min_weight = 0.1f; t.jitter[0] = 0.3f; t.jitter[1] = -0.2f; t.sharpness = 1.0f; t.confidence_floor = 0.0625f;
    t.out_width = W; t.out_height = H;
    return t;
}

// kind: -1 no velocity plane, 0 ordinary, 1 far outside, 2 NaN, 3 infinite, 4 1e30
static void run(const std::string &name, const uint32_t *s, int kind, bool have, const ArcticTaaUpscale &t) {
    const uint32_t w = s[0], h = s[1], W = s[2], H = s[3];
    std::mt19937 g(4321);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const size_t n_in = (size_t)w * h, n = (size_t)W * H;
    std::vector<float> cur(3 * n_in), vel(2 * n_in), prev(4 * n), out(4 * n, -7.0f);
    std::vector<int32_t> xy(2 * n);
    for (size_t k = 0; k < n_in; ++k) {
        for (int a = 0; a < 3; ++a) cur[3 * k + a] = 4.0f * u(g);
        if (k % 11 == 5) cur[3 * k + 1] = q_nan;
        for (int a = 0; a < 2; ++a) {
            float v = 4.0f * u(g) - 2.0f;
            if (kind == 1) v = (k % 2 ? 1.0f : -1.0f) * (200.0f + 100.0f * u(g));
            if (kind == 2 && k % 3 == (size_t)a) v = q_nan;
            if (kind == 3 && k % 3 == (size_t)a) v = k % 2 ? p_inf : -p_inf;
            if (kind == 4 && k % 3 == (size_t)a) v = k % 2 ? 1e30f : -1e30f;
            vel[2 * k + a] = v;
        }
    }
    for (size_t k = 0; k < n; ++k) {
        xy[2 * k] = (int32_t)(k % W); xy[2 * k + 1] = (int32_t)(k / W);
        for (int a = 0; a < 3; ++a) prev[4 * k + a] = 4.0f * u(g);
        prev[4 * k + 3] = 0.0625f + (float)(k % 5);
        if (k % 7 == 3) { prev[4 * k + 3] = 0.0f; prev[4 * k] = q_nan; }   // a rejected tap with a NaN colour behind it
    }
    if (arctic_taa_upscale_pixels(&t, n, xy.data(), w, h, cur.data(), kind < 0 ? nullptr : vel.data(), have ? prev.data() : nullptr, out.data()) != ARCTIC_OK) return bad(name, "refused");
    size_t fresh = 0, blended = 0;
    const float least = t.confidence_floor < 0.0625f ? t.confidence_floor : 0.0625f;
    for (size_t k = 0; k < n; ++k) {
        const float N = out[4 * k + 3];
        if (!(N >= least && N <= (t.max_history > 1.0f ? t.max_history : 1.0f))) return bad(name, "N outside [confidence_floor, max_history]");
        // a pixel that was not blended holds an input colour by bits (step 4): N is then max(beta, confidence_floor) <= 1
        bool is_input = false;
        for (size_t q = 0; q < n_in && !is_input; ++q) is_input = std::memcmp(&out[4 * k], &cur[3 * q], 12) == 0;
        fresh += is_input; blended += !is_input;
    }
    if (!have && blended) return bad(name, "an empty history blended");
    if (kind == 1 && blended) return bad(name, "a tap outside the frame blended");
    std::printf("ok %s: %ux%u -> %ux%u, flags %u: %zu blended, %zu fresh\n", name.c_str(), w, h, W, H, t.flags, blended, fresh);
}

int main() {
    const uint32_t sizes[6][4] = {{1, 1, 1, 1}, {1, 1, 4, 4}, {8, 8, 16, 16}, {17, 9, 29, 14}, {40, 24, 64, 40}, {37, 23, 148, 92}};
    for (const auto &s : sizes) {
        const std::string f = "-" + std::to_string(s[0]) + "x" + std::to_string(s[1]) + "-" + std::to_string(s[2]) + "x" + std::to_string(s[3]);
        run("empty" + f, s, 0, false, record(0, s[2], s[3]));
        run("ordinary" + f, s, 0, true, record(0, s[2], s[3]));
        run("luma" + f, s, 0, true, record(ARCTIC_TAA_UPSCALE_LUMA_WEIGHT, s[2], s[3]));
        run("no-clamp" + f, s, 0, true, record(ARCTIC_TAA_UPSCALE_NO_CLAMP | ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED, s[2], s[3]));
        run("no-velocity" + f, s, -1, true, record(0, s[2], s[3]));
        run("outside" + f, s, 1, true, record(0, s[2], s[3]));
        run("nan" + f, s, 2, true, record(ARCTIC_TAA_UPSCALE_LUMA_WEIGHT, s[2], s[3]));
        run("inf" + f, s, 3, true, record(0, s[2], s[3]));
        run("1e30" + f, s, 4, true, record(ARCTIC_TAA_UPSCALE_NO_CLAMP, s[2], s[3]));
        // the record at the limits of its ranges
        ArcticTaaUpscale t = record(0, s[2], s[3]);
        t.jitter[0] = -1.0f; t.jitter[1] = 1.0f; t.sharpness = 65536.0f; t.confidence_floor = std::numeric_limits<float>::denorm_min(); t.max_history = 65536.0f; t.min_weight = 0.0f;
        run("limits-a" + f, s, 0, true, t);
        t.jitter[0] = 1.0f; t.jitter[1] = -1.0f; t.sharpness = 0.0f; t.confidence_floor = 1.0f; t.max_history = 1.0f; t.min_weight = 0.99999994f;
        run("limits-b" + f, s, 4, true, t);
    }

    // arctic_taa_upscale_jitter: a 2-float buffer sized exactly; every index of two periods and the largest; the exact phases
    {
        std::vector<float> j(2);
        bool fine = true;
        for (const auto &s : sizes) {
            const uint32_t L = 8u * ((s[2] + s[0] - 1) / s[0]) * ((s[3] + s[1] - 1) / s[1]);
            std::vector<float> first(2);
            for (uint32_t i = 0; i <= 2 * L; ++i) {
                fine = fine && arctic_taa_upscale_jitter(i, s[0], s[2], s[1], s[3], j.data()) == ARCTIC_OK && std::fabs(j[0]) <= 0.5f && std::fabs(j[1]) <= 0.5f;
                if (i == 0) first = j;
                if (i == L || i == 2 * L) fine = fine && j == first;
            }
            fine = fine && arctic_taa_upscale_jitter(0x7FFFFFFFu, s[0], s[2], s[1], s[3], j.data()) == ARCTIC_OK;
        }
        for (uint32_t s = 1; s <= 4; s *= 2)
            for (uint32_t i = 0; i < s * s; ++i) {
                fine = fine && arctic_taa_upscale_jitter(i | ARCTIC_TAA_UPSCALE_JITTER_EXACT, 17, 17 * s, 9, 9 * s, j.data()) == ARCTIC_OK;
                fine = fine && j[0] == 0.5f - ((float)(i % s) + 0.5f) / (float)s && j[1] == 0.5f - ((float)(i / s) + 0.5f) / (float)s;
            }
        const std::vector<float> after = j;
        fine = fine && arctic_taa_upscale_jitter(0, 8, 16, 8, 16, nullptr) == ARCTIC_E_INVALID && arctic_taa_upscale_jitter(0, 0, 0, 8, 16, j.data()) == ARCTIC_E_INVALID &&
               arctic_taa_upscale_jitter(0, 8, 7, 8, 16, j.data()) == ARCTIC_E_INVALID && arctic_taa_upscale_jitter(0, 8, 33, 8, 16, j.data()) == ARCTIC_E_INVALID &&
               arctic_taa_upscale_jitter(0, 8192, 16385, 8, 16, j.data()) == ARCTIC_E_INVALID &&
               arctic_taa_upscale_jitter(ARCTIC_TAA_UPSCALE_JITTER_EXACT, 8, 24, 8, 24, j.data()) == ARCTIC_E_INVALID &&
               arctic_taa_upscale_jitter(ARCTIC_TAA_UPSCALE_JITTER_EXACT, 8, 16, 8, 32, j.data()) == ARCTIC_E_INVALID && j == after;
        if (!fine) bad("jitter", "arctic_taa_upscale_jitter"); else std::printf("ok jitter\n");
    }

    // refusals: each leaves the output as it was
    const float cur[3] = {1, 2, 3}, vel[2] = {0, 0}, prev[4] = {2, 2, 2, 1};
    const int32_t xy[2] = {0, 0}, outside[2] = {1, 0}, negative[2] = {0, -1};
    ArcticTaaUpscale good = record(1, 1, 1);
    float out[4] = {77, 77, 77, 77};
    int refused = 0, tried = 0;
    auto untouched = [&] { return out[0] == 77 && out[1] == 77 && out[2] == 77 && out[3] == 77; };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_taa_upscale_pixels(&good, 1, xy, 1, 1, cur, vel, prev, out) != ARCTIC_OK || untouched()) bad("refusals", "the good call");
    out[0] = out[1] = out[2] = out[3] = 77;
    if (arctic_taa_upscale_pixels(&good, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr) != ARCTIC_OK) bad("refusals", "no pixel");
    expect(arctic_taa_upscale_pixels(nullptr, 1, xy, 1, 1, cur, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, nullptr, 1, 1, cur, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, xy, 1, 1, nullptr, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, xy, 1, 1, cur, vel, prev, nullptr));
    expect(arctic_taa_upscale_pixels(&good, 1, xy, 0, 1, cur, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, xy, 1, 16385, cur, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, xy, 2, 1, cur, vel, prev, out));          // the output is smaller than the input
    expect(arctic_taa_upscale_pixels(&good, 1, outside, 1, 1, cur, vel, prev, out));
    expect(arctic_taa_upscale_pixels(&good, 1, negative, 1, 1, cur, vel, prev, out));
    for (int k = 0; k < 24; ++k) {
        ArcticTaaUpscale c = good;
        switch (k) {
        case 0: c.flags = 8; break;
        case 1: c.flags = 0x80000001u; break;
        case 2: c.max_history = 0.5f; break;
        case 3: c.max_history = 65537.0f; break;
        case 4: c.max_history = q_nan; break;
        case 5: c.max_history = p_inf; break;
        case 6: c.min_weight = -0.001f; break;
        case 7: c.min_weight = 1.0f; break;
        case 8: c.min_weight = q_nan; break;
        case 9: c.jitter[0] = 1.001f; break;
        case 10: c.jitter[1] = -p_inf; break;
        case 11: c.jitter[1] = q_nan; break;
        case 12: c.sharpness = -0.001f; break;
        case 13: c.sharpness = 65537.0f; break;
        case 14: c.sharpness = q_nan; break;
        case 15: c.confidence_floor = 0.0f; break;
        case 16: c.confidence_floor = 1.001f; break;
        case 17: c.confidence_floor = q_nan; break;
        case 18: c.out_width = 0; break;
        case 19: c.out_width = 5; break;          // above four times the input's
        case 20: c.out_height = 16385; break;
        case 21: c.out_height = 0; break;
        case 22: c.reserved[0] = 1; break;
        default: c.reserved[2] = 1; break;
        }
        expect(arctic_taa_upscale_pixels(&c, 1, xy, 1, 1, cur, vel, prev, out));
    }
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
