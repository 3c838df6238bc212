// ao_history_sanitize.cpp -- the host arbiter of the temporal accumulation (arctic-renderer_amd/csrc/ao_history.cpp, ao_history.h, on ray_ao.h and
// ray_query.h) under -fsanitize=address,undefined, in a program of its own (tests/test_ao_history_abi.py builds and runs it; it is never loaded
// into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/ao_history_sanitize.cpp \
//       arctic-renderer_amd/csrc/ao_history.cpp
// Sequences of calls on frames of 1 x 1, 7 x 5 and 61 x 37 pixels under matrices that throw the taps everywhere: inside, across every border,
// far outside (coordinates of 1e30 and beyond the range of an int), behind the camera, onto NaNs.  Normals that are zero, overflow, underflow
// or are not finite; world positions that are NaN or infinite; pixels without geometry whose inputs are NaNs; a previous history that holds NaNs
// and counts of zero.  Buffers are sized exactly, so a read or write past an end is caught, and a float that does not fit an int is caught where
// it is converted.  Then the refusals, each of which must leave the output untouched.  Prints one "ok <case>" line per case, or "BAD <case>:
// why" and exits 1.
#include "../../arctic-renderer_amd/csrc/ao_history.h"
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

// `calls` calls on a W x H frame whose positions span `span`; matrix k of the sequence scales and shifts the frame, every third one looks backwards
static void run(const std::string &name, uint32_t W, uint32_t H, int calls, float span) {
    std::mt19937 g(4321);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    const size_t n = (size_t)W * H;
    const ArcticAoHistory hist = {6.0f, 0.5f, 0.25f * span, 0.1f, {0, 0, 0, 0}};
    std::vector<float> value(n), count(n), hw(3 * n), hm(3 * n), P(16), prevP;
    size_t blended = 0, fresh = 0, open = 0;
    for (int c = 0; c < calls; ++c) {
        std::vector<float> world(3 * n), normal(3 * n), ov(n, -7.0f), oc(n, -7.0f), ow(3 * n, -7.0f), om(3 * n, -7.0f);
        std::vector<uint8_t> geometry(n), cur(n), out(n, 99);
        for (size_t k = 0; k < n; ++k) {
            const uint32_t x = (uint32_t)(k % W), y = (uint32_t)(k / W);
            world[3 * k] = span * ((x + 0.5f) * 2.0f / W - 1.0f); world[3 * k + 1] = span * (1.0f - (y + 0.5f) * 2.0f / H); world[3 * k + 2] = span * 0.01f * u(g);
            normal[3 * k] = 0.05f * (u(g) - 0.5f); normal[3 * k + 1] = 0.05f * (u(g) - 0.5f); normal[3 * k + 2] = 1.0f + u(g);
            geometry[k] = 1; cur[k] = (uint8_t)(u(g) < 0.5f ? 0 : 255);
            float *nr = &normal[3 * k], *w = &world[3 * k];
            switch ((k + c) % 16) {
            case 1: nr[0] = nr[1] = nr[2] = 0.0f; break;
            case 2: nr[0] = 3e19f; nr[1] = 3e19f; break;
            case 3: nr[1] = q_nan; break;
            case 4: nr[2] = p_inf; break;
            case 5: nr[0] = nr[1] = 1e-30f; nr[2] = 0.0f; break;
            case 6: w[0] = q_nan; break;
            case 7: w[1] = p_inf; break;
            case 8: w[0] = 3e38f; w[1] = -3e38f; break;
            case 9: geometry[k] = 0; nr[0] = q_nan; w[2] = q_nan; break;
            case 10: w[2] = span * 5.0f; break;                                  // another surface: rejected by the plane test
            default: break;
            }
        }
        // this call's matrix, [col][row]: x and y scaled and shifted, c3 = 1 -- or, every third call, c3 = -1 - z: everything is behind it
        const float s = (c % 2 ? 1.07f : 0.93f) / span, shift = 0.31f * (float)(c % 4) - 0.4f;
        std::fill(P.begin(), P.end(), 0.0f);
        P[0] = s; P[5] = s; P[12] = shift; P[13] = -shift; P[15] = 1.0f;
        if (c % 3 == 2) { P[11] = -1.0f / span; P[15] = -1.0f; }
        if (c == 3) { P[12] = 1e30f; }                                            // the whole frame lands far outside: ix is about 1e30
        if (c == 4) { P[0] = q_nan; }
        const float *pp = prevP.empty() ? nullptr : prevP.data();
        if (arctic_accumulate_pixels(&hist, n, world.data(), normal.data(), geometry.data(), cur.data(), pp, W, H, value.data(), count.data(), hw.data(), hm.data(), out.data(),
                                     ov.data(), oc.data(), ow.data(), om.data()) != ARCTIC_OK)
            return bad(name, "refused");
        for (size_t k = 0; k < n; ++k) {
            const uint32_t kind = (uint32_t)((k + c) % 16);
            const bool uncovered = (kind >= 1 && kind <= 5) || kind == 9;
            if (uncovered && !(out[k] == 255 && ov[k] == 0.0f && oc[k] == 0.0f && ow[3 * k] == 0.0f && om[3 * k + 2] == 0.0f)) return bad(name, "a pixel step 1 leaves out has an entry");
            if (!uncovered && !(oc[k] >= 1.0f && oc[k] <= 6.0f && ov[k] >= -0.001f && ov[k] <= 255.001f)) return bad(name, "a count or a value out of range");   // (V / S of equal values may round a step past them)
            if (!uncovered && oc[k] == 1.0f && out[k] != cur[k]) return bad(name, "N = 1 but the byte is not the input");
            if (!uncovered && std::fabs((float)out[k] - ov[k]) > 0.5f) return bad(name, "the byte is not the rounded value");
            open += uncovered; blended += !uncovered && oc[k] > 1.0f; fresh += !uncovered && oc[k] == 1.0f;
        }
        if (c == 0 && blended) return bad(name, "an empty history was used");
        value.swap(ov); count.swap(oc); hw.swap(ow); hm.swap(om);
        if (c == 1) for (size_t k = 0; k < n; k += 7) { value[k] = q_nan; if (k % 2) count[k] = 0.0f; else hw[3 * k + 1] = q_nan; }   // a history with NaNs no tap may accept
        prevP = P;
    }
    if (n >= 35 && calls >= 2 && !blended) return bad(name, "no pixel ever used its history");
    std::printf("ok %s: %u x %u, %d calls: %zu blended, %zu fresh, %zu left out\n", name.c_str(), W, H, calls, blended, fresh, open);
}

int main() {
    run("one-pixel", 1, 1, 6, 1.0f);
    run("small-7x5", 7, 5, 6, 1.0f);
    run("ragged-61x37", 61, 37, 6, 3.0f);
    run("huge-1e30", 16, 8, 6, 1e30f);
    run("tiny-1e-30", 16, 8, 6, 1e-30f);
    run("one-call", 61, 37, 1, 1.0f);

    // refusals: each leaves the output as it was
    const float world[3] = {0, 0, 0}, normal[3] = {0, 0, 1}, P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, hv = 50, hc = 2, hw[3] = {0, 0, 0}, hm[3] = {0, 0, 1};
    const uint8_t geometry = 1, cur = 200;
    const ArcticAoHistory good = {8.0f, 0.9f, 0.05f, 0.0f, {0, 0, 0, 0}};
    uint8_t out = 77;
    float ov = 77;
    int refused = 0, tried = 0;
    auto untouched = [&] { return out == 77 && ov == 77; };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr) != ARCTIC_OK || out != 100 || ov != 100.0f)
        bad("refusals", "the good call");   // hv = 50, hn = 2, N = 3, 50 + 150 / 3
    out = 77; ov = 77;
    expect(arctic_accumulate_pixels(nullptr, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, nullptr, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, nullptr, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, nullptr, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, nullptr, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 0, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 16385, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, nullptr, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, nullptr, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, nullptr, hm, &out, &ov, nullptr, nullptr, nullptr));
    expect(arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, nullptr, &out, &ov, nullptr, nullptr, nullptr));
    for (int k = 0; k < 13; ++k) {
        ArcticAoHistory h = good;
        switch (k) {
        case 0: h.max_history = 0.999f; break;
        case 1: h.max_history = 65537.0f; break;
        case 2: h.max_history = q_nan; break;
        case 3: h.max_history = p_inf; break;
        case 4: h.normal_cos = p_inf; break;
        case 5: h.normal_cos = q_nan; break;
        case 6: h.plane_dist = -0.001f; break;
        case 7: h.plane_dist = q_nan; break;
        case 8: h.min_weight = -0.001f; break;
        case 9: h.min_weight = 1.0f; break;
        case 10: h.min_weight = q_nan; break;
        case 11: h.reserved[0] = 1; break;
        default: h.reserved[3] = 1; break;
        }
        expect(arctic_accumulate_pixels(&h, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, &out, &ov, nullptr, nullptr, nullptr));
    }
    {   // the byte plane is required only when there is a pixel
        uint8_t none = 5;
        ++tried; refused += arctic_accumulate_pixels(&good, 1, world, normal, &geometry, &cur, P, 1, 1, &hv, &hc, hw, hm, nullptr, &ov, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID && untouched();
        if (arctic_accumulate_pixels(&good, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ARCTIC_OK || none != 5)
            bad("refusals", "no pixel needs no array");
    }
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
