// compose_sanitize.cpp -- the host arbiter of the composition (arctic-renderer_amd/csrc/compose.cpp, compose.h, on ray_ao.h and ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_compose_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/compose_sanitize.cpp \
//       arctic-renderer_amd/csrc/compose.cpp
// No pixel, one pixel, many; normals that are zero, overflow, underflow or are not finite; reflections with a = 0 and NaN colours; pixels without
// geometry whose inputs are NaNs; an eye that sits on the surface; coordinates of 1e30; every flag alone and both -- buffers are sized exactly, so
// a read or write past an end is caught, and a plane whose flag is absent is a null pointer, so a read of it is caught too.  Then the refusals,
// each of which must leave the output untouched.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/compose.h"
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

static void run(const std::string &name, size_t n, uint32_t flags, float span) {
    std::mt19937 g(1234);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> hdr(3 * n), base(3 * n), metal(n), rough(n), normal(3 * n), world(3 * n), refl(4 * n), out(3 * n, -7.0f);
    std::vector<uint8_t> ao(n), geometry(n);
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) {
            hdr[3 * k + a] = 4.0f * u(g); base[3 * k + a] = u(g); normal[3 * k + a] = 2.0f * u(g) - 1.0f; world[3 * k + a] = span * (2.0f * u(g) - 1.0f);
            refl[4 * k + a] = 3.0f * u(g);
        }
        metal[k] = u(g); rough[k] = u(g); ao[k] = (uint8_t)(k * 37); geometry[k] = 1;
        refl[4 * k + 3] = (k % 3) * 0.5f;
        if (k % 3 == 0) refl[4 * k] = refl[4 * k + 1] = refl[4 * k + 2] = q_nan;
        float *nr = &normal[3 * k];
        switch (k % 16) {
        case 1: nr[0] = nr[1] = nr[2] = 0.0f; break;
        case 2: nr[0] = nr[1] = 0.0f; nr[2] = -0.0f; break;
        case 3: nr[0] = 3e19f; nr[1] = 3e19f; break;
        case 4: nr[1] = q_nan; break;
        case 5: nr[2] = p_inf; break;
        case 6: nr[0] = 1e-30f; nr[1] = 1e-30f; nr[2] = 1e-30f; break;
        case 7: world[3 * k] = 0.5f; world[3 * k + 1] = 0.5f; world[3 * k + 2] = 0.5f; break;   // the eye itself: wo is 0 / 0
        case 8: world[3 * k + 1] = q_nan; break;
        case 9: world[3 * k] = p_inf; break;
        case 10: geometry[k] = 0; base[3 * k] = q_nan; metal[k] = q_nan; rough[k] = q_nan; nr[0] = q_nan; world[3 * k + 2] = q_nan; refl[4 * k + 3] = q_nan; break;
        case 11: ao[k] = 0; break;
        case 12: ao[k] = 255; break;
        case 13: refl[4 * k + 3] = q_nan; break;   // not > 0: no reflection
        default: break;
        }
    }
    const float eye[3] = {0.5f, 0.5f, 0.5f};
    const ArcticRayCompose c = {flags, 0.75f, 1.5f, 0.0f, {0, 0, 0, 0}};
    const uint8_t *pa = (flags & ARCTIC_COMPOSE_AO) ? ao.data() : nullptr;
    const float *pr = (flags & ARCTIC_COMPOSE_REFLECTIONS) ? refl.data() : nullptr;
    if (arctic_compose_pixels(&c, eye, 0.1f, n, hdr.data(), base.data(), metal.data(), rough.data(), normal.data(), world.data(), pa, pr, geometry.data(), out.data()) != ARCTIC_OK)
        return bad(name, "refused");
    size_t same = 0, moved = 0;
    for (size_t k = 0; k < n; ++k) {
        const bool equal = std::memcmp(&out[3 * k], &hdr[3 * k], 12) == 0;
        same += equal; moved += !equal;
        if (k % 16 == 10 && !equal) return bad(name, "a pixel without geometry moved");
        if (!(flags & ARCTIC_COMPOSE_AO) && (k % 3 == 0 || (k % 16 >= 1 && k % 16 <= 6) || k % 16 == 13) && !equal) return bad(name, "a pixel without a reflection moved");
        if ((flags & ARCTIC_COMPOSE_AO) && !(flags & ARCTIC_COMPOSE_REFLECTIONS) && k % 16 == 12 && !equal) return bad(name, "an open pixel moved");
    }
    std::printf("ok %s: %zu pixels, flags %u: %zu moved, %zu as they were\n", name.c_str(), n, flags, moved, same);
}

int main() {
    for (uint32_t flags = 1; flags <= 3; ++flags) {
        const std::string f = "-flags-" + std::to_string(flags);
        run("no-pixel" + f, 0, flags, 1.0f);
        run("one-pixel" + f, 1, flags, 1.0f);
        run("many-20000" + f, 20000, flags, 3.0f);
        run("huge-1e30" + f, 500, flags, 1e30f);
        run("tiny-1e-40" + f, 500, flags, 1e-40f);
    }

    // refusals: each leaves the output as it was
    const float hdr[3] = {1, 2, 3}, base[3] = {0.5f, 0.5f, 0.5f}, metal = 0.5f, rough = 0.5f, normal[3] = {0, 0, 1}, world[3] = {0, 0, 0}, refl[4] = {1, 1, 1, 1}, eye[3] = {0, 0, 2};
    const uint8_t ao = 100, geometry = 1;
    const ArcticRayCompose good = {3, 0.5f, 1.0f, 0.0f, {0, 0, 0, 0}};
    float out[3] = {77, 77, 77};
    int refused = 0, tried = 0;
    auto untouched = [&] { return out[0] == 77 && out[1] == 77 && out[2] == 77; };
    auto expect = [&](int rc) { ++tried; refused += rc == ARCTIC_E_INVALID && untouched(); };
    if (arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, &geometry, out) != ARCTIC_OK || untouched()) bad("refusals", "the good call");
    out[0] = out[1] = out[2] = 77;
    expect(arctic_compose_pixels(nullptr, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, nullptr, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, nullptr, base, &metal, &rough, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, nullptr, &metal, &rough, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, nullptr, &rough, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, nullptr, normal, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, nullptr, world, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, nullptr, &ao, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, nullptr, refl, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, nullptr, &geometry, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, nullptr, out));
    expect(arctic_compose_pixels(&good, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, &geometry, nullptr));
    for (int k = 0; k < 11; ++k) {
        ArcticRayCompose c = good;
        switch (k) {
        case 0: c.flags = 0; break;
        case 1: c.flags = 4; break;
        case 2: c.flags = 0x80000003u; break;
        case 3: c.ao_strength = -0.001f; break;
        case 4: c.ao_strength = 1.001f; break;
        case 5: c.ao_strength = q_nan; break;
        case 6: c.reflection_strength = -1.0f; break;
        case 7: c.reflection_strength = p_inf; break;
        case 8: c.reflection_strength = q_nan; break;
        case 9: c.reserved[0] = 1; break;
        default: c.reserved[3] = 1; break;
        }
        expect(arctic_compose_pixels(&c, eye, 0.1f, 1, hdr, base, &metal, &rough, normal, world, &ao, refl, &geometry, out));
    }
    if (refused != tried) bad("refusals", "a refusal is missing, or wrote");
    else std::printf("ok refusals: %d\n", tried);
    return failures ? 1 : 0;
}
