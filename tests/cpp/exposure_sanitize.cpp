// exposure_sanitize.cpp -- the host arbiters of auto-exposure (arctic-renderer_amd/csrc/exposure.cpp, exposure.h, on ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_exposure_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/exposure_sanitize.cpp \
//       arctic-renderer_amd/csrc/exposure.cpp
// Frames of 1x1, 3x5, 17x9, 40x24 and 136x72 under four windows and two records; colours that are ordinary, NaN, infinite of either sign,
// negative, -0 or 1e30 -- every array is sized exactly, so a read or write past an end is caught; the histogram must sum to the window, six
// calls thread the state through, every pixel of the output must be written.  Then the refusals, each of which must leave the outputs
// untouched.  Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/exposure.h"
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

static ArcticExposure record(int which) {
    ArcticExposure e = {};
    if (which == 0) { e.low_q16 = 32768; e.high_q16 = 62259; e.key_value = 0.18f; e.min_exposure = 1.0f / 1024.0f; e.max_exposure = 1024.0f; e.rate_up = 1.0f; e.rate_down = 1.0f; e.fallback_exposure = 1.0f; }
    else { e.flags = ARCTIC_EXPOSURE_SKIP_BLACK; e.low_q16 = 6554; e.high_q16 = 65536; e.key_value = 0.5f; e.min_exposure = 0.01f; e.max_exposure = 8.0f; e.rate_up = 0.25f; e.rate_down = 0.0625f; e.fallback_exposure = 2.0f; }
    return e;
}

// kind: 0 ordinary, 1 with NaN, infinite, negative and huge colours
static void run(const std::string &name, uint32_t W, uint32_t H, int which, int window, int kind) {
    std::mt19937 g(4321 + W);
    std::uniform_real_distribution<float> u(-20.0f, 18.0f);
    const size_t n = (size_t)W * H;
    std::vector<float> rgb(3 * n), out(3 * n, -7.0f);
    const float odd[6] = {q_nan, p_inf, -p_inf, -2.0f, 1e30f, -0.0f};
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 3; ++a) rgb[3 * k + a] = std::exp2(u(g));
        if (kind == 1 && k % 3 == 0) rgb[3 * k + k % 2] = odd[(k / 3) % 6];
    }
    ArcticExposure e = record(which);
    const uint32_t windows[4][4] = {{0, 0, 0, 0}, {W / 2, H / 2, W / 2 + 1, H / 2 + 1}, {0, H - 1, W, H}, {W > 2 ? 1u : 0u, H > 3 ? 1u : 0u, W > 2 ? W - 1 : W, H > 3 ? H - 2 : H}};
    std::memcpy(e.window, windows[window], sizeof e.window);
    const uint64_t pixels = window == 0 ? n : (uint64_t)(e.window[2] - e.window[0]) * (e.window[3] - e.window[1]);
    std::vector<uint32_t> hist(256, 0xDEADu);
    if (arctic_exposure_histogram(&e, W, H, rgb.data(), hist.data()) != ARCTIC_OK) return bad(name, "histogram refused");
    uint64_t sum = 0;
    for (uint32_t h : hist) sum += h;
    if (sum != pixels) return bad(name, "the histogram does not sum to the window");
    ArcticExposureState state, prev;
    std::memset(&state, 0x5A, sizeof state);
    if (arctic_exposure_resolve(&e, hist.data(), nullptr, &state) != ARCTIC_OK) return bad(name, "resolve refused");
    for (int call = 0; call < 6; ++call) {
        prev = state;
        if (call == 3) e.flags |= ARCTIC_EXPOSURE_RESET;
        if (arctic_exposure_resolve(&e, hist.data(), &prev, &state) != ARCTIC_OK) return bad(name, "resolve refused");
        e.flags &= ~ARCTIC_EXPOSURE_RESET;
        if (!(state.exposure >= e.min_exposure && state.exposure <= e.max_exposure) || state.reserved != 0u) return bad(name, "E outside its clamp");
        if (state.valid && !(state.adapted_key >= 888.5 && state.adapted_key <= 888.5 + 255.0 && state.luminance > 0.0f)) return bad(name, "the adapted key left the histogram");
    }
    if (arctic_exposure_pixels(n, rgb.data(), state.exposure, out.data()) != ARCTIC_OK) return bad(name, "pixels refused");
    size_t finite = 0;
    for (size_t k = 0; k < 3 * n; ++k) {
        if (out[k] == -7.0f) return bad(name, "a pixel was not written");
        if (std::isnan(out[k]) != std::isnan(rgb[k])) return bad(name, "a NaN that is not the colour's own");
        finite += std::isfinite(out[k]);
    }
    std::printf("ok %s: %ux%u, record %d, window %d: M = %u, E = %g, %zu of %zu values finite\n", name.c_str(), W, H, which, window, state.metered, state.exposure, finite, 3 * n);
}

static void refusals() {
    const std::string name = "refusals";
    std::vector<float> rgb(3 * 4 * 4, 1.0f), out(3 * 4 * 4, -7.0f);
    std::vector<uint32_t> hist(256, 0xDEADu);
    ArcticExposureState state;
    std::memset(&state, 0x5A, sizeof state);
    const ArcticExposureState untouched = state;
    const ArcticExposure good = record(0);
    std::vector<ArcticExposure> bads;
    const auto with = [&](auto change) { ArcticExposure e = good; change(e); bads.push_back(e); };
    with([](ArcticExposure &e) { e.flags = 512u; });
    with([](ArcticExposure &e) { e.flags = 3u; });
    with([](ArcticExposure &e) { e.flags = 16u | 8u; });
    with([](ArcticExposure &e) { e.flags = ARCTIC_EXPOSURE_HOLD | ARCTIC_EXPOSURE_METER_ONLY; });
    with([](ArcticExposure &e) { e.flags = ARCTIC_EXPOSURE_HOLD | ARCTIC_EXPOSURE_RESET; });
    with([](ArcticExposure &e) { e.low_q16 = e.high_q16; });
    with([](ArcticExposure &e) { e.high_q16 = 65537u; });
    with([](ArcticExposure &e) { e.key_value = 0.0f; });
    with([](ArcticExposure &e) { e.key_value = q_nan; });
    with([](ArcticExposure &e) { e.min_exposure = 0.0f; });
    with([](ArcticExposure &e) { e.min_exposure = 2.0f; e.max_exposure = 1.0f; });
    with([](ArcticExposure &e) { e.max_exposure = p_inf; });
    with([](ArcticExposure &e) { e.rate_up = 1.5f; });
    with([](ArcticExposure &e) { e.rate_down = q_nan; });
    with([](ArcticExposure &e) { e.fallback_exposure = -1.0f; });
    with([](ArcticExposure &e) { e.window[2] = 5; e.window[3] = 4; });
    with([](ArcticExposure &e) { e.window[0] = 2; e.window[2] = 2; e.window[3] = 4; });
    with([](ArcticExposure &e) { e.reserved = 1u; });
    for (const ArcticExposure &e : bads) {
        if (arctic_exposure_histogram(&e, 4, 4, rgb.data(), hist.data()) != ARCTIC_E_INVALID) return bad(name, "a bad record was taken by the histogram");
        const bool windowed = (e.window[0] | e.window[1] | e.window[2] | e.window[3]) != 0u;   // (the resolve knows no frame: it takes any window a 16384 x 16384 one admits)
        if (!(windowed && e.window[0] < e.window[2]) && arctic_exposure_resolve(&e, hist.data(), nullptr, &state) != ARCTIC_E_INVALID) return bad(name, "a bad record was taken by the resolve");
    }
    if (arctic_exposure_histogram(nullptr, 4, 4, rgb.data(), hist.data()) != ARCTIC_E_INVALID || arctic_exposure_histogram(&good, 0, 4, rgb.data(), hist.data()) != ARCTIC_E_INVALID ||
        arctic_exposure_histogram(&good, 4, 16385, rgb.data(), hist.data()) != ARCTIC_E_INVALID || arctic_exposure_histogram(&good, 4, 4, nullptr, hist.data()) != ARCTIC_E_INVALID ||
        arctic_exposure_histogram(&good, 4, 4, rgb.data(), nullptr) != ARCTIC_E_INVALID)
        return bad(name, "the histogram took a null or a bad size");
    if (arctic_exposure_resolve(nullptr, hist.data(), nullptr, &state) != ARCTIC_E_INVALID || arctic_exposure_resolve(&good, nullptr, nullptr, &state) != ARCTIC_E_INVALID ||
        arctic_exposure_resolve(&good, hist.data(), nullptr, nullptr) != ARCTIC_E_INVALID)
        return bad(name, "the resolve took a null");
    if (arctic_exposure_pixels(16, nullptr, 1.0f, out.data()) != ARCTIC_E_INVALID || arctic_exposure_pixels(16, rgb.data(), 1.0f, nullptr) != ARCTIC_E_INVALID ||
        arctic_exposure_pixels(0, nullptr, 1.0f, nullptr) != ARCTIC_OK)
        return bad(name, "the pixels");
    uint64_t lay[3] = {7, 7, 7};
    if (arctic_exposure_layout(0, 4, lay) != ARCTIC_E_INVALID || arctic_exposure_layout(4, 16385, lay) != ARCTIC_E_INVALID || arctic_exposure_layout(4, 4, nullptr) != ARCTIC_E_INVALID || lay[0] != 7)
        return bad(name, "the layout");
    for (uint32_t h : hist) if (h != 0xDEADu) return bad(name, "a refused call wrote the histogram");
    for (float v : out) if (v != -7.0f) return bad(name, "a refused call wrote the output");
    if (std::memcmp(&state, &untouched, sizeof state) != 0) return bad(name, "a refused call wrote the state");
    if (!(arctic_exposure_rate(0.0f, 3.0f) == 0.0f && arctic_exposure_rate(1e9f, 3.0f) == 1.0f && arctic_exposure_rate(q_nan, 1.0f) == 0.0f && arctic_exposure_rate(-1.0f, 1.0f) == 0.0f))
        return bad(name, "the rate");
    std::printf("ok %s: %zu bad records\n", name.c_str(), bads.size());
}

int main() {
    const uint32_t sizes[5][2] = {{1, 1}, {3, 5}, {17, 9}, {40, 24}, {136, 72}};
    for (const auto &s : sizes)
        for (int which = 0; which < 2; ++which)
            for (int window = 0; window < 4; ++window) {
                const std::string f = "-" + std::to_string(s[0]) + "x" + std::to_string(s[1]) + "-" + std::to_string(which) + "-" + std::to_string(window);
                run((window % 2 ? "odd" : "ordinary") + f, s[0], s[1], which, window, window % 2);
            }
    refusals();
    return failures ? 1 : 0;
}
