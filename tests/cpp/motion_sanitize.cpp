// motion_sanitize.cpp -- the two host arbiters of the motion vectors (csrc/motion.cpp: arctic_motion_pixels, arctic_accumulate_pixels_motion) under
// the address and undefined-behaviour sanitizers, in a program of its own (tests/test_motion_abi.py builds and runs it; the sanitizers' runtime is
// never loaded into python).  Inputs that are not finite, 1e30 and 1e-30 on top of ordinary ones, a ragged frame, every refusal.  Prints one
// line per case: "ok <name> ..." or "BAD <name> ...".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../include/arctic_hip.h"

namespace {

const float NaN = std::numeric_limits<float>::quiet_NaN(), INF = std::numeric_limits<float>::infinity();
int failures = 0;

void report(const char *name, bool ok, const char *what = "") {
    std::printf("%s %s %s\n", ok ? "ok" : "BAD", name, what);
    if (!ok) ++failures;
}

// a perspective matrix looking down -z from (0, 1, 4), [col][row]
void camera(float *P) {
    const float f = 1.0f / std::tan(0.4f), n = 0.1f, fa = 100.0f, a = 1.5f;
    const float m[16] = {f / a, 0, 0, 0, 0, f, 0, 0, 0, 0, fa / (n - fa), -1, 0, -f, -4.0f * fa / (n - fa) + n * fa / (n - fa), 4.0f};
    std::memcpy(P, m, sizeof m);
}

struct Pixels {
    std::vector<float> bary, pos, trs;
    std::vector<uint32_t> object;
    std::vector<int32_t> xy;
};

Pixels make_pixels(uint64_t n, uint32_t n_objects, uint32_t W, uint32_t H, float scale, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    Pixels p;
    p.bary.resize(3 * n); p.pos.resize(9 * n); p.object.resize(n); p.xy.resize(2 * n); p.trs.assign(16 * (size_t)n_objects, 0.0f);
    for (uint32_t o = 0; o < n_objects; ++o) {
        float *t = &p.trs[16 * o];
        t[0] = t[5] = t[10] = t[15] = 1.0f;
        t[12] = u(rng); t[13] = u(rng); t[14] = u(rng);
    }
    for (uint64_t k = 0; k < n; ++k) {
        const float a = 0.5f * (u(rng) + 1.0f), b = (1.0f - a) * 0.5f * (u(rng) + 1.0f);
        p.bary[3 * k] = a; p.bary[3 * k + 1] = b; p.bary[3 * k + 2] = 1.0f - a - b;
        for (int i = 0; i < 9; ++i) p.pos[9 * k + i] = scale * u(rng);
        p.object[k] = k % 7 == 0 ? 0xFFFFFFFFu : k % 11 == 0 ? n_objects + 3 : (uint32_t)(k % n_objects);
        p.xy[2 * k] = (int32_t)(k % W); p.xy[2 * k + 1] = (int32_t)((k / W) % H);
    }
    return p;
}

// the motion arbiter on n pixels; `poison`: what goes into a tenth of the positions, barycentrics and matrices
bool motion_case(uint64_t n, uint32_t W, uint32_t H, float scale, float poison, bool empty) {
    Pixels p = make_pixels(n, 5, W, H, scale, 17u + (unsigned)n);
    if (poison != 0.0f) {
        for (uint64_t k = 0; k < n; k += 10) { p.pos[9 * k + (k % 9)] = poison; p.bary[3 * ((k + 5) % n) + 1] = poison; }
        p.trs[16 * 2 + 13] = poison;
    }
    float P[16];
    camera(P);
    std::vector<float> pw(4 * n, -7.0f), vel(2 * n, -7.0f);
    if (arctic_motion_pixels(n, p.bary.data(), p.object.data(), p.pos.data(), p.xy.data(), p.trs.data(), 5, empty ? nullptr : P, W, H, pw.data(), vel.data()) != ARCTIC_OK) return false;
    bool ok = true;
    for (uint64_t k = 0; k < n; ++k) {
        const float flag = pw[4 * k + 3];
        const bool has = !empty && p.object[k] < 5;
        ok = ok && (has ? (flag == 1.0f || flag == 2.0f) : (flag == 0.0f && pw[4 * k] == 0.0f && pw[4 * k + 1] == 0.0f && pw[4 * k + 2] == 0.0f));
        if (flag != 2.0f) ok = ok && vel[2 * k] == 0.0f && vel[2 * k + 1] == 0.0f;                 // a velocity only with flag 2 ...
        else ok = ok && !std::isnan(vel[2 * k]) && !std::isnan(vel[2 * k + 1]);                    // ... and then it is a number
    }
    // without the optional output
    return ok && arctic_motion_pixels(n, p.bary.data(), p.object.data(), p.pos.data(), p.xy.data(), p.trs.data(), 5, empty ? nullptr : P, W, H, pw.data(), nullptr) == ARCTIC_OK;
}

// the accumulation's arbiter over a W x H frame whose previous history and prev_world4 plane hold `poison` here and there
bool accumulate_case(uint32_t W, uint32_t H, float scale, float poison) {
    const uint64_t n = (uint64_t)W * H;
    std::mt19937 rng(23u + W);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> world(3 * n), pw4(4 * n), normal(3 * n), pv(n), pc(n), pwd(3 * n), pn(3 * n);
    std::vector<uint8_t> geometry(n), cur(n);
    for (uint64_t k = 0; k < n; ++k) {
        for (int i = 0; i < 3; ++i) {
            world[3 * k + i] = scale * u(rng); pw4[4 * k + i] = world[3 * k + i] + 0.01f * u(rng); pwd[3 * k + i] = pw4[4 * k + i];
            normal[3 * k + i] = i == 2 ? 2.0f : 0.0f; pn[3 * k + i] = i == 2 ? 1.0f : 0.0f;
        }
        pw4[4 * k + 3] = (float)(k % 3);
        geometry[k] = k % 13 != 0; cur[k] = (uint8_t)(k * 37u);
        pv[k] = 255.0f * 0.5f * (u(rng) + 1.0f); pc[k] = (float)(k % 5);
    }
    if (poison != 0.0f)
        for (uint64_t k = 0; k < n; k += 9) { pw4[4 * k + (k % 4)] = poison; pwd[3 * ((k + 4) % n)] = poison; pv[(k + 2) % n] = poison; normal[3 * ((k + 6) % n) + 1] = poison; }
    const ArcticAoHistory hist = {8.0f, 0.9f, 0.05f, 0.1f, {0, 0, 0, 0}};
    float P[16];
    camera(P);
    std::vector<uint8_t> out(n, 7);
    std::vector<float> ov(n), oc(n), ow(3 * n), on(3 * n);
    bool ok = true;
    for (const float *prev : {(const float *)nullptr, (const float *)P}) {
        if (arctic_accumulate_pixels_motion(&hist, n, world.data(), pw4.data(), normal.data(), geometry.data(), cur.data(), prev, W, H, pv.data(), pc.data(), pwd.data(), pn.data(), out.data(),
                                            ov.data(), oc.data(), ow.data(), on.data()) != ARCTIC_OK) return false;
        for (uint64_t k = 0; k < n; ++k) {
            ok = ok && oc[k] >= 0.0f && oc[k] <= 8.0f;                                                 // a count, never a NaN
            if (!geometry[k]) ok = ok && out[k] == 255 && oc[k] == 0.0f;
            if (geometry[k] && oc[k] == 1.0f) ok = ok && out[k] == cur[k];                             // rejected: the current byte
            if (!(pw4[4 * k + 3] >= 1.0f)) ok = ok && oc[k] <= 1.0f;                                   // a flag below 1, or a NaN: no history
        }
    }
    return ok && arctic_accumulate_pixels_motion(&hist, n, world.data(), pw4.data(), normal.data(), geometry.data(), cur.data(), P, W, H, pv.data(), pc.data(), pwd.data(), pn.data(),
                                                 out.data(), nullptr, nullptr, nullptr, nullptr) == ARCTIC_OK;
}

bool refusals() {
    const ArcticAoHistory hist = {8.0f, 0.9f, 0.05f, 0.1f, {0, 0, 0, 0}};
    ArcticAoHistory bad = hist;
    bad.max_history = 0.5f;
    float f[16] = {0}, P[16];
    camera(P);
    uint32_t o[1] = {0};
    int32_t xy[2] = {0, 0};
    uint8_t b[1] = {0};
    bool ok = arctic_motion_pixels(0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1, 1, nullptr, nullptr) == ARCTIC_OK;
    ok = ok && arctic_motion_pixels(1, f, o, f, xy, f, 1, P, 0, 4, f, f) == ARCTIC_E_INVALID;
    ok = ok && arctic_motion_pixels(1, f, o, f, xy, f, 1, P, 4, 16385, f, f) == ARCTIC_E_INVALID;
    ok = ok && arctic_motion_pixels(1, nullptr, o, f, xy, f, 1, P, 4, 4, f, f) == ARCTIC_E_INVALID;
    ok = ok && arctic_motion_pixels(1, f, o, f, xy, f, 1, P, 4, 4, nullptr, f) == ARCTIC_E_INVALID;
    ok = ok && arctic_motion_pixels(1, f, o, f, xy, nullptr, 1, P, 4, 4, f, f) == ARCTIC_E_INVALID;
    ok = ok && arctic_accumulate_pixels_motion(nullptr, 1, f, f, f, b, b, nullptr, 4, 4, nullptr, nullptr, nullptr, nullptr, b, nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    ok = ok && arctic_accumulate_pixels_motion(&bad, 1, f, f, f, b, b, nullptr, 4, 4, nullptr, nullptr, nullptr, nullptr, b, nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    ok = ok && arctic_accumulate_pixels_motion(&hist, 1, f, nullptr, f, b, b, nullptr, 4, 4, nullptr, nullptr, nullptr, nullptr, b, nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    ok = ok && arctic_accumulate_pixels_motion(&hist, 1, f, f, f, b, b, P, 4, 4, nullptr, f, f, f, b, nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    ok = ok && arctic_accumulate_pixels_motion(&hist, 1, f, f, f, b, b, nullptr, 4, 4, nullptr, nullptr, nullptr, nullptr, b, nullptr, nullptr, nullptr, nullptr) == ARCTIC_OK;
    return ok;
}

}  // namespace

int main() {
    report("motion-ordinary", motion_case(5000, 96, 64, 2.0f, 0.0f, false));
    report("motion-empty", motion_case(777, 61, 37, 2.0f, 0.0f, true));
    report("motion-nan", motion_case(5000, 61, 37, 2.0f, NaN, false));
    report("motion-inf", motion_case(5000, 61, 37, 2.0f, -INF, false));
    report("motion-1e30", motion_case(5000, 96, 64, 1e30f, 1e30f, false));
    report("accumulate-ordinary", accumulate_case(96, 64, 2.0f, 0.0f));
    report("accumulate-nan", accumulate_case(61, 37, 2.0f, NaN));
    report("accumulate-inf", accumulate_case(61, 37, 2.0f, INF));
    report("accumulate-1e30", accumulate_case(96, 64, 1e30f, 1e30f));
    report("refusals", refusals());
    return failures ? 1 : 0;
}
