// gi_sanitize.cpp -- the host arbiters of the indirect diffuse light (arctic-renderer_amd/csrc/gi.cpp, gi.h, on ray_ao.h and ray_query.h) under
// -fsanitize=address,undefined, in a program of its own (tests/test_gi_abi.py builds and runs it; it is never loaded into python):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/gi_sanitize.cpp \
//       arctic-renderer_amd/csrc/gi.cpp arctic-renderer_amd/csrc/ao_history.cpp
// arctic_gi_points over ordinary and hostile points (zero, NaN, infinite, overflowing normals, m2 = -0.0, worlds that are not finite) for every
// pattern and round; arctic_gi_estimate_pixels on frames of 1x1, 3x5, 13x11 and 64x40 with n_rays of 1, 3 and 16, every pattern, filtered and
// not, with colours that hold NaN, infinities, negatives and 3e38.  Every array is sized exactly, so a read or write past an end is caught.
// Every record and every entry of S and E must be written; a point that is not covered must give the all-zero record; S must hold no NaN and
// nothing negative; E.a must be 0 or lie in [n_rays, n_rays * P * P].  arctic_gi_accumulate_pixels over three calls whose matrices send the taps
// inside the frame, onto its border rows and columns, behind the camera and to infinity, with a history that holds NaN and infinities: N must lie
// in [1, max_history] or be 0 with an all-zero entry.  arctic_gi_compose_pixels with NaN behind E.a == 0.  Then the refusals, each of which must
// leave the outputs untouched.
// Prints one "ok <case>" line per case, or "BAD <case>: why" and exits 1.
#include "../../arctic-renderer_amd/csrc/gi.h"
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

static ArcticGi record(uint32_t n_rays, uint32_t P, uint32_t filter) {
    ArcticGi g = {};
    g.n_rays = n_rays; g.pattern = P; g.max_distance = 25.0f; g.bias = 1e-3f; g.clamp_max = 3e38f; g.filter = filter; g.normal_cos = 0.9f; g.plane_dist = 0.05f;
    return g;
}

static std::vector<float> table(uint32_t n_rays, uint32_t P, std::mt19937 &g) {
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<float> d((size_t)P * P * n_rays * 3);
    for (float &x : d) x = u(g);
    d[0] = 0.0f; d[1] = 0.0f; d[2] = 0.0f;   // a direction that comes out zero
    return d;
}

static const float HOSTILE[][3] = {{0.0f, 1.0f, -0.0f}, {0.0f, 0.0f, 0.0f}, {q_nan, 0.0f, 1.0f}, {0.0f, p_inf, 0.0f}, {3e19f, 3e19f, 3e19f}, {1e-30f, 1e-30f, 0.0f},
                                   {0.0f, 0.0f, -1.0f}, {-0.0f, -0.0f, -0.0f}};
static const bool HOSTILE_COVERED[] = {true, false, false, false, false, false, true, false};

static void points(uint32_t n_rays, uint32_t P) {
    const std::string name = "points-" + std::to_string(n_rays) + "-" + std::to_string(P);
    std::mt19937 g(31 + n_rays + P);
    std::uniform_real_distribution<float> u(-3.0f, 3.0f);
    const std::vector<float> dirs = table(n_rays, P, g);
    const size_t n_hostile = sizeof HOSTILE / sizeof HOSTILE[0], n = 64 + n_hostile + 2;
    std::vector<float> pts(6 * n);
    std::vector<uint32_t> sets(n);
    for (size_t k = 0; k < n; ++k) {
        for (int a = 0; a < 6; ++a) pts[6 * k + a] = u(g);
        sets[k] = (uint32_t)(k % (P * P));
        if (k >= 64 && k < 64 + n_hostile) for (int a = 0; a < 3; ++a) pts[6 * k + 3 + a] = HOSTILE[k - 64][a];
    }
    pts[6 * (n - 2)] = q_nan; pts[6 * (n - 1) + 1] = -p_inf;   // worlds that are not finite: a record all the same
    const ArcticGi gi = record(n_rays, P, 0);
    for (uint32_t round = 0; round < n_rays; ++round) {
        std::vector<ArcticRay> rays(n);
        std::memset(rays.data(), 0xCD, n * sizeof(ArcticRay));
        if (arctic_gi_points(pts.data(), sets.data(), n, &gi, dirs.data(), round, rays.data()) != ARCTIC_OK) return bad(name, "refused");
        for (size_t k = 0; k < n; ++k) {
            const bool covered = k < 64 || k >= 64 + n_hostile || HOSTILE_COVERED[k - 64];
            static const ArcticRay zero = {};
            if (!covered && std::memcmp(&rays[k], &zero, sizeof zero) != 0) return bad(name, "a point that is not covered has a record");
            if (covered && !(rays[k].t_max == 25.0f && rays[k].t_min == 0.0f)) return bad(name, "a covered point's extent");
        }
    }
    std::printf("ok %s\n", name.c_str());
}

static void frame(uint32_t W, uint32_t H, uint32_t n_rays, uint32_t P, uint32_t filter) {
    const std::string name = "frame-" + std::to_string(W) + "x" + std::to_string(H) + "-" + std::to_string(n_rays) + "-" + std::to_string(P) + "-" + std::to_string(filter);
    std::mt19937 g(977 + W + n_rays + P);
    std::uniform_real_distribution<float> u(0.0f, 4.0f), s(-1.0f, 1.0f);
    const size_t n = (size_t)W * H;
    std::vector<ArcticRay> rays(n_rays * n);
    std::vector<float> colors(4 * n_rays * n), normal(3 * n), world(3 * n), S(4 * n, -7.0f), E(4 * n, -7.0f);
    std::vector<uint8_t> geometry(n);
    const float odd[] = {q_nan, p_inf, -p_inf, -2.0f, 3e38f, 3.3e38f, 0.0f, -0.0f};
    for (size_t p = 0; p < n; ++p) {
        const bool right = (p % W) * 2 >= W;
        normal[3 * p] = right ? 1.5f : 0.01f * s(g); normal[3 * p + 1] = right ? 0.01f * s(g) : 2.0f; normal[3 * p + 2] = 0.01f * s(g);
        world[3 * p] = right ? 0.0f : 0.1f * (float)(p % W); world[3 * p + 1] = right ? 0.1f * (float)(p % W) : 0.0f; world[3 * p + 2] = 0.1f * (float)(p / W);
        geometry[p] = p % 7 != 3;
        if (p % 11 == 5) for (int a = 0; a < 3; ++a) normal[3 * p + a] = HOSTILE[(p / 11) % 8][a];
        if (p % 13 == 6) world[3 * p + 1] = q_nan;
    }
    for (uint32_t k = 0; k < n_rays; ++k) {
        for (size_t p = 0; p < n; ++p) {
            ArcticRay &r = rays[k * n + p];
            std::memset(&r, 0, sizeof r);
            float m[3];
            if (geometry[p] && arctic::ao_normal(normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], m)) { r.direction[0] = 1.0f; r.t_max = p_inf; }
            for (int a = 0; a < 4; ++a) colors[4 * (k * n + p) + a] = (p + k) % 5 == 2 ? odd[(p + k + a) % 8] : u(g);
        }
    }
    const ArcticGi gi = record(n_rays, P, filter);
    if (arctic_gi_estimate_pixels(&gi, W, H, rays.data(), colors.data(), filter ? normal.data() : nullptr, filter ? world.data() : nullptr, filter ? geometry.data() : nullptr,
                                  S.data(), E.data()) != ARCTIC_OK)
        return bad(name, "refused");
    for (size_t p = 0; p < n; ++p) {
        for (int a = 0; a < 4; ++a) {
            if (S[4 * p + a] == -7.0f || E[4 * p + a] == -7.0f) return bad(name, "an entry was not written");
            if (std::isnan(S[4 * p + a]) || S[4 * p + a] < 0.0f) return bad(name, "S holds a NaN or a negative");
        }
        const float cnt = E[4 * p + 3];
        if (!(cnt == 0.0f || (cnt >= (float)n_rays && cnt <= (float)(n_rays * (filter ? P * P : 1))))) return bad(name, "E.a outside its range");
        if (S[4 * p + 3] != (rays[p].t_max > 0.0f ? (float)n_rays : 0.0f)) return bad(name, "S.cnt is not the pixel's rays");
    }
    std::printf("ok %s\n", name.c_str());
}

static void history(uint32_t W, uint32_t H, int which) {
    const std::string name = "history-" + std::to_string(W) + "x" + std::to_string(H) + "-" + std::to_string(which);
    std::mt19937 g(4242 + W + which);
    std::uniform_real_distribution<float> u(0.0f, 3.0f), s(-1.0f, 1.0f);
    const size_t n = (size_t)W * H;
    ArcticGiHistory hist = {};
    hist.max_history = 4.0f; hist.normal_cos = 0.9f; hist.plane_dist = 0.5f; hist.min_weight = 0.1f;
    // [col][row]: x and y pass through scaled, w = 1 -- so NDC = world.xy --, or hostile variants
    float P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (which == 1) { P[12] = 0.999f; P[13] = -0.999f; }          // onto the last column and the first row
    if (which == 2) { P[15] = -1.0f; }                             // behind the camera
    if (which == 3) { P[0] = 3e38f; P[5] = 3e38f; P[15] = 1e-38f; }   // to infinity
    if (which == 4) { P[12] = -2.0f; }                             // off the left: ix = -1 at most
    std::vector<float> world(3 * n), normal(3 * n), cur(4 * n), pa(3 * n), pc(n), pw(3 * n), pn(3 * n);
    std::vector<uint8_t> geometry(n);
    for (size_t p = 0; p < n; ++p) {
        world[3 * p] = ((float)(p % W) + 0.5f) / (float)W * 2.0f - 1.0f + 0.01f * s(g); world[3 * p + 1] = 1.0f - ((float)(p / W) + 0.5f) / (float)H * 2.0f; world[3 * p + 2] = 0.0f;
        normal[3 * p] = 0.01f * s(g); normal[3 * p + 1] = 0.01f * s(g); normal[3 * p + 2] = 2.0f;
        geometry[p] = p % 7 != 3;
        if (p % 11 == 5) for (int a = 0; a < 3; ++a) normal[3 * p + a] = HOSTILE[(p / 11) % 8][a];
        for (int a = 0; a < 3; ++a) { cur[4 * p + a] = u(g); pa[3 * p + a] = p % 5 == 1 ? q_nan : (p % 5 == 2 ? p_inf : u(g)); pw[3 * p + a] = world[3 * p + a]; pn[3 * p + a] = a == 2 ? 1.0f : 0.0f; }
        cur[4 * p + 3] = p % 9 == 4 ? 0.0f : 3.0f;
        pc[p] = p % 6 == 0 ? 0.0f : 2.0f;
    }
    for (int first = 0; first < 2; ++first) {
        std::vector<float> out(4 * n, -7.0f), oa(3 * n, -7.0f), oc(n, -7.0f), ow(3 * n, -7.0f), on(3 * n, -7.0f);
        if (arctic_gi_accumulate_pixels(&hist, n, world.data(), normal.data(), geometry.data(), cur.data(), first ? nullptr : P, W, H, first ? nullptr : pa.data(),
                                        first ? nullptr : pc.data(), first ? nullptr : pw.data(), first ? nullptr : pn.data(), out.data(), oa.data(), oc.data(), ow.data(),
                                        on.data()) != ARCTIC_OK)
            return bad(name, "refused");
        for (size_t p = 0; p < n; ++p) {
            const float N = out[4 * p + 3];
            if (N != oc[p]) return bad(name, "the output's count is not the entry's");
            if (!(N == 0.0f || (N >= 1.0f && N <= 4.0f))) return bad(name, "N outside [1, max_history]");
            if (N == 0.0f) for (int a = 0; a < 3; ++a) if (out[4 * p + a] != 0.0f || oa[3 * p + a] != 0.0f || ow[3 * p + a] != 0.0f || on[3 * p + a] != 0.0f) return bad(name, "a pixel that is not covered has an entry");
            if ((cur[4 * p + 3] == 0.0f || !geometry[p]) && N != 0.0f) return bad(name, "a pixel without a ray or without geometry is covered");
            if (first && N > 1.0f) return bad(name, "a first call has a history");
        }
    }
    std::printf("ok %s\n", name.c_str());
}

static void composition() {
    std::mt19937 g(99);
    std::uniform_real_distribution<float> u(0.0f, 4.0f);
    const size_t n = 777;
    std::vector<float> hdr(3 * n), base(3 * n), metal(n), E(4 * n), out(3 * n, -7.0f);
    std::vector<uint8_t> geometry(n);
    for (size_t p = 0; p < n; ++p) {
        for (int a = 0; a < 3; ++a) { hdr[3 * p + a] = u(g); base[3 * p + a] = 0.25f * u(g); E[4 * p + a] = p % 3 == 0 ? q_nan : u(g); }
        metal[p] = 0.25f * u(g); E[4 * p + 3] = p % 3 == 0 ? (p % 2 ? 0.0f : q_nan) : 3.0f; geometry[p] = p % 5 != 0;
    }
    ArcticGiCompose c = {};
    c.gi_strength = 0.7f; c.ambient_scale = 0.25f;
    if (arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), out.data()) != ARCTIC_OK) return bad("composition", "refused");
    for (size_t p = 0; p < 3 * n; ++p) if (out[p] == -7.0f || !std::isfinite(out[p])) return bad("composition", "an entry was not written, or a NaN behind E.a == 0 came through");
    for (size_t p = 0; p < n; ++p) if (!geometry[p] && std::memcmp(&out[3 * p], &hdr[3 * p], 12) != 0) return bad("composition", "a pixel without geometry changed");
    c.gi_strength = 0.0f; c.ambient_scale = 1.0f;
    if (arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), out.data()) != ARCTIC_OK || std::memcmp(out.data(), hdr.data(), 12 * n) != 0)
        return bad("composition", "strength 0 and scale 1 is not the identity");
    std::vector<float> untouched(3 * n, -7.0f);
    int refused = 0;
    c.gi_strength = -1.0f; refused += arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    c.gi_strength = 1.0f; c.ambient_scale = 1.5f; refused += arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    c.ambient_scale = 1.0f; c.flags = 2; refused += arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    c.flags = 0; c.reserved[4] = 1; refused += arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    c.reserved[4] = 0; refused += arctic_gi_compose_pixels(&c, 0.3f, n, hdr.data(), nullptr, metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    refused += arctic_gi_compose_pixels(nullptr, 0.3f, n, hdr.data(), base.data(), metal.data(), E.data(), geometry.data(), untouched.data()) == ARCTIC_E_INVALID;
    ArcticGiHistory h = {};
    h.max_history = 0.5f; h.plane_dist = 0.1f;
    refused += arctic_gi_accumulate_pixels(&h, 1, hdr.data(), hdr.data(), geometry.data(), E.data(), nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr, untouched.data(), nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    h.max_history = 4.0f;
    refused += arctic_gi_accumulate_pixels(&h, 1, hdr.data(), hdr.data(), geometry.data(), E.data(), hdr.data(), 1, 1, nullptr, nullptr, nullptr, nullptr, untouched.data(), nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    refused += arctic_gi_accumulate_pixels(&h, 1, hdr.data(), hdr.data(), geometry.data(), E.data(), nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, untouched.data(), nullptr, nullptr, nullptr, nullptr) == ARCTIC_E_INVALID;
    if (refused != 9) return bad("composition", "a call that had to be refused was not");
    for (float x : untouched) if (x != -7.0f) return bad("composition", "a refused call wrote");
    std::printf("ok composition\n");
}

static void refusals() {
    std::mt19937 g(5);
    const std::vector<float> dirs = table(3, 4, g);
    std::vector<float> pts(12, 1.0f), S(16, -7.0f), E(16, -7.0f), colors(3 * 4 * 4, 1.0f);
    std::vector<uint32_t> sets(2, 0);
    std::vector<ArcticRay> rays(12);
    std::memset(rays.data(), 0xCD, rays.size() * sizeof(ArcticRay));
    const std::vector<ArcticRay> before = rays;
    int refused = 0, tried = 0;
    const auto both = [&](ArcticGi gi, const float *d = nullptr) {
        tried += d ? 1 : 2;
        refused += arctic_gi_points(pts.data(), sets.data(), 2, &gi, d ? d : dirs.data(), 0, rays.data()) == ARCTIC_E_INVALID;
        if (!d) refused += arctic_gi_estimate_pixels(&gi, 2, 2, rays.data(), colors.data(), nullptr, nullptr, nullptr, S.data(), E.data()) == ARCTIC_E_INVALID;
    };
    ArcticGi gi = record(3, 4, 0);
    gi.n_rays = 0; both(gi); gi.n_rays = 17; both(gi); gi = record(3, 4, 0);
    gi.pattern = 3; both(gi); gi = record(3, 4, 0);
    gi.max_distance = 0.0f; both(gi); gi.max_distance = q_nan; both(gi); gi = record(3, 4, 0);
    gi.bias = p_inf; both(gi); gi = record(3, 4, 0);
    gi.clamp_max = 0.0f; both(gi); gi.clamp_max = p_inf; both(gi); gi.clamp_max = q_nan; both(gi); gi = record(3, 4, 0);
    gi.filter = 2; both(gi); gi = record(3, 4, 0);
    gi.reserved[3] = 1; both(gi); gi = record(3, 4, 1);
    gi.normal_cos = q_nan; both(gi); gi = record(3, 4, 1);
    gi.plane_dist = -1.0f; both(gi); gi = record(3, 4, 0);
    std::vector<float> poisoned = dirs;
    poisoned.back() = q_nan;
    both(gi, poisoned.data());   // (the table is arctic_gi_points' alone)
    tried += 6;
    refused += arctic_gi_points(pts.data(), sets.data(), 2, nullptr, dirs.data(), 0, rays.data()) == ARCTIC_E_INVALID;
    refused += arctic_gi_points(pts.data(), sets.data(), 2, &gi, dirs.data(), 3, rays.data()) == ARCTIC_E_INVALID;
    sets[1] = 16;
    refused += arctic_gi_points(pts.data(), sets.data(), 2, &gi, dirs.data(), 0, rays.data()) == ARCTIC_E_INVALID;
    refused += arctic_gi_estimate_pixels(&gi, 0, 2, rays.data(), colors.data(), nullptr, nullptr, nullptr, S.data(), E.data()) == ARCTIC_E_INVALID;
    refused += arctic_gi_estimate_pixels(&gi, 2, 2, rays.data(), nullptr, nullptr, nullptr, nullptr, S.data(), E.data()) == ARCTIC_E_INVALID;
    gi.filter = 1;
    refused += arctic_gi_estimate_pixels(&gi, 2, 2, rays.data(), colors.data(), nullptr, nullptr, nullptr, S.data(), E.data()) == ARCTIC_E_INVALID;
    if (refused != tried) return bad("refusals", "a call that had to be refused was not");
    if (std::memcmp(rays.data(), before.data(), rays.size() * sizeof(ArcticRay)) != 0) return bad("refusals", "a refused call wrote records");
    for (float x : S) if (x != -7.0f) return bad("refusals", "a refused call wrote S");
    for (float x : E) if (x != -7.0f) return bad("refusals", "a refused call wrote E");
    std::printf("ok refusals\n");
}

int main() {
    for (uint32_t P : {1u, 2u, 4u}) for (uint32_t n_rays : {1u, 3u, 16u}) points(n_rays, P);
    const uint32_t sizes[][2] = {{1, 1}, {3, 5}, {13, 11}, {64, 40}};
    for (const auto &wh : sizes) for (uint32_t n_rays : {1u, 3u, 16u}) for (uint32_t P : {1u, 2u, 4u}) for (uint32_t filter : {0u, 1u}) frame(wh[0], wh[1], n_rays, P, filter);
    for (const auto &wh : sizes) for (int which = 0; which < 5; ++which) history(wh[0], wh[1], which);
    composition();
    refusals();
    return failures ? 1 : 0;
}
