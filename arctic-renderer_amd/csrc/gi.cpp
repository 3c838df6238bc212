// gi.cpp -- the host side of the indirect diffuse light (include/arctic_hip.h: arctic_trace_gi): what the entry points refuse, and the arbiters
// arctic_gi_points, arctic_gi_estimate_pixels, arctic_gi_accumulate_pixels and arctic_gi_compose_pixels -- the functions of gi.h, ray_ao.h and
// ao_history.h that gi.hip runs, on the CPU.  No HIP type: it also compiles with a host compiler alone (tests/cpp/gi_sanitize.cpp, next to
// ao_history.cpp, whose refusal of the history's block it shares).
#include "gi.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticGi) == 48 && sizeof(GiDesc) == 48, "ArcticGi");
static_assert(offsetof(ArcticGi, max_distance) == offsetof(GiDesc, max_distance) && offsetof(ArcticGi, clamp_max) == offsetof(GiDesc, clamp_max) &&
              offsetof(ArcticGi, filter) == offsetof(GiDesc, filter) && offsetof(ArcticGi, plane_dist) == offsetof(GiDesc, plane_dist) &&
              offsetof(ArcticGi, reserved) == offsetof(GiDesc, reserved), "the public record is the internal one");
static_assert(sizeof(ArcticRay) == sizeof(RayIn) && sizeof(GiSum) == 16, "the records of the planes");
static_assert(sizeof(ArcticGiHistory) == 32 && sizeof(GiHistoryDesc) == 32, "ArcticGiHistory");
static_assert(offsetof(ArcticGiHistory, max_history) == offsetof(GiHistoryDesc, max_history) && offsetof(ArcticGiHistory, normal_cos) == offsetof(GiHistoryDesc, normal_cos) &&
              offsetof(ArcticGiHistory, plane_dist) == offsetof(GiHistoryDesc, plane_dist) && offsetof(ArcticGiHistory, min_weight) == offsetof(GiHistoryDesc, min_weight) &&
              offsetof(ArcticGiHistory, reserved) == offsetof(GiHistoryDesc, reserved), "the public record is the internal one");
static_assert(sizeof(ArcticGiCompose) == 32 && sizeof(GiComposeDesc) == 32, "ArcticGiCompose");
static_assert(offsetof(ArcticGiCompose, gi_strength) == offsetof(GiComposeDesc, gi_strength) && offsetof(ArcticGiCompose, ambient_scale) == offsetof(GiComposeDesc, ambient_scale) &&
              offsetof(ArcticGiCompose, reserved) == offsetof(GiComposeDesc, reserved), "the public record is the internal one");
static_assert(ARCTIC_GI_SOURCE_COMPOSED == GI_SOURCE_COMPOSED, "the flag");

const char *gi_refusal(const GiDesc *gi, const float *dirs) {
    if (!gi || !dirs) return "null parameters or directions";
    if (gi->n_rays < 1 || gi->n_rays > GI_MAX_RAYS) return "n_rays outside 1..16";
    if (gi->pattern != 1 && gi->pattern != 2 && gi->pattern != 4) return "pattern is not 1, 2 or 4";
    if (!(gi->max_distance > 0.0f)) return "max_distance is not > 0";
    if (!rq_finite(gi->bias)) return "the bias is not finite";
    if (!(gi->clamp_max > 0.0f) || !rq_finite(gi->clamp_max)) return "clamp_max is not > 0 and finite";
    if (gi->filter > 1 || gi->reserved[0] != 0 || gi->reserved[1] != 0 || gi->reserved[2] != 0 || gi->reserved[3] != 0) return "filter above 1 or reserved not 0";
    if (gi->filter && (!rq_finite(gi->normal_cos) || !(gi->plane_dist >= 0.0f))) return "normal_cos is not finite or plane_dist is negative or a NaN";
    const size_t n = (size_t)gi->pattern * gi->pattern * gi->n_rays * 3;
    for (size_t k = 0; k < n; ++k) if (!rq_finite(dirs[k])) return "a direction component is not finite";
    return nullptr;
}

const char *gi_compose_refusal(const GiComposeDesc *d) {
    if (!d) return "null parameters";
    if (d->flags & ~GI_SOURCE_COMPOSED) return "flags have unknown bits";
    if (!(d->gi_strength >= 0.0f) || !rq_finite(d->gi_strength)) return "gi_strength is negative or not finite";
    if (!(d->ambient_scale >= 0.0f && d->ambient_scale <= 1.0f)) return "ambient_scale outside [0, 1]";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3] | d->reserved[4]) return "reserved not 0";
    return nullptr;
}

namespace {
// the previous history as the caller's four row-major arrays
struct GiRowFetch {
    const float *acc3, *count, *world3, *normal3;
    uint32_t width;
    void operator()(uint32_t qx, uint32_t qy, GiHistoryEntry &e) const {
        const size_t q = (size_t)qy * width + qx;
        for (int i = 0; i < 3; ++i) { e.world[i] = world3[3 * q + i]; e.m[i] = normal3[3 * q + i]; e.acc[i] = acc3[3 * q + i]; }
        e.count = count[q];
    }
};
}  // namespace

}  // namespace arctic

extern "C" int arctic_gi_accumulate_pixels(const ArcticGiHistory *hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const float *cur4,
                                           const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_acc3, const float *prev_count,
                                           const float *prev_world3, const float *prev_normal3, float *out4, float *out_acc3, float *out_count, float *out_world3,
                                           float *out_normal3) {
    using namespace arctic;
    GiHistoryDesc d;
    if (hist) std::memcpy(&d, hist, sizeof d);
    if (ao_history_refusal(hist ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (prev_proj_view && (!prev_acc3 || !prev_count || !prev_world3 || !prev_normal3)) return ARCTIC_E_INVALID;
    if (n && (!world3 || !normal3 || !geometry || !cur4 || !out4)) return ARCTIC_E_INVALID;
    const GiRowFetch fetch = {prev_acc3, prev_count, prev_world3, prev_normal3, width};
    for (uint64_t k = 0; k < n; ++k) {
        GiHistoryEntry h;
        const GiSum cur = {cur4[4 * k], cur4[4 * k + 1], cur4[4 * k + 2], cur4[4 * k + 3]};
        const GiSum o = gih_pixel(geometry[k] != 0, normal3 + 3 * k, world3 + 3 * k, cur, prev_proj_view, width, height, d, fetch, h);
        out4[4 * k] = o.r; out4[4 * k + 1] = o.g; out4[4 * k + 2] = o.b; out4[4 * k + 3] = o.cnt;
        if (out_count) out_count[k] = h.count;
        for (int i = 0; i < 3; ++i) {
            if (out_acc3) out_acc3[3 * k + i] = h.acc[i];
            if (out_world3) out_world3[3 * k + i] = h.world[i];
            if (out_normal3) out_normal3[3 * k + i] = h.m[i];
        }
    }
    return ARCTIC_OK;
}

extern "C" int arctic_gi_compose_pixels(const ArcticGiCompose *compose, float ambient, uint64_t n, const float *hdr3, const float *base3, const float *metal,
                                        const float *gi4, const uint8_t *geometry, float *out_hdr3) {
    using namespace arctic;
    GiComposeDesc d;
    if (compose) std::memcpy(&d, compose, sizeof d);
    if (gi_compose_refusal(compose ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (n && (!hdr3 || !base3 || !metal || !gi4 || !geometry || !out_hdr3)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k) {
        float C[3] = {hdr3[3 * k], hdr3[3 * k + 1], hdr3[3 * k + 2]};
        if (geometry[k]) {
            gi_compose_ambient(C, base3 + 3 * k, ambient, d.ambient_scale);
            if (gi_compose_lit(gi4[4 * k + 3])) gi_compose_indirect(C, base3 + 3 * k, metal[k], d.gi_strength, gi4 + 4 * k);
        }
        out_hdr3[3 * k] = C[0]; out_hdr3[3 * k + 1] = C[1]; out_hdr3[3 * k + 2] = C[2];
    }
    return ARCTIC_OK;
}

extern "C" int arctic_gi_points(const float *points6, const uint32_t *sets, uint64_t n_points, const ArcticGi *gi, const float *dirs, uint32_t round, ArcticRay *rays) {
    using namespace arctic;
    GiDesc d;
    if (gi) std::memcpy(&d, gi, sizeof d);
    if (gi_refusal(gi ? &d : nullptr, dirs) || round >= d.n_rays || (n_points && (!points6 || !sets || !rays))) return ARCTIC_E_INVALID;
    const uint32_t n_sets = d.pattern * d.pattern;
    for (uint64_t k = 0; k < n_points; ++k) if (sets[k] >= n_sets) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n_points; ++k) {
        const float *p = points6 + 6 * k;
        RayIn r;
        gi_ray(p, p + 3, true, dirs + ((size_t)sets[k] * d.n_rays + round) * 3, d.bias, d.max_distance, r);
        std::memcpy(rays + k, &r, sizeof r);
    }
    return ARCTIC_OK;
}

extern "C" int arctic_gi_estimate_pixels(const ArcticGi *gi, uint32_t width, uint32_t height, const ArcticRay *rays, const float *colors4, const float *normal3,
                                         const float *world3, const uint8_t *geometry, float *sum4, float *estimate4) {
    using namespace arctic;
    static const float no_dirs[16 * GI_MAX_RAYS * 3] = {};   // (the table plays no part behind the rays: the record is checked against zeros)
    GiDesc d;
    if (gi) std::memcpy(&d, gi, sizeof d);
    if (gi_refusal(gi ? &d : nullptr, no_dirs)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u || !rays || !colors4 || !sum4 || !estimate4) return ARCTIC_E_INVALID;
    if (d.filter && (!normal3 || !world3 || !geometry)) return ARCTIC_E_INVALID;
    const size_t n = (size_t)width * height;
    std::vector<GiSum> S(n);
    for (uint32_t k = 0; k < d.n_rays; ++k) {
        for (size_t p = 0; p < n; ++p) {
            const float *c = colors4 + ((size_t)k * n + p) * 4;
            RayIn r;
            std::memcpy(&r, rays + (size_t)k * n + p, sizeof r);
            S[p] = gi_add(S[p], k == 0, gi_had_ray(r.t_max), c[0], c[1], c[2], d.clamp_max);
        }
    }
    std::vector<GiSum> E(n);
    if (!d.filter) {
        for (size_t p = 0; p < n; ++p) E[p] = gi_estimate(S[p]);
    } else {
        std::vector<float> m(n * 3);
        std::vector<uint8_t> covered(n);
        for (size_t p = 0; p < n; ++p) covered[p] = ao_normal(normal3[3 * p], normal3[3 * p + 1], normal3[3 * p + 2], &m[3 * p]) && geometry[p] != 0;
        const int32_t lo = gi_window_lo(d.pattern);
        for (uint32_t y = 0; y < height; ++y) {
            for (uint32_t x = 0; x < width; ++x) {
                const size_t p = (size_t)y * width + x;
                GiSum acc = {0.0f, 0.0f, 0.0f, 0.0f};
                if (covered[p]) {
                    for (int32_t j = lo; j < lo + (int32_t)d.pattern; ++j) {
                        for (int32_t i = lo; i < lo + (int32_t)d.pattern; ++i) {
                            const int32_t qx = (int32_t)x + i, qy = (int32_t)y + j;
                            bool accept = i == 0 && j == 0;
                            size_t q = p;
                            if (!accept) {
                                if (qx < 0 || qy < 0 || qx >= (int32_t)width || qy >= (int32_t)height) continue;
                                q = (size_t)qy * width + qx;
                                accept = covered[q] && ao_accepts(&m[3 * p], world3 + 3 * p, &m[3 * q], world3 + 3 * q, d.normal_cos, d.plane_dist);
                            }
                            if (accept) acc = GiSum{acc.r + S[q].r, acc.g + S[q].g, acc.b + S[q].b, acc.cnt + S[q].cnt};
                        }
                    }
                }
                E[p] = gi_estimate(acc);
            }
        }
    }
    std::memcpy(sum4, S.data(), n * sizeof(GiSum));
    std::memcpy(estimate4, E.data(), n * sizeof(GiSum));
    return ARCTIC_OK;
}
