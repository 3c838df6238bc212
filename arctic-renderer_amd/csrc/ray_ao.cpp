// ray_ao.cpp -- the host side of the ambient occlusion (include/arctic_hip.h: arctic_trace_ambient_occlusion): what the entry points refuse, and
// the arbiter arctic_ambient_occlusion_points -- the functions of ray_ao.h and the walk of ray_query.h that ray_ao.hip runs, on the CPU, or
// the loop over every triangle.  No HIP type: it also compiles with a host compiler alone (tests/cpp/ao_sanitize.cpp).
#include "ray_ao.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticAmbientOcclusion) == 32 && sizeof(AoDesc) == 32, "ArcticAmbientOcclusion");
static_assert(offsetof(ArcticAmbientOcclusion, radius) == offsetof(AoDesc, radius) && offsetof(ArcticAmbientOcclusion, filter) == offsetof(AoDesc, filter) &&
              offsetof(ArcticAmbientOcclusion, plane_dist) == offsetof(AoDesc, plane_dist) && offsetof(ArcticAmbientOcclusion, reserved) == offsetof(AoDesc, reserved), "the public record is the internal one");

const char *ao_refusal(const AoDesc *ao, const float *dirs) {
    if (!ao || !dirs) return "null parameters or directions";
    if (ao->n_rays < 1 || ao->n_rays > AO_MAX_RAYS) return "n_rays outside 1..64";
    if (ao->pattern != 1 && ao->pattern != 2 && ao->pattern != 4) return "pattern is not 1, 2 or 4";
    if (!(ao->radius > 0.0f)) return "radius is not > 0";
    if (!rq_finite(ao->bias)) return "the bias is not finite";
    if (ao->filter > 1 || ao->reserved != 0) return "filter above 1 or reserved not 0";
    if (ao->filter && (!rq_finite(ao->normal_cos) || !(ao->plane_dist >= 0.0f))) return "normal_cos is not finite or plane_dist is negative or a NaN";
    const size_t n = (size_t)ao->pattern * ao->pattern * ao->n_rays * 3;
    for (size_t k = 0; k < n; ++k) if (!rq_finite(dirs[k])) return "a direction component is not finite";
    return nullptr;
}

}  // namespace arctic

extern "C" int arctic_ambient_occlusion_points(const float *tris9, uint64_t n_tris, const float *points6, const uint32_t *sets, uint64_t n_points,
                                               const ArcticAmbientOcclusion *ao, const float *dirs, uint32_t flags, uint8_t *hits) {
    using namespace arctic;
    AoDesc d;
    if (ao) std::memcpy(&d, ao, sizeof d);
    if (ao_refusal(ao ? &d : nullptr, dirs) || (flags & ~ARCTIC_TRACE_BRUTE) || (n_tris && !tris9) || (n_points && (!points6 || !sets || !hits))) return ARCTIC_E_INVALID;
    if (n_tris > 0xFFFFFFFEull) return ARCTIC_E_CAPACITY;
    const uint32_t n_sets = d.pattern * d.pattern;
    for (uint64_t k = 0; k < n_points; ++k) if (sets[k] >= n_sets) return ARCTIC_E_INVALID;
    Bvh b;
    if (!(flags & ARCTIC_TRACE_BRUTE)) {
        if (!bvh_build(tris9, n_tris, nullptr, b)) return ARCTIC_E_CAPACITY;
        if (!bvh_validate(b)) return ARCTIC_E_INVALID;
    }
    std::vector<RayIn> rays(d.n_rays);
    std::vector<RayOut> out(d.n_rays);
    for (uint64_t k = 0; k < n_points; ++k) {
        const float *p = points6 + 6 * k;
        float m[3], t[3], bt[3], o[3];
        uint32_t n_hit = 0;
        if (ao_normal(p[3], p[4], p[5], m)) {
            ao_frame(m, t, bt);
            ao_origin(p, m, d.bias, o);
            for (uint32_t j = 0; j < d.n_rays; ++j) rays[j] = ao_ray(o, m, t, bt, dirs + ((size_t)sets[k] * d.n_rays + j) * 3, d.radius);
            if (flags & ARCTIC_TRACE_BRUTE) brute_trace_host(tris9, n_tris, rays.data(), d.n_rays, true, out.data());
            else bvh_trace_host(b, rays.data(), d.n_rays, true, out.data(), nullptr);
            for (uint32_t j = 0; j < d.n_rays; ++j) n_hit += out[j].prim != RAY_NO_PRIM;
        }
        hits[k] = (uint8_t)n_hit;
    }
    return ARCTIC_OK;
}
