// hit_attributes.cpp -- the host side of the hit attributes (include/arctic_hip.h: arctic_hit_attributes): the prim-indexed source table and the
// arbiter arctic_interpolate_hits -- the functions of hit_attributes.h that hit_shade.hip runs, on the CPU.  No HIP type: it also compiles with a
// host compiler alone (tests/cpp/hit_attributes_sanitize.cpp).
#include "hit_attributes.h"
#include "../../include/arctic_hip.h"

namespace arctic {

static_assert(sizeof(ArcticHit) == sizeof(RayOut) && sizeof(ArcticVertex) == 14 * sizeof(float), "the public records are the internal ones");

void hit_triangle_sources(uint32_t object, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, std::vector<HitSource> &out) {
    for (uint32_t t = 0; t < n_triangles; ++t) {
        const uint32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
        const bool ok = i0 < n_vertices && i1 < n_vertices && i2 < n_vertices;
        out.push_back(ok ? HitSource{object, i0, i1, i2} : HitSource{HIT_NO_OBJECT, 0u, 0u, 0u});
    }
}

}  // namespace arctic

extern "C" int arctic_interpolate_hits(const ArcticVertex *vertices, uint64_t n_vertices, const uint32_t *indices, uint64_t n_indices, const float *trs,
                                       const float *light_proj_view, uint32_t material, uint64_t first_prim, const ArcticHit *hits, uint64_t n, float *attrs,
                                       uint32_t *material_out) {
    using namespace arctic;
    if ((n_vertices && !vertices) || (n_indices && !indices) || !trs || !light_proj_view || (n && (!hits || !attrs || !material_out))) return ARCTIC_E_INVALID;
    const uint64_t n_triangles = n_indices / 3;
    if (n_vertices > 0xFFFFFFFFull || first_prim + n_triangles > 0xFFFFFFFEull) return ARCTIC_E_CAPACITY;
    const float *v14 = reinterpret_cast<const float *>(vertices);
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t prim = hits[k].prim;
        if (prim == RAY_NO_PRIM || prim < first_prim || prim - first_prim >= n_triangles) continue;   // another object's, or nobody's: left as it is
        const uint32_t *ix = indices + 3 * (size_t)(prim - first_prim);
        float *out = attrs + HIT_ATTRS * k;
        if (ix[0] < n_vertices && ix[1] < n_vertices && ix[2] < n_vertices) {
            ha_hit(HitSource{0u, ix[0], ix[1], ix[2]}, trs, v14, light_proj_view, hits[k].u, hits[k].v, out);
            material_out[k] = material;
        } else {
            for (uint32_t j = 0; j < HIT_ATTRS; ++j) out[j] = 0.0f;
            material_out[k] = HIT_NO_MATERIAL;
        }
    }
    return ARCTIC_OK;
}
