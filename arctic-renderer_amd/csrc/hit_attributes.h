// hit_attributes.h -- the interpolated VSOut at a ray hit (include/arctic_hip.h: arctic_hit_attributes and the text in front of it, which is the
// definition; nothing here restates it, it only carries it out).  ONE copy of the per-vertex arithmetic and of the interpolation, compiled for the
// host (hit_attributes.cpp: the arbiter arctic_interpolate_hits, the source table) and for the device (hit_shade.hip: k_hit_attributes,
// k_shade_hits), both with contraction off.  Plain C++ like ray_query.h, whose records and helpers it uses.
#pragma once
#include "ray_query.h"

namespace arctic {

constexpr uint32_t HIT_ATTRS = 18;                  // uv2, t3, b3, n3, world3, light_space4: arctic_read_gbuffer's order
constexpr uint32_t HIT_NO_MATERIAL = 0xFFFFFFFFu;   // a miss, a prim the scene does not have, a skipped triangle
constexpr uint32_t HIT_NO_OBJECT = 0xFFFFFFFFu;

// Where a PRIM's vertices come from: the object (the scene's objects order) and the three vertex indices of its mesh -- or object = HIT_NO_OBJECT
// for the triangle with an index out of range, which is skipped but numbered.  Indexed by prim (the refit's RefitSource table is indexed by slot)
struct alignas(16) HitSource { uint32_t object, i0, i1, i2; };
// what a call uploads per object: its trs, the mesh's vertices in use (14 floats per vertex) and the mesh's material
struct alignas(16) HitObject { float trs[16]; const float *vertices; uint32_t n_vertices, material; };
static_assert(sizeof(HitSource) == 16 && sizeof(HitObject) == 80, "hit attribute records");

// k_vertex's product (geometry.hip: mat_vec), all four rows
RQ_HD void ha_mat_vec(const float *m, float x, float y, float z, float w, float *o) {
    for (int i = 0; i < 4; ++i) o[i] = ((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i] * w;
}
RQ_HD void ha_normalize3(const float *v, float *o) {
    const float inv = 1.0f / __builtin_sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o[0] = v[0] * inv; o[1] = v[1] * inv; o[2] = v[2] * inv;
}
// one vertex (14 floats: position, normal, tangent, bitangent, uv) -> the 18 attributes k_vertex writes for it
RQ_HD void ha_vertex(const float *trs, const float *light_proj_view, const float *s, float *a) {
    float world[4], ls[4];
    ha_mat_vec(trs, s[0], s[1], s[2], 1.0f, world);
    ha_mat_vec(light_proj_view, world[0], world[1], world[2], world[3], ls);
    a[0] = s[12]; a[1] = s[13];
    ha_normalize3(s + 6, a + 2);
    ha_normalize3(s + 9, a + 5);
    ha_normalize3(s + 3, a + 8);
    a[11] = world[0]; a[12] = world[1]; a[13] = world[2];
    a[14] = ls[0]; a[15] = ls[1]; a[16] = ls[2]; a[17] = ls[3];
}
// the interpolation: u and v as given
RQ_HD void ha_interpolate(const float *a0, const float *a1, const float *a2, float u, float v, float *out) {
    const float w0 = (1.0f - u) - v;
    for (uint32_t k = 0; k < HIT_ATTRS; ++k) out[k] = (w0 * a0[k] + u * a1[k]) + v * a2[k];
}
// a resolved hit: its source record and object -> the 18 attributes
RQ_HD void ha_hit(const HitSource &s, const float *trs, const float *vertices, const float *light_proj_view, float u, float v, float *out) {
    float a0[HIT_ATTRS], a1[HIT_ATTRS], a2[HIT_ATTRS];
    ha_vertex(trs, light_proj_view, vertices + (size_t)s.i0 * 14, a0);
    ha_vertex(trs, light_proj_view, vertices + (size_t)s.i1 * 14, a1);
    ha_vertex(trs, light_proj_view, vertices + (size_t)s.i2 * 14, a2);
    ha_interpolate(a0, a1, a2, u, v, out);
}

// The reflection ray of a G-buffer pixel (arctic_trace_reflections): m = the unit normal (ray_ao.h: ao_normal), i = world - eye.  false: the surface
// faces away (k >= 0), no ray
RQ_HD bool ha_reflect(const float *world, const float *m, const float *eye, float bias, RayIn &r) {
    const float i[3] = {world[0] - eye[0], world[1] - eye[1], world[2] - eye[2]};
    const float k = (m[0] * i[0] + m[1] * i[1]) + m[2] * i[2];
    if (k >= 0.0f) return false;
    for (int j = 0; j < 3; ++j) { r.d[j] = i[j] - (2.0f * k) * m[j]; r.o[j] = world[j] + bias * m[j]; }
    r.t_min = 0.0f; r.t_max = rq_inf();
    return true;
}

// ---- host side (hit_attributes.cpp) ----------------------------------------------------------------------------------------------------------
// one object's part of the prim-indexed table, appended: n_triangles records, HIT_NO_OBJECT where an index is out of range
void hit_triangle_sources(uint32_t object, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, std::vector<HitSource> &out);


}  // namespace arctic
