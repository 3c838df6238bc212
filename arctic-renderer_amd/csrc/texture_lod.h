// texture_lod.h -- the per-pixel level of detail of ARCTIC_OPT_TEXTURE_MIPS (semantics: include/arctic_hip.h next to the option).
// ONE definition for the two places that know a pixel's triangle -- k_resolve_lod (geometry.hip: the G-buffer path's plane) and the walk
// over the visibility plane (shade.hip: k_miplit_vis) -- so that the two paths stay bit-identical.  Both files are compiled with fp
// contraction off; every operation below rounds once, in this order.
#pragma once
#include "common.h"
#include "edges.h"

namespace arctic {

// what a lane needs of its material: level-0 size and the last level of its chain; false (one level: lambda = 0) for materials without a
// chain -- plain ones, and packed ones created with the option off (common.h: the MipTable in descriptor 3 m + 1)
__device__ __forceinline__ bool lod_material(const TexDesc *tex, uint32_t mat, float &wf, float &hf, float &last_level) {
    const TexDesc &d0 = tex[3 * mat], &d1 = tex[3 * mat + 1];
    if (!(d0.w & TEX_INTERLEAVED) || (d1.w & TEX_INTERLEAVED)) return false;
    wf = d0.wf; hf = d0.hf; last_level = (float)(d1.w - 1u);
    return true;
}

// lambda from the texture coordinates at (px, py), (px + 1, py), (px, py + 1): rho^2 = the longer of the two pixel steps in texels, squared;
// lambda = log2(rho) clamped to [0, last_level], a NaN giving 0.  (v_log_f32: one instruction, ~1 ulp, the same bits in both kernels.)
__device__ __forceinline__ float lod_from_uv(float u00, float v00, float u10, float v10, float u01, float v01, float wf, float hf, float last_level) {
#pragma clang fp contract(off)
    const float dux = wf * (u10 - u00), dvx = hf * (v10 - v00), duy = wf * (u01 - u00), dvy = hf * (v01 - v00);
    const float rx = dux * dux + dvx * dvx, ry = duy * duy + dvy * dvy;
    const float rho2 = rx > ry ? rx : ry;
    const float lambda = 0.5f * __builtin_amdgcn_logf(rho2);
    if (!(rx == rx) || !(ry == ry) || !(lambda > 0.0f)) return 0.0f;
    return lambda < last_level ? lambda : last_level;
}

// the whole of it for a covered pixel (px, py) of set-up record t: the record's own interpolation evaluated one pixel to the right and one
// down, extrapolating past the triangle's edge (what a GPU's helper lanes do -- not a difference across lanes, which would mix triangles at
// every silhouette).  uv00: the value interpolated for the pixel itself.
__device__ __forceinline__ float pixel_lod(const SetupRec &t, const RasterRec &q, int32_t px, int32_t py, const float *A0, const float *A1, const float *A2,
                                           float u00, float v00, float wf, float hf, float last_level) {
    float Bx[3], By[3];
    source_barycentrics(t, q, px + 1, py, Bx);
    source_barycentrics(t, q, px, py + 1, By);
    return lod_from_uv(u00, v00, interpolate_attr(Bx, A0, A1, A2, 0), interpolate_attr(Bx, A0, A1, A2, 1),
                       interpolate_attr(By, A0, A1, A2, 0), interpolate_attr(By, A0, A1, A2, 1), wf, hf, last_level);
}

}  // namespace arctic
