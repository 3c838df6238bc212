// hit_shade.h -- the launchers of hit_shade.hip (arctic_hit_attributes, arctic_shade_hits, arctic_trace_reflections: include/arctic_hip.h).
// Every launcher enqueues on `s` and returns the launch error, never synchronises.  Device compilation only (renderer.cpp, hit_shade.hip).
#pragma once
#include "common.h"
#include "hit_attributes.h"

namespace arctic {

// n hit records (16 bytes each) -> 18 floats and a material per hit.  src: n_prims records; objs: the scene's objects; lpv: the sun's matrix.  n < 2^32
hipError_t launch_hit_attributes(const void *hits, uint64_t n, const HitSource *src, uint32_t n_prims, const HitObject *objs, const float *lpv, float *attrs,
                                 uint32_t *material, hipStream_t s);

// what k_shade_hits reads besides the rays and their hits: the handle's images, sun map, lights and environment map as they stand
struct HitShadeParams {
    const HitSource *src; const HitObject *objs;
    const TexDesc *tex; const float *srgb_lut;          // 3 descriptors per material (level 0 of a chain is descriptor 3 m itself); 256 floats
    const float *shadow_map; const float4 *lights;      // S * S floats row-major, or null; 2 float4 per light, caller order
    const float4 *env;                                  // RGBA32F equirect, row-major, or null
    uint32_t n_prims, shadow_size, n_lights, env_w, env_h;
    float ambient, sun_dir[3], sun_color[3];
    float lpv[16];
};
// rays[k], hits[k] -> out[k] = {r, g, b, a}; all three 16-byte aligned, n < 2^32
hipError_t launch_shade_hits(const void *rays, const void *hits, uint64_t n, const HitShadeParams &p, float4 *out, hipStream_t s);
// the reflection ray of every pixel of the handle's rows (row-major, rows * width records of 32 bytes) from G-buffer planes b, c, e; a pixel
// without a ray gets the all-zero record
hipError_t launch_reflect_rays(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                               uint32_t row0_in_tile, const float eye[3], float bias, void *rays, hipStream_t s);

}  // namespace arctic
