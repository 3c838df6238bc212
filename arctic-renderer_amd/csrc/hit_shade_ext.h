// hit_shade_ext.h -- the launcher of hit_shade_ext.hip: k_shade_hits_ext, the hit shading of ARCTIC_OPT_HIT_MODEL = 1 (include/arctic_hip.h in front of
// arctic_shade_hits).  Enqueues on `s` and returns the launch error, never synchronises.  Device compilation only (ray_calls.cpp, hit_shade_ext.hip).
#pragma once
#include "hit_shade.h"

namespace arctic {

// k_shade_hits' block, and behind it what the forward pass has gained since: the handle's tables as they stand.  An empty list is a null pointer and a
// count of zero; a null `extras` or `env_tables` leaves that feature out
struct HitShadeExtParams {
    HitShadeParams base;
    const float4 *spots;            // n_spots x SPOT_F4 float4 (common.h SpotDev), caller order
    const float4 *cubes;            // n_cubes x CUBE_F4 float4 (common.h CubeDev), then n_cubes x 6 faces of cube_size^2 floats
    const TexDesc *extras;          // base.tex + 3 n_materials: one MaterialExtra per material (has_extras()), or null
    const EnvTables *env_tables;    // image-based ambient (env_active()), or null
    uint32_t n_spots, n_cubes, cube_size, pad;
};
// rays[k], hits[k] -> out[k] = {r, g, b, a}; all three 16-byte aligned, n < 2^32
hipError_t launch_shade_hits_ext(const void *rays, const void *hits, uint64_t n, const HitShadeExtParams &p, float4 *out, hipStream_t s);

}  // namespace arctic
