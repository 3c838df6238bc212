// post_process.h -- the tonemapper, the gamma curve and the store to the R8G8B8A8_UNORM target (post_process.hlsl:39-93), RESTATED from shade.hip --
// the operations of k_post_process in its order -- because shade.hip stays as it is.  One copy for the streaming kernels that end in the tonemapper:
// k_compose (compose.hip) and k_taa_resolve (taa.hip).  Device only; every function is inlined into its kernel.
#pragma once
#include "common.h"

namespace arctic {

namespace {

// ---- post_process.hlsl:59-93, as shade.hip's k_post_process carries it out ------------------------------------------------------------------------
typedef float v2 __attribute__((ext_vector_type(2)));
typedef float f3v __attribute__((ext_vector_type(3), aligned(4)));
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ float fm(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float sat(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
__device__ __forceinline__ float rrt_odt(float c) {
    const float a = fm(c, c + 0.0245786f, -0.000090537f);
    const float b = fm(c, fm(0.983729f, c, 0.4329510f), 0.238081f);
    return a * rcp(b);
}
// the tonemappers, post_process.hlsl:39-57
__device__ __forceinline__ f3 tonemap(f3 c, int tm, float exposure) {
    f3 t;
    if (tm == 1) {          // tm_exposure: 1 - exp(-c * exposure), the series below 1/64 where the subtraction cancels
        const float LOG2E = 1.4426950408889634f;
        const f3 x = mk(c.x * exposure, c.y * exposure, c.z * exposure);
        auto one_minus_exp = [&](float v) {
            const float direct = 1.0f - __builtin_amdgcn_exp2f(-v * LOG2E);
            const float series = v * fm(v, fm(v, 1.0f / 6.0f, -0.5f), 1.0f);
            return fabsf(v) < 0.015625f ? series : direct;
        };
        t = mk(one_minus_exp(x.x), one_minus_exp(x.y), one_minus_exp(x.z));
    } else if (tm == 2) {   // tm_aces: the input matrix, rrt_and_odt_fit, the output matrix, saturate
        auto pfm = [](v2 a, v2 b, v2 c2) { return __builtin_elementwise_fma(a, b, c2); };
        const v2 cx = {c.x, c.x}, cy = {c.y, c.y}, cz = {c.z, c.z};
        v2 ixy = pfm((v2){0.04823f, 0.01566f}, cz, pfm((v2){0.35458f, 0.90834f}, cy, (v2){0.59719f, 0.07600f} * cx));
        float iz = fm(0.837f, c.z, fm(0.13383f, c.y, 0.02840f * c.x));
        {
            const v2 a = pfm(ixy, ixy + (v2){0.0245786f, 0.0245786f}, (v2){-0.000090537f, -0.000090537f});
            const v2 b = pfm(ixy, pfm((v2){0.983729f, 0.983729f}, ixy, (v2){0.4329510f, 0.4329510f}), (v2){0.238081f, 0.238081f});
            ixy = a * (v2){rcp(b.x), rcp(b.y)};
            iz = rrt_odt(iz);
        }
        const float ox = fm(-0.07367f, iz, fm(-0.53108f, ixy.y, 1.60475f * ixy.x));
        const float oy = fm(-0.00605f, iz, fm(1.10813f, ixy.y, -0.10208f * ixy.x));
        const float oz = fm(1.07f, iz, fm(-0.07276f, ixy.y, -0.00327f * ixy.x));
        t = mk(sat(ox), sat(oy), sat(oz));
    } else {                // tm_reinhard (and `default:`)
        t = mk(c.x * rcp(c.x + 1.0f), c.y * rcp(c.y + 1.0f), c.z * rcp(c.z + 1.0f));
    }
    return t;
}
// correct_gamma: pow(abs(t), 1 / gamma) = exp2(log2|t| / gamma)
__device__ __forceinline__ float gamma_curve(float t, float inv_gamma) { return __builtin_amdgcn_exp2f(inv_gamma * __builtin_amdgcn_logf(fabsf(t))); }
// the store to the R8G8B8A8_UNORM target: saturate (NaN -> 0), * 255, + 0.5, truncate
__device__ __forceinline__ uint32_t unorm8(float x) { return (uint32_t)__builtin_fmaf(sat(x), 255.0f, 0.5f); }

}  // namespace

}  // namespace arctic
