// hit_shade_device.h -- what the hit kernels of hit_shade.hip (k_hit_attributes, k_shade_hits) and hit_shade_ext.hip (k_shade_hits_ext) share: a hit's
// source and attributes, calculate_shadow on the sun's map, the BRDF one light at a time, the environment map along a ray.  ONE copy of each, so
// that the two shading kernels round alike wherever they do the same thing.  Device compilation only; compile with contraction off.
#pragma once
#include "hit_shade.h"
#include "ray_ao.h"
#include "material_sampler.h"

namespace arctic {

namespace {

constexpr uint32_t HIT_THREADS = 256;
constexpr uint32_t HIT_MAX_BLOCKS = 256 * 8;   // the grid-stride loops' grid: 8 workgroups per CU of the largest part

// the source of a hit, or false: a miss, a prim the scene does not have, the triangle with an index out of range.  Every index the kernels follow
// was checked by the host when it built the table (object < the scene's objects, i0..i2 < the mesh's vertex count)
__device__ __forceinline__ bool hit_source(const RayOut &h, const HitSource *__restrict__ src, uint32_t n_prims, HitSource &s) {
    if (h.prim >= n_prims) return false;   // (RAY_NO_PRIM included: n_prims <= 2^32 - 2)
    const rq_f4 raw = *reinterpret_cast<const rq_f4 *>(src + h.prim);
    s.object = rq_bits(raw[0]); s.i0 = rq_bits(raw[1]); s.i1 = rq_bits(raw[2]); s.i2 = rq_bits(raw[3]);
    return s.object != HIT_NO_OBJECT;
}

__device__ __forceinline__ uint32_t hit_attributes(const RayOut &h, const HitSource *__restrict__ src, uint32_t n_prims, const HitObject *__restrict__ objs,
                                                   const float *lpv, float *out) {
    HitSource s;
    if (!hit_source(h, src, n_prims, s)) {
#pragma unroll
        for (uint32_t k = 0; k < HIT_ATTRS; ++k) out[k] = 0.0f;
        return HIT_NO_MATERIAL;
    }
    const HitObject &o = objs[s.object];
    float trs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) trs[k] = o.trs[k];
    ha_hit(s, trs, o.vertices, lpv, h.u, h.v, out);
    return o.material;
}

__device__ __forceinline__ RayOut load_hit(const RayOut *__restrict__ hits, uint64_t k) {
    const rq_f4 raw = *reinterpret_cast<const rq_f4 *>(hits + k);
    const RayOut h = {raw[0], raw[1], raw[2], rq_bits(raw[3])};
    return h;
}

// ---- the sampler: material_sampler.h (shared with compose.hip) -------------------------------------------------------------------------------

// ---- calculate_shadow (forward.hlsl:68-96): 5 x 5 taps, each a bilinear fetch of the R32 map under WRAP; the oracle's operations in its order ----
__device__ __forceinline__ void hs_wrap_axis(float u, uint32_t n, int &i0, int &i1, float &f) {
    const float uw = u - floorf(u);
    const float x = uw * (float)n - 0.5f;
    const float xf = floorf(x);
    f = x - xf;
    i0 = min(max((int)xf, -1), (int)n - 1);   // (as hs_axis: a no-op for a coordinate that is a number)
    i1 = i0 + 1;
    i0 = i0 < 0 ? (int)n - 1 : i0;
    i1 = i1 == (int)n ? 0 : i1;
}
__device__ __forceinline__ float hs_lerp(float a, float b, float t) { return __builtin_fmaf(t, b - a, a); }
__device__ __forceinline__ float hit_shadow(const float *__restrict__ map, uint32_t S, const float *ls) {
    if (map == nullptr || S == 0u) return 0.0f;
    float px = ls[0] / ls[3], py = ls[1] / ls[3];
    const float pz = ls[2] / ls[3];
    px = px * 0.5f + 0.5f;
    py = py * 0.5f + 0.5f;
    py = 1.0f - py;
    if (pz > 1.0f || px < 0.0f || py < 0.0f || px > 1.0f || py > 1.0f) return 0.0f;
    float shadow = 0.0f;
    for (int i = -2; i <= 2; ++i) {
        int x0, x1;
        float fx;
        hs_wrap_axis(px + (float)i * 0.0001f, S, x0, x1, fx);
        for (int j = -2; j <= 2; ++j) {
            int y0, y1;
            float fy;
            hs_wrap_axis(py + (float)j * 0.0001f, S, y0, y1, fy);
            const float *r0 = map + (size_t)y0 * S, *r1 = map + (size_t)y1 * S;
            const float top = hs_lerp(r0[x0], r0[x1], fx), bot = hs_lerp(r1[x0], r1[x1], fx);
            shadow += pz > hs_lerp(top, bot, fy) ? 1.0f : 0.0f;
        }
    }
    return shadow / 25.0f;
}

// ---- the BRDF (forward.hlsl:126-193), one light at a time --------------------------------------------------------------------------------
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 normalize(f3 v) { return v * (1.0f / __builtin_sqrtf(dot(v, v))); }
constexpr float HS_PI = 3.14159265f;   // PI as written at forward.hlsl:1
// 2 s / 255 - 1 for a normal-map channel s on the 0..255 scale, 2 / 255 carried as two floats (the fp32 constant alone tilts every normal by 1e-7)
__device__ __forceinline__ float hs_snorm(float s) {
    constexpr float HI = 0x1.010102p-7f, LO = -0x1.fdfdfep-32f;
    return __builtin_fmaf(s, LO, __builtin_fmaf(s, HI, -1.0f));
}
// what the light loop needs of a hit, everything that does not depend on the light taken out of it (as shade.hip does for a pixel):
//   kdb = (1 - metal) base / PI,   num = a2 g1(n.wo) / PI with g1(x) = x / (x (1 - k) + k),   omk = 1 - k,   four_ndwo = 4 n.wo
struct Surface { f3 n, wo, F0, kdb; float a2, k, omk, num, four_ndwo; };
// calculate_outgoing_radiance for unit wi and radiance Li:  ((1 - F) kdb + spec F) Li n.wi  with
//   spec = D G / (4 n.wo n.wi + 1e-4) = num n.wi / (dd^2 (n.wi (1 - k) + k) (4 n.wo n.wi + 1e-4))       -- ONE division per light.
// Conditioning as in shade.hip, which the HLSL's own order does not have in fp32: the GGX denominator n.h^2 (a2 - 1) + 1 as dd = sin^2 (1 - a2) + a2
// with sin^2 from e = n - h / |h| (no cancellation at a highlight), and Schlick's 1 - h.wo as 1 - |h| / 2 for unit wo, wi.  (Where n.h <= 0 the
// HLSL clamps it, but then n.wo or n.wi is clamped to 0 and so is G.)  1 / |h| is the IEEE one: e is a small difference of unit vectors.
__device__ __forceinline__ f3 hs_radiance(const Surface &s, f3 wi, f3 Li) {
    const f3 h = s.wo + wi;
    const float hh = dot(h, h), rh = 1.0f / __builtin_sqrtf(hh);
    const float m = 1.0f - 0.5f * (hh * rh), m2 = m * m, p5 = (m2 * m2) * m;
    const f3 e = s.n - h * rh;
    const float e2 = dot(e, e), sin2 = e2 * (1.0f - 0.25f * e2);
    const float dd = sin2 * (1.0f - s.a2) + s.a2;
    const float ndwi = fmaxf(dot(s.n, wi), 0.0f);
    const float den = (dd * dd) * ((ndwi * s.omk + s.k) * (s.four_ndwo * ndwi + 0.0001f));
    const float sp = (s.num * ndwi) * __builtin_amdgcn_rcpf(den);   // (1 ulp: the bar is 1e-4)
    const f3 F = mk(s.F0.x + (1.0f - s.F0.x) * p5, s.F0.y + (1.0f - s.F0.y) * p5, s.F0.z + (1.0f - s.F0.z) * p5);
    return mk(((1.0f - F.x) * s.kdb.x + sp * F.x) * (Li.x * ndwi), ((1.0f - F.y) * s.kdb.y + sp * F.y) * (Li.y * ndwi),
              ((1.0f - F.z) * s.kdb.z + sp * F.z) * (Li.z * ndwi));
}

// ---- the environment map along a ray (skybox.hlsl:61-90; shade.hip: sample_environment): level 0, bilinear, WRAP.  The lookup coordinates are
// computed in float64: they feed a bilinear filter over an HDR image whose texel-to-texel contrast can be thousands
__device__ __forceinline__ void hs_wrap_axis64(double u, uint32_t n, int &i0, int &i1, float &f) {
    const double uw = u - floor(u);
    const double x = uw * (double)n - 0.5;
    const double xf = floor(x);
    f = (float)(x - xf);
    i0 = min(max((int)xf, -1), (int)n - 1);
    i1 = i0 + 1;
    if (i0 < 0) i0 += (int)n;
    if (i1 >= (int)n) i1 -= (int)n;
}
__device__ __forceinline__ f3 hit_environment(const float4 *__restrict__ env, uint32_t w, uint32_t h, const float *d) {
    double x = d[0], y = d[1], z = d[2];
    const double inv = 1.0 / sqrt((x * x + y * y) + z * z);
    x *= inv; y *= inv; z *= inv;
    const double u = atan2(z, x) * (double)0.1591f + 0.5;
    const double v = -(asin(fmin(fmax(y, -1.0), 1.0)) * (double)0.3183f + 0.5);
    int x0, x1, y0, y1;
    float fx, fy;
    hs_wrap_axis64(u, w, x0, x1, fx);
    hs_wrap_axis64(v, h, y0, y1, fy);
    const float4 a = env[(size_t)y0 * w + x0], b = env[(size_t)y0 * w + x1], c = env[(size_t)y1 * w + x0], e = env[(size_t)y1 * w + x1];
    const Weights k = hs_weights(fx, fy);
    return mk(hs_filter(k, a.x, b.x, c.x, e.x), hs_filter(k, a.y, b.y, c.y, e.y), hs_filter(k, a.z, b.z, c.z, e.z));
}

inline uint32_t hit_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + HIT_THREADS - 1) / HIT_THREADS, HIT_MAX_BLOCKS); }

}  // namespace

}  // namespace arctic
