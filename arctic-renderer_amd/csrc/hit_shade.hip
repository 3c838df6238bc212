// hit_shade.hip -- what is AT a ray hit, and what colour it has (arctic_hit_attributes, arctic_shade_hits, arctic_trace_reflections; the
// arithmetic of the attributes and of the reflection ray is written once, in include/arctic_hip.h in front of the calls, and carried out by
// hit_attributes.h -- the very functions the host arbiter arctic_interpolate_hits runs):
//   k_hit_attributes   one hit per lane, grid-stride over n: prim -> source record -> object record -> three vertices of 14 floats -> the 18
//                      attributes k_vertex writes for each -> the interpolation
//   k_shade_hits       the same attributes, then ps_main (forward.hlsl:208-235) on them with eye = the ray's origin: the material's level 0
//                      under the default sampler, the 25 taps of calculate_shadow on the sun's map, the sun and the point lights in a plain
//                      fp32 loop; then, in a second loop over the same rays, a miss takes the environment map along the ray
//   k_reflect_rays     G-buffer planes b, c, e -> one reflection ray per pixel of the handle's rows; a wave is one 8x8 tile as in k_trace_ao
// Everything a lane reads after its hit record depends on the prim, which diverges across a wave: source record, object record, vertices,
// texture descriptors and texels are gathered with vector loads, per lane (a scatter / gather kernel: no waterfall over a wave's materials,
// whose 64 lanes may hold 64 of them).  The sampler (material_sampler.h) and the BRDF are RESTATED, for one pixel at a time and without shade.hip's tile
// machinery; the sun map's taps are calculate_shadow's operations in the oracle's order (a flipped compare is 1/25 of the sun).
// No LDS, no barrier, no atomics; vector stores only.  Compiled with contraction off: every operation of the definitions rounds once, and a
// fused multiply-add appears only where it is written.
#include "hit_shade.h"
#include "ray_ao.h"
#include "material_sampler.h"

namespace arctic {

namespace {

constexpr uint32_t HIT_THREADS = 256;
constexpr uint32_t HIT_MAX_BLOCKS = 256 * 8;   // the grid-stride loops' grid: 8 workgroups per CU of the largest part

struct LightMatrix { float m[16]; };

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

__global__ __launch_bounds__(HIT_THREADS) void k_hit_attributes(const RayOut *__restrict__ hits, uint32_t n, const HitSource *__restrict__ src, uint32_t n_prims,
                                                                const HitObject *__restrict__ objs, const LightMatrix lpv, float *__restrict__ attrs,
                                                                uint32_t *__restrict__ material) {
    for (uint64_t k = (uint64_t)blockIdx.x * HIT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * HIT_THREADS) {
        float a[HIT_ATTRS];
        const uint32_t mat = hit_attributes(load_hit(hits, k), src, n_prims, objs, lpv.m, a);
        float2 *out = reinterpret_cast<float2 *>(attrs + k * HIT_ATTRS);   // 72 bytes per hit: 8-byte aligned
#pragma unroll
        for (uint32_t j = 0; j < HIT_ATTRS / 2; ++j) out[j] = make_float2(a[2 * j], a[2 * j + 1]);
        material[k] = mat;
    }
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

// Two grid-stride loops, a lane taking the same rays in both: the hits, then the sky along the misses.  In ONE loop the sky's binary64 lookup
// cost the kernel 193 VGPRs and 2 waves per SIMD (its constants live across the hit path); as a function of its own it cost a stack frame.  Apart,
// each loop has its own registers: the larger of the two, no call, no scratch
__global__ __launch_bounds__(HIT_THREADS) void k_shade_hits(const RayIn *__restrict__ rays, const RayOut *__restrict__ hits, uint32_t n, const HitShadeParams p,
                                                            float4 *__restrict__ out) {
    for (uint64_t k = (uint64_t)blockIdx.x * HIT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * HIT_THREADS) {
        const rq_f4 ro = *reinterpret_cast<const rq_f4 *>(rays + k);   // {origin, t_min}
        float a[HIT_ATTRS];
        const uint32_t mat = hit_attributes(load_hit(hits, k), p.src, p.n_prims, p.objs, p.lpv, a);
        float4 color = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mat != HIT_NO_MATERIAL) {
            const Channels c = sample_material(p.tex, p.srgb_lut, mat, a[0], a[1]);
            Surface s;
            // get_normal (forward.hlsl:104-111): rgb with g -> 1 - g, * 2 - 1, through the tangent frame (columns t, b, n), normalised
            const float tr = hs_snorm(c.nrm[0]), tg = -hs_snorm(c.nrm[1]), tb = hs_snorm(c.nrm[2]);
            s.n = normalize(mk((a[2] * tr + a[5] * tg) + a[8] * tb, (a[3] * tr + a[6] * tg) + a[9] * tb, (a[4] * tr + a[7] * tg) + a[10] * tb));
            const f3 world = mk(a[11], a[12], a[13]);
            s.wo = normalize(mk(ro[0], ro[1], ro[2]) - world);
            const f3 base = mk(c.base[0], c.base[1], c.base[2]);
            s.F0 = mk(0.04f + (base.x - 0.04f) * c.metal, 0.04f + (base.y - 0.04f) * c.metal, 0.04f + (base.z - 0.04f) * c.metal);
            s.kdb = base * ((1.0f - c.metal) / HS_PI);
            const float al = c.rough * c.rough, r1 = c.rough + 1.0f, ndwo = fmaxf(dot(s.n, s.wo), 0.0f);
            s.a2 = al * al;
            s.k = (r1 * r1) * 0.125f;
            s.omk = 1.0f - s.k;
            s.num = (s.a2 / HS_PI) * (ndwo / (ndwo * s.omk + s.k));
            s.four_ndwo = 4.0f * ndwo;
            const float lit = 1.0f - hit_shadow(p.shadow_map, p.shadow_size, a + 14);
            f3 Lo = mk(0.0f, 0.0f, 0.0f);
            if (lit != 0.0f) {   // all 25 taps shadowed: Lo is multiplied by zero, the hit is ambient * base (the shading pass's exact culling)
                Lo = hs_radiance(s, mk(-p.sun_dir[0], -p.sun_dir[1], -p.sun_dir[2]), mk(p.sun_color[0], p.sun_color[1], p.sun_color[2]));
                for (uint32_t i = 0; i < p.n_lights; ++i) {
                    const float4 lp = p.lights[2 * i], lc = p.lights[2 * i + 1];
                    const f3 d = mk(lp.x, lp.y, lp.z) - world;
                    const float inv = __builtin_amdgcn_rsqf(dot(d, d)), inv2 = inv * inv;   // wi = d / |d|, radiance = colour / |d|^2
                    Lo = Lo + hs_radiance(s, d * inv, mk(lc.x * inv2, lc.y * inv2, lc.z * inv2));
                }
            }
            color = make_float4(Lo.x * lit + p.ambient * base.x, Lo.y * lit + p.ambient * base.y, Lo.z * lit + p.ambient * base.z, 1.0f);
        }
        out[k] = color;   // (a miss: {0, 0, 0, 0} until the loop below says otherwise)
    }
    if (p.env == nullptr) return;
    for (uint64_t k = (uint64_t)blockIdx.x * HIT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * HIT_THREADS) {
        HitSource s;
        if (hit_source(load_hit(hits, k), p.src, p.n_prims, s) && p.objs[s.object].material != HIT_NO_MATERIAL) continue;   // shaded above
        const rq_f4 rd = reinterpret_cast<const rq_f4 *>(rays + k)[1];   // {direction, t_max}
        const float d[3] = {rd[0], rd[1], rd[2]};
        if (rq_finite(d[0]) && rq_finite(d[1]) && rq_finite(d[2]) && !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f)) {
            const f3 e = hit_environment(p.env, p.env_w, p.env_h, d);
            out[k] = make_float4(e.x, e.y, e.z, 0.0f);   // this lane's own store above is behind it in program order
        }
    }
}

// Lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)) of the shard's tile rows; row r of the shard is tile-row pixel r + row0_in_tile
__global__ __launch_bounds__(HIT_THREADS) void k_reflect_rays(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                              uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t row0_in_tile, float eye0,
                                                              float eye1, float eye2, float bias, RayIn *__restrict__ rays) {
    const uint32_t tile = blockIdx.x * (HIT_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), yy = (tile / tiles_x) * TILE + (lane >> 3);
    if (!(x < width && yy >= row0_in_tile && yy - row0_in_tile < rows)) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane;
    const uint32_t mat = __builtin_bit_cast(uint32_t, plane_b[px * 3 + 2]);
    const float4 c = plane_c[px], e = plane_e[px];
    const float world[3] = {c.x, c.y, c.z}, eye[3] = {eye0, eye1, eye2};
    float m[3];
    RayIn r;
    rq_f4 o = {0.0f, 0.0f, 0.0f, 0.0f}, d = {0.0f, 0.0f, 0.0f, 0.0f};
    if (mat != NO_MATERIAL && ao_normal(e.y, e.z, e.w, m) && ha_reflect(world, m, eye, bias, r)) {
        o = (rq_f4){r.o[0], r.o[1], r.o[2], r.t_min};
        d = (rq_f4){r.d[0], r.d[1], r.d[2], r.t_max};
    }
    rq_f4 *dst = reinterpret_cast<rq_f4 *>(rays + ((size_t)(yy - row0_in_tile) * width + x));
    dst[0] = o; dst[1] = d;
}

uint32_t hit_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + HIT_THREADS - 1) / HIT_THREADS, HIT_MAX_BLOCKS); }

}  // namespace

hipError_t launch_hit_attributes(const void *hits, uint64_t n, const HitSource *src, uint32_t n_prims, const HitObject *objs, const float *lpv, float *attrs,
                                 uint32_t *material, hipStream_t s) {
    if (n == 0) return hipSuccess;
    LightMatrix L;
    for (int k = 0; k < 16; ++k) L.m[k] = lpv[k];
    k_hit_attributes<<<hit_grid(n), HIT_THREADS, 0, s>>>(static_cast<const RayOut *>(hits), (uint32_t)n, src, n_prims, objs, L, attrs, material);
    return hipGetLastError();
}

hipError_t launch_shade_hits(const void *rays, const void *hits, uint64_t n, const HitShadeParams &p, float4 *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_shade_hits<<<hit_grid(n), HIT_THREADS, 0, s>>>(static_cast<const RayIn *>(rays), static_cast<const RayOut *>(hits), (uint32_t)n, p, out);
    return hipGetLastError();
}

hipError_t launch_reflect_rays(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                               uint32_t row0_in_tile, const float eye[3], float bias, void *rays, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y, per = HIT_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_reflect_rays<<<(n_tiles + per - 1) / per, HIT_THREADS, 0, s>>>(plane_b, static_cast<const float4 *>(plane_c), static_cast<const float4 *>(plane_e), n_tiles, tiles_x, width,
                                                                     rows, row0_in_tile, eye[0], eye[1], eye[2], bias, static_cast<RayIn *>(rays));
    return hipGetLastError();
}

}  // namespace arctic
