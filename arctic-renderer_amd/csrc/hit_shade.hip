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
// The device functions the kernels are made of stand in hit_shade_device.h, which hit_shade_ext.hip (ARCTIC_OPT_HIT_MODEL = 1) includes too.
#include "hit_shade.h"
#include "ray_ao.h"
#include "material_sampler.h"
#include "hit_shade_device.h"

namespace arctic {

namespace {

struct LightMatrix { float m[16]; };

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
