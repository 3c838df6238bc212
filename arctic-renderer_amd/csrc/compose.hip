// compose.hip -- ray-traced occlusion and reflections folded into the shaded frame, in front of the tonemapper (arctic_compose_planes_device,
// arctic_pass_ray_effects; the arithmetic of the two terms is written once, in include/arctic_hip.h in front of the calls, and carried out by
// compose.h -- the very functions the host arbiter arctic_compose_pixels runs):
//   k_compose   a wave is one 8x8 tile of the tile-major G-buffer, as in k_reflect_rays and k_trace_ao.  Every pixel reads its float HDR colour
//               (12 B) and its material (plane b); a pixel with geometry and a term to add reads its uv (plane a) and samples the material's
//               channels (material_sampler.h: level 0, the default sampler, per-lane descriptors); the occlusion reads one byte; the reflection
//               reads its 16 B and, only in the lanes where refl.a > 0, planes c and e (a tile without such a lane skips both loads by its exec
//               mask).  Then post_process and three stores: RGBA8 (4 B), float LDR and the composed HDR (12 B each).
// A streaming kernel: about 33 B of row-major planes in, 28 B out and 28 to 60 B of G-buffer per pixel, a few dozen operations and five
// transcendentals.  The material's descriptors are gathered per lane as in k_shade_hits: the 32 bytes sit in one cache line for a whole tile in
// almost every tile, and a scalar path would need a second, per-lane copy of the sampler for the tiles with a material boundary.
// post_process is RESTATED from shade.hip (tonemap, gamma, unorm8: the operations of k_post_process in its order), because shade.hip stays as it is.
// No LDS, no barrier, no atomics; vector stores only.  Compiled with contraction off: every operation of the definition rounds once, and a fused
// multiply-add appears only where it is written.
#include "common.h"
#include "compose.h"
#include "material_sampler.h"

namespace arctic {

namespace {

constexpr uint32_t COMPOSE_THREADS = 256;

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

// Lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)) of the shard's tile rows; row r of the shard is tile-row pixel r + row0_in_tile.
// Every index is bounded before it is used: the tile by n_tiles, the pixel by the handle's rows and width, the material by the table's length
__global__ __launch_bounds__(COMPOSE_THREADS) void k_compose(const ComposeParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * (COMPOSE_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), yy = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (!(x < p.width && yy >= p.row0_in_tile && yy - p.row0_in_tile < p.rows)) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)(yy - p.row0_in_tile) * p.width + x;
    const uint32_t mat = __builtin_bit_cast(uint32_t, p.plane_b[px * 3 + 2]);
    const f3v h = *reinterpret_cast<const f3v *>(p.hdr + o * 3);
    float C[3] = {h.x, h.y, h.z};
    if (mat < p.n_materials) {   // (NO_MATERIAL, and an index the handle has no material for -- the shading pass's own test of "covered")
        float refl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.flags & COMPOSE_REFLECTIONS) {
            const rq_f4 r = static_cast<const rq_f4 *>(p.refl)[o];
            refl[0] = r[0]; refl[1] = r[1]; refl[2] = r[2]; refl[3] = r[3];
        }
        const bool occludes = (p.flags & COMPOSE_AO) != 0u, reflects = compose_reflects(p.flags, refl[3]);
        if (occludes || reflects) {
            const float4 a = static_cast<const float4 *>(p.plane_a)[px];
            const Channels ch = sample_material(p.tex, p.srgb_lut, mat, a.x, a.y);
            if (occludes) compose_occlusion(C, ch.base, p.ambient, p.ao_strength, p.ao[o]);
            if (reflects) {
                const float4 c = static_cast<const float4 *>(p.plane_c)[px], e = static_cast<const float4 *>(p.plane_e)[px];
                const float world[3] = {c.x, c.y, c.z};
                float m[3];
                if (ao_normal(e.y, e.z, e.w, m)) compose_reflection(C, ch.base, ch.metal, ch.rough, m, world, p.eye, refl, p.reflection_strength);
            }
        }
    }
    const f3 t = tonemap(mk(C[0], C[1], C[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){C[0], C[1], C[2]};
}

}  // namespace

hipError_t launch_compose(const ComposeParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, per = COMPOSE_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_compose<<<(n_tiles + per - 1) / per, COMPOSE_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
