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
// post_process (tonemap, gamma, unorm8) is post_process.h's: RESTATED from shade.hip, because shade.hip stays as it is.
// No LDS, no barrier, no atomics; vector stores only.  Compiled with contraction off: every operation of the definition rounds once, and a fused
// multiply-add appears only where it is written.
#include "common.h"
#include "compose.h"
#include "material_sampler.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t COMPOSE_THREADS = 256;

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
