// fog.hip -- volumetric fog, the first stage behind the shading or the composition (arctic_fog_device, arctic_pass_fog; the arithmetic is written
// once, in include/arctic_hip.h in front of the calls, and carried out by fog.h -- the very functions the host arbiter runs):
//   k_fog_march   a wave is one 8x8 tile, a lane one pixel, as in k_dof_gather.  The two records arrive as kernel arguments: the step count, the
//                 view and the light rows are the same for the 64 lanes and live in SGPRs.  A lane reads its colour (12 B), its depth (4 B) and
//                 its entry of the 64-byte offset table, then marches `steps` samples along its ray: per sample three affine rows, two floors,
//                 one 4-byte load of the sun's map at a texel bounded inside fog_visible, one compare.  Neighbouring lanes march neighbouring
//                 rays, so a sample's 64 texels lie near each other in the map.  The lookups do not depend on the transmittance chain, the only
//                 loop-carried value: fog_pixel finds the V_k of FOG_BATCH samples -- each sample tests, loads and compares in turn, and leaves at
//                 the first bounds test that fails -- and then runs their part of the chain.  With 8 waves per SIMD the wait behind a load is
//                 hidden by the other waves: the kernel is bound by its arithmetic (where a form that issues a batch's loads
//                 together and a min/max table in front of the map were measured).  Stores the HDR colour (12 B), RGBA8 (4 B) and float LDR (12 B) per pixel.
// Whole frames only.  No LDS, no barrier, no atomics, vector stores only.  Compiled with contraction off: every operation of the definition
// rounds once.
#include "common.h"
#include "fog.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t FOG_THREADS = 256, FOG_WAVES = FOG_THREADS / TILE_PIXELS;

// one texel of the sun's map; fog_visible has bounded (tu, tv) by the map's side
struct FogMapFetch {
    const float *map;
    uint32_t S;
    __device__ __forceinline__ float operator()(uint32_t tu, uint32_t tv) const { return map[(size_t)tv * S + tu]; }
#if defined(ARCTIC_FOG_TABLE_VARIANT)
    // the variant's table: min/max of the 4 x 4 texel block of a texel inside the map (so the block lies inside the nb x nb table).  wb <= min: no
    // texel of the block lies below wb, lit; wb > max: every texel does, shadowed -- the compare's own answer for every texel that is no NaN (the
    // table's minima and maxima skip a NaN texel, which the compare calls lit); else undecided: the texel itself
    const float2 *blocks;
    uint32_t nb;
    __device__ __forceinline__ bool decided(uint32_t tu, uint32_t tv, float wb, bool &lit) const {
        if (!blocks) return false;
        const float2 mm = blocks[(size_t)(tv >> 2) * nb + (tu >> 2)];
        if (!(wb > mm.x)) { lit = true; return true; }
        if (wb > mm.y) { lit = false; return true; }
        return false;
    }
#endif
};

// Every index is bounded before it is used: the tile by n_tiles, the pixel by the frame's width and rows, a texel by the map inside fog_visible,
// the offset table by fog_offset_index (below 16), the step count by the calls (FOG_MAX_STEPS)
__global__ __launch_bounds__(FOG_THREADS) void k_fog_march(const FogParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * FOG_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t o = (size_t)y * p.width + x;
    const f3v h = *reinterpret_cast<const f3v *>(p.color + o * 3);
    const float c[3] = {h.x, h.y, h.z};
    const float depth = p.depth ? p.depth[o] : 1.0f;
    const float offset = p.offsets[fog_offset_index(x, y)];
#if defined(ARCTIC_FOG_TABLE_VARIANT)
    const FogMapFetch map = {p.map, p.S, p.blocks, p.nb};
#else
    const FogMapFetch map = {p.map, p.S};
#endif
    float out[3];
    fog_pixel(x, y, p.d, p.v, offset, c, depth, p.map ? p.S : 0u, map, out, nullptr);
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){out[0], out[1], out[2]};
    const f3 t = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

}  // namespace

hipError_t launch_fog_march(const FogParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    if (p.d.steps < 1u || p.d.steps > FOG_MAX_STEPS || !p.color || !p.offsets || !p.out_hdr || !p.out_rgba8 || !p.out_ldr) return hipErrorInvalidValue;
    k_fog_march<<<(n_tiles + FOG_WAVES - 1) / FOG_WAVES, FOG_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
