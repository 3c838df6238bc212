// dof.hip -- depth of field, in front of the tonemapper and behind the motion blur (arctic_dof_device, arctic_pass_dof; the arithmetic is written
// once, in include/arctic_hip.h in front of the calls, and carried out by dof.h -- the very functions the host arbiters run):
//   k_dof_prepare        a wave is one 8x8 tile.  Every pixel reads its depth (4 B) ONCE, works out its view distance and signed radius and stores
//                        P = {s, zv} (8 B); the tile's largest |s| is found by ONE wave reduction without LDS -- |s| >= 0, so its bits order
//                        as integers; six __shfl_xor steps, then lane 0 stores the tile's float.
//   k_dof_neighbour_max  one thread per tile over the small tile plane: the largest of the (2 Rt + 1)^2 window, at most 17 x 17 loads of 4 B
//                        that neighbouring threads share.
//   k_dof_gather         a wave is one tile, as in k_motion_blur.  The tile's radius R is the same for the 64 lanes: it is read through
//                        readfirstlane and lives in an SGPR.  The tap table is read at a wave-uniform index, so a tap's offset, its distance and
//                        k are the same for the 64 lanes: tap i of the wave is the tile translated by taps2[i] * R, and the taps of neighbouring
//                        lanes share cache lines: per tap 8 B of P and, where the weight enters, 12 B of colour (16 B from the anti-aliasing's
//                        history), through the cache.  A tile whose R is not above half a pixel copies its colour.  Stores the HDR colour
//                        (12 B), RGBA8 (4 B) and float LDR (12 B) per pixel.
// Whole frames only (a shard's taps lie on other ranks).  No LDS, no barrier, no atomics, vector stores only.  Compiled with contraction off:
// every operation of the definition rounds once.
#include "common.h"
#include "dof.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t DOF_THREADS = 256, DOF_WAVES = DOF_THREADS / TILE_PIXELS;

// row-major float3 colour of a pixel inside the frame
struct DofPlaneColor {
    const float *color;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const f3v h = *reinterpret_cast<const f3v *>(color + ((size_t)qy * width + qx) * 3);
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};
// the anti-aliasing's history: tile-major float4 {r, g, b, N}
struct DofHistoryColor {
    const float4 *t;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const float4 h = t[((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE];
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};
struct DofPrepFetch {
    const float2 *prep;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float &s, float &z) const {
        const float2 e = prep[(size_t)qy * width + qx];
        s = e.x; z = e.y;
    }
};

// Every lane of a live wave reaches the shuffles, a lane outside the frame with the bits of 0.0, which no pixel's |s| lies below
__global__ __launch_bounds__(DOF_THREADS) void k_dof_prepare(const DofParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * DOF_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    uint32_t best = 0u;
    if (x < p.width && y < p.rows) {
        const size_t o = (size_t)y * p.width + x;
        float s, zv;
        dof_signed_radius(p.d, p.depth[o], s, zv);
        static_cast<float2 *>(p.prep)[o] = make_float2(s, zv);
        best = __float_as_uint(__builtin_fabsf(s));
    }
    for (int m = TILE_PIXELS / 2; m > 0; m >>= 1) {
        const uint32_t other = __shfl_xor(best, m, TILE_PIXELS);
        best = other > best ? other : best;
    }
    if (lane == 0) p.tile_max[tile] = __uint_as_float(best);   // (lane 0 is pixel (0, 0) of the tile: inside the frame for every tile of the grid)
}

__global__ __launch_bounds__(DOF_THREADS) void k_dof_neighbour_max(const DofParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, tile = blockIdx.x * DOF_THREADS + threadIdx.x;
    if (tile >= n_tiles) return;
    const float *tm = p.tile_max;
    const uint32_t tiles_x = p.tiles_x;
    const auto fetch = [tm, tiles_x](uint32_t tx, uint32_t ty) { return tm[(size_t)ty * tiles_x + tx]; };   // (dof_neighbour_max bounds the tile by the grid)
    p.neighbour_max[tile] = dof_neighbour_max(tile % p.tiles_x, tile / p.tiles_x, p.tiles_x, p.tiles_y, dof_window(p.d), fetch);
}

// Every index is bounded before it is used: the tile by n_tiles, the pixel by the frame's width and rows, a tap by the frame inside dof_pixel,
// the tap table by d.samples, which the calls hold to DOF_MAX_SAMPLES
template <class Color>
__global__ __launch_bounds__(DOF_THREADS) void k_dof_gather(const DofParams p, const Color color) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * DOF_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    // the same for the 64 lanes: in an SGPR from here on
    const float R = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(p.neighbour_max[tile])));
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t o = (size_t)y * p.width + x;
    const DofPrepFetch prep = {static_cast<const float2 *>(p.prep), p.width};
    float out[3];
    dof_pixel(x, y, p.width, p.rows, p.d, R, p.taps, color, prep, out);
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){out[0], out[1], out[2]};
    const f3 t = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

}  // namespace

hipError_t launch_dof_prepare(const DofParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_dof_prepare<<<(n_tiles + DOF_WAVES - 1) / DOF_WAVES, DOF_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_dof_neighbour_max(const DofParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_dof_neighbour_max<<<(n_tiles + DOF_THREADS - 1) / DOF_THREADS, DOF_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_dof_gather(const DofParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0 || p.d.samples > DOF_MAX_SAMPLES) return n_tiles == 0 ? hipSuccess : hipErrorInvalidValue;
    const uint32_t grid = (n_tiles + DOF_WAVES - 1) / DOF_WAVES;
    if (p.color_taa) k_dof_gather<<<grid, DOF_THREADS, 0, s>>>(p, DofHistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_dof_gather<<<grid, DOF_THREADS, 0, s>>>(p, DofPlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

}  // namespace arctic
