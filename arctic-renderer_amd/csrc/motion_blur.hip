// motion_blur.hip -- the motion blur, in front of the tonemapper (arctic_motion_blur_device, arctic_pass_motion_blur; the arithmetic is written
// once, in include/arctic_hip.h in front of the calls, and carried out by motion_blur.h -- the very functions the host arbiters run):
//   k_mb_depth           the depth word of the visibility plane as a row-major float plane: 8 B in, 4 B out per pixel.
//   k_mb_tile_max        a wave is one 8x8 tile.  Every pixel reads its velocity (8 B) and its depth (4 B) ONCE, prepares its half velocity and
//                        stores P = {l, z} (8 B); the tile's longest half velocity is found by ONE wave reduction without LDS -- the key
//                        bits(l2) << 32 | (64 - lane) orders by length first (l2 >= 0: its bits order as integers) and by the lower lane among
//                        equals; six __shfl_xor steps, then the lane that owns the winning key stores the tile's float2.
//   k_mb_neighbour_max   one thread per tile over the small tile plane: the longest of the (2 Rt + 1)^2 window, at most 17 x 17 loads of 8 B
//                        that neighbouring threads share.
//   k_motion_blur        a wave is one tile, as in k_taa_resolve.  The tile's direction d is the same for the 64 lanes: it is read through
//                        readfirstlane and lives in SGPRs.  Tap i of the wave is the tile translated by t * d (t differs between lanes only by
//                        the dither), so the taps of neighbouring lanes share cache lines: per tap 8 B of P and, where the weight enters, 12 B
//                        of colour (16 B from the anti-aliasing's history), through the cache.  A tile whose d is not longer than half a pixel
//                        copies its colour.  Stores the blurred HDR colour (12 B), RGBA8 (4 B) and float LDR (12 B) per pixel.
// Whole frames only (a shard's taps lie on other ranks).  No LDS, no barrier, no atomics, vector stores only.  Compiled with contraction off:
// every operation of the definition rounds once.
#include "common.h"
#include "motion_blur.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t MB_THREADS = 256, MB_WAVES = MB_THREADS / TILE_PIXELS;

// row-major float3 colour of a pixel inside the frame
struct PlaneColor {
    const float *color;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const f3v h = *reinterpret_cast<const f3v *>(color + ((size_t)qy * width + qx) * 3);
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};
// the anti-aliasing's history: tile-major float4 {r, g, b, N}
struct HistoryColor {
    const float4 *t;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const float4 h = t[((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE];
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};
struct PrepFetch {
    const float2 *prep;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float &l, float &z) const {
        const float2 e = prep[(size_t)qy * width + qx];
        l = e.x; z = e.y;
    }
};

// the tile is bounded by n_tiles, the pixel by the handle's rows and width
__global__ __launch_bounds__(MB_THREADS) void k_mb_depth(const unsigned long long *vis, float *depth, uint32_t tiles_x, uint32_t n_tiles, uint32_t width, uint32_t rows, uint32_t row0_in_tile) {
    const uint32_t tile = blockIdx.x * MB_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), yy = (tile / tiles_x) * TILE + (lane >> 3);
    if (!(x < width && yy >= row0_in_tile && yy - row0_in_tile < rows)) return;   // (a tile's padding: not a pixel of the handle's rows)
    const unsigned long long key = vis[(size_t)tile * TILE_PIXELS + lane];
    depth[(size_t)(yy - row0_in_tile) * width + x] = key == ~0ull ? 1.0f : __uint_as_float((uint32_t)(key >> 32));
}

// Every lane of a live wave reaches the shuffles, a lane outside the frame with the key 0, which is below every pixel's (64 - lane >= 1)
__global__ __launch_bounds__(MB_THREADS) void k_mb_tile_max(const MotionBlurParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * MB_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    const bool inside = x < p.width && y < p.rows;
    float h[2] = {0.0f, 0.0f}, l2 = 0.0f, l = 0.5f;
    unsigned long long key = 0ull;
    if (inside) {
        const size_t o = (size_t)y * p.width + x;
        const float2 v = static_cast<const float2 *>(p.velocity)[o];
        mb_half_velocity(p.d, v.x, v.y, h, l2, l);
        static_cast<float2 *>(p.prep)[o] = make_float2(l, p.depth ? p.depth[o] : 0.0f);
        key = ((unsigned long long)__float_as_uint(l2) << 32) | (unsigned long long)(TILE_PIXELS - lane);
    }
    unsigned long long best = key;
    for (int m = TILE_PIXELS / 2; m > 0; m >>= 1) {
        const unsigned long long other = __shfl_xor(best, m, TILE_PIXELS);
        best = other > best ? other : best;
    }
    if (inside && key == best) static_cast<float2 *>(p.tile_max)[tile] = make_float2(h[0], h[1]);   // (the lane is part of the key: one lane stores)
}

__global__ __launch_bounds__(MB_THREADS) void k_mb_neighbour_max(const MotionBlurParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, tile = blockIdx.x * MB_THREADS + threadIdx.x;
    if (tile >= n_tiles) return;
    const float2 *tm = static_cast<const float2 *>(p.tile_max);
    const uint32_t tiles_x = p.tiles_x;
    const auto fetch = [tm, tiles_x](uint32_t tx, uint32_t ty, float *h) {   // (mb_neighbour_max bounds the tile by the grid)
        const float2 e = tm[(size_t)ty * tiles_x + tx];
        h[0] = e.x; h[1] = e.y;
    };
    float out[2] = {0.0f, 0.0f};
    mb_neighbour_max(tile % p.tiles_x, tile / p.tiles_x, p.tiles_x, p.tiles_y, mb_window(p.d), fetch, out);
    static_cast<float2 *>(p.neighbour_max)[tile] = make_float2(out[0], out[1]);
}

// Every index is bounded before it is used: the tile by n_tiles, the pixel by the frame's width and rows, a tap by the frame inside mb_pixel
template <class Color>
__global__ __launch_bounds__(MB_THREADS) void k_motion_blur(const MotionBlurParams p, const Color color) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * MB_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const float2 nm = static_cast<const float2 *>(p.neighbour_max)[tile];
    // the same for the 64 lanes: in SGPRs from here on
    const float dx = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(nm.x))), dy = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(nm.y)));
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t o = (size_t)y * p.width + x;
    const PrepFetch prep = {static_cast<const float2 *>(p.prep), p.width};
    float out[3];
    mb_pixel(x, y, p.width, p.rows, p.d, dx, dy, color, prep, out);
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){out[0], out[1], out[2]};
    const f3 t = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

}  // namespace

hipError_t launch_mb_depth(const unsigned long long *vis, float *depth, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows, uint32_t row0_in_tile, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_mb_depth<<<(n_tiles + MB_WAVES - 1) / MB_WAVES, MB_THREADS, 0, s>>>(vis, depth, tiles_x, n_tiles, width, rows, row0_in_tile);
    return hipGetLastError();
}

hipError_t launch_mb_tile_max(const MotionBlurParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_mb_tile_max<<<(n_tiles + MB_WAVES - 1) / MB_WAVES, MB_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_mb_neighbour_max(const MotionBlurParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_mb_neighbour_max<<<(n_tiles + MB_THREADS - 1) / MB_THREADS, MB_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_motion_blur(const MotionBlurParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    const uint32_t grid = (n_tiles + MB_WAVES - 1) / MB_WAVES;
    if (p.color_taa) k_motion_blur<<<grid, MB_THREADS, 0, s>>>(p, HistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_motion_blur<<<grid, MB_THREADS, 0, s>>>(p, PlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

}  // namespace arctic
