// taa_upscale.hip -- the temporal upscaler, in front of the tonemapper (arctic_taa_upscale_device, arctic_pass_taa_upscale; the arithmetic is
// written once, in include/arctic_hip.h in front of the calls, and carried out by taa_upscale.h -- the very function the host arbiter
// arctic_taa_upscale_pixels runs):
//   k_taa_upscale   a wave is one 8x8 tile of the OUTPUT frame, one lane per output pixel, as in k_taa_resolve.  The wave first brings the
//                   input pixels its tile can name -- the nearest samples of its 64 pixels and the boxes around them, at most 11 x 11 input
//                   pixels of 12 B for any ratio from 1 to 4 and any jitter (taa_upscale.h derives the bound), clamped at the input frame's
//                   edge as the definition clamps a neighbour -- into its own 1452 B of LDS; then every pixel takes its sample and the eight
//                   around it from there, reads the sample's velocity (8 B) and up to four entries of the previous U (16 B each), and stores
//                   its entry of the new U (16 B), its RGBA8 (4 B) and its float LDR (12 B).
// U is tile-major like T: the store is one contiguous 1 KiB per wave, and on a still scene the gather is the wave's own tile plus an apron of one
// pixel.  Whole frames only.  Output pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile (y / 8) * tiles_x + x / 8.
// A streaming kernel: per OUTPUT pixel 32 B out and a gather of 81 / 64 x 16 B of history as in the resolve, and rx * ry times 20 B of input
// (between 1/16 and all of it).  One barrier, between the footprint's stores and its loads; no atomics; vector stores only.  Compiled with
// contraction off: every operation of the definition rounds once.
#include "common.h"
#include "taa_upscale.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t TAA_UPSCALE_THREADS = 256;
static_assert(TILE == 8 && TAA_UPSCALE_SPAN == TILE - 1 + 2, "taa_upscale.h's bound is for tiles of 8 x 8 output pixels");

// The footprint: FOOT x FOOT input pixels of three floats per wave; entry (ax, ay) is the input pixel (clamp(qx0 - 1 + ax), clamp(qy0 - 1 + ay)),
// (qx0, qy0) being the nearest sample of the tile's first pixel.  The nearest sample is monotone in the output pixel and so is clamping, so the
// pixel the definition names for a neighbour of any of the tile's samples -- (clamp(qx + dx), clamp(qy + dy)) with qx0 <= qx <= qx0 + 8 -- is
// found at (that x + 1 - qx0, that y + 1 - qy0), which lies in 0 .. 10; the min() keeps the index inside the wave's LDS whatever happens
constexpr uint32_t FOOT = TAA_UPSCALE_FOOTPRINT, FOOT_FLOATS = FOOT * FOOT * 3;
struct UpscaleColorFetch {
    const float *foot;
    uint32_t qx0, qy0;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const uint32_t ax = min(qx + 1u - qx0, FOOT - 1u), ay = min(qy + 1u - qy0, FOOT - 1u);
        const uint32_t a = (ay * FOOT + ax) * 3u;
        c[0] = foot[a]; c[1] = foot[a + 1]; c[2] = foot[a + 2];
    }
};
// velocity2 of an input pixel inside the input frame
struct UpscaleVelocityFetch {
    const float2 *velocity;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *v) const {
        v[0] = 0.0f; v[1] = 0.0f;
        if (velocity) {
            const float2 w = velocity[(size_t)qy * width + qx];
            v[0] = w.x; v[1] = w.y;
        }
    }
};
// the previous U's entry of the output pixel at (qx, qy), which taa_upscale_pixel has bounded by the output frame
struct UpscaleHistoryFetch {
    const float4 *prev;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *e) const {
        const size_t q = ((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE;
        const float4 h = prev[q];
        e[0] = h.x; e[1] = h.y; e[2] = h.z; e[3] = h.w;
    }
};

// Every index is bounded before it is used: the tile by n_tiles, a footprint pixel by the clamp to the input frame, the output pixel by the
// output's width and height, the sample by taa_upscale_nearest's clamp, a tap by the output frame inside taa_upscale_pixel.  Every wave of the
// workgroup reaches the barrier, a wave without a tile included
__global__ __launch_bounds__(TAA_UPSCALE_THREADS) void k_taa_upscale(const TaaUpscaleParams p) {
    __shared__ float lds[TAA_UPSCALE_THREADS / TILE_PIXELS][FOOT_FLOATS];
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t wave = threadIdx.x / TILE_PIXELS, tile = blockIdx.x * (TAA_UPSCALE_THREADS / TILE_PIXELS) + wave, lane = threadIdx.x % TILE_PIXELS;
    const bool live = tile < n_tiles;   // (whole waves: a wave is one tile)
    const uint32_t x0 = live ? (tile % p.tiles_x) * TILE : 0u, y0 = live ? (tile / p.tiles_x) * TILE : 0u;
    // the nearest sample of the tile's first pixel, by the definition's own function
    const float rx = (float)p.width / (float)p.d.out_width, ry = (float)p.height / (float)p.d.out_height;
    float unused;
    const uint32_t qx0 = taa_upscale_nearest(x0, p.width, rx, p.d.jitter[0], &unused), qy0 = taa_upscale_nearest(y0, p.height, ry, p.d.jitter[1], &unused);
    if (live) {
        for (uint32_t k = lane; k < FOOT * FOOT; k += TILE_PIXELS) {
            const int32_t ax = (int32_t)qx0 - 1 + (int32_t)(k % FOOT), ay = (int32_t)qy0 - 1 + (int32_t)(k / FOOT);
            const uint32_t qx = (uint32_t)(ax < 0 ? 0 : ax > (int32_t)p.width - 1 ? (int32_t)p.width - 1 : ax);
            const uint32_t qy = (uint32_t)(ay < 0 ? 0 : ay > (int32_t)p.height - 1 ? (int32_t)p.height - 1 : ay);
            const f3v h = *reinterpret_cast<const f3v *>(p.color + ((size_t)qy * p.width + qx) * 3);
            lds[wave][k * 3] = h.x; lds[wave][k * 3 + 1] = h.y; lds[wave][k * 3 + 2] = h.z;
        }
    }
    __syncthreads();
    if (!live) return;
    const uint32_t x = x0 + (lane & 7u), y = y0 + (lane >> 3);
    if (x >= p.d.out_width || y >= p.d.out_height) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)y * p.d.out_width + x;
    const UpscaleColorFetch color = {lds[wave], qx0, qy0};
    const UpscaleVelocityFetch velocity = {static_cast<const float2 *>(p.velocity), p.width};
    const UpscaleHistoryFetch history = {static_cast<const float4 *>(p.prev), p.tiles_x};
    float out[4];
    taa_upscale_pixel(x, y, p.width, p.height, p.d, color, velocity, p.prev != nullptr, history, out);
    static_cast<float4 *>(p.next)[px] = make_float4(out[0], out[1], out[2], out[3]);
    const f3 t = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

// U's colour of one output tile, row-major: what a later stage takes as its explicit colour plane.  Bounded like k_taa_upscale: the tile by
// n_tiles, the pixel by the output's width and height
__global__ __launch_bounds__(TAA_UPSCALE_THREADS) void k_taa_upscale_hdr(const float4 *u, float *out, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t n_tiles) {
    const uint32_t tile = blockIdx.x * (TAA_UPSCALE_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), y = (tile / tiles_x) * TILE + (lane >> 3);
    if (x >= width || y >= height) return;
    const float4 e = u[(size_t)tile * TILE_PIXELS + lane];
    *reinterpret_cast<f3v *>(out + ((size_t)y * width + x) * 3) = (f3v){e.x, e.y, e.z};
}

}  // namespace

hipError_t launch_taa_upscale_hdr(const void *u, float *out, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tiles_y, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y, per = TAA_UPSCALE_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_taa_upscale_hdr<<<(n_tiles + per - 1) / per, TAA_UPSCALE_THREADS, 0, s>>>(static_cast<const float4 *>(u), out, width, height, tiles_x, n_tiles);
    return hipGetLastError();
}

hipError_t launch_taa_upscale(const TaaUpscaleParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, per = TAA_UPSCALE_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_taa_upscale<<<(n_tiles + per - 1) / per, TAA_UPSCALE_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
