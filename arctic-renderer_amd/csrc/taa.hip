// taa.hip -- the temporal anti-aliasing resolve, in front of the tonemapper (arctic_taa_resolve_device, arctic_pass_taa; the arithmetic is written
// once, in include/arctic_hip.h in front of the calls, and carried out by taa.h -- the very functions the host arbiter arctic_taa_pixels runs):
//   k_taa_resolve   a wave is one 8x8 tile, as in k_compose and k_ao_accumulate.  The wave first brings the HDR colours of its tile and an apron
//                   of one pixel -- 10 x 10 pixels of 12 B, clamped at the frame's edge as the definition clamps a neighbour -- into its own
//                   1200 B of LDS; then every pixel takes its colour and the eight around it from there, reads its velocity (8 B) and up to
//                   four entries of the previous T (16 B each), and stores its entry of the new T (16 B), its RGBA8 (4 B) and its float LDR
//                   (12 B).
// T is tile-major like the occlusion's history: the store is one contiguous 1 KiB per wave, and on a still scene the gather is the wave's own tile
// plus an apron of one pixel -- the four taps of neighbouring lanes share cache lines.  Whole frames only (the taps' rows are elsewhere on a
// shard), so pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile (y / 8) * tiles_x + x / 8.  The resolve reads no G-buffer.
// A streaming kernel: per pixel 20 B in (the apron: 100 / 64 x 12 B of colour), 32 B out, a gather of 81 / 64 x 16 B of history, a few dozen
// operations, four divisions and post_process.h's transcendentals.  The 3x3 box through LDS was measured against nine loads per lane through the
// cache: 7 to 10 % faster, the same bytes.  One barrier, between the apron's stores and its loads; no atomics; vector stores
// only.  Compiled with contraction off: every operation of the definition rounds once.
#include "common.h"
#include "taa.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t TAA_THREADS = 256;

// The apron: APRON x APRON pixels of three floats per wave; entry (ax, ay) is the frame's pixel (clamp(x0 - 1 + ax), clamp(y0 - 1 + ay)), x0 and y0
// being the tile's first pixel.  Clamping is monotone, so the pixel the definition names for a neighbour -- (clamp(px + dx), clamp(py + dy)) --
// is found at (that x + 1 - x0, that y + 1 - y0), which lies in 0 .. 9 for every pixel of the tile inside the frame
constexpr uint32_t APRON = TILE + 2, APRON_FLOATS = APRON * APRON * 3;
struct ColorFetch {
    const float *apron;
    uint32_t x0, y0;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const uint32_t a = ((qy + 1u - y0) * APRON + (qx + 1u - x0)) * 3u;
        c[0] = apron[a]; c[1] = apron[a + 1]; c[2] = apron[a + 2];
    }
};
// the previous T's entry of the pixel at (qx, qy), bounded by the frame likewise
struct HistoryFetch {
    const float4 *prev;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *e) const {
        const size_t q = ((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE;
        const float4 h = prev[q];
        e[0] = h.x; e[1] = h.y; e[2] = h.z; e[3] = h.w;
    }
};

// Every index is bounded before it is used: the tile by n_tiles, an apron pixel by the clamp, the pixel by the frame's width and rows, a tap
// by the frame inside taa_pixel.  Every wave of the workgroup reaches the barrier, a wave without a tile included
__global__ __launch_bounds__(TAA_THREADS) void k_taa_resolve(const TaaParams p) {
    __shared__ float lds[TAA_THREADS / TILE_PIXELS][APRON_FLOATS];
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t wave = threadIdx.x / TILE_PIXELS, tile = blockIdx.x * (TAA_THREADS / TILE_PIXELS) + wave, lane = threadIdx.x % TILE_PIXELS;
    const bool live = tile < n_tiles;   // (whole waves: a wave is one tile)
    const uint32_t x0 = live ? (tile % p.tiles_x) * TILE : 0u, y0 = live ? (tile / p.tiles_x) * TILE : 0u;
    if (live) {
        for (uint32_t k = lane; k < APRON * APRON; k += TILE_PIXELS) {
            const int32_t ax = (int32_t)x0 - 1 + (int32_t)(k % APRON), ay = (int32_t)y0 - 1 + (int32_t)(k / APRON);
            const uint32_t qx = (uint32_t)(ax < 0 ? 0 : ax > (int32_t)p.width - 1 ? (int32_t)p.width - 1 : ax);
            const uint32_t qy = (uint32_t)(ay < 0 ? 0 : ay > (int32_t)p.rows - 1 ? (int32_t)p.rows - 1 : ay);
            const f3v h = *reinterpret_cast<const f3v *>(p.color + ((size_t)qy * p.width + qx) * 3);
            lds[wave][k * 3] = h.x; lds[wave][k * 3 + 1] = h.y; lds[wave][k * 3 + 2] = h.z;
        }
    }
    __syncthreads();
    if (!live) return;
    const uint32_t x = x0 + (lane & 7u), y = y0 + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)y * p.width + x;
    float v[2] = {0.0f, 0.0f};
    if (p.velocity) {
        const float2 w = static_cast<const float2 *>(p.velocity)[o];
        v[0] = w.x; v[1] = w.y;
    }
    const ColorFetch color = {lds[wave], x0, y0};
    const HistoryFetch history = {static_cast<const float4 *>(p.prev), p.tiles_x};
    float out[4];
    taa_pixel(x, y, p.width, p.rows, p.d, color, v, p.prev != nullptr, history, out);
    static_cast<float4 *>(p.next)[px] = make_float4(out[0], out[1], out[2], out[3]);
    const f3 t = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

}  // namespace

hipError_t launch_taa_resolve(const TaaParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, per = TAA_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_taa_resolve<<<(n_tiles + per - 1) / per, TAA_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
