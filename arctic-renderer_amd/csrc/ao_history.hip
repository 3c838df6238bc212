// ao_history.hip -- temporal accumulation of the ambient occlusion's byte plane (arctic_accumulate_ambient_occlusion_device,
// arctic_pass_ray_effects_temporal; the arithmetic is written once, in include/arctic_hip.h in front of the calls, and carried out by ao_history.h --
// the very functions the host arbiter arctic_accumulate_pixels runs):
//   k_ao_accumulate   a wave is one 8x8 tile of the tile-major G-buffer, as in k_compose and k_trace_ao.  Every pixel reads its material (plane b),
//                     its normal (plane e), its world position (plane c) and its current byte; a covered pixel reprojects through the previous
//                     call's matrix and gathers up to four entries of the previous history (two float4 each); every pixel of the frame stores
//                     its byte and its entry of the new history (two float4).
// The history is tile-major like the G-buffer: each of the two stores is one contiguous 1 KiB per wave, and under a still camera the gather is the
// wave's own tile plus an apron of one pixel -- the four taps of neighbouring lanes share cache lines, as the window of k_ao_filter does.  Whole
// frames only (the taps' rows are elsewhere on a shard), so pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile (y / 8) * tiles_x + x / 8.
// A streaming kernel: per pixel 44 B of G-buffer (planes b, c, e) and 1 B in, 33 B out, and for a covered pixel a gather of 32 B per history entry -- 81 / 64
// entries per pixel when the taps are the tile and its apron.  No LDS (what was measured), no barrier, no atomics; vector stores
// only.  Compiled with contraction off: every operation of the definition rounds once.
#include "common.h"
#include "ao_history.h"

namespace arctic {

namespace {

constexpr uint32_t AOH_THREADS = 256;

// the previous history's entry of the pixel at (qx, qy) of the frame; the caller has bounded both by the frame, so the index is inside the planes
struct TiledFetch {
    const float4 *a, *b;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, AoHistoryEntry &e) const {
        const size_t q = ((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE;
        const float4 ha = a[q], hb = b[q];
        e.world[0] = ha.x; e.world[1] = ha.y; e.world[2] = ha.z; e.value = ha.w;
        e.m[0] = hb.x; e.m[1] = hb.y; e.m[2] = hb.z; e.count = hb.w;
    }
};

// Every index is bounded before it is used: the tile by n_tiles, the pixel by the frame's width and rows, a tap by the frame inside aoh_pixel
__global__ __launch_bounds__(AOH_THREADS) void k_ao_accumulate(const AoHistoryParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * (AOH_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)y * p.width + x;
    const uint32_t mat = __builtin_bit_cast(uint32_t, p.plane_b[px * 3 + 2]);
    const float4 e = static_cast<const float4 *>(p.plane_e)[px], c = static_cast<const float4 *>(p.plane_c)[px];
    const float n[3] = {e.y, e.z, e.w}, w[3] = {c.x, c.y, c.z};
    const float cur = (float)p.ao_in[o];
    const TiledFetch fetch = {static_cast<const float4 *>(p.prev_a), static_cast<const float4 *>(p.prev_b), p.tiles_x};
    AoHistoryEntry h;
    const uint32_t byte = aoh_pixel(mat != NO_MATERIAL, n, w, cur, p.prev_a ? p.P : nullptr, p.width, p.rows, p.d, fetch, h);
    p.ao_out[o] = (uint8_t)byte;
    static_cast<float4 *>(p.next_a)[px] = make_float4(h.world[0], h.world[1], h.world[2], h.value);
    static_cast<float4 *>(p.next_b)[px] = make_float4(h.m[0], h.m[1], h.m[2], h.count);
}

}  // namespace

hipError_t launch_ao_accumulate(const AoHistoryParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, per = AOH_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_ao_accumulate<<<(n_tiles + per - 1) / per, AOH_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
