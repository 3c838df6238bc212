// bloom.hip -- bloom, the last stage in front of the tonemapper, behind the depth of field (arctic_bloom_device; the arithmetic is written once,
// in include/arctic_hip.h in front of the calls, and carried out by bloom.h -- the very functions the host arbiters run):
//   k_bloom_down_first  a workgroup is a 16 x 16 block of level 1.  Its 36 x 36 source pixels (the block's 32 x 32 and the 2-texel halo, clamped
//                       to the frame by integer clamps in front of the load) are read ONCE: every thread prefilters its share -- a division and a
//                       select chain per source pixel instead of per tap -- and writes b(q) to LDS; behind ONE __syncthreads() each thread
//                       reads its 36 texels from LDS and stores D_1 (12 B).  LDS: three planes (r, g, b) of 36 rows of BLOOM_LDS_STRIDE = 48
//                       floats, 20736 B static.  A thread reads a row of its footprint as three aligned float2 at the column 2 * lx: the 16
//                       lanes of a block row cover 32 consecutive dwords, and the next block row's lanes lie 2 * 48 = 96 dwords further,
//                       that is 32 banks further of the 64: the 32 lanes that are served together touch every bank once.  (Float3 texels of
//                       12 B would put lane l at dword 6 l: lanes 16 apart on the same bank.)  Threads outside the level take part in the
//                       staging and skip only the store: every thread of every workgroup reaches the barrier.
//   k_bloom_down        levels 2 .. L, one thread per destination pixel: 36 cached loads of 12 B that neighbouring threads share.
//   k_bloom_up          U_k = D_k + spread * UP(U_{k+1}), one thread per destination pixel: 16 cached loads of the coarser level.
//   k_bloom_composite   UP(U_1) at the frame's size, the select, then HDR (12 B), RGBA8 (4 B) and float LDR (12 B) per pixel as k_dof_gather ends.
// 2 L launches per call.  Whole frames only.  No atomics, vector stores only, no barrier outside the first kernel.  Compiled with contraction
// off: every operation of the definition rounds once.
#include "common.h"
#include "bloom.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t BLOOM_BLOCK = 16, BLOOM_THREADS = BLOOM_BLOCK * BLOOM_BLOCK;
constexpr uint32_t BLOOM_SRC = 2 * BLOOM_BLOCK + 4;   // the block's source pixels a side, halo included
constexpr uint32_t BLOOM_LDS_STRIDE = 48;             // floats a row: >= BLOOM_SRC, and 2 * 48 = 32 (mod 64) banks between two block rows

// row-major float3 colour of a pixel inside the frame
struct BloomPlaneColor {
    const float *color;
    uint32_t width;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const f3v h = *reinterpret_cast<const f3v *>(color + ((size_t)qy * width + qx) * 3);
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};
// the anti-aliasing's history: tile-major float4 {r, g, b, N}
struct BloomHistoryColor {
    const float4 *t;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const float4 h = t[((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE];
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};

// Every index is bounded before it is used: a source pixel by the frame (bloom_clamp) in front of the load, an LDS element by BLOOM_SRC rows and
// columns (e < BLOOM_SRC * BLOOM_SRC; a thread's footprint ends at row and column 2 * 15 + 5 = 35), the destination by level 1's size
#if defined(ARCTIC_BLOOM_UNSTAGED)
// The measurement's other side (tools/bloom_time.py builds a library with this switch, the Makefile never sets it): no LDS and no barrier, the
// prefilter evaluated at every tap through the cache -- the same bloom.h functions, the same bytes
template <class Color>
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom_down_first(const BloomParams p, const Color color) {
    const uint32_t x = blockIdx.x * BLOOM_BLOCK + threadIdx.x % BLOOM_BLOCK, y = blockIdx.y * BLOOM_BLOCK + threadIdx.x / BLOOM_BLOCK;
    if (x >= p.layout.w[0] || y >= p.layout.h[0]) return;
    const auto texel = [&](uint32_t i, uint32_t j, float *b) {
        float c[3];
        color(bloom_clamp((int32_t)(2 * x + i) - 2, p.width), bloom_clamp((int32_t)(2 * y + j) - 2, p.rows), c);
        bloom_prefilter(p.d, c, b);
    };
    float out[3];
    bloom_down<true>(texel, out);
    *reinterpret_cast<f3v *>(p.down + ((size_t)y * p.layout.w[0] + x) * 3) = (f3v){out[0], out[1], out[2]};
}
#else
template <class Color>
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom_down_first(const BloomParams p, const Color color) {
    __shared__ __attribute__((aligned(8))) float staged[3][BLOOM_SRC][BLOOM_LDS_STRIDE];
    const uint32_t lx = threadIdx.x % BLOOM_BLOCK, ly = threadIdx.x / BLOOM_BLOCK;
    const int32_t sx0 = (int32_t)(blockIdx.x * 2 * BLOOM_BLOCK) - 2, sy0 = (int32_t)(blockIdx.y * 2 * BLOOM_BLOCK) - 2;
    for (uint32_t e = threadIdx.x; e < BLOOM_SRC * BLOOM_SRC; e += BLOOM_THREADS) {
        const uint32_t row = e / BLOOM_SRC, col = e % BLOOM_SRC;
        float c[3], b[3];
        color(bloom_clamp(sx0 + (int32_t)col, p.width), bloom_clamp(sy0 + (int32_t)row, p.rows), c);
        bloom_prefilter(p.d, c, b);
        staged[0][row][col] = b[0]; staged[1][row][col] = b[1]; staged[2][row][col] = b[2];
    }
    __syncthreads();   // (every thread of the workgroup arrives: nothing returns in front of it)
    const uint32_t x = blockIdx.x * BLOOM_BLOCK + lx, y = blockIdx.y * BLOOM_BLOCK + ly;
    if (x >= p.layout.w[0] || y >= p.layout.h[0]) return;
    const auto texel = [&](uint32_t i, uint32_t j, float *c) {   // S~(i, j): clamped when it was staged
        const uint32_t row = 2 * ly + j, pair = 2 * lx + (i & ~1u);
        const float2 r = *reinterpret_cast<const float2 *>(&staged[0][row][pair]), g = *reinterpret_cast<const float2 *>(&staged[1][row][pair]),
                     b = *reinterpret_cast<const float2 *>(&staged[2][row][pair]);
        c[0] = (i & 1u) ? r.y : r.x; c[1] = (i & 1u) ? g.y : g.x; c[2] = (i & 1u) ? b.y : b.x;
    };
    float out[3];
    bloom_down<true>(texel, out);
    *reinterpret_cast<f3v *>(p.down + ((size_t)y * p.layout.w[0] + x) * 3) = (f3v){out[0], out[1], out[2]};
}
#endif

// a level of a pyramid as a texel fetch
struct BloomLevel {
    const float *t;
    uint32_t w;
    __device__ __forceinline__ void operator()(uint32_t x, uint32_t y, float *c) const {
        const f3v h = *reinterpret_cast<const f3v *>(t + ((size_t)y * w + x) * 3);
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};

// D_level from D_{level-1}; k = level - 1 indexes the layout.  The destination is bounded by the level's size, the footprint by the source's (bloom_clamp)
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom_down(const BloomParams p, const uint32_t k) {
    const uint32_t x = blockIdx.x * BLOOM_BLOCK + threadIdx.x % BLOOM_BLOCK, y = blockIdx.y * BLOOM_BLOCK + threadIdx.x / BLOOM_BLOCK;
    if (x >= p.layout.w[k] || y >= p.layout.h[k]) return;
    const uint32_t ws = p.layout.w[k - 1], hs = p.layout.h[k - 1];
    const BloomLevel src = {p.down + p.layout.offset[k - 1], ws};
    const auto texel = [&](uint32_t i, uint32_t j, float *c) { src(bloom_clamp((int32_t)(2 * x + i) - 2, ws), bloom_clamp((int32_t)(2 * y + j) - 2, hs), c); };
    float out[3];
    bloom_down<false>(texel, out);
    *reinterpret_cast<f3v *>(p.down + p.layout.offset[k] + ((size_t)y * p.layout.w[k] + x) * 3) = (f3v){out[0], out[1], out[2]};
}

// U_level from D_level and U_{level+1} (D_L when level + 1 = L); k = level - 1 indexes the layout
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom_up(const BloomParams p, const uint32_t k) {
    const uint32_t x = blockIdx.x * BLOOM_BLOCK + threadIdx.x % BLOOM_BLOCK, y = blockIdx.y * BLOOM_BLOCK + threadIdx.x / BLOOM_BLOCK;
    if (x >= p.layout.w[k] || y >= p.layout.h[k]) return;
    const BloomLevel coarse = {(k + 2 == p.d.levels ? p.down : p.up) + p.layout.offset[k + 1], p.layout.w[k + 1]};
    const size_t o = p.layout.offset[k] + ((size_t)y * p.layout.w[k] + x) * 3;
    float t[3], dk[3], out[3];
    bloom_up(x, y, p.layout.w[k + 1], p.layout.h[k + 1], coarse, t);
    const f3v h = *reinterpret_cast<const f3v *>(p.down + o);   // D_k of this pixel
    dk[0] = h.x; dk[1] = h.y; dk[2] = h.z;
    bloom_up_add(p.d, dk, t, out);
    *reinterpret_cast<f3v *>(p.up + o) = (f3v){out[0], out[1], out[2]};
}

template <class Color>
__global__ __launch_bounds__(BLOOM_THREADS) void k_bloom_composite(const BloomParams p, const Color color) {
    const uint32_t x = blockIdx.x * BLOOM_BLOCK + threadIdx.x % BLOOM_BLOCK, y = blockIdx.y * BLOOM_BLOCK + threadIdx.x / BLOOM_BLOCK;
    if (x >= p.width || y >= p.rows) return;
    const BloomLevel u1 = {p.d.levels == 1u ? p.down : p.up, p.layout.w[0]};
    const size_t o = (size_t)y * p.width + x;
    float t[3], c[3], out[3];
    bloom_up(x, y, p.layout.w[0], p.layout.h[0], u1, t);
    color(x, y, c);
    bloom_composite(p.d, c, t, out);
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){out[0], out[1], out[2]};
    const f3 m = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(m.x, p.inv_gamma), l1 = gamma_curve(m.y, p.inv_gamma), l2 = gamma_curve(m.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

dim3 bloom_grid(uint32_t w, uint32_t h) { return dim3((w + BLOOM_BLOCK - 1) / BLOOM_BLOCK, (h + BLOOM_BLOCK - 1) / BLOOM_BLOCK); }
bool bloom_level_ok(const BloomParams &p, uint32_t level) { return level >= 1 && level <= p.d.levels && p.d.levels == p.layout.levels && p.d.levels <= BLOOM_MAX_LEVELS; }

}  // namespace

hipError_t launch_bloom_down_first(const BloomParams &p, hipStream_t s) {
    if (!bloom_level_ok(p, 1)) return hipErrorInvalidValue;
    if (p.width == 0 || p.rows == 0) return hipSuccess;
    const dim3 grid = bloom_grid(p.layout.w[0], p.layout.h[0]);
    if (p.color_taa) k_bloom_down_first<<<grid, BLOOM_THREADS, 0, s>>>(p, BloomHistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_bloom_down_first<<<grid, BLOOM_THREADS, 0, s>>>(p, BloomPlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

hipError_t launch_bloom_down(const BloomParams &p, uint32_t level, hipStream_t s) {
    if (!bloom_level_ok(p, level) || level < 2) return hipErrorInvalidValue;
    if (p.width == 0 || p.rows == 0) return hipSuccess;
    k_bloom_down<<<bloom_grid(p.layout.w[level - 1], p.layout.h[level - 1]), BLOOM_THREADS, 0, s>>>(p, level - 1);
    return hipGetLastError();
}

hipError_t launch_bloom_up(const BloomParams &p, uint32_t level, hipStream_t s) {
    if (!bloom_level_ok(p, level) || level >= p.d.levels) return hipErrorInvalidValue;
    if (p.width == 0 || p.rows == 0) return hipSuccess;
    k_bloom_up<<<bloom_grid(p.layout.w[level - 1], p.layout.h[level - 1]), BLOOM_THREADS, 0, s>>>(p, level - 1);
    return hipGetLastError();
}

hipError_t launch_bloom_composite(const BloomParams &p, hipStream_t s) {
    if (!bloom_level_ok(p, 1)) return hipErrorInvalidValue;
    if (p.width == 0 || p.rows == 0) return hipSuccess;
    const dim3 grid = bloom_grid(p.width, p.rows);
    if (p.color_taa) k_bloom_composite<<<grid, BLOOM_THREADS, 0, s>>>(p, BloomHistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_bloom_composite<<<grid, BLOOM_THREADS, 0, s>>>(p, BloomPlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

}  // namespace arctic
