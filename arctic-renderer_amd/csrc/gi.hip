// gi.hip -- one bounce of indirect diffuse light from the resident G-buffer (arctic_trace_gi; the arithmetic is written once, in
// include/arctic_hip.h in front of the call, and carried out by gi.h and ray_ao.h -- the very functions the host arbiters arctic_gi_points and
// arctic_gi_estimate_pixels run):
//   k_gi_rays       G-buffer planes b, c, e -> round k's ray of every pixel of the handle's rows, into the reflection plane's ray buffer; a wave
//                   is one 8x8 tile as in k_reflect_rays (the same 1 KiB loads of planes c and e, the same row-major records)
//   k_gi_add        streaming, grid-stride over the pixels: the round's colour, sanitised by selects, into the float4 sum S (round 0 stores)
//   k_gi_accumulate the occlusion history's kernel with a colour for a value: reprojection through the previous call's matrix, four taps of three
//                   float4 each from the previous history, every pixel stores {acc, N} and its entry of the new history (tile-major)
//   k_gi_compose    k_compose's shape: the pixel's HDR colour, its material's channels (material_sampler.h), the ambient correction and
//                   base * E, then the shared tonemapper (post_process.h) to RGBA8, float LDR and float HDR
//   k_gi_estimate   E = S.rgb / S.cnt, streaming; or, filtered, over the P x P window of the pattern: a wave stages S, the unit normals and the
//                   world positions of its 8x8 tile and the window's halo (at most 11 x 11 cells of 48 bytes) in LDS once, so that the up to
//                   15 neighbours of a pixel cost LDS reads, not 48 bytes of global loads each
// The closest-hit walk and the radiance between k_gi_rays and k_gi_add are trace.hip's and hit_shade.hip's kernels, unchanged.  The direction
// table (at most 3 KiB) is read through the vector cache as in k_trace_ao.  One barrier, in the filtered estimate, reached by every thread; no
// atomics; vector stores only.  Compiled with contraction off: every operation of the definition rounds once.
#include "common.h"
#include "gi.h"
#include "material_sampler.h"
#include "post_process.h"

namespace arctic {

namespace {

constexpr uint32_t GI_THREADS = 256;
constexpr uint32_t GI_WAVES = GI_THREADS / TILE_PIXELS;
constexpr uint32_t GI_MAX_BLOCKS = 256 * 8;      // the grid-stride loops' grid: 8 workgroups per CU of the largest part
constexpr uint32_t GI_SPAN = TILE + 3;           // a tile and the halo of the widest window (P = 4: offsets -2..1)
constexpr uint32_t GI_CELLS = GI_SPAN * GI_SPAN;

// the pixel at px of the tile-major planes: has it geometry?
__device__ __forceinline__ bool gi_geometry(const float *__restrict__ plane_b, size_t px) { return __builtin_bit_cast(uint32_t, plane_b[px * 3 + 2]) != NO_MATERIAL; }
__device__ __forceinline__ GiSum gi_load(const float4 *p) { const float4 v = *p; return GiSum{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 gi_f4(const GiSum &s) { return make_float4(s.r, s.g, s.b, s.cnt); }

// Lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)) of the shard's tile rows; row r of the shard is tile-row pixel r + row0_in_tile
// and row frame_row0 + r of the frame
__global__ __launch_bounds__(GI_THREADS) void k_gi_rays(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                        uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t row0_in_tile, uint32_t frame_row0,
                                                        uint32_t n_rays, uint32_t pattern, float max_distance, float bias, uint32_t round,
                                                        const float *__restrict__ dirs, RayIn *__restrict__ rays) {
    const uint32_t tile = blockIdx.x * GI_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), yy = (tile / tiles_x) * TILE + (lane >> 3);
    if (!(x < width && yy >= row0_in_tile && yy - row0_in_tile < rows)) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane;
    const float4 c = plane_c[px], e = plane_e[px];
    const float world[3] = {c.x, c.y, c.z}, n[3] = {e.y, e.z, e.w};
    const float *l = dirs + ((size_t)ao_set(x, frame_row0 + (yy - row0_in_tile), pattern) * n_rays + round) * 3;   // (the set stays below pattern * pattern, round below n_rays)
    const float local[3] = {l[0], l[1], l[2]};
    RayIn r;
    gi_ray(world, n, gi_geometry(plane_b, px), local, bias, max_distance, r);
    rq_f4 *dst = reinterpret_cast<rq_f4 *>(rays + ((size_t)(yy - row0_in_tile) * width + x));
    dst[0] = (rq_f4){r.o[0], r.o[1], r.o[2], r.t_min};
    dst[1] = (rq_f4){r.d[0], r.d[1], r.d[2], r.t_max};
}

// 16 bytes of the record ({direction, t_max}: did the pixel have a ray?), 16 of the colour, 16 of S in (not in round 0), 16 out
__global__ __launch_bounds__(GI_THREADS) void k_gi_add(const RayIn *__restrict__ rays, const float4 *__restrict__ colors, uint64_t n, float clamp_max, uint32_t round,
                                                       float4 *__restrict__ S) {
    for (uint64_t k = (uint64_t)blockIdx.x * GI_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * GI_THREADS) {
        const rq_f4 rd = reinterpret_cast<const rq_f4 *>(rays + k)[1];
        const float4 c = colors[k];
        GiSum s = {0.0f, 0.0f, 0.0f, 0.0f};
        if (round != 0) s = gi_load(S + k);
        S[k] = gi_f4(gi_add(s, round == 0, gi_had_ray(rd[3]), c.x, c.y, c.z, clamp_max));
    }
}

__global__ __launch_bounds__(GI_THREADS) void k_gi_estimate(const float4 *__restrict__ S, uint64_t n, float4 *__restrict__ E) {
    for (uint64_t k = (uint64_t)blockIdx.x * GI_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * GI_THREADS) E[k] = gi_f4(gi_estimate(gi_load(S + k)));
}

// The filtered form.  Whole frames only (row0_in_tile = 0, rows = the frame's height): pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile
// (y / 8) * tiles_x + x / 8.  Cell (cx, cy) of a wave's LDS is pixel (x0 + lo + cx, y0 + lo + cy): {S}, {m, covered}, {world}.  A cell outside
// the frame is not covered.  Every thread reaches the barrier; a wave behind the last tile stages nothing
__global__ __launch_bounds__(GI_THREADS) void k_gi_estimate_window(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                                   uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t pattern, float normal_cos,
                                                                   float plane_dist, const float4 *__restrict__ S, float4 *__restrict__ E) {
    __shared__ float4 cells[GI_WAVES][3][GI_CELLS];
    const uint32_t wave = threadIdx.x / TILE_PIXELS, tile = blockIdx.x * GI_WAVES + wave, lane = threadIdx.x % TILE_PIXELS;
    const bool live = tile < n_tiles;
    const int32_t lo = gi_window_lo(pattern);
    const uint32_t span = TILE + pattern - 1;   // (<= GI_SPAN: pattern <= 4)
    const int32_t x0 = (int32_t)((tile % tiles_x) * TILE), y0 = (int32_t)((tile / tiles_x) * TILE);
    if (live) {
        for (uint32_t cell = lane; cell < span * span; cell += TILE_PIXELS) {
            const int32_t qx = x0 + lo + (int32_t)(cell % span), qy = y0 + lo + (int32_t)(cell / span);
            float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mm = s, ww = s;
            if (qx >= 0 && qy >= 0 && qx < (int32_t)width && qy < (int32_t)rows) {
                const size_t q = ((size_t)((uint32_t)qy / TILE) * tiles_x + (uint32_t)qx / TILE) * TILE_PIXELS + ((uint32_t)qy % TILE) * TILE + (uint32_t)qx % TILE;
                const float4 e = plane_e[q], c = plane_c[q];
                float m[3];
                const bool covered = ao_normal(e.y, e.z, e.w, m) && gi_geometry(plane_b, q);
                s = S[(size_t)qy * width + qx];
                mm = make_float4(m[0], m[1], m[2], covered ? 1.0f : 0.0f);
                ww = make_float4(c.x, c.y, c.z, 0.0f);
            }
            cells[wave][0][cell] = s; cells[wave][1][cell] = mm; cells[wave][2][cell] = ww;
        }
    }
    __syncthreads();
    const uint32_t x = (uint32_t)x0 + (lane & 7u), y = (uint32_t)y0 + (lane >> 3);
    if (!live || x >= width || y >= rows) return;
    const uint32_t own = ((lane >> 3) - lo) * span + (lane & 7u) - lo;
    const float4 pm = cells[wave][1][own], pw = cells[wave][2][own];
    GiSum acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (pm.w != 0.0f) {
        const float mp[3] = {pm.x, pm.y, pm.z}, wp[3] = {pw.x, pw.y, pw.z};
        for (int32_t j = 0; j < (int32_t)pattern; ++j) {
            for (int32_t i = 0; i < (int32_t)pattern; ++i) {
                const uint32_t cell = ((lane >> 3) + j) * span + (lane & 7u) + i;   // pixel (x + lo + i, y + lo + j)
                bool accept = cell == own;
                if (!accept) {
                    const float4 qm = cells[wave][1][cell], qw = cells[wave][2][cell];
                    const float mq[3] = {qm.x, qm.y, qm.z}, wq[3] = {qw.x, qw.y, qw.z};
                    accept = qm.w != 0.0f && ao_accepts(mp, wp, mq, wq, normal_cos, plane_dist);
                }
                if (accept) {   // (a select: a rejected pixel's S is not looked at)
                    const float4 s = cells[wave][0][cell];
                    acc = GiSum{acc.r + s.x, acc.g + s.y, acc.b + s.z, acc.cnt + s.w};
                }
            }
        }
    }
    E[(size_t)y * width + x] = gi_f4(gi_estimate(acc));
}

// the previous history's entry of the pixel at (qx, qy) of the frame; the caller has bounded both by the frame, so the index is inside the planes
struct GiTiledFetch {
    const float4 *a, *b, *c;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, GiHistoryEntry &e) const {
        const size_t q = ((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE;
        const float4 ha = a[q], hb = b[q], hc = c[q];
        e.world[0] = ha.x; e.world[1] = ha.y; e.world[2] = ha.z; e.count = ha.w;
        e.m[0] = hb.x; e.m[1] = hb.y; e.m[2] = hb.z;
        e.acc[0] = hc.x; e.acc[1] = hc.y; e.acc[2] = hc.z;
    }
};

// k_ao_accumulate's shape.  Whole frames only.  Every index is bounded before it is used: the tile by n_tiles, the pixel by the frame's width and
// rows, a tap by the frame inside gih_pixel
__global__ __launch_bounds__(GI_THREADS) void k_gi_accumulate(const GiHistoryParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * GI_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)y * p.width + x;
    const float4 e = static_cast<const float4 *>(p.plane_e)[px], c = static_cast<const float4 *>(p.plane_c)[px];
    const float n[3] = {e.y, e.z, e.w}, w[3] = {c.x, c.y, c.z};
    const GiSum cur = gi_load(static_cast<const float4 *>(p.gi_in) + o);
    const GiTiledFetch fetch = {static_cast<const float4 *>(p.prev[0]), static_cast<const float4 *>(p.prev[1]), static_cast<const float4 *>(p.prev[2]), p.tiles_x};
    GiHistoryEntry h;
    const GiSum out = gih_pixel(gi_geometry(p.plane_b, px), n, w, cur, p.prev[0] ? p.P : nullptr, p.width, p.rows, p.d, fetch, h);
    static_cast<float4 *>(p.gi_out)[o] = gi_f4(out);
    static_cast<float4 *>(p.next[0])[px] = make_float4(h.world[0], h.world[1], h.world[2], h.count);
    static_cast<float4 *>(p.next[1])[px] = make_float4(h.m[0], h.m[1], h.m[2], 0.0f);
    static_cast<float4 *>(p.next[2])[px] = make_float4(h.acc[0], h.acc[1], h.acc[2], 0.0f);
}

// k_compose's shape: a wave is one 8x8 tile.  Every pixel reads its HDR colour and its material; a pixel with geometry reads its uv (plane a),
// samples the material's channels (material_sampler.h: level 0, the default sampler) and its E.  Then post_process and three stores
__global__ __launch_bounds__(GI_THREADS) void k_gi_compose(const GiComposeParams p) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * GI_WAVES + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), yy = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (!(x < p.width && yy >= p.row0_in_tile && yy - p.row0_in_tile < p.rows)) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)(yy - p.row0_in_tile) * p.width + x;
    const uint32_t mat = __builtin_bit_cast(uint32_t, p.plane_b[px * 3 + 2]);
    const f3v h = *reinterpret_cast<const f3v *>(p.hdr + o * 3);
    float C[3] = {h.x, h.y, h.z};
    if (mat < p.n_materials) {   // (NO_MATERIAL, and an index the handle has no material for: k_compose's test of "covered")
        const float4 a = static_cast<const float4 *>(p.plane_a)[px];
        const Channels ch = sample_material(p.tex, p.srgb_lut, mat, a.x, a.y);
        const rq_f4 g = static_cast<const rq_f4 *>(p.gi)[o];
        const float E[3] = {g[0], g[1], g[2]};
        gi_compose_ambient(C, ch.base, p.ambient, p.ambient_scale);
        if (gi_compose_lit(g[3])) gi_compose_indirect(C, ch.base, ch.metal, p.gi_strength, E);
    }
    const f3 t = tonemap(mk(C[0], C[1], C[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(t.x, p.inv_gamma), l1 = gamma_curve(t.y, p.inv_gamma), l2 = gamma_curve(t.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){C[0], C[1], C[2]};
}

uint32_t gi_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + GI_THREADS - 1) / GI_THREADS, GI_MAX_BLOCKS); }

}  // namespace

hipError_t launch_gi_rays(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                          uint32_t row0_in_tile, uint32_t frame_row0, const GiDesc &gi, uint32_t round, const float *d_dirs, void *rays, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_gi_rays<<<(n_tiles + GI_WAVES - 1) / GI_WAVES, GI_THREADS, 0, s>>>(plane_b, static_cast<const float4 *>(plane_c), static_cast<const float4 *>(plane_e), n_tiles, tiles_x, width,
                                                                        rows, row0_in_tile, frame_row0, gi.n_rays, gi.pattern, gi.max_distance, gi.bias, round, d_dirs,
                                                                        static_cast<RayIn *>(rays));
    return hipGetLastError();
}

hipError_t launch_gi_add(const void *rays, const void *colors, uint64_t n, float clamp_max, uint32_t round, void *S, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_gi_add<<<gi_grid(n), GI_THREADS, 0, s>>>(static_cast<const RayIn *>(rays), static_cast<const float4 *>(colors), n, clamp_max, round, static_cast<float4 *>(S));
    return hipGetLastError();
}

hipError_t launch_gi_estimate(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                              const GiDesc &gi, const void *S, void *E, hipStream_t s) {
    const uint64_t n = (uint64_t)rows * width;
    const uint32_t n_tiles = tiles_x * tiles_y;
    if (n == 0 || n_tiles == 0) return hipSuccess;
    if (!gi.filter) k_gi_estimate<<<gi_grid(n), GI_THREADS, 0, s>>>(static_cast<const float4 *>(S), n, static_cast<float4 *>(E));
    else k_gi_estimate_window<<<(n_tiles + GI_WAVES - 1) / GI_WAVES, GI_THREADS, 0, s>>>(plane_b, static_cast<const float4 *>(plane_c), static_cast<const float4 *>(plane_e), n_tiles,
                                                                                        tiles_x, width, rows, gi.pattern, gi.normal_cos, gi.plane_dist,
                                                                                        static_cast<const float4 *>(S), static_cast<float4 *>(E));
    return hipGetLastError();
}

hipError_t launch_gi_accumulate(const GiHistoryParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_gi_accumulate<<<(n_tiles + GI_WAVES - 1) / GI_WAVES, GI_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_gi_compose(const GiComposeParams &p, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    if (n_tiles == 0) return hipSuccess;
    k_gi_compose<<<(n_tiles + GI_WAVES - 1) / GI_WAVES, GI_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace arctic
