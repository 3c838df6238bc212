// ray_ao.hip -- ambient occlusion from the resident G-buffer (arctic_trace_ambient_occlusion; the arithmetic is written once, in
// include/arctic_hip.h in front of the call, and carried out by ray_ao.h and ray_query.h -- the very functions the host arbiter
// arctic_ambient_occlusion_points runs):
//   k_trace_ao     n_rays short any-hit rays per pixel over the hemisphere of its normal; a wave is one 8x8 tile as in k_trace_sun (the same 1 KiB
//                  loads of planes c and e, the same de-tiling of the one byte it stores per pixel); the lane loops over its rays
//   k_ao_filter    the edge-aware sum over the P x P window of the interleave pattern: the hits plane and planes b, c, e of up to 15 neighbours
// The walk is rq_walk unchanged: the node index strictly increases, so there is no stack and a corrupt structure cannot hang the device.  Per ray
// the WAVE chooses the plain or the odd walk by ballot, as trace.hip does.  The direction table (at most 12 KiB) is read through the vector cache:
// a wave's 64 lanes read at most P * P = 16 distinct 12-byte entries per ray, the table is small against a CU's 32 KiB L1, and the three loads
// stand in front of a walk of hundreds of instructions -- staging it in LDS would add a barrier and a block-wide copy to save nothing that
// shows.  No LDS, no barrier, no atomics; vector stores only.  Compiled with contraction off: every operation of the definition rounds once.
#include "common.h"
#include "ray_ao.h"

namespace arctic {

namespace {

constexpr uint32_t AO_THREADS = 256;

// trace.hip's choice of the walk: wave-uniform, the odd walk when any valid lane carries an odd ray
__device__ __forceinline__ bool any_hit_wave(const RayPrep &r, const RayNode *__restrict__ nodes, const RayTri *__restrict__ tris, uint32_t n_nodes) {
    RayOut h = {0.0f, 0.0f, 0.0f, RAY_NO_PRIM};
    if (__builtin_amdgcn_ballot_w64(r.valid && r.odd) != 0ull) {
        if (r.valid) h = rq_walk<true, true>(r, nodes, tris, n_nodes);
    } else {
        if (r.valid) h = rq_walk<true, false>(r, nodes, tris, n_nodes);
    }
    return h.prim != RAY_NO_PRIM;
}

// the pixel at px of the tile-major planes: covered?  m: its unit normal
__device__ __forceinline__ bool ao_pixel(const float *__restrict__ plane_b, const float4 *__restrict__ plane_e, size_t px, float *m) {
    const uint32_t mat = __builtin_bit_cast(uint32_t, plane_b[px * 3 + 2]);
    const float4 e = plane_e[px];
    return ao_normal(e.y, e.z, e.w, m) && mat != NO_MATERIAL;
}

// Lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)) of the shard's tile rows; row r of the shard is tile-row pixel r + row0_in_tile
// and row frame_row0 + r of the frame.  n_rays is wave-uniform, so every lane of a wave reaches every ballot
__global__ __launch_bounds__(AO_THREADS) void k_trace_ao(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                         uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t row0_in_tile, uint32_t frame_row0,
                                                         uint32_t n_rays, uint32_t pattern, float radius, float bias, const float *__restrict__ dirs,
                                                         const RayNode *__restrict__ nodes, const RayTri *__restrict__ tris, uint32_t n_nodes, int as_result,
                                                         uint8_t *__restrict__ out) {
    const uint32_t tile = blockIdx.x * (AO_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), yy = (tile / tiles_x) * TILE + (lane >> 3);
    const bool stored = x < width && yy >= row0_in_tile && yy - row0_in_tile < rows;
    const size_t px = (size_t)tile * TILE_PIXELS + lane;
    const float4 c = plane_c[px];
    float m[3], t[3], bt[3], o[3];
    const bool covered = ao_pixel(plane_b, plane_e, px, m) && stored;
    const float world[3] = {c.x, c.y, c.z};
    ao_frame(m, t, bt);
    ao_origin(world, m, bias, o);
    // (a lane that is not stored may wrap here: the set stays below pattern * pattern, the loads inside the table)
    const float *l = dirs + (size_t)ao_set(x, frame_row0 + (yy - row0_in_tile), pattern) * n_rays * 3;
    uint32_t hits = 0;
    for (uint32_t k = 0; k < n_rays; ++k, l += 3) {
        const float local[3] = {l[0], l[1], l[2]};
        RayPrep r = rq_prepare(ao_ray(o, m, t, bt, local, radius));
        r.valid = r.valid && covered;
        hits += any_hit_wave(r, nodes, tris, n_nodes) ? 1u : 0u;
    }
    if (stored) out[(size_t)(yy - row0_in_tile) * width + x] = (uint8_t)(as_result ? ao_result(n_rays - hits, n_rays) : hits);
}

// Whole frames only (row0_in_tile = 0, rows = the frame's height): pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile (y / 8) * tiles_x + x / 8
__global__ __launch_bounds__(AO_THREADS) void k_ao_filter(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                          uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t n_rays, uint32_t pattern,
                                                          float normal_cos, float plane_dist, const uint8_t *__restrict__ hits, uint8_t *__restrict__ out) {
    const uint32_t tile = blockIdx.x * (AO_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), y = (tile / tiles_x) * TILE + (lane >> 3);
    if (x >= width || y >= rows) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane;
    float mp[3];
    uint32_t result = 255u;
    if (ao_pixel(plane_b, plane_e, px, mp)) {
        const float4 c = plane_c[px];
        const float wp[3] = {c.x, c.y, c.z};
        uint32_t V = n_rays - hits[(size_t)y * width + x], accepted = 1;
        const int32_t lo = -(int32_t)(pattern / 2);
        for (int32_t j = lo; j < lo + (int32_t)pattern; ++j) {
            for (int32_t i = lo; i < lo + (int32_t)pattern; ++i) {
                const int32_t qx = (int32_t)x + i, qy = (int32_t)y + j;
                if ((i == 0 && j == 0) || qx < 0 || qy < 0 || qx >= (int32_t)width || qy >= (int32_t)rows) continue;
                const size_t q = ((size_t)((uint32_t)qy / TILE) * tiles_x + (uint32_t)qx / TILE) * TILE_PIXELS + ((uint32_t)qy % TILE) * TILE + (uint32_t)qx % TILE;
                float mq[3];
                if (!ao_pixel(plane_b, plane_e, q, mq)) continue;
                const float4 cq = plane_c[q];
                const float wq[3] = {cq.x, cq.y, cq.z};
                if (!ao_accepts(mp, wp, mq, wq, normal_cos, plane_dist)) continue;
                V += n_rays - hits[(size_t)qy * width + qx];
                ++accepted;
            }
        }
        result = ao_result(V, n_rays * accepted);
    }
    out[(size_t)y * width + x] = (uint8_t)result;
}

}  // namespace

hipError_t launch_trace_ao(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                           uint32_t row0_in_tile, uint32_t frame_row0, const AoDesc &ao, const float *d_dirs, const void *nodes, const void *tris, uint32_t n_nodes,
                           int as_result, uint8_t *out, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y, per = AO_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_trace_ao<<<(n_tiles + per - 1) / per, AO_THREADS, 0, s>>>(plane_b, static_cast<const float4 *>(plane_c), static_cast<const float4 *>(plane_e), n_tiles, tiles_x, width, rows,
                                                                row0_in_tile, frame_row0, ao.n_rays, ao.pattern, ao.radius, ao.bias, d_dirs, static_cast<const RayNode *>(nodes),
                                                                static_cast<const RayTri *>(tris), n_nodes, as_result, out);
    return hipGetLastError();
}

hipError_t launch_ao_filter(const float *plane_b, const void *plane_c, const void *plane_e, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows,
                            const AoDesc &ao, const uint8_t *hits, uint8_t *out, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y, per = AO_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_ao_filter<<<(n_tiles + per - 1) / per, AO_THREADS, 0, s>>>(plane_b, static_cast<const float4 *>(plane_c), static_cast<const float4 *>(plane_e), n_tiles, tiles_x, width, rows,
                                                                 ao.n_rays, ao.pattern, ao.normal_cos, ao.plane_dist, hits, out);
    return hipGetLastError();
}

}  // namespace arctic
