// trace.hip -- ray queries on the device (arctic_trace_rays / arctic_trace_sun_visibility; the arithmetic is written once, in include/arctic_hip.h
// in front of the calls, and carried out by ray_query.h -- the very functions the host arbiter arctic_trace_triangles runs):
//   k_trace<ANY>      one ArcticRay per lane -> one ArcticHit, each a 16-byte access (32 B in, 16 B out per lane: contiguous per wave)
//   k_trace_sun       one any-hit ray per pixel of the resident G-buffer towards the sun; a wave is one 8x8 tile, so its loads of planes c and e
//                     are 1 KiB contiguous each and its rays start next to each other and run parallel: the most coherent walk there is
// The MI355X has no ray accelerator: the walk is ordinary vector code.  It is the skip-link loop of ray_query.h -- the node index strictly
// increases and the loop ends at n_nodes, so there is NO stack (a runtime-indexed per-lane array would live in scratch), no data-dependent
// `while (true)`, and a corrupt structure cannot hang the device: termination is by construction, not by the data.  A node is two 16-byte
// loads, a leaf triangle three; lanes of a wave that stand at the same node hit the same cache line.  No LDS, no barrier, no atomics; vector
// stores only.  Compiled with contraction off: every operation of the definition rounds once.
//
// Two walks per kernel, chosen per WAVE: a ray with a zero direction component, or one whose reciprocal overflows, can meet 0 * inf in the node
// test and has to look for the NaN (three compares and six selects per node); a wave without such a ray takes the walk without them.
#include "common.h"
#include "ray_query.h"

namespace arctic {

namespace {

constexpr uint32_t TRACE_THREADS = 256;

template <bool ANY>
__device__ __forceinline__ RayOut walk_wave(const RayPrep &r, const RayNode *__restrict__ nodes, const RayTri *__restrict__ tris, uint32_t n_nodes) {
    RayOut h = {0.0f, 0.0f, 0.0f, RAY_NO_PRIM};
    // wave-uniform: does any active lane carry an odd ray?
    if (__builtin_amdgcn_ballot_w64(r.valid && r.odd) != 0ull) {
        if (r.valid) h = rq_walk<ANY, true>(r, nodes, tris, n_nodes);
    } else {
        if (r.valid) h = rq_walk<ANY, false>(r, nodes, tris, n_nodes);
    }
    return h;
}

template <bool ANY>
__global__ __launch_bounds__(TRACE_THREADS) void k_trace(const RayIn *__restrict__ rays, uint64_t n, const RayNode *__restrict__ nodes, const RayTri *__restrict__ tris,
                                                         uint32_t n_nodes, RayOut *__restrict__ hits) {
    const uint64_t g = (uint64_t)blockIdx.x * TRACE_THREADS + threadIdx.x;
    if (g >= n) return;
    const RayIn in = rays[g];
    const RayPrep r = rq_prepare(in);
    hits[g] = walk_wave<ANY>(r, nodes, tris, n_nodes);
}

// G-buffer planes (common.h): b = 3 floats per pixel, the third the material's bits (NO_MATERIAL: no geometry); c = {world.xyz, t.x}; e = {b.z, n.xyz}.
// Lane l of tile (tx, ty) is pixel (8 tx + (l & 7), 8 ty + (l >> 3)) of the shard's tile rows; row r of the shard is tile-row pixel r + row0_in_tile.
__global__ __launch_bounds__(TRACE_THREADS) void k_trace_sun(const float *__restrict__ plane_b, const float4 *__restrict__ plane_c, const float4 *__restrict__ plane_e,
                                                             uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t rows, uint32_t row0_in_tile, float bias,
                                                             float dx, float dy, float dz, const RayNode *__restrict__ nodes, const RayTri *__restrict__ tris,
                                                             uint32_t n_nodes, uint8_t *__restrict__ mask) {
    const uint32_t tile = blockIdx.x * (TRACE_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % tiles_x) * TILE + (lane & 7u), yy = (tile / tiles_x) * TILE + (lane >> 3);
    const bool stored = x < width && yy >= row0_in_tile && yy - row0_in_tile < rows;
    const size_t px = (size_t)tile * TILE_PIXELS + lane;
    const uint32_t mat = __builtin_bit_cast(uint32_t, plane_b[px * 3 + 2]);
    const float4 c = plane_c[px], e = plane_e[px];
    RayIn in;
    in.o[0] = c.x + bias * e.y; in.o[1] = c.y + bias * e.z; in.o[2] = c.z + bias * e.w;
    in.d[0] = dx; in.d[1] = dy; in.d[2] = dz;
    in.t_min = 0.0f; in.t_max = rq_inf();
    RayPrep r = rq_prepare(in);
    r.valid = r.valid && stored && mat != NO_MATERIAL;
    const RayOut h = walk_wave<true>(r, nodes, tris, n_nodes);
    if (stored) mask[(size_t)(yy - row0_in_tile) * width + x] = h.prim == RAY_NO_PRIM ? (uint8_t)255 : (uint8_t)0;
}

}  // namespace

hipError_t launch_trace(const void *rays, uint64_t n, const void *nodes, const void *tris, uint32_t n_nodes, int any, void *hits, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t grid = (uint32_t)((n + TRACE_THREADS - 1) / TRACE_THREADS);   // (the caller keeps n below 2^32)
    if (any) k_trace<true><<<grid, TRACE_THREADS, 0, s>>>(static_cast<const RayIn *>(rays), n, static_cast<const RayNode *>(nodes), static_cast<const RayTri *>(tris), n_nodes, static_cast<RayOut *>(hits));
    else k_trace<false><<<grid, TRACE_THREADS, 0, s>>>(static_cast<const RayIn *>(rays), n, static_cast<const RayNode *>(nodes), static_cast<const RayTri *>(tris), n_nodes, static_cast<RayOut *>(hits));
    return hipGetLastError();
}

hipError_t launch_trace_sun(GBuffer g, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t rows, uint32_t row0_in_tile, float bias, const float minus_sun[3],
                            const void *nodes, const void *tris, uint32_t n_nodes, uint8_t *mask, hipStream_t s) {
    const uint32_t n_tiles = tiles_x * tiles_y, per = TRACE_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_trace_sun<<<(n_tiles + per - 1) / per, TRACE_THREADS, 0, s>>>(g.b, g.c, g.e, n_tiles, tiles_x, width, rows, row0_in_tile, bias, minus_sun[0], minus_sun[1], minus_sun[2],
                                                                   static_cast<const RayNode *>(nodes), static_cast<const RayTri *>(tris), n_nodes, mask);
    return hipGetLastError();
}

}  // namespace arctic
