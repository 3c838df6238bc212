// motion.hip -- per-pixel motion vectors and the accumulation that uses them (arctic_motion_vectors_device,
// arctic_accumulate_ambient_occlusion_motion_device, arctic_pass_ray_effects_motion; the arithmetic is written once, in include/arctic_hip.h in front
// of the calls, and carried out by motion.h -- the very functions the host arbiters arctic_motion_pixels and arctic_accumulate_pixels_motion run):
//   k_motion                 a wave is one 8x8 tile of the tile-major visibility plane, as in k_resolve.  A covered pixel finds its record and its
//                            source triangle as k_resolve does (rec_of, source_barycentrics, ObjectRec::indices), reads the call's MotionObject of
//                            its object and the three PREVIOUS object-space positions, and stores where the point lay in the previous call and
//                            the offset to it on the screen.  A pixel reads no neighbour, so row ranges and band shards run it as they run k_resolve.
//   k_motion_snapshot        a thread is one vertex: its position out of the vertex buffer in use (56 B apart) into the mesh's float4 snapshot.
//   k_ao_accumulate_motion   k_ao_accumulate (ao_history.hip) with one more load per pixel, the previous point, which the reprojection and the plane
//                            test take in place of the current one.
// Per pixel k_motion reads 8 B of visibility and, covered, a gather: 4 B of rec_of, the SetupRec's and RasterRec's fields source_barycentrics uses,
// 12 B of indices, the MotionObject and 3 x 12 B of positions -- a tile's 64 pixels mostly share a handful of triangles, so the gather is served by
// the cache --, and writes 16 B (+ 8 B of velocity).  No LDS, no barrier, no atomics; vector stores only.  Compiled with contraction off: every
// operation of the definition rounds once.
#include "common.h"
#include "edges.h"
#include "motion.h"

namespace arctic {

namespace {

constexpr uint32_t MOTION_THREADS = 256;

// Every index is bounded before it is used: the tile by n_tiles, the stored pixel by the frame's width and the handle's rows, the object by the
// call's table, the triangle by the object's count, a vertex by the mesh's count.  (rec_of, recs and the prepass's own object table are read as
// k_resolve reads them: the prepass that wrote the keys wrote them.)
__global__ __launch_bounds__(MOTION_THREADS) void k_motion(const MotionParams p) {
    const uint32_t tile = blockIdx.x * (MOTION_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= p.n_tiles) return;   // (whole waves: a wave is one tile)
    const uint32_t x = (tile % p.gp.tiles_x) * TILE + (lane & 7u), yy = (tile / p.gp.tiles_x) * TILE + (lane >> 3);
    if (!(x < p.width && yy >= p.row0_in_tile && yy - p.row0_in_tile < p.rows)) return;   // (a tile's padding: not a pixel of the handle's rows)
    const size_t o = (size_t)(yy - p.row0_in_tile) * p.width + x;
    const unsigned long long key = p.vis[(size_t)tile * TILE_PIXELS + lane];
    float pw4[4] = {0.0f, 0.0f, 0.0f, MOTION_NONE}, vel[2] = {0.0f, 0.0f}, B[3] = {0.0f, 0.0f, 0.0f};
    uint4 src = make_uint4(MOTION_NO_OBJECT, 0u, 0u, 0u);
    if (key != ~0ull) {
        const uint32_t ri = p.rec_of[(uint32_t)key];   // low word = order id (k_setup)
        const SetupRec &t = p.recs[ri];
        const int32_t tx = (int32_t)(tile % (uint32_t)p.gp.tiles_x);
        const int32_t ty = row_global((int)(tile / (uint32_t)p.gp.tiles_x), p.gp.band_tiles, p.gp.shard_count, p.gp.shard_index) + p.gp.tile_y0;
        const int32_t px = tx * 8 + (int32_t)(lane & 7), py = ty * 8 + (int32_t)(lane >> 3);
        source_barycentrics(t, p.rrecs[ri], px, py, B);
        const ObjectRec &ob = p.objs[t.object];
        const uint32_t lt = t.src_tri - ob.first_triangle;
        if (lt < ob.n_triangles) {
            const uint32_t i0 = ob.indices[3 * lt], i1 = ob.indices[3 * lt + 1], i2 = ob.indices[3 * lt + 2];
            src = make_uint4(t.object, i0, i1, i2);
            if (t.object < p.n_objs) {
                const MotionObject &mo = p.mobjs[t.object];
                src.x = mo.scene_object;
                const bool has_prev = mo.has_prev != 0u && i0 < mo.n_vertices && i1 < mo.n_vertices && i2 < mo.n_vertices;
                float q[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
                if (has_prev) {
                    const uint32_t ix[3] = {i0, i1, i2};
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float *v = mo.prev + (size_t)ix[k] * mo.stride;
                        q[k][0] = v[0]; q[k][1] = v[1]; q[k][2] = v[2];
                    }
                }
                mo_pixel(has_prev, mo.prev_trs, q[0], q[1], q[2], B, p.P, p.width, p.height, px, py, pw4, vel);
            }
        }
    }
    p.prev_world4[o] = make_float4(pw4[0], pw4[1], pw4[2], pw4[3]);
    if (p.velocity2) p.velocity2[o] = make_float2(vel[0], vel[1]);
    if (p.bary3) { p.bary3[3 * o] = B[0]; p.bary3[3 * o + 1] = B[1]; p.bary3[3 * o + 2] = B[2]; }
    if (p.source4) p.source4[o] = src;
}

__global__ __launch_bounds__(MOTION_THREADS) void k_motion_snapshot(const float *__restrict__ vertices, uint32_t n, float4 *__restrict__ snapshot) {
    const uint32_t i = blockIdx.x * MOTION_THREADS + threadIdx.x;
    if (i >= n) return;
    const float *v = vertices + (size_t)i * 14;
    snapshot[i] = make_float4(v[0], v[1], v[2], 0.0f);
}

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

// Whole frames only, like k_ao_accumulate: pixel (x, y) is lane (y & 7) * 8 + (x & 7) of tile (y / 8) * tiles_x + x / 8.  Every index is bounded
// before it is used: the tile by n_tiles, the pixel by the frame's width and rows, a tap by the frame inside aoh_pixel_motion
__global__ __launch_bounds__(MOTION_THREADS) void k_ao_accumulate_motion(const AoHistoryParams p, const float4 *__restrict__ prev_world4) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y;
    const uint32_t tile = blockIdx.x * (MOTION_THREADS / TILE_PIXELS) + threadIdx.x / TILE_PIXELS, lane = threadIdx.x % TILE_PIXELS;
    if (tile >= n_tiles) return;
    const uint32_t x = (tile % p.tiles_x) * TILE + (lane & 7u), y = (tile / p.tiles_x) * TILE + (lane >> 3);
    if (x >= p.width || y >= p.rows) return;
    const size_t px = (size_t)tile * TILE_PIXELS + lane, o = (size_t)y * p.width + x;
    const uint32_t mat = __builtin_bit_cast(uint32_t, p.plane_b[px * 3 + 2]);
    const float4 e = static_cast<const float4 *>(p.plane_e)[px], c = static_cast<const float4 *>(p.plane_c)[px], pw = prev_world4[o];
    const float n[3] = {e.y, e.z, e.w}, w[3] = {c.x, c.y, c.z}, pw4[4] = {pw.x, pw.y, pw.z, pw.w};
    const float cur = (float)p.ao_in[o];
    const TiledFetch fetch = {static_cast<const float4 *>(p.prev_a), static_cast<const float4 *>(p.prev_b), p.tiles_x};
    AoHistoryEntry h;
    const uint32_t byte = aoh_pixel_motion(mat != NO_MATERIAL, n, w, pw4, cur, p.prev_a ? p.P : nullptr, p.width, p.rows, p.d, fetch, h);
    p.ao_out[o] = (uint8_t)byte;
    static_cast<float4 *>(p.next_a)[px] = make_float4(h.world[0], h.world[1], h.world[2], h.value);
    static_cast<float4 *>(p.next_b)[px] = make_float4(h.m[0], h.m[1], h.m[2], h.count);
}

}  // namespace

hipError_t launch_motion(const MotionParams &p, hipStream_t s) {
    const uint32_t per = MOTION_THREADS / TILE_PIXELS;
    if (p.n_tiles == 0) return hipSuccess;
    k_motion<<<(p.n_tiles + per - 1) / per, MOTION_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_motion_snapshot(const float *vertices, uint32_t n, void *snapshot, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_motion_snapshot<<<(n + MOTION_THREADS - 1) / MOTION_THREADS, MOTION_THREADS, 0, s>>>(vertices, n, static_cast<float4 *>(snapshot));
    return hipGetLastError();
}

hipError_t launch_ao_accumulate_motion(const AoHistoryParams &p, const void *prev_world4, hipStream_t s) {
    const uint32_t n_tiles = p.tiles_x * p.tiles_y, per = MOTION_THREADS / TILE_PIXELS;
    if (n_tiles == 0) return hipSuccess;
    k_ao_accumulate_motion<<<(n_tiles + per - 1) / per, MOTION_THREADS, 0, s>>>(p, static_cast<const float4 *>(prev_world4));
    return hipGetLastError();
}

}  // namespace arctic
