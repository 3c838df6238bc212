// ray_resplit.hip -- the ray structure is split again for the pose the scene has NOW, on the device (include/arctic_hip.h: "a re-split structure" is
// the definition; bvh.cpp's bvh_resplit is the same thing on the host).  The builder's topology depends on the slot count alone (ray_query.h:
// rq_segment), so nothing but the ORDER of the triangles in the slots is computed here; launch_ray_refit then fills slots and boxes as ever.
//   k_resplit_prims      per slot: its prim and its slot number, the input of the one sort by prim
//   k_resplit_centroids  per triangle IN PRIM ORDER ("item" below = a triangle's rank by prim): the world triangle from its source record, its box
//                        centroid as three order-preserving keys (RQ_KEY_DEAD when a float of it is not finite), a copy of the source record
//   k_resplit_assign     per slot position of the order so far: the segment of the level at hand (arithmetic on the position), noted per item, and
//                        -- where the segment is still to be split -- the item's live keys into the segment's min / max (32-bit vector atomics, one
//                        per wave where the wave lies in one segment)
//   k_resplit_keys       per item: its segment's axis from that table (the definition's fp32 subtraction and strict >), and the 64-bit sort key
//                        segment << 32 | key[axis]; a segment that is a leaf already sorts by its number alone
//   k_resplit_apply      per slot: the source record and the prim of the item the last sort put there
// The sorts are rocprim's device radix sort (LSD, stable: onesweep passes, or its single-block sort for small counts), always FROM PRIM ORDER, so a
// tie between keys falls to the prim without the prim being part of the key; sorting a whole segment refines the builder's nth_element (the
// halves are the same sets).  The pass after the last split sorts by the leaf alone: prim order inside every leaf.  One sort per level, bits
// [0, 32 + bits of the slot count).  Everything is enqueued on one stream; nothing is read back.
// Bounds: every loop is bounded by a host-made count clamped to its structural limit; every item or slot number read from memory is compared
// with the count before use; no scratch in the kernels of this file, vector stores only.  Compiled with contraction off: a centroid rounds as in
// bvh_build.
#include "common.h"
#include "ray_query.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace arctic {

namespace {

constexpr uint32_t RESPLIT_BLOCK = 256;
constexpr uint32_t RESPLIT_LEVELS_MAX = 32;   // (2^29 slots split 27 times)

typedef const float __attribute__((address_space(1))) *GlobalFloats;

// the workspace, carved on the host: every part 256-byte aligned
struct Workspace {
    uint32_t *prim_in, *prim, *slot_in, *slot;   // per slot -> sorted by prim (prim[item], slot[item])
    uint32_t *key;                               // [3][n] per item
    RefitSource *src;                            // per item
    uint32_t *seg, *ident;                       // per item: the lo of its segment at the level at hand; 0 .. n - 1
    uint32_t *ext;                               // [6][n]: min key per axis, max key per axis, indexed by a segment's lo
    uint64_t *sort_in, *sort_out;
    uint32_t *order;                             // per slot position: the item there after the latest sort
    void *temp;
    size_t temp_bytes, bytes;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

uint32_t key_bits(uint32_t n) {
    uint32_t b = 1;
    while (b < 32 && (n >> b)) ++b;
    return b;
}

hipError_t carve(void *base, uint32_t n, Workspace &w) {
    size_t t32 = 0, t64 = 0, t64b = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, t32, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 32u);
    if (e != hipSuccess) return e;
    // (the two bit ranges launch_ray_resplit sorts over: the requirement may depend on the number of passes)
    e = rocprim::radix_sort_pairs(nullptr, t64, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0u, 32u + key_bits(n));
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, t64b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 32u, 32u + key_bits(n));
    if (e != hipSuccess) return e;
    w.temp_bytes = std::max<size_t>(std::max(t32, std::max(t64, t64b)), 256);
    size_t at = 0;
    char *b = static_cast<char *>(base);
    const auto take = [&](size_t bytes) { char *p = b + at; at += align256(std::max<size_t>(bytes, 16)); return p; };
    const size_t m = n;
    w.prim_in = (uint32_t *)take(4 * m); w.prim = (uint32_t *)take(4 * m); w.slot_in = (uint32_t *)take(4 * m); w.slot = (uint32_t *)take(4 * m);
    w.key = (uint32_t *)take(12 * m);
    w.src = (RefitSource *)take(sizeof(RefitSource) * m);
    w.seg = (uint32_t *)take(4 * m); w.ident = (uint32_t *)take(4 * m);
    w.ext = (uint32_t *)take(24 * m);
    w.sort_in = (uint64_t *)take(8 * m); w.sort_out = (uint64_t *)take(8 * m);
    w.order = (uint32_t *)take(4 * m);
    w.temp = take(w.temp_bytes);
    w.bytes = at;
    return hipSuccess;
}

__global__ __launch_bounds__(RESPLIT_BLOCK) void k_resplit_prims(const RayTri *__restrict__ tris, uint32_t n, uint32_t *__restrict__ prim_in, uint32_t *__restrict__ slot_in) {
    const uint32_t p = blockIdx.x * RESPLIT_BLOCK + threadIdx.x;
    if (p >= n) return;
    prim_in[p] = tris[p].prim;
    slot_in[p] = p;
}

__global__ __launch_bounds__(RESPLIT_BLOCK) void k_resplit_centroids(uint32_t n, const uint32_t *__restrict__ slot, const RefitSource *__restrict__ slot_src,
                                                                     const RefitObject *__restrict__ objs, uint32_t n_objs, uint32_t *__restrict__ key,
                                                                     RefitSource *__restrict__ src, uint32_t *__restrict__ ident) {
    const uint32_t i = blockIdx.x * RESPLIT_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t from = slot[i];
    if (from >= n) from = i;                     // (a permutation of 0 .. n - 1 by construction)
    const RefitSource s = slot_src[from];
    uint32_t k[3] = {RQ_KEY_DEAD, RQ_KEY_DEAD, RQ_KEY_DEAD};
    if (s.object < n_objs) {
        const RefitObject &o = objs[s.object];
        if (s.i0 < o.n_vertices && s.i1 < o.n_vertices && s.i2 < o.n_vertices) {   // (k_ray_refit_leaves' rule: such a slot is left alone there)
            float p[9];
            const GlobalFloats v = (GlobalFloats)o.vertices;
            const float v0[3] = {v[(size_t)s.i0 * 14], v[(size_t)s.i0 * 14 + 1], v[(size_t)s.i0 * 14 + 2]};
            const float v1[3] = {v[(size_t)s.i1 * 14], v[(size_t)s.i1 * 14 + 1], v[(size_t)s.i1 * 14 + 2]};
            const float v2[3] = {v[(size_t)s.i2 * 14], v[(size_t)s.i2 * 14 + 1], v[(size_t)s.i2 * 14 + 2]};
            rq_world_vertex(o.m, 3, v0, p);
            rq_world_vertex(o.m, 3, v1, p + 3);
            rq_world_vertex(o.m, 3, v2, p + 6);
            if (rq_finite9(p)) {
                float c[3];
                rq_centroid(p, c);
                k[0] = rq_float_key(c[0]); k[1] = rq_float_key(c[1]); k[2] = rq_float_key(c[2]);
            }
        }
    }
    key[i] = k[0]; key[(size_t)n + i] = k[1]; key[2 * (size_t)n + i] = k[2];
    src[i] = s;
    ident[i] = i;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t x) { for (int d = 32; d > 0; d >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, d)); return x; }
__device__ __forceinline__ uint32_t wave_max(uint32_t x) { for (int d = 32; d > 0; d >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, d)); return x; }

// order: the item at every slot position (the latest sort's values; level 0: ident).  ext has been filled with {0xFFFFFFFF x 3n, 0 x 3n}
__global__ __launch_bounds__(RESPLIT_BLOCK) void k_resplit_assign(uint32_t n, uint32_t level, const uint32_t *__restrict__ order, const uint32_t *__restrict__ key,
                                                                  uint32_t *__restrict__ seg, uint32_t *ext, int with_extents) {
    const uint32_t p = blockIdx.x * RESPLIT_BLOCK + threadIdx.x;
    const bool in_range = p < n;
    uint32_t lo = 0, hi = 0, item = 0;
    if (in_range) {
        rq_segment(n, level, p, lo, hi);
        item = order[p];
        if (item >= n) item = p;
        seg[item] = lo;
    }
    if (!with_extents) return;
    uint32_t k[3] = {RQ_KEY_DEAD, RQ_KEY_DEAD, RQ_KEY_DEAD};
    const bool open = in_range && hi - lo > RAY_LEAF_MAX;
    if (open) { k[0] = key[item]; k[1] = key[(size_t)n + item]; k[2] = key[2 * (size_t)n + item]; }
    const bool live = open && k[0] != RQ_KEY_DEAD;
    // a wave inside one segment (every wave of the upper levels): one atomic per bound instead of 64
    const uint32_t lo0 = (uint32_t)__shfl((int)lo, 0);
    const bool lane0_in = __shfl((int)in_range, 0) != 0;
    if (lane0_in && __all(!in_range || lo == lo0)) {
        uint32_t mn[3], mx[3];
        for (int a = 0; a < 3; ++a) { mn[a] = wave_min(live ? k[a] : 0xFFFFFFFFu); mx[a] = wave_max(live ? k[a] : 0u); }
        if ((threadIdx.x & 63u) == 0 && mn[0] <= mx[0] && lo0 < n)
            for (int a = 0; a < 3; ++a) { atomicMin(ext + (size_t)a * n + lo0, mn[a]); atomicMax(ext + (size_t)(3 + a) * n + lo0, mx[a]); }
    } else if (live) {
        for (int a = 0; a < 3; ++a) { atomicMin(ext + (size_t)a * n + lo, k[a]); atomicMax(ext + (size_t)(3 + a) * n + lo, k[a]); }
    }
}

__global__ __launch_bounds__(RESPLIT_BLOCK) void k_resplit_keys(uint32_t n, uint32_t level, const uint32_t *__restrict__ seg, const uint32_t *__restrict__ key,
                                                                const uint32_t *__restrict__ ext, uint64_t *__restrict__ sort_in) {
    const uint32_t i = blockIdx.x * RESPLIT_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t at = seg[i];
    if (at >= n) at = 0;
    uint32_t lo, hi, k = 0;
    rq_segment(n, level, at, lo, hi);            // (at IS a segment's lo: this finds its hi)
    if (hi - lo > RAY_LEAF_MAX) {
        int axis = 0;
        const uint32_t mn[3] = {ext[lo], ext[(size_t)n + lo], ext[2 * (size_t)n + lo]};
        const uint32_t mx[3] = {ext[3 * (size_t)n + lo], ext[4 * (size_t)n + lo], ext[5 * (size_t)n + lo]};
        if (mn[0] <= mx[0]) {                    // (a segment with no live member: axis 0)
            const float cmin[3] = {rq_key_float(mn[0]), rq_key_float(mn[1]), rq_key_float(mn[2])};
            const float cmax[3] = {rq_key_float(mx[0]), rq_key_float(mx[1]), rq_key_float(mx[2])};
            axis = rq_split_axis(cmin, cmax);
        }
        k = key[(size_t)axis * n + i];
    }
    sort_in[i] = (uint64_t)lo << 32 | k;
}

__global__ __launch_bounds__(RESPLIT_BLOCK) void k_resplit_apply(uint32_t n, const uint32_t *__restrict__ order, const RefitSource *__restrict__ src, const uint32_t *__restrict__ prim,
                                                                 RefitSource *__restrict__ slot_src, RayTri *tris) {
    const uint32_t p = blockIdx.x * RESPLIT_BLOCK + threadIdx.x;
    if (p >= n) return;
    uint32_t item = order[p];
    if (item >= n) item = p;
    slot_src[p] = src[item];
    tris[p].prim = prim[item];                   // the one place a slot's prim is rewritten; the refit behind this writes the rest of the slot
}

}  // namespace

hipError_t ray_resplit_workspace(uint32_t n_slots, size_t *bytes) {
    Workspace w;
    const hipError_t e = carve(nullptr, n_slots, w);
    *bytes = e == hipSuccess ? w.bytes : 0;
    return e;
}

hipError_t launch_ray_resplit(void *ws, size_t ws_bytes, void *tris_, uint32_t n, RefitSource *slot_src, const RefitObject *objs, uint32_t n_objs, hipStream_t s,
                              uint32_t *launches) {
    *launches = 0;
    if (n == 0) return hipSuccess;
    Workspace w;
    hipError_t e = carve(ws, n, w);
    if (e != hipSuccess) return e;
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws & 255u)) return hipErrorInvalidValue;
    RayTri *tris = static_cast<RayTri *>(tris_);
    const uint32_t grid = (n + RESPLIT_BLOCK - 1) / RESPLIT_BLOCK;
    const uint32_t levels = std::min(rq_split_levels(n), RESPLIT_LEVELS_MAX), seg_bits = key_bits(n);
#define RESPLIT_STEP(call) do { call; e = hipGetLastError(); if (e != hipSuccess) return e; ++*launches; } while (0)
#define RESPLIT_CALL(call) do { e = (call); if (e != hipSuccess) return e; ++*launches; } while (0)
    RESPLIT_STEP((k_resplit_prims<<<grid, RESPLIT_BLOCK, 0, s>>>(tris, n, w.prim_in, w.slot_in)));
    size_t temp = w.temp_bytes;
    RESPLIT_CALL(rocprim::radix_sort_pairs(w.temp, temp, (const uint32_t *)w.prim_in, w.prim, (const uint32_t *)w.slot_in, w.slot, (size_t)n, 0u, 32u, s));
    RESPLIT_STEP((k_resplit_centroids<<<grid, RESPLIT_BLOCK, 0, s>>>(n, w.slot, slot_src, objs, n_objs, w.key, w.src, w.ident)));
    for (uint32_t level = 0; level <= levels; ++level) {
        const bool splits = level < levels;      // the pass behind the last split only orders the leaves by prim
        if (splits) {
            RESPLIT_CALL(hipMemsetAsync(w.ext, 0xFF, 12 * (size_t)n, s));
            RESPLIT_CALL(hipMemsetAsync(w.ext + 3 * (size_t)n, 0, 12 * (size_t)n, s));
        }
        RESPLIT_STEP((k_resplit_assign<<<grid, RESPLIT_BLOCK, 0, s>>>(n, level, level == 0 ? w.ident : w.order, w.key, w.seg, w.ext, splits ? 1 : 0)));
        RESPLIT_STEP((k_resplit_keys<<<grid, RESPLIT_BLOCK, 0, s>>>(n, level, w.seg, w.key, w.ext, w.sort_in)));
        temp = w.temp_bytes;
        RESPLIT_CALL(rocprim::radix_sort_pairs(w.temp, temp, (const uint64_t *)w.sort_in, w.sort_out, (const uint32_t *)w.ident, w.order, (size_t)n,
                                               splits ? 0u : 32u, 32u + seg_bits, s));
    }
    RESPLIT_STEP((k_resplit_apply<<<grid, RESPLIT_BLOCK, 0, s>>>(n, w.order, w.src, w.prim, slot_src, tris)));
#undef RESPLIT_STEP
#undef RESPLIT_CALL
    return hipSuccess;
}

}  // namespace arctic
