// ray_refit.hip -- the ray structure follows a scene that moves (include/arctic_hip.h: "a refitted structure" is the definition; ray_query.h
// carries the arithmetic, bvh.cpp's bvh_refit is the same thing on the host and refit_schedule makes the tables these kernels read):
//   k_ray_refit_leaves   stage 0: one wave per TREELET -- a maximal subtree of at most 64 leaves --, a lane per leaf.  The lane gathers the source
//                        vertices of its leaf's <= 4 slots (12 of each vertex's 56 bytes), transforms them with the object's trs, writes the 48-byte
//                        records (16-byte stores), forms the leaf's box and writes it; the wave then joins the treelet's <= 63 interior nodes
//   k_ray_refit_upper    stages 1 ...: the same join one level up -- the inputs are the roots an earlier launch wrote, read from memory
// Why stages and not one launch that walks up the tree on arrival counters: the per-XCD L2s are not coherent, so a child's box written by one
// workgroup reaches its parent's workgroup only behind a device-scope fence -- microseconds each, once per level per thread.  A kernel boundary on
// one stream gives the same visibility for nothing; 65,536 leaves are 1,024 + 16 + 1 waves in three launches.
// INSIDE a launch no workgroup talks to another: a workgroup is one wave, a task is one wave, and its interior boxes travel through 3 KiB of LDS
// in rounds by height (a node of height h reads children of lower height, written in an earlier round; __syncthreads() of a one-wave workgroup
// orders the LDS traffic and costs no wait for anyone else).  Each box goes to memory once.  No atomics, no spinning, every loop bound a host-made
// count clamped to its structural limit, vector stores only, no scratch.  The topology words of a node (skip, leaf) are never written here: a box is
// two 12-byte stores.  Every index read from a table is compared with its count before use (the host has checked the tables already:
// refit_schedule_validate, bvh_validate, ray_triangle_sources): a stale table can cost a wrong box, never an access out of bounds.
// Compiled with contraction off: a world vertex rounds exactly as in ray_world_triangles and k_vertex.
#include "common.h"
#include "ray_query.h"

namespace arctic {

namespace {

constexpr uint32_t REFIT_SLOTS = 2 * REFIT_WAVE - 1;   // inputs + interiors of a task

typedef const float __attribute__((address_space(1))) *GlobalFloats;

struct TaskHead { uint32_t n_in, n_int, heights; };
__device__ __forceinline__ TaskHead task_head(uint32_t word) {
    TaskHead h;
    h.n_in = min(word & 255u, REFIT_WAVE); h.n_int = min(word >> 8 & 255u, REFIT_WAVE - 1); h.heights = min(word >> 16, REFIT_WAVE - 1);
    return h;
}

__device__ __forceinline__ void store_box(RayNode *node, const RayBox &b) {   // (skip and leaf stay as the build wrote them)
    node->bmin[0] = b.lo[0]; node->bmin[1] = b.lo[1]; node->bmin[2] = b.lo[2];
    node->bmax[0] = b.hi[0]; node->bmax[1] = b.hi[1]; node->bmax[2] = b.hi[2];
}

// the task's interior nodes, round by round; `mine` is lane's input box (lane < n_in)
__device__ __forceinline__ void join_task(float (*box)[6], const RayBox &mine, uint32_t lane, const TaskHead &t, const RefitInterior &e, RayNode *nodes, uint32_t n_nodes) {
    if (lane < t.n_in) for (int a = 0; a < 3; ++a) { box[lane][a] = mine.lo[a]; box[lane][3 + a] = mine.hi[a]; }
    __syncthreads();
    const uint32_t c0 = e.link & 255u, c1 = e.link >> 8 & 255u, height = e.link >> 16;
    for (uint32_t h = 1; h <= t.heights; ++h) {
        if (lane < t.n_int && height == h && c0 < REFIT_SLOTS && c1 < REFIT_SLOTS) {
            RayBox x = rq_empty_box(), c;
            for (int a = 0; a < 3; ++a) { c.lo[a] = box[c0][a]; c.hi[a] = box[c0][3 + a]; }
            rq_grow(x, c);
            for (int a = 0; a < 3; ++a) { c.lo[a] = box[c1][a]; c.hi[a] = box[c1][3 + a]; }
            rq_grow(x, c);
            for (int a = 0; a < 3; ++a) { box[t.n_in + lane][a] = x.lo[a]; box[t.n_in + lane][3 + a] = x.hi[a]; }
            if (e.node < n_nodes) store_box(nodes + e.node, x);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(REFIT_WAVE) void k_ray_refit_leaves(const uint32_t *__restrict__ head, const uint32_t *__restrict__ inputs, const RefitInterior *__restrict__ interior,
                                                                 uint32_t task0, RayNode *nodes, uint32_t n_nodes, RayTri *tris, uint32_t n_slots,
                                                                 const RefitSource *__restrict__ src, const RefitObject *__restrict__ objs, uint32_t n_objs) {
    __shared__ float box[REFIT_SLOTS][6];
    const uint32_t task = task0 + blockIdx.x, lane = threadIdx.x;
    const TaskHead t = task_head(head[task]);
    const uint32_t node = inputs[(size_t)task * REFIT_WAVE + lane];
    const RefitInterior e = interior[(size_t)task * REFIT_WAVE + lane];
    RayBox mine = rq_empty_box();
    if (lane < t.n_in && node < n_nodes) {
        const uint32_t leaf = nodes[node].leaf, count = min(leaf & 7u, RAY_LEAF_MAX), first = leaf >> 3;
        for (uint32_t k = 0; k < count; ++k) {
            const uint32_t slot = first + k;
            if (slot >= n_slots) continue;
            const RefitSource s = src[slot];
            if (s.object >= n_objs) continue;
            const RefitObject &o = objs[s.object];
            if (!(s.i0 < o.n_vertices && s.i1 < o.n_vertices && s.i2 < o.n_vertices)) continue;
            float p[9];
            const GlobalFloats v = (GlobalFloats)o.vertices;   // (a pointer read from memory: tell the compiler it is device memory, not LDS or scratch)
            const float v0[3] = {v[(size_t)s.i0 * 14], v[(size_t)s.i0 * 14 + 1], v[(size_t)s.i0 * 14 + 2]};
            const float v1[3] = {v[(size_t)s.i1 * 14], v[(size_t)s.i1 * 14 + 1], v[(size_t)s.i1 * 14 + 2]};
            const float v2[3] = {v[(size_t)s.i2 * 14], v[(size_t)s.i2 * 14 + 1], v[(size_t)s.i2 * 14 + 2]};
            rq_world_vertex(o.m, 3, v0, p);
            rq_world_vertex(o.m, 3, v1, p + 3);
            rq_world_vertex(o.m, 3, v2, p + 6);
            const bool live = rq_finite9(p);
            if (live) rq_grow(mine, rq_triangle_box(p));
            else for (int j = 0; j < 9; ++j) p[j] = rq_dead();
            rq_f4 *tp = reinterpret_cast<rq_f4 *>(tris + slot);
            rq_f4 c = tp[2];                                   // {p2.z, prim, -, -}: the prim is kept
            c[0] = p[8];
            tp[0] = rq_f4{p[0], p[1], p[2], p[3]};
            tp[1] = rq_f4{p[4], p[5], p[6], p[7]};
            tp[2] = c;
        }
        store_box(nodes + node, mine);
    }
    join_task(box, mine, lane, t, e, nodes, n_nodes);
}

__global__ __launch_bounds__(REFIT_WAVE) void k_ray_refit_upper(const uint32_t *__restrict__ head, const uint32_t *__restrict__ inputs, const RefitInterior *__restrict__ interior,
                                                                uint32_t task0, RayNode *nodes, uint32_t n_nodes) {
    __shared__ float box[REFIT_SLOTS][6];
    const uint32_t task = task0 + blockIdx.x, lane = threadIdx.x;
    const TaskHead t = task_head(head[task]);
    const uint32_t node = inputs[(size_t)task * REFIT_WAVE + lane];
    const RefitInterior e = interior[(size_t)task * REFIT_WAVE + lane];
    RayBox mine = rq_empty_box();
    if (lane < t.n_in && node < n_nodes) {   // a root an earlier launch wrote
        const rq_f4 *np = reinterpret_cast<const rq_f4 *>(nodes + node);
        const rq_f4 lo = np[0], hi = np[1];
        for (int a = 0; a < 3; ++a) { mine.lo[a] = lo[a]; mine.hi[a] = hi[a]; }
    }
    join_task(box, mine, lane, t, e, nodes, n_nodes);
}

}  // namespace

hipError_t launch_ray_refit(const RefitTablesDev &T, const uint32_t *stage_first, uint32_t n_stages, void *nodes, uint32_t n_nodes, void *tris, uint32_t n_slots,
                            const RefitObject *objs, uint32_t n_objs, hipStream_t s, uint32_t *launches) {
    *launches = 0;
    for (uint32_t st = 0; st < n_stages; ++st) {
        const uint32_t first = stage_first[st], count = stage_first[st + 1] - first;
        if (count == 0) continue;
        if (st == 0) k_ray_refit_leaves<<<count, REFIT_WAVE, 0, s>>>(T.head, T.inputs, T.interior, first, static_cast<RayNode *>(nodes), n_nodes, static_cast<RayTri *>(tris), n_slots, T.src, objs, n_objs);
        else k_ray_refit_upper<<<count, REFIT_WAVE, 0, s>>>(T.head, T.inputs, T.interior, first, static_cast<RayNode *>(nodes), n_nodes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
    }
    return hipSuccess;
}

}  // namespace arctic
