// morph.hip -- morph targets (blend shapes) of a mesh's vertex buffer (arctic_set_mesh_morph_weights; the arithmetic is written once, in
// include/arctic_hip.h next to the call, and restated on the host by arctic_morph_vertices in host_math.cpp):
//   k_morph   the mesh's own vertices + the delta arrays of the ACTIVE targets (weight != 0) -> a second vertex buffer of the same layout, which
//             ObjectRec::vertices points at (or k_skin reads) while any weight is non-zero.  Nothing downstream knows.
// One launch per morphed mesh per weights change.  Compiled with contraction off: the product rounds, then the sum rounds, target after target in
// ascending index, so numpy in float32 reproduces the buffer bit for bit (tests/morph_reference.py).
//
// Access pattern.  The blend is element-wise and a delta record is 12 floats = three float4: a 16-byte piece of a target's array never straddles
// two vertices.  Thread g of the launch owns piece g of every array: vertex g / 3, third g % 3 (position+normal.x | normal.yz+tangent.xy |
// tangent.z+bitangent).  Its delta loads are lane-contiguous 16-byte loads in every target -- 1 KiB per wave instruction, no LDS, no barrier.
// Its four base elements are at byte 56 v + 16 j, which is only 8-byte aligned: two 8-byte loads, and two 8-byte stores on the way out; three
// consecutive lanes cover 48 contiguous bytes of the vertex's 56 and the third lane carries the texture coordinates (8 bytes) across, so a wave's
// base traffic is contiguous too.  A workgroup of 256 threads owns 85 1/3 vertices: the pieces, not the vertices, are what is divided.
// The active list {target, weight} is the same for every lane: it is indexed uniformly and read through scalar loads; a target at rest is never
// addressed.  The loop is unrolled by MORPH_UNROLL: that many independent 16-byte loads are in flight before the first sum, the sums keep the
// defined order.
#include "common.h"

namespace arctic {

namespace {

constexpr uint32_t MORPH_THREADS = 256;
constexpr int MORPH_UNROLL = 4;

__global__ __launch_bounds__(MORPH_THREADS) void k_morph(const float *__restrict__ in, const float *__restrict__ deltas, const MorphActive *__restrict__ active,
                                                         uint32_t n_active, uint32_t n_vertices, float *__restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * MORPH_THREADS + threadIdx.x;   // piece index: 3 per vertex
    const uint64_t pieces = (uint64_t)n_vertices * 3;
    if (g >= pieces) return;
    const uint64_t v = g / 3;
    const uint32_t j = (uint32_t)(g - v * 3);
    const float *src = in + v * 14 + j * 4;
    const float2 a = *reinterpret_cast<const float2 *>(src), b = *reinterpret_cast<const float2 *>(src + 2);
    float2 uv = make_float2(0.0f, 0.0f);
    if (j == 2) uv = *reinterpret_cast<const float2 *>(src + 4);
    float m0 = a.x, m1 = a.y, m2 = b.x, m3 = b.y;
    const uint64_t target_floats = pieces * 4;                              // floats of one target's array (64-bit: n_targets * this passes 2^32)
    const float *mine = deltas + g * 4;
    uint32_t k = 0;
    for (; k + MORPH_UNROLL <= n_active; k += MORPH_UNROLL) {
        float4 d[MORPH_UNROLL];
        float w[MORPH_UNROLL];
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; ++u) {
            const MorphActive t = active[k + u];
            w[u] = t.weight;
            d[u] = *reinterpret_cast<const float4 *>(mine + (uint64_t)t.target * target_floats);
        }
#pragma unroll
        for (int u = 0; u < MORPH_UNROLL; ++u) {
            m0 = m0 + w[u] * d[u].x; m1 = m1 + w[u] * d[u].y; m2 = m2 + w[u] * d[u].z; m3 = m3 + w[u] * d[u].w;
        }
    }
    for (; k < n_active; ++k) {
        const MorphActive t = active[k];
        const float4 d = *reinterpret_cast<const float4 *>(mine + (uint64_t)t.target * target_floats);
        m0 = m0 + t.weight * d.x; m1 = m1 + t.weight * d.y; m2 = m2 + t.weight * d.z; m3 = m3 + t.weight * d.w;
    }
    float *dst = out + v * 14 + j * 4;
    *reinterpret_cast<float2 *>(dst) = make_float2(m0, m1);
    *reinterpret_cast<float2 *>(dst + 2) = make_float2(m2, m3);
    if (j == 2) *reinterpret_cast<float2 *>(dst + 4) = uv;
}

}  // namespace

hipError_t launch_morph(const float *vertices, const float *deltas, const MorphActive *active, uint32_t n_active, uint32_t n_vertices, float *out,
                        hipStream_t s) {
    if (n_vertices == 0) return hipSuccess;
    const uint64_t pieces = (uint64_t)n_vertices * 3;
    const uint32_t grid = (uint32_t)((pieces + MORPH_THREADS - 1) / MORPH_THREADS);   // (< 2^26 for any uint32 vertex count)
    k_morph<<<grid, MORPH_THREADS, 0, s>>>(vertices, deltas, active, n_active, n_vertices, out);
    return hipGetLastError();
}

}  // namespace arctic
