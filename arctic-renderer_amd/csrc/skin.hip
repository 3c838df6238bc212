// skin.hip -- skeletal skinning of a mesh's vertex buffer (arctic_set_mesh_pose; the arithmetic is written once, in include/arctic_hip.h
// next to the call, and restated on the host by arctic_skin_vertices in host_math.cpp):
//   k_skin   bind-pose vertices + per-vertex joints / weights + the pose's joint matrices -> a second vertex buffer of the same layout,
//            which ObjectRec::vertices points at while the pose is set.  Nothing downstream knows: k_vertex reads 14 floats per vertex.
// One launch per posed mesh per pose change, never per frame of an unchanged pose.  Compiled with contraction off: every fp32 operation rounds
// once, in the written order, so numpy in float32 reproduces the buffer bit for bit (tests/skin_reference.py).
//
// Access pattern.  A vertex is 56 bytes and its skin record 24: neither is a lane-contiguous access, and 14 (or 6) loads per lane 56 (24) bytes
// apart would each touch 64 cache lines for 256 bytes of use.  A workgroup of 256 lanes owns 256 consecutive vertices instead -- 14336 + 6144
// contiguous bytes -- moves them as whole wave-contiguous 16-byte loads into LDS, and each lane then reads ITS vertex back as seven ds_read_b64
// (8-byte reads 56 bytes apart: 14 l mod 64 is distinct for the 32 lanes of a half, no bank conflict) and its skin record as three.  The posed
// vertex goes back into the lane's own LDS slot and leaves as wave-contiguous 16-byte stores.
// The joint table is wave-shared, randomly indexed data: up to SKIN_LDS_JOINTS joints it is staged in LDS too -- the 12 floats of rows 0..2 a
// joint contributes, 48 bytes each, read as three ds_read_b128 --, beyond that the lanes gather the matrices' columns from global memory (16-byte
// loads; a few hundred joints stay in L2 / the vector cache).  Two instantiations, chosen by the joint count on the host.
#include "common.h"

namespace arctic {

namespace {

constexpr uint32_t SKIN_THREADS = 256;
constexpr uint32_t VERT_DWORDS = 14, SKINREC_DWORDS = 6;

// `count` dwords from src (16-byte aligned) to LDS: whole float4 where four are left, single dwords at the end of the buffer
__device__ __forceinline__ void stage_in(float *lds, const float *__restrict__ src, uint32_t count) {
    for (uint32_t q = threadIdx.x; q * 4 < count; q += SKIN_THREADS) {
        const uint32_t d = q * 4;
        if (d + 4 <= count) *reinterpret_cast<float4 *>(lds + d) = *reinterpret_cast<const float4 *>(src + d);
        else for (uint32_t k = d; k < count; ++k) lds[k] = src[k];
    }
}

__device__ __forceinline__ void stage_out(float *__restrict__ dst, const float *lds, uint32_t count) {
    for (uint32_t q = threadIdx.x; q * 4 < count; q += SKIN_THREADS) {
        const uint32_t d = q * 4;
        if (d + 4 <= count) *reinterpret_cast<float4 *>(dst + d) = *reinterpret_cast<const float4 *>(lds + d);
        else for (uint32_t k = d; k < count; ++k) dst[k] = lds[k];
    }
}

// S = ((w0 J0 + w1 J1) + w2 J2) + w3 J3, one element
__device__ __forceinline__ float blend(float w0, float a, float w1, float b, float w2, float c, float w3, float d) {
    return ((w0 * a + w1 * b) + w2 * c) + w3 * d;
}

template <bool TABLE_IN_LDS>
__global__ __launch_bounds__(SKIN_THREADS) void k_skin(const float *__restrict__ in, const float *__restrict__ skin, const float *__restrict__ joints,
                                                       uint32_t n_vertices, uint32_t n_joints, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_vert[SKIN_THREADS * VERT_DWORDS];
    __shared__ __attribute__((aligned(16))) float s_skin[SKIN_THREADS * SKINREC_DWORDS];
    __shared__ __attribute__((aligned(16))) float s_joint[TABLE_IN_LDS ? SKIN_LDS_JOINTS * 12 : 4];
    const uint32_t first = blockIdx.x * SKIN_THREADS;                 // (n_vertices < 2^31: no overflow)
    const uint32_t here = min(SKIN_THREADS, n_vertices - first);      // vertices of this workgroup (>= 1 by the grid's size)
    stage_in(s_vert, in + (size_t)first * VERT_DWORDS, here * VERT_DWORDS);
    stage_in(s_skin, skin + (size_t)first * SKINREC_DWORDS, here * SKINREC_DWORDS);
    if (TABLE_IN_LDS)   // rows 0..2 of the four columns of every joint: element 4 c + i of the matrix goes to 3 c + i of the joint's 12 floats
        for (uint32_t k = threadIdx.x; k < n_joints * 12; k += SKIN_THREADS) {
            const uint32_t j = k / 12, e = k % 12;                     // e = 3 * column + row
            s_joint[k] = joints[(size_t)j * 16 + (e / 3) * 4 + e % 3];
        }
    __syncthreads();
    if (threadIdx.x < here) {
        float *v = s_vert + threadIdx.x * VERT_DWORDS;
        const float *sk = s_skin + threadIdx.x * SKINREC_DWORDS;
        float x[VERT_DWORDS];
#pragma unroll
        for (int k = 0; k < 7; ++k) { const float2 t = *reinterpret_cast<const float2 *>(v + 2 * k); x[2 * k] = t.x; x[2 * k + 1] = t.y; }
        const uint2 jj = *reinterpret_cast<const uint2 *>(sk);        // four uint16 joint indices
        const float2 wa = *reinterpret_cast<const float2 *>(sk + 2), wb = *reinterpret_cast<const float2 *>(sk + 4);
        const uint32_t j0 = jj.x & 0xFFFFu, j1 = jj.x >> 16, j2 = jj.y & 0xFFFFu, j3 = jj.y >> 16;
        float S[12];   // S[3 c + i] = row i of column c of the blended matrix
        if (TABLE_IN_LDS) {
            const float4 *a = reinterpret_cast<const float4 *>(s_joint + j0 * 12), *b = reinterpret_cast<const float4 *>(s_joint + j1 * 12);
            const float4 *c = reinterpret_cast<const float4 *>(s_joint + j2 * 12), *d = reinterpret_cast<const float4 *>(s_joint + j3 * 12);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 A = a[q], B = b[q], Cc = c[q], D = d[q];
                S[4 * q + 0] = blend(wa.x, A.x, wa.y, B.x, wb.x, Cc.x, wb.y, D.x);
                S[4 * q + 1] = blend(wa.x, A.y, wa.y, B.y, wb.x, Cc.y, wb.y, D.y);
                S[4 * q + 2] = blend(wa.x, A.z, wa.y, B.z, wb.x, Cc.z, wb.y, D.z);
                S[4 * q + 3] = blend(wa.x, A.w, wa.y, B.w, wb.x, Cc.w, wb.y, D.w);
            }
        } else {
            const float4 *a = reinterpret_cast<const float4 *>(joints + (size_t)j0 * 16), *b = reinterpret_cast<const float4 *>(joints + (size_t)j1 * 16);
            const float4 *c = reinterpret_cast<const float4 *>(joints + (size_t)j2 * 16), *d = reinterpret_cast<const float4 *>(joints + (size_t)j3 * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) {   // column q
                const float4 A = a[q], B = b[q], Cc = c[q], D = d[q];
                S[3 * q + 0] = blend(wa.x, A.x, wa.y, B.x, wb.x, Cc.x, wb.y, D.x);
                S[3 * q + 1] = blend(wa.x, A.y, wa.y, B.y, wb.x, Cc.y, wb.y, D.y);
                S[3 * q + 2] = blend(wa.x, A.z, wa.y, B.z, wb.x, Cc.z, wb.y, D.z);
            }
        }
        float y[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            y[i] = ((S[i] * x[0] + S[3 + i] * x[1]) + S[6 + i] * x[2]) + S[9 + i] * 1.0f;      // position: geometry.hip's mat_vec order
            y[3 + i] = (S[i] * x[3] + S[3 + i] * x[4]) + S[6 + i] * x[5];                        // normal
            y[6 + i] = (S[i] * x[6] + S[3 + i] * x[7]) + S[6 + i] * x[8];                        // tangent
            y[9 + i] = (S[i] * x[9] + S[3 + i] * x[10]) + S[6 + i] * x[11];                      // bitangent
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) *reinterpret_cast<float2 *>(v + 2 * k) = make_float2(y[2 * k], y[2 * k + 1]);   // (the texture coordinates stay in place)
    }
    __syncthreads();
    stage_out(out + (size_t)first * VERT_DWORDS, s_vert, here * VERT_DWORDS);
}

}  // namespace

hipError_t launch_skin(const float *vertices, const void *skin, const float *joints, uint32_t n_vertices, uint32_t n_joints, float *out, hipStream_t s) {
    if (n_vertices == 0) return hipSuccess;
    const uint32_t grid = (n_vertices + SKIN_THREADS - 1) / SKIN_THREADS;
    if (n_joints <= SKIN_LDS_JOINTS) k_skin<true><<<grid, SKIN_THREADS, 0, s>>>(vertices, static_cast<const float *>(skin), joints, n_vertices, n_joints, out);
    else k_skin<false><<<grid, SKIN_THREADS, 0, s>>>(vertices, static_cast<const float *>(skin), joints, n_vertices, n_joints, out);
    return hipGetLastError();
}

}  // namespace arctic
