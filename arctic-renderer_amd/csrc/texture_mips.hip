// texture_mips.hip -- the mip chain of a packed material (ARCTIC_OPT_TEXTURE_MIPS; the semantics are written once, in
// include/arctic_hip.h next to the option), built on the device when the material is created:
//   k_mip_reduce   level k + 1 from level k.  Both are packed images of 8-byte texels {d.r, d.g, d.b, n.r, n.g, n.b, mr.g, mr.b} with a
//                  one-texel WRAP border (common.h TexDesc); the source in whatever layout it has (row-major or 4 x 4-texel tiles: level 0
//                  is the image arctic_create_material uploaded, untouched), the destination row-major WITH its own border, so that the
//                  footprint code of shade.hip works on every level.  One thread per texel of the bordered destination.
//   k_plane_tile   the level-of-detail plane between the handle's rows and the tile-major layout (arctic_read_lod / arctic_write_lod)
// None of this runs per frame.  The reduction is exact by definition: the five UNORM8 channels are integer means, the three sRGB8
// channels go through the kernels' own 256-entry table in binary64 (the sum of four fp32 table values is exact there) and back to the
// code whose table value is nearest, the lower code on a tie -- no pow on either side, so a numpy reference reproduces it bit for bit
// (tests/mip_reference.py).
#include "common.h"

namespace arctic {

namespace {

// byte offset of padded texel (X, Y) of a packed image (common.h TexDesc: pitch, tile_row_bytes)
__device__ __forceinline__ size_t packed_texel_offset(uint32_t X, uint32_t Y, uint32_t pitch, uint32_t tile_row_bytes) {
    if (tile_row_bytes) return (size_t)(Y >> 2) * tile_row_bytes + (size_t)(X >> 2) * 128u + ((Y & 3u) * 4u + (X & 3u)) * 8u;
    return ((size_t)Y * pitch + X) * 8u;
}

// the sRGB8 code whose table value is nearest to s4 / 4, the lower code on a tie: code c is left for c + 1 when s4 / 4 > (t[c] + t[c + 1]) / 2,
// i.e. s4 > 2 (t[c] + t[c + 1]) -- every term exact in binary64.  The table is strictly increasing: a bisection over the 255 midpoints.
__device__ __forceinline__ uint32_t srgb_encode_sum4(double s4, const float *t) {
    uint32_t lo = 0, hi = 255;   // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s4 > 2.0 * ((double)t[mid] + (double)t[mid + 1])) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mip_reduce(const uint8_t *__restrict__ src, uint32_t sw, uint32_t sh, uint32_t spitch, uint32_t stile_row_bytes,
                                                    uint8_t *__restrict__ dst, uint32_t dw, uint32_t dh, uint32_t dpitch, const float *__restrict__ srgb_lut) {
    __shared__ float lut[256];
    lut[threadIdx.x] = srgb_lut[threadIdx.x];
    __syncthreads();
    const uint32_t X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);   // padded destination texel
    if (X >= dw + 2 || Y >= dh + 2) return;
    const uint32_t x = (X + dw - 1) % dw, y = (Y + dh - 1) % dh;                                       // destination texel (WRAP border)
    const uint32_t x0 = min(2 * x, sw - 1), x1 = min(2 * x + 1, sw - 1), y0 = min(2 * y, sh - 1), y1 = min(2 * y + 1, sh - 1);
    const auto texel = [&](uint32_t sx, uint32_t sy) {
        return *reinterpret_cast<const uint2 *>(src + packed_texel_offset(sx + 1, sy + 1, spitch, stile_row_bytes));
    };
    const uint2 t[4] = {texel(x0, y0), texel(x1, y0), texel(x0, y1), texel(x1, y1)};
    const auto byte_of = [&](int i, int k) { return ((k < 4 ? t[i].x : t[i].y) >> (8 * (k & 3))) & 0xFFu; };
    uint32_t out[8];
#pragma unroll
    for (int k = 0; k < 3; ++k)   // diffuse rgb: sRGB8
        out[k] = srgb_encode_sum4(((double)lut[byte_of(0, k)] + (double)lut[byte_of(1, k)]) + ((double)lut[byte_of(2, k)] + (double)lut[byte_of(3, k)]), lut);
#pragma unroll
    for (int k = 3; k < 8; ++k) out[k] = (byte_of(0, k) + byte_of(1, k) + byte_of(2, k) + byte_of(3, k) + 2u) >> 2;
    uint2 r;
    r.x = out[0] | (out[1] << 8) | (out[2] << 16) | (out[3] << 24);
    r.y = out[4] | (out[5] << 8) | (out[6] << 16) | (out[7] << 24);
    *reinterpret_cast<uint2 *>(dst + ((size_t)Y * dpitch + X) * 8u) = r;
}

__global__ __launch_bounds__(256) void k_plane_tile(float *__restrict__ tiled, float *__restrict__ rows, uint32_t width, uint32_t n_rows, uint32_t row0_in_tile,
                                                    uint32_t tiles_x, uint32_t tiles_y, int to_tiled) {
    const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= tiles_x * tiles_y) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t x = (tile % tiles_x) * 8 + (lane & 7);
    const int32_t y = (int32_t)((tile / tiles_x) * 8 + (lane >> 3)) - (int32_t)row0_in_tile;   // row inside the shard
    const size_t idx = (size_t)tile * 64 + lane;
    const bool in = x < width && y >= 0 && y < (int32_t)n_rows;
    if (to_tiled) tiled[idx] = in ? rows[(size_t)y * width + x] : 0.0f;
    else if (in) rows[(size_t)y * width + x] = tiled[idx];
}

}  // namespace

hipError_t launch_mip_reduce(const TexDesc &src, const TexDesc &dst, const float *srgb_lut, hipStream_t s) {
    const uint32_t sw = src.w & ~TEX_INTERLEAVED, dw = dst.w & ~TEX_INTERLEAVED;
    const dim3 grid((dw + 2 + 63) / 64, (dst.h + 2 + 3) / 4);
    k_mip_reduce<<<grid, 256, 0, s>>>(reinterpret_cast<const uint8_t *>(src.texels), sw, src.h, src.pitch, src.tile_row_bytes,
                                      reinterpret_cast<uint8_t *>(const_cast<uint32_t *>(dst.texels)), dw, dst.h, dst.pitch, srgb_lut);
    return hipGetLastError();
}

hipError_t launch_plane_tile(float *tiled, float *rows, uint32_t width, uint32_t n_rows, uint32_t row0_in_tile, uint32_t tiles_x, uint32_t tiles_y, int to_tiled, hipStream_t s) {
    if (tiles_x * tiles_y == 0) return hipSuccess;
    k_plane_tile<<<(tiles_x * tiles_y + 3) / 4, 256, 0, s>>>(tiled, rows, width, n_rows, row0_in_tile, tiles_x, tiles_y, to_tiled);
    return hipGetLastError();
}

}  // namespace arctic
