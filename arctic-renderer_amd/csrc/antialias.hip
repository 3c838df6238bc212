// antialias.hip -- the edge anti-aliasing pass on the finished RGBA8 image (include/arctic_hip.h: ARCTIC_OPT_ANTIALIAS, arctic_antialias*).
// All integers: the header's text is the definition, tests/antialias_reference.py restates it in numpy, and the kernel is held to it bit for bit.
//
// One launch.  A 256-thread workgroup owns a tile of 64 x 16 pixels, a lane four horizontally adjacent ones (16-byte loads and stores
// where the rows allow it).
//   1. the tile's luma plus a one-pixel halo goes to LDS as 16-bit values (a position outside the image holds the clamped pixel's luma:
//      the definition's addressing), the lane's four pixels stay in registers;
//   2. every pixel takes the early-exit test from its five lumas; the pixels past it -- a few per cent of a rendered frame -- are
//      compacted into an LDS list (ballot + prefix), so that
//   3. the list is processed densely, one lane per edge pixel: orientation, side, the two searches of up to 12 steps, both offsets and
//      the blend.  A search reads its lumas from the LDS tile where the step is still inside it and from the image (L1 / L2) beyond;
//   4. each lane stores its four pixels once: the register copy, with the blended pixels swapped in from LDS.
// Every output byte is written exactly once, and nothing of the input is written: the two images must not overlap.
#include "common.h"

namespace arctic {

namespace {

constexpr int AA_TW = 64, AA_TH = 16;                 // the tile (ANTIALIAS_TILE_W / _H of common.h)
constexpr int AA_LW = AA_TW + 2, AA_LH = AA_TH + 2;   // ... with its halo
constexpr int AA_LS = 68;                             // row pitch of the luma tile in LDS (16-bit entries)
constexpr int AA_K = 12;
constexpr uint32_t AA_T_MIN = 4096;
static_assert(AA_TW == (int)ANTIALIAS_TILE_W && AA_TH == (int)ANTIALIAS_TILE_H, "the tile the host sizes the grid by");
static_assert(AA_TW * AA_TH == 4 * 256 && 2 * AA_LW + 2 * AA_TH <= 256, "four pixels per lane; one halo pixel per lane");

__device__ __forceinline__ uint32_t aa_luma(uint32_t c) { return 77u * (c & 255u) + 150u * ((c >> 8) & 255u) + 29u * ((c >> 16) & 255u); }
__device__ __forceinline__ int aa_clamp(int v, int hi) { return min(max(v, 0), hi); }

struct AaTile {
    const uint16_t *y;      // the luma tile in LDS
    const uint32_t *in;
    int x0, y0, w, h;       // the tile's origin, the image's size
    // luma at image coordinates that are already clamped
    __device__ __forceinline__ int luma_at(int cx, int cy) const {
        const int lx = cx - x0 + 1, ly = cy - y0 + 1;
        if ((unsigned)lx < (unsigned)AA_LW && (unsigned)ly < (unsigned)AA_LH) return y[ly * AA_LS + lx];
        return (int)aa_luma(in[(size_t)cy * (size_t)w + (size_t)cx]);
    }
};

// steps 2..7 of the definition for the pixel at (ex, ey) of the tile, which has passed the early exit
__device__ uint32_t aa_edge_pixel(const AaTile &t, int ex, int ey) {
    const uint16_t *c = t.y + (ey + 1) * AA_LS + ex + 1;
    const int M = c[0], N = c[-AA_LS], S = c[AA_LS], Wl = c[-1], E = c[1];
    const int NW = c[-AA_LS - 1], NE = c[-AA_LS + 1], SW = c[AA_LS - 1], SE = c[AA_LS + 1];
    const int rng = max(max(max(M, N), max(S, Wl)), E) - min(min(min(M, N), min(S, Wl)), E);
    // 2. orientation
    const int eh = abs(NW + SW - 2 * Wl) + 2 * abs(N + S - 2 * M) + abs(NE + SE - 2 * E);
    const int ev = abs(NW + NE - 2 * N) + 2 * abs(Wl + E - 2 * M) + abs(SW + SE - 2 * S);
    const bool horiz = eh >= ev;
    // 3. side
    const int a = horiz ? N : Wl, b = horiz ? S : E;
    const int ga = abs(a - M), gb = abs(b - M), g = max(ga, gb);
    const bool side_a = ga >= gb;
    const int step = side_a ? -1 : 1;
    const int nx = horiz ? 0 : step, ny = horiz ? step : 0, tx = horiz ? 1 : 0, ty = horiz ? 0 : 1;
    const int Ls = side_a ? a : b, avg2 = M + Ls;
    const int px = t.x0 + ex, py = t.y0 + ey, xmax = t.w - 1, ymax = t.h - 1;
    // 4. search
    int d[2], e_end[2];
    for (int k = 0; k < 2; ++k) {
        const int s = k ? 1 : -1;
        int ds = AA_K, e = 0;
        for (int i = 1; i <= AA_K; ++i) {
            const int qx = aa_clamp(px + s * i * tx, xmax), qy = aa_clamp(py + s * i * ty, ymax);
            e = t.luma_at(qx, qy) + t.luma_at(aa_clamp(qx + nx, xmax), aa_clamp(qy + ny, ymax)) - avg2;
            if (2 * abs(e) >= g) { ds = i; break; }
        }
        d[k] = ds; e_end[k] = e;
    }
    // 5. edge offset
    const int span = d[0] + d[1], dmin = min(d[0], d[1]);
    const int ee = d[0] < d[1] ? e_end[0] : e_end[1];
    const bool good = (ee < 0) != (M < Ls);
    const uint32_t off_e = good ? (uint32_t)(128 * (span - 2 * dmin)) / (uint32_t)span : 0u;
    // 6. sub-pixel offset
    const uint32_t A = (uint32_t)abs(2 * (N + S + E + Wl) + NW + NE + SW + SE - 12 * M);
    const uint32_t s1 = min(256u, (256u * A) / (12u * (uint32_t)rng));
    const uint32_t s2 = (s1 * s1 * (768u - 2u * s1)) >> 16;
    const uint32_t off_s = (s2 * s2 * 3u) >> 10;
    // 7. blend
    const uint32_t off = min(max(off_e, off_s), 192u), keep = 256u - off;
    const uint32_t p = t.in[(size_t)py * (size_t)t.w + (size_t)px];
    const uint32_t q = t.in[(size_t)aa_clamp(py + ny, ymax) * (size_t)t.w + (size_t)aa_clamp(px + nx, xmax)];
    uint32_t out = p & 0xFF000000u;
    for (int sh = 0; sh < 24; sh += 8) out |= ((((p >> sh) & 255u) * keep + ((q >> sh) & 255u) * off + 128u) >> 8) << sh;
    return out;
}

__global__ __launch_bounds__(256) void k_antialias(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t width, uint32_t height,
                                                   uint32_t tiles_x, uint32_t vec /* rows are 16-byte units: width % 4 == 0, both images 16-byte aligned */) {
    __shared__ uint16_t s_y[AA_LH * AA_LS];
    __shared__ uint32_t s_res[AA_TW * AA_TH];
    __shared__ uint16_t s_list[AA_TW * AA_TH];
    __shared__ uint32_t s_count;
    const int tid = (int)threadIdx.x, w = (int)width, h = (int)height;
    const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = (int)tile_x * AA_TW, y0 = (int)tile_y * AA_TH;
    const int lx = (tid & 15) * 4, ly = tid >> 4, gx = x0 + lx, gy = y0 + ly;
    if (tid == 0) s_count = 0;

    // 1. the lane's four pixels and their lumas; then one pixel of the halo
    const bool whole = vec && gy < h && gx + 3 < w;
    uint32_t px[4];
    if (whole) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + (size_t)gy * width + (size_t)gx);
        px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
    } else {
        const size_t row = (size_t)min(gy, h - 1) * width;
        for (int j = 0; j < 4; ++j) px[j] = in[row + (size_t)min(gx + j, w - 1)];
    }
    for (int j = 0; j < 4; ++j) s_y[(ly + 1) * AA_LS + lx + 1 + j] = (uint16_t)aa_luma(px[j]);
    if (tid < 2 * AA_LW + 2 * AA_TH) {
        int hx, hy;
        if (tid < AA_LW) { hx = tid; hy = 0; }
        else if (tid < 2 * AA_LW) { hx = tid - AA_LW; hy = AA_LH - 1; }
        else if (tid < 2 * AA_LW + AA_TH) { hx = 0; hy = tid - 2 * AA_LW + 1; }
        else { hx = AA_LW - 1; hy = tid - 2 * AA_LW - AA_TH + 1; }
        const int sx = aa_clamp(x0 + hx - 1, w - 1), sy = aa_clamp(y0 + hy - 1, h - 1);
        s_y[hy * AA_LS + hx] = (uint16_t)aa_luma(in[(size_t)sy * width + (size_t)sx]);
    }
    __syncthreads();

    // 2. early exit; the others into the list
    uint32_t edge_bits = 0;
    for (int j = 0; j < 4; ++j) {
        const uint16_t *c = s_y + (ly + 1) * AA_LS + lx + 1 + j;
        const uint32_t M = c[0], N = c[-AA_LS], S = c[AA_LS], Wl = c[-1], E = c[1];
        const uint32_t hi = max(max(max(M, N), max(S, Wl)), E), lo = min(min(min(M, N), min(S, Wl)), E);
        const bool is_edge = gx + j < w && gy < h && hi - lo >= max(AA_T_MIN, hi >> 3);
        const unsigned long long m = __ballot(is_edge);
        if (m) {   // (wave-uniform)
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            uint32_t base = 0;
            if (is_edge && rank == 0) base = atomicAdd(&s_count, (uint32_t)__popcll(m));
            base = __shfl(base, __ffsll((long long)m) - 1);
            if (is_edge) { s_list[base + rank] = (uint16_t)(ly * AA_TW + lx + j); edge_bits |= 1u << j; }
        }
    }
    __syncthreads();

    // 3. the edge pixels, densely
    const uint32_t count = s_count;
    if (count) {   // (the same in every lane of the workgroup)
        const AaTile t = {s_y, in, x0, y0, w, h};
        for (uint32_t k = (uint32_t)tid; k < count; k += 256) {
            const uint32_t idx = s_list[k];
            s_res[idx] = aa_edge_pixel(t, (int)(idx & (AA_TW - 1)), (int)(idx / AA_TW));
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) if (edge_bits >> j & 1u) px[j] = s_res[ly * AA_TW + lx + j];
    }

    // 4. one store per pixel
    if (whole) *reinterpret_cast<uint4 *>(out + (size_t)gy * width + (size_t)gx) = make_uint4(px[0], px[1], px[2], px[3]);
    else if (gy < h)
        for (int j = 0; j < 4; ++j) if (gx + j < w) out[(size_t)gy * width + (size_t)(gx + j)] = px[j];
}

}  // namespace

hipError_t launch_antialias(const void *in, void *out, uint32_t width, uint32_t height, hipStream_t s) {
    if (width == 0 || height == 0) return hipSuccess;
    const uint64_t tiles_x = (width + ANTIALIAS_TILE_W - 1) / ANTIALIAS_TILE_W, tiles_y = (height + ANTIALIAS_TILE_H - 1) / ANTIALIAS_TILE_H;
    if (tiles_x * tiles_y > 0x7FFFFFFFull || width > 0x40000000u || height > 0x40000000u) return hipErrorInvalidValue;   // (one grid; coordinates are ints)
    const uint32_t vec = (width % 4 == 0 && ((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & 15) == 0) ? 1u : 0u;
    k_antialias<<<(uint32_t)(tiles_x * tiles_y), 256, 0, s>>>(static_cast<const uint32_t *>(in), static_cast<uint32_t *>(out), width, height, (uint32_t)tiles_x, vec);
    return hipGetLastError();
}

}  // namespace arctic
