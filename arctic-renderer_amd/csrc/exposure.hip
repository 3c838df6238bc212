// exposure.hip -- auto-exposure, the last stage in front of the tonemapper, behind bloom (arctic_exposure_device; the arithmetic is written once, in
// include/arctic_hip.h in front of the calls, and carried out by exposure.h -- the very functions the host arbiters run):
//   k_exposure_meter    G workgroups of 256 threads (G and the pixels a workgroup takes per trip: exposure_layout) walk the metering window's
//                       pixels in row order, 4 runs of 256 consecutive pixels a workgroup a trip, so that a wave loads contiguous runs of float3
//                       and has four loads in flight per lane.  The
//                       workgroup's 256-bin histogram lives in LDS: zeroed in front of the first __syncthreads(), filled with LDS atomic adds
//                       whose result nobody reads, flushed behind the second to the workgroup's OWN row of the partials table T[G][256] with
//                       plain stores.  The trip count is the workgroup's, not the thread's: a thread with no pixel left skips only its add, and
//                       every thread of every workgroup reaches both barriers.  No global atomic, no clear: a call depends on nothing an earlier
//                       one left in T.
//   k_exposure_resolve  one workgroup.  Thread b sums column b of T over the G rows (H[b], stored), the prefix sums go through an LDS scan, M and S
//                       through an LDS tree, and thread 0 does the binary64 tail and stores the state record.  Every loop is bounded by G or 256.
//   k_exposure_apply    one thread per pixel like k_bloom_composite: E from the state record (a uniform address), out = C * E, then HDR (12 B),
//                       RGBA8 (4 B) and float LDR (12 B) through post_process.h.
// Three launches per call, nothing read back.  Whole frames only.  Vector stores only.  Compiled with contraction off: every operation of the
// definition rounds once.
#include "common.h"
#include "exposure.h"
#include "post_process.h"

// How the meter meets contention (DESIGN.md 6w holds the measurement that chose): 0 = every lane adds to the workgroup's one histogram; 1 = a
// histogram per wave, summed at the flush; 2 = as 0, but a wave whose lanes all hold one bin adds their count once.  tools/exposure_time.py alone
// builds libraries with another value (the Makefile never sets it); all three give the same bytes
#if !defined(ARCTIC_EXPOSURE_METER_VARIANT)
#define ARCTIC_EXPOSURE_METER_VARIANT 0
#endif

namespace arctic {

namespace {

constexpr uint32_t EXPOSURE_BLOCK = 16;   // k_exposure_apply's workgroup is 16 x 16 pixels
constexpr uint32_t EXPOSURE_WAVES = EXPOSURE_THREADS / 64;
constexpr uint32_t EXPOSURE_HISTS = ARCTIC_EXPOSURE_METER_VARIANT == 1 ? EXPOSURE_WAVES : 1;

// row-major float3 colour of a pixel inside the frame
struct ExposurePlaneColor {
    static constexpr bool LINEAR = true;   // pixel o of the plane is at float 3 o: a window of full rows is one run, no division
    const float *color;
    uint32_t width;
    __device__ __forceinline__ void linear(size_t o, float *c) const {
        const f3v h = *reinterpret_cast<const f3v *>(color + o * 3);
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const { linear((size_t)qy * width + qx, c); }
};
// the anti-aliasing's history: tile-major float4 {r, g, b, N}
struct ExposureHistoryColor {
    static constexpr bool LINEAR = false;
    const float4 *t;
    uint32_t tiles_x;
    __device__ __forceinline__ void operator()(uint32_t qx, uint32_t qy, float *c) const {
        const float4 h = t[((size_t)(qy / TILE) * tiles_x + qx / TILE) * TILE_PIXELS + (qy % TILE) * TILE + qx % TILE];
        c[0] = h.x; c[1] = h.y; c[2] = h.z;
    }
};

// Every index is bounded before it is used: a pixel by the window (i < n, and the window lies in the frame: launch_exposure_meter), a bin by
// exposure_bin's integer clamp, a row of T by gridDim.x == p.groups (launch_exposure_meter checks it against the layout)
template <class Color>
__global__ __launch_bounds__(EXPOSURE_THREADS) void k_exposure_meter(const ExposureParams p, const Color color) {
    __shared__ uint32_t hist[EXPOSURE_HISTS][EXPOSURE_BINS];
    for (uint32_t k = 0; k < EXPOSURE_HISTS; ++k) hist[k][threadIdx.x] = 0u;
    __syncthreads();   // (every thread of the workgroup arrives: nothing returns in front of it)
    uint32_t *mine = hist[EXPOSURE_HISTS == 1 ? 0u : threadIdx.x / 64u];
    const uint32_t ww = p.window[2] - p.window[0], n = ww * (p.window[3] - p.window[1]);   // (<= 2^28)
    const uint32_t stride = gridDim.x * EXPOSURE_TRIP;   // (<= 2^21)
    for (uint32_t base = blockIdx.x * EXPOSURE_TRIP; base < n; base += stride) {           // (uniform in the workgroup)
        float c[EXPOSURE_PER_THREAD][3];
        bool has[EXPOSURE_PER_THREAD];
#pragma unroll
        for (uint32_t j = 0; j < EXPOSURE_PER_THREAD; ++j) {   // the trip's loads first: EXPOSURE_PER_THREAD of them in flight per lane
            const uint32_t i = base + j * EXPOSURE_THREADS + threadIdx.x;
            has[j] = i < n;
            c[j][0] = c[j][1] = c[j][2] = 0.0f;
            if (has[j]) {
                if constexpr (Color::LINEAR) {
                    if (ww == p.width) color.linear((size_t)p.window[1] * p.width + i, c[j]);
                    else color(p.window[0] + i % ww, p.window[1] + i / ww, c[j]);
                } else color(p.window[0] + i % ww, p.window[1] + i / ww, c[j]);
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < EXPOSURE_PER_THREAD; ++j) {
            const uint32_t bin = has[j] ? exposure_bin(c[j]) : EXPOSURE_BINS;   // (no pixel: no bin)
#if ARCTIC_EXPOSURE_METER_VARIANT == 2
            const uint32_t first = __builtin_amdgcn_readfirstlane(bin);
            if (__builtin_amdgcn_ballot_w64(bin != first) == 0ull) {   // one bin in the whole wave (or no pixel in it): one add of the count
                if (first < EXPOSURE_BINS && (threadIdx.x & 63u) == 0u) __hip_atomic_fetch_add(&mine[first], 64u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else
#endif
            if (has[j]) __hip_atomic_fetch_add(&mine[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();   // (... and the second: the loop's bounds are the workgroup's)
    uint32_t sum = hist[0][threadIdx.x];
    for (uint32_t k = 1; k < EXPOSURE_HISTS; ++k) sum += hist[k][threadIdx.x];
    p.partials[(size_t)blockIdx.x * EXPOSURE_BINS + threadIdx.x] = sum;
}

__global__ __launch_bounds__(EXPOSURE_THREADS) void k_exposure_resolve(const ExposureParams p) {
    __shared__ uint32_t scan[2][EXPOSURE_BINS];
    __shared__ uint64_t tree_m[EXPOSURE_BINS], tree_s[EXPOSURE_BINS];
    const uint32_t b = threadIdx.x;
    uint32_t h = 0u;
#pragma unroll 16
    for (uint32_t g = 0; g < p.groups; ++g) h += p.partials[(size_t)g * EXPOSURE_BINS + b];
    p.hist[b] = h;
    const uint32_t counted = exposure_counted(p.d, b, h);
    scan[0][b] = counted;
    __syncthreads();
    uint32_t cur = 0u;
    for (uint32_t step = 1u; step < EXPOSURE_BINS; step <<= 1) {   // P_{b+1}: an inclusive scan, two buffers in turn, one barrier a step
        scan[cur ^ 1u][b] = scan[cur][b] + (b >= step ? scan[cur][b - step] : 0u);
        __syncthreads();
        cur ^= 1u;
    }
    const uint64_t p1 = scan[cur][b], p0 = p1 - counted, total = scan[cur][EXPOSURE_BINS - 1u];
    uint64_t lo, hi;
    exposure_band(p.d, total, lo, hi);
    const uint64_t share = exposure_share(p0, p1, lo, hi);
    tree_m[b] = share; tree_s[b] = share * b;
    __syncthreads();
    for (uint32_t half = EXPOSURE_BINS / 2u; half >= 1u; half >>= 1) {
        if (b < half) { tree_m[b] += tree_m[b + half]; tree_s[b] += tree_s[b + half]; }
        __syncthreads();
    }
    if (b == 0u) {
        ExposureState prev = {}, out;
        if (!p.fresh) prev = *p.state;
        exposure_adapt(p.d, tree_m[0], tree_s[0], prev, !p.fresh && prev.valid != 0u, out);
        *p.state = out;
    }
}

template <class Color>
__global__ __launch_bounds__(EXPOSURE_THREADS) void k_exposure_apply(const ExposureParams p, const Color color) {
    const uint32_t x = blockIdx.x * EXPOSURE_BLOCK + threadIdx.x % EXPOSURE_BLOCK, y = blockIdx.y * EXPOSURE_BLOCK + threadIdx.x / EXPOSURE_BLOCK;
    if (x >= p.width || y >= p.rows) return;
    const float e = p.state->exposure;
    const size_t o = (size_t)y * p.width + x;
    float c[3], out[3];
    color(x, y, c);
    exposure_apply(c, e, out);
    *reinterpret_cast<f3v *>(p.out_hdr + o * 3) = (f3v){out[0], out[1], out[2]};
    const f3 m = tonemap(mk(out[0], out[1], out[2]), p.tm, p.exposure);
    const float l0 = gamma_curve(m.x, p.inv_gamma), l1 = gamma_curve(m.y, p.inv_gamma), l2 = gamma_curve(m.z, p.inv_gamma);
    p.out_rgba8[o] = unorm8(l0) | (unorm8(l1) << 8) | (unorm8(l2) << 16) | 0xFF000000u;
    *reinterpret_cast<f3v *>(p.out_ldr + o * 3) = (f3v){l0, l1, l2};
}

bool exposure_frame_ok(const ExposureParams &p) { return p.width >= 1 && p.rows >= 1 && p.width <= EXPOSURE_MAX_SIDE && p.rows <= EXPOSURE_MAX_SIDE; }

}  // namespace

hipError_t launch_exposure_meter(const ExposureParams &p, hipStream_t s) {
    if (!exposure_frame_ok(p) || !p.color || !p.partials) return hipErrorInvalidValue;
    if (!(p.window[0] < p.window[2] && p.window[2] <= p.width && p.window[1] < p.window[3] && p.window[3] <= p.rows)) return hipErrorInvalidValue;
    if (p.groups != exposure_layout(p.width, p.rows).groups) return hipErrorInvalidValue;   // (T has that many rows)
    if (p.color_taa) k_exposure_meter<<<p.groups, EXPOSURE_THREADS, 0, s>>>(p, ExposureHistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_exposure_meter<<<p.groups, EXPOSURE_THREADS, 0, s>>>(p, ExposurePlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

hipError_t launch_exposure_resolve(const ExposureParams &p, hipStream_t s) {
    if (!exposure_frame_ok(p) || !p.partials || !p.hist || !p.state) return hipErrorInvalidValue;
    if (p.groups != exposure_layout(p.width, p.rows).groups) return hipErrorInvalidValue;
    k_exposure_resolve<<<1, EXPOSURE_THREADS, 0, s>>>(p);
    return hipGetLastError();
}

hipError_t launch_exposure_apply(const ExposureParams &p, hipStream_t s) {
    if (!exposure_frame_ok(p) || !p.color || !p.state || !p.out_hdr || !p.out_rgba8 || !p.out_ldr) return hipErrorInvalidValue;
    const dim3 grid((p.width + EXPOSURE_BLOCK - 1) / EXPOSURE_BLOCK, (p.rows + EXPOSURE_BLOCK - 1) / EXPOSURE_BLOCK);
    if (p.color_taa) k_exposure_apply<<<grid, EXPOSURE_THREADS, 0, s>>>(p, ExposureHistoryColor{static_cast<const float4 *>(p.color), p.tiles_x});
    else k_exposure_apply<<<grid, EXPOSURE_THREADS, 0, s>>>(p, ExposurePlaneColor{static_cast<const float *>(p.color), p.width});
    return hipGetLastError();
}

}  // namespace arctic
