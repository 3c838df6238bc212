// env_light.hip -- the once-per-map precompute of the image-based ambient term (ARCTIC_OPT_ENV_LIGHTING; semantics in
// include/arctic_hip.h next to the option).  From the equirect environment map, on the device, in stream order:
//   k_env_mip       the 2x2 box-filtered mip chain the prefilter samples (filtered importance sampling)
//   k_env_sh_rows   per map row, the 27 weighted SH sums in binary64 (fixed tree order in LDS) ...
//   k_env_sh_final  ... summed over the rows in a fixed order, A_l folded in: no float atomics, so the same map gives the same
//                   bits on every handle (shards of one frame stitch bit for bit)
//   k_env_prefilter specular levels 1..5: Karis' split-sum prefilter (N = V = R), 512 Hammersley samples, GGX with alpha = r^2
//   k_env_brdf      the 64 x 64 (A, B) table: 1024 Hammersley samples, Smith-Schlick with k = r^2 / 2
// None of this runs per frame.  The arithmetic is binary64 throughout (the tables are stored in fp32): the tests compare against an
// independent float64 numpy implementation (tests/env_reference.py), and a one-off pass has no reason to be approximate.
#include "common.h"

namespace arctic {

namespace {

// the skybox's mapping (skybox.hlsl:74-85, shade.hip sample_environment): u = atan2(z, x) C_U + 0.5, v = -(asin(y) C_V + 0.5),
// with the fp32 constants the reference writes
constexpr double C_U = (double)0.1591f, C_V = (double)0.3183f;
constexpr double PI_D = 3.14159265358979323846;

struct d3 { double x, y, z; };
__device__ __forceinline__ d3 dmk(double x, double y, double z) { d3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ double ddot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 dcross(d3 a, d3 b) { return dmk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ d3 dnorm(d3 a) { const double s = 1.0 / sqrt(ddot(a, a)); return dmk(a.x * s, a.y * s, a.z * s); }

// direction of the centre of texel (i, j) of a W x H equirect
__device__ __forceinline__ d3 texel_dir(uint32_t i, uint32_t j, uint32_t W, uint32_t H, double &cos_theta) {
    const double u = ((double)i + 0.5) / (double)W, v = ((double)j + 0.5) / (double)H;
    const double phi = (u - 0.5) / C_U, theta = (0.5 - v) / C_V;
    cos_theta = cos(theta);
    return dmk(cos_theta * cos(phi), sin(theta), cos_theta * sin(phi));
}

// bilinear + WRAP lookup of a W x H RGBA32F equirect along a unit direction (binary64 coordinates and weights)
__device__ __forceinline__ void wrap64(double u, uint32_t n, uint32_t &i0, uint32_t &i1, double &f) {
    const double x = (u - floor(u)) * (double)n - 0.5, xf = floor(x);
    f = x - xf;
    int a = (int)xf, b = a + 1;
    if (a < 0) a += (int)n;
    if (b >= (int)n) b -= (int)n;
    i0 = (uint32_t)a; i1 = (uint32_t)b;
}
__device__ __forceinline__ d3 sample_dir(const float4 *img, uint32_t W, uint32_t H, d3 d) {
    const double u = atan2(d.z, d.x) * C_U + 0.5;
    const double v = -(asin(fmin(fmax(d.y, -1.0), 1.0)) * C_V + 0.5);
    uint32_t x0, x1, y0, y1;
    double fx, fy;
    wrap64(u, W, x0, x1, fx);
    wrap64(v, H, y0, y1, fy);
    const float4 a = img[(size_t)y0 * W + x0], b = img[(size_t)y0 * W + x1], c = img[(size_t)y1 * W + x0], e = img[(size_t)y1 * W + x1];
    const double w00 = (1 - fx) * (1 - fy), w10 = fx * (1 - fy), w01 = (1 - fx) * fy, w11 = fx * fy;
    return dmk(w00 * a.x + w10 * b.x + w01 * c.x + w11 * e.x, w00 * a.y + w10 * b.y + w01 * c.y + w11 * e.y,
               w00 * a.z + w10 * b.z + w01 * c.z + w11 * e.z);
}

// Hammersley point i of n: (i / n, radical inverse of i in base 2)
__device__ __forceinline__ double radical_inverse(uint32_t i) { return (double)__brev(i) * (1.0 / 4294967296.0); }
// GGX importance sample (Karis 2013): the half vector around n for Hammersley point (x1, x2), alpha = r^2; frame: up = z unless n is
// within 0.999 of it, then x
__device__ __forceinline__ d3 ggx_half(double x1, double x2, double alpha, d3 n, double &cos_h) {
    const double a2 = alpha * alpha, phi = 2.0 * PI_D * x1;
    cos_h = sqrt((1.0 - x2) / (1.0 + (a2 - 1.0) * x2));
    const double sin_h = sqrt(fmax(0.0, 1.0 - cos_h * cos_h));
    const d3 up = fabs(n.z) < 0.999 ? dmk(0, 0, 1) : dmk(1, 0, 0);
    const d3 tx = dnorm(dcross(up, n)), ty = dcross(n, tx);
    const double hx = sin_h * cos(phi), hy = sin_h * sin(phi);
    return dmk(tx.x * hx + ty.x * hy + n.x * cos_h, tx.y * hx + ty.y * hy + n.y * cos_h, tx.z * hx + ty.z * hy + n.z * cos_h);
}

// ---- mip chain: level m + 1 from level m (env_mip_count's rule, common.h) --------------------------------------------------
__global__ __launch_bounds__(256) void k_env_mip(const float4 *__restrict__ src, uint32_t sw, uint32_t sh, float4 *__restrict__ dst, uint32_t dw, uint32_t dh) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= dw || j >= dh) return;
    const uint32_t x0 = min(2 * i, sw - 1), x1 = min(2 * i + 1, sw - 1), y0 = min(2 * j, sh - 1), y1 = min(2 * j + 1, sh - 1);
    const float4 a = src[(size_t)y0 * sw + x0], b = src[(size_t)y0 * sw + x1], c = src[(size_t)y1 * sw + x0], d = src[(size_t)y1 * sw + x1];
    dst[(size_t)j * dw + i] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                                          ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

// ---- SH projection: one workgroup per map row, 27 sums per thread over a fixed set of texels, a fixed tree in LDS ------------
// real SH basis, k = 0..8: 1 / (2 sqrt(pi)); sqrt(3 / 4pi) (y, z, x); sqrt(15 / 4pi) (xy, yz), sqrt(5 / 16pi) (3z^2 - 1), sqrt(15 / 4pi) xz,
// sqrt(15 / 16pi) (x^2 - y^2)
__device__ __forceinline__ void sh_basis(d3 d, double *Y) {
    const double c0 = 0.28209479177387814, c1 = 0.4886025119029199, c2 = 1.0925484305920792, c3 = 0.31539156525252005, c4 = 0.5462742152960396;
    Y[0] = c0; Y[1] = c1 * d.y; Y[2] = c1 * d.z; Y[3] = c1 * d.x;
    Y[4] = c2 * d.x * d.y; Y[5] = c2 * d.y * d.z; Y[6] = c3 * (3.0 * d.z * d.z - 1.0); Y[7] = c2 * d.x * d.z; Y[8] = c4 * (d.x * d.x - d.y * d.y);
}
constexpr int SH_THREADS = 256;
__global__ __launch_bounds__(SH_THREADS) void k_env_sh_rows(const float4 *__restrict__ env, uint32_t W, uint32_t H, double *__restrict__ rows) {
    __shared__ double red[SH_THREADS];
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    double acc[27];
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (uint32_t i = t; i < W; i += SH_THREADS) {
        double ct;
        const d3 d = texel_dir(i, j, W, H, ct);
        double Y[9];
        sh_basis(d, Y);
        const float4 L = env[(size_t)j * W + i];
        for (int k = 0; k < 9; ++k) { acc[3 * k] += (double)L.x * Y[k]; acc[3 * k + 1] += (double)L.y * Y[k]; acc[3 * k + 2] += (double)L.z * Y[k]; }
    }
    // the row's solid angle per texel: max(cos theta, 0) dphi dtheta
    double ct;
    (void)texel_dir(0, j, W, H, ct);
    const double w = fmax(ct, 0.0) * (1.0 / (C_U * (double)W)) * (1.0 / (C_V * (double)H));
    for (int k = 0; k < 27; ++k) {
        red[t] = acc[k];
        __syncthreads();
        for (uint32_t s = SH_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        if (t == 0) rows[(size_t)j * 27 + k] = red[0] * w;
        __syncthreads();
    }
}
// coefficient k = blockIdx.x: thread t sums rows t, t + 256, ... in order, then the same fixed tree; A_l folded in
__global__ __launch_bounds__(SH_THREADS) void k_env_sh_final(const double *__restrict__ rows, uint32_t H, EnvTables *__restrict__ out) {
    __shared__ double red[SH_THREADS];
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (uint32_t j = t; j < H; j += SH_THREADS) s += rows[(size_t)j * 27 + k];
    red[t] = s;
    __syncthreads();
    for (uint32_t h = SH_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t band = k / 3 == 0 ? 0 : (k / 3 < 4 ? 1 : 2);
        const double A = band == 0 ? PI_D : (band == 1 ? 2.0 * PI_D / 3.0 : PI_D / 4.0);
        out->sh[k] = (float)(red[0] * A);
    }
}

// ---- specular levels: one thread per output texel --------------------------------------------------------------------------
struct MipChain { const float4 *level[16]; uint32_t w[16], h[16]; uint32_t n; };
__device__ __forceinline__ d3 sample_lod(const MipChain &m, d3 d, double lod) {
    const double top = (double)(m.n - 1);
    if (lod >= top) return sample_dir(m.level[m.n - 1], m.w[m.n - 1], m.h[m.n - 1], d);
    const uint32_t l0 = (uint32_t)floor(lod);
    const double f = lod - (double)l0;
    const d3 a = sample_dir(m.level[l0], m.w[l0], m.h[l0], d);
    if (f == 0.0) return a;
    const d3 b = sample_dir(m.level[l0 + 1], m.w[l0 + 1], m.h[l0 + 1], d);
    return dmk(a.x + (b.x - a.x) * f, a.y + (b.y - a.y) * f, a.z + (b.z - a.z) * f);
}
__global__ __launch_bounds__(256) void k_env_prefilter(MipChain m, double alpha, uint32_t W, uint32_t H, float4 *__restrict__ out, uint32_t w, uint32_t h) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= w || j >= h) return;
    double ct;
    const d3 n = texel_dir(i, j, w, h, ct);
    const double omega_p = 4.0 * PI_D / ((double)W * (double)H), a2 = alpha * alpha;
    double sx = 0, sy = 0, sz = 0, ws = 0;
    for (uint32_t s = 0; s < ENV_SAMPLES; ++s) {
        double nh;
        const d3 hv = ggx_half((double)s / ENV_SAMPLES, radical_inverse(s), alpha, n, nh);
        const double vh = ddot(n, hv);
        const d3 l = dmk(2 * vh * hv.x - n.x, 2 * vh * hv.y - n.y, 2 * vh * hv.z - n.z);
        const double nl = ddot(n, l);
        if (nl <= 0.0) continue;
        const double q = nh * nh * (a2 - 1.0) + 1.0, D = a2 / (PI_D * q * q);
        const double omega_s = 4.0 / ((double)ENV_SAMPLES * D);
        const double lod = fmax(0.0, 0.5 * log2(omega_s / omega_p) + 1.0);
        const d3 c = sample_lod(m, l, lod);
        sx += c.x * nl; sy += c.y * nl; sz += c.z * nl; ws += nl;
    }
    const double inv = ws > 0 ? 1.0 / ws : 0.0;
    out[(size_t)j * w + i] = make_float4((float)(sx * inv), (float)(sy * inv), (float)(sz * inv), 1.0f);
}

// ---- the BRDF table: cell (i, j) = (n.v, roughness) at cell centres -------------------------------------------------------
__global__ __launch_bounds__(256) void k_env_brdf(float2 *__restrict__ lut) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ENV_LUT * ENV_LUT) return;
    const uint32_t i = c % ENV_LUT, j = c / ENV_LUT;
    const double nv = ((double)i + 0.5) / ENV_LUT, r = ((double)j + 0.5) / ENV_LUT, alpha = r * r, k = r * r / 2.0;
    const d3 n = dmk(0, 0, 1), v = dmk(sqrt(1.0 - nv * nv), 0, nv);
    double A = 0, B = 0;
    for (uint32_t s = 0; s < ENV_LUT_SAMPLES; ++s) {
        double nh;
        const d3 hv = ggx_half((double)s / ENV_LUT_SAMPLES, radical_inverse(s), alpha, n, nh);
        const double vh_raw = ddot(v, hv);
        const d3 l = dmk(2 * vh_raw * hv.x - v.x, 2 * vh_raw * hv.y - v.y, 2 * vh_raw * hv.z - v.z);
        const double nl = fmin(fmax(l.z, 0.0), 1.0), nhc = fmin(fmax(hv.z, 0.0), 1.0), vh = fmin(fmax(vh_raw, 0.0), 1.0);
        if (nl <= 0.0) continue;
        const double g = (nv / (nv * (1 - k) + k)) * (nl / (nl * (1 - k) + k));
        const double gv = g * vh / (nhc * nv);
        const double fc = pow(1.0 - vh, 5.0);
        A += (1.0 - fc) * gv; B += fc * gv;
    }
    lut[c] = make_float2((float)(A / ENV_LUT_SAMPLES), (float)(B / ENV_LUT_SAMPLES));
}

}  // namespace

size_t env_levels_bytes(uint32_t W, uint32_t H) {
    size_t n = 0;
    for (uint32_t k = 1; k < ENV_LEVELS; ++k) { uint32_t w, h; env_level_size(W, H, k, w, h); n += (size_t)w * h; }
    return n * sizeof(float4);
}
size_t env_mips_bytes(uint32_t W, uint32_t H) {
    size_t n = 0;
    uint32_t w = W, h = H;
    while (w > 1 || h > 1) { w = std::max(1u, w >> 1); h = std::max(1u, h >> 1); n += (size_t)w * h; }
    return std::max<size_t>(n, 1) * sizeof(float4);
}

// everything on stream s; b.tables must already hold the level pointers / sizes and the LUT pointer (the host writes them before)
hipError_t launch_env_build(const EnvBuild &b, hipStream_t s) {
    MipChain m;
    m.level[0] = b.env; m.w[0] = b.W; m.h[0] = b.H; m.n = 1;
    float4 *p = b.mips;
    while ((m.w[m.n - 1] > 1 || m.h[m.n - 1] > 1) && m.n < 16) {
        const uint32_t sw = m.w[m.n - 1], sh = m.h[m.n - 1], dw = std::max(1u, sw >> 1), dh = std::max(1u, sh >> 1);
        k_env_mip<<<dim3((dw + 255) / 256, dh), 256, 0, s>>>(m.level[m.n - 1], sw, sh, p, dw, dh);
        m.level[m.n] = p; m.w[m.n] = dw; m.h[m.n] = dh; ++m.n;
        p += (size_t)dw * dh;
    }
    k_env_sh_rows<<<b.H, SH_THREADS, 0, s>>>(b.env, b.W, b.H, b.sh_rows);
    k_env_sh_final<<<27, SH_THREADS, 0, s>>>(b.sh_rows, b.H, b.tables);
    float4 *lv = b.levels;
    for (uint32_t k = 1; k < ENV_LEVELS; ++k) {
        uint32_t w, h;
        env_level_size(b.W, b.H, k, w, h);
        const double r = (double)k / (ENV_LEVELS - 1);
        k_env_prefilter<<<dim3((w + 255) / 256, h), 256, 0, s>>>(m, r * r, b.W, b.H, lv, w, h);
        lv += (size_t)w * h;
    }
    k_env_brdf<<<(ENV_LUT * ENV_LUT + 255) / 256, 256, 0, s>>>(b.lut);
    return hipGetLastError();
}

}  // namespace arctic
