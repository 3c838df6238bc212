// hit_shade_ext.hip -- k_shade_hits_ext: the colour at a ray hit under ARCTIC_OPT_HIT_MODEL = 1 (include/arctic_hip.h in front of arctic_shade_hits).
// k_shade_hits' pixel (hit_shade.hip) with what the forward pass has gained since, each by the definition the header gives next to its call or option,
// one light at a time in the caller's order:
//   material extras    factors on base, metal and rough, the normal scale on tangent-space x and y, emission outside (1 - shadow), occlusion on the
//                      ambient term only (material_sampler.h: sample_extras, both storage layouts, level 0)
//   spot lights        behind the point lights: squared cone ramp sat(cd scale + offset)^2, range window sat(1 - (d2 ir2)^2), colour / d2
//   cube lights        behind the spots: face by the largest |d| (ties x, y, z), the header's face rows, four clamped texels, compare then bilinear,
//                      v = 1 outside the near and far planes; under the sun's (1 - shadow) like every other light
//   image-based ambient   ambient * ibl(n, wo, base, metal, rough) from the resident EnvTables in place of ambient * base; R and its texel
//                      coordinates in binary64 from the hit's own numbers, as the shading pass has them
// The same shape as k_shade_hits: one hit per lane, grid-stride; everything behind the hit record gathered per lane with vector loads (no waterfall
// over a wave's materials or lights' faces); the misses' environment lookup in a second loop of its own.  No LDS, no barrier, no atomics; vector
// stores only.  Compiled with contraction off.
// The base part is k_shade_hits' text, operation for operation, from the same device functions (hit_shade_device.h): with no spot light, no cube
// light, no extras and no tables the kernel leaves k_shade_hits' bytes (a loop of zero trips and a branch not taken change no bits).
// A hit has no pixel footprint: every image is taken at level 0, mip chains (ARCTIC_OPT_TEXTURE_MIPS) do not take part.
#include "hit_shade_ext.h"
#include "hit_shade_device.h"

namespace arctic {

namespace {

__device__ __forceinline__ float hx_sat(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// ---- shadow-casting point lights: v of d = world - p on one light's six faces (shade.hip: cube_visibility, the same operations) ----------------
// lookAt rows  +X: s = -z, u = -y   -X: s = +z, u = -y   +Y: s = +x, u = +z   -Y: s = +x, u = -z   +Z: s = +x, u = -y   -Z: s = -x, u = -y
// Every texel index is clamped to the face behind the conversion to int, whatever d holds
__device__ __forceinline__ float hx_cube_visibility(const float *__restrict__ faces, uint32_t F, f3 d, float pz_scale, float zn) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    float m, sd, ud;
    uint32_t face;
    if (ax >= ay && ax >= az) { m = ax; face = d.x >= 0.0f ? 0u : 1u; sd = d.x >= 0.0f ? -d.z : d.z; ud = -d.y; }   // ties: x, then y, then z
    else if (ay >= az) { m = ay; face = d.y >= 0.0f ? 2u : 3u; sd = d.x; ud = d.y >= 0.0f ? d.z : -d.z; }
    else { m = az; face = d.z >= 0.0f ? 4u : 5u; sd = d.z >= 0.0f ? d.x : -d.x; ud = -d.y; }
    if (!(m > zn)) return 1.0f;                                   // inside the near plane (or not a number): no lookup
    const float im = 1.0f / m;
    const float pz = pz_scale * (1.0f - zn * im);
    if (pz > 1.0f) return 1.0f;                                   // beyond the far plane
    const float hf = 0.5f * (float)F;
    const float x = __builtin_fmaf(sd * im, hf, hf - 0.5f), y = __builtin_fmaf(-(ud * im), hf, hf - 0.5f);   // px F - 0.5, py F - 0.5
    const float x0 = floorf(x), y0 = floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int32_t last = (int32_t)F - 1, ix = (int32_t)x0, iy = (int32_t)y0;
    const uint32_t c0 = (uint32_t)min(max(ix, 0), last), c1 = (uint32_t)min(max(ix + 1, 0), last);
    const uint32_t r0 = (uint32_t)min(max(iy, 0), last) * F, r1 = (uint32_t)min(max(iy + 1, 0), last) * F;
    const float *f = faces + (size_t)face * F * F;
    const float s00 = pz > f[r0 + c0] ? 1.0f : 0.0f, s10 = pz > f[r0 + c1] ? 1.0f : 0.0f, s01 = pz > f[r1 + c0] ? 1.0f : 0.0f, s11 = pz > f[r1 + c1] ? 1.0f : 0.0f;
    return 1.0f - hs_lerp(hs_lerp(s00, s10, fx), hs_lerp(s01, s11, fx), fy);
}

// ---- image-based ambient (ARCTIC_OPT_ENV_LIGHTING; shade.hip: env_level, env_specular64, env_reflection, env_ambient restated for one hit) ------
__device__ __forceinline__ f3 hx_env_level(const EnvTables *__restrict__ T, uint32_t k, double u, double v) {
    const float4 *img = T->level[k];
    const uint32_t w = T->w[k], h = T->h[k];
    int x0, x1, y0, y1;
    float fx, fy;
    hs_wrap_axis64(u, w, x0, x1, fx);
    hs_wrap_axis64(v, h, y0, y1, fy);
    const float4 a = img[(size_t)y0 * w + x0], b = img[(size_t)y0 * w + x1], c = img[(size_t)y1 * w + x0], e = img[(size_t)y1 * w + x1];
    const Weights k4 = hs_weights(fx, fy);
    return mk(hs_filter(k4, a.x, b.x, c.x, e.x), hs_filter(k4, a.y, b.y, c.y, e.y), hs_filter(k4, a.z, b.z, c.z, e.z));
}
// P(R, rough), R = 2 (n.wo) n - wo in binary64 from the attributes a[], the normal map's channels (0..255 scale), the normal scale and the eye
__device__ __forceinline__ f3 hx_env_specular(const EnvTables *__restrict__ T, const float *a, const float *nrm, float ns, const rq_f4 &eye, float rough) {
    const double r = ((double)nrm[0] * (2.0 / 255.0) - 1.0) * ns, g = -((double)nrm[1] * (2.0 / 255.0) - 1.0) * ns, b = (double)nrm[2] * (2.0 / 255.0) - 1.0;
    double nx = (double)a[8] * b + ((double)a[5] * g + (double)a[2] * r), ny = (double)a[9] * b + ((double)a[6] * g + (double)a[3] * r),
           nz = (double)a[10] * b + ((double)a[7] * g + (double)a[4] * r);
    const double ni = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
    nx *= ni; ny *= ni; nz *= ni;
    double wx = (double)eye[0] - a[11], wy = (double)eye[1] - a[12], wz = (double)eye[2] - a[13];
    const double wi = 1.0 / sqrt(wx * wx + wy * wy + wz * wz);
    wx *= wi; wy *= wi; wz *= wi;
    const double two = 2.0 * (nx * wx + ny * wy + nz * wz);
    const double x = two * nx - wx, y = two * ny - wy, z = two * nz - wz;
    const double inv = 1.0 / sqrt(x * x + y * y + z * z);
    const double u = atan2(z * inv, x * inv) * (double)0.1591f + 0.5;
    const double v = -(asin(fmin(fmax(y * inv, -1.0), 1.0)) * (double)0.3183f + 0.5);
    const float t = rough * (float)(ENV_LEVELS - 1);
    const uint32_t k0 = min((uint32_t)t, ENV_LEVELS - 1), k1 = min(k0 + 1u, ENV_LEVELS - 1);
    const float f = t - (float)k0;
    const f3 P0 = hx_env_level(T, k0, u, v), P1 = hx_env_level(T, k1, u, v);
    return mk(hs_lerp(P0.x, P1.x, f), hs_lerp(P0.y, P1.y, f), hs_lerp(P0.z, P1.z, f));
}
// the bracket  (1 - F)(1 - metal) base E(n) / pi + P (F0 A + B)
__device__ __forceinline__ f3 hx_env_ambient(const EnvTables *__restrict__ T, f3 n, f3 wo, f3 P, f3 base, float metal, float rough) {
    const float *sh = T->sh;
    const float Y[9] = {0.28209479f, 0.48860251f * n.y, 0.48860251f * n.z, 0.48860251f * n.x, 1.09254843f * (n.x * n.y), 1.09254843f * (n.y * n.z),
                        0.31539157f * (3.0f * (n.z * n.z) - 1.0f), 1.09254843f * (n.x * n.z), 0.54627422f * (n.x * n.x - n.y * n.y)};
    float E[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float e = sh[c] * Y[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) e = __builtin_fmaf(sh[3 * k + c], Y[k], e);
        E[c] = e;
    }
    const float ndwo = fmaxf(dot(n, wo), 0.0f);
    const f3 F0 = mk(0.04f + (base.x - 0.04f) * metal, 0.04f + (base.y - 0.04f) * metal, 0.04f + (base.z - 0.04f) * metal);
    const float om = 1.0f - ndwo, om2 = om * om, p5 = (om2 * om2) * om, omr = 1.0f - rough;
    const f3 F = mk(F0.x + (fmaxf(omr, F0.x) - F0.x) * p5, F0.y + (fmaxf(omr, F0.y) - F0.y) * p5, F0.z + (fmaxf(omr, F0.z) - F0.z) * p5);
    // (A, B): bilinear, clamped, cell centres
    const float lx = fminf(fmaxf(ndwo * (float)ENV_LUT - 0.5f, 0.0f), (float)(ENV_LUT - 1)), ly = fminf(fmaxf(rough * (float)ENV_LUT - 0.5f, 0.0f), (float)(ENV_LUT - 1));
    const uint32_t i0 = min((uint32_t)lx, ENV_LUT - 1), j0 = min((uint32_t)ly, ENV_LUT - 1), i1 = min(i0 + 1u, ENV_LUT - 1), j1 = min(j0 + 1u, ENV_LUT - 1);
    const float2 *lut = T->lut;
    const float2 l00 = lut[j0 * ENV_LUT + i0], l10 = lut[j0 * ENV_LUT + i1], l01 = lut[j1 * ENV_LUT + i0], l11 = lut[j1 * ENV_LUT + i1];
    const Weights w = hs_weights(lx - (float)i0, ly - (float)j0);
    const float A = hs_filter(w, l00.x, l10.x, l01.x, l11.x), B = hs_filter(w, l00.y, l10.y, l01.y, l11.y);
    const float kb = (1.0f - metal) / HS_PI;
    return mk(((1.0f - F.x) * kb) * base.x * E[0] + P.x * (F0.x * A + B), ((1.0f - F.y) * kb) * base.y * E[1] + P.y * (F0.y * A + B),
              ((1.0f - F.z) * kb) * base.z * E[2] + P.z * (F0.z * A + B));
}

// The hits, then the sky along the misses, in two loops for the register reason written above k_shade_hits: the second loop is that kernel's
__global__ __launch_bounds__(HIT_THREADS) void k_shade_hits_ext(const RayIn *__restrict__ rays, const RayOut *__restrict__ hits, uint32_t n, const HitShadeExtParams q,
                                                                float4 *__restrict__ out) {
    const HitShadeParams &p = q.base;
    for (uint64_t k = (uint64_t)blockIdx.x * HIT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * HIT_THREADS) {
        const rq_f4 ro = *reinterpret_cast<const rq_f4 *>(rays + k);   // {origin, t_min}
        float a[HIT_ATTRS];
        const uint32_t mat = hit_attributes(load_hit(hits, k), p.src, p.n_prims, p.objs, p.lpv, a);
        float4 color = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mat != HIT_NO_MATERIAL) {
            Channels c = sample_material(p.tex, p.srgb_lut, mat, a[0], a[1]);
            float ns = 1.0f, ao = 1.0f;
            f3 emis = mk(0.0f, 0.0f, 0.0f);
            if (q.extras != nullptr) {   // base' = base f, metal' = metal f, rough' = rough f; a neutral record multiplies by 1.0f
                const ExtraChannels x = sample_extras(q.extras, p.srgb_lut, mat, a[0], a[1]);
                c.base[0] *= x.base[0]; c.base[1] *= x.base[1]; c.base[2] *= x.base[2];
                c.metal *= x.metal; c.rough *= x.rough;
                ns = x.nscale; ao = x.ao;
                emis = mk(x.emis[0], x.emis[1], x.emis[2]);
            }
            Surface s;
            // get_normal (forward.hlsl:104-111) with the normal scale on the tangent-space x and y (a scale of 1 multiplies exactly)
            float tr = hs_snorm(c.nrm[0]), tg = -hs_snorm(c.nrm[1]);
            const float tb = hs_snorm(c.nrm[2]);
            if (q.extras != nullptr) { tr = tr * ns; tg = tg * ns; }
            s.n = normalize(mk((a[2] * tr + a[5] * tg) + a[8] * tb, (a[3] * tr + a[6] * tg) + a[9] * tb, (a[4] * tr + a[7] * tg) + a[10] * tb));
            const f3 world = mk(a[11], a[12], a[13]);
            s.wo = normalize(mk(ro[0], ro[1], ro[2]) - world);
            const f3 base = mk(c.base[0], c.base[1], c.base[2]);
            s.F0 = mk(0.04f + (base.x - 0.04f) * c.metal, 0.04f + (base.y - 0.04f) * c.metal, 0.04f + (base.z - 0.04f) * c.metal);
            s.kdb = base * ((1.0f - c.metal) / HS_PI);
            const float al = c.rough * c.rough, r1 = c.rough + 1.0f, ndwo = fmaxf(dot(s.n, s.wo), 0.0f);
            s.a2 = al * al;
            s.k = (r1 * r1) * 0.125f;
            s.omk = 1.0f - s.k;
            s.num = (s.a2 / HS_PI) * (ndwo / (ndwo * s.omk + s.k));
            s.four_ndwo = 4.0f * ndwo;
            const float lit = 1.0f - hit_shadow(p.shadow_map, p.shadow_size, a + 14);
            f3 Lo = mk(0.0f, 0.0f, 0.0f);
            if (lit != 0.0f) {   // all 25 taps shadowed: every light's term is multiplied by zero
                Lo = hs_radiance(s, mk(-p.sun_dir[0], -p.sun_dir[1], -p.sun_dir[2]), mk(p.sun_color[0], p.sun_color[1], p.sun_color[2]));
                for (uint32_t i = 0; i < p.n_lights; ++i) {
                    const float4 lp = p.lights[2 * i], lc = p.lights[2 * i + 1];
                    const f3 d = mk(lp.x, lp.y, lp.z) - world;
                    const float inv = __builtin_amdgcn_rsqf(dot(d, d)), inv2 = inv * inv;   // wi = d / |d|, radiance = colour / |d|^2
                    Lo = Lo + hs_radiance(s, d * inv, mk(lc.x * inv2, lc.y * inv2, lc.z * inv2));
                }
                for (uint32_t i = 0; i < q.n_spots; ++i) {   // {p.xyz, scale} {s.xyz, offset} {rgb, ir2}
                    const float4 la = q.spots[SPOT_F4 * i], lb = q.spots[SPOT_F4 * i + 1], lc = q.spots[SPOT_F4 * i + 2];
                    const f3 d = mk(la.x, la.y, la.z) - world;
                    const float d2 = dot(d, d), inv = __builtin_amdgcn_rsqf(d2), inv2 = inv * inv;
                    const float cd = -dot(mk(lb.x, lb.y, lb.z), d) * inv;
                    const float att = hx_sat(cd * la.w + lb.w), w = d2 * lc.w;
                    const float f = ((att * att) * hx_sat(1.0f - w * w)) * inv2;
                    if (f > 0.0f) Lo = Lo + hs_radiance(s, d * inv, mk(lc.x * f, lc.y * f, lc.z * f));   // (outside the cone or the range the term is exactly zero)
                }
                const float *faces = reinterpret_cast<const float *>(q.cubes + CUBE_F4 * q.n_cubes);
                for (uint32_t i = 0; i < q.n_cubes; ++i) {   // {p.xyz, zf / (zf - zn)} {rgb, zn}
                    const float4 la = q.cubes[CUBE_F4 * i], lc = q.cubes[CUBE_F4 * i + 1];
                    const f3 d = mk(la.x, la.y, la.z) - world;
                    if (!(dot(s.n, d) > 0.0f)) continue;   // behind the surface n.wi clamps to 0: no texel is read
                    const float v = hx_cube_visibility(faces + (size_t)i * 6u * q.cube_size * q.cube_size, q.cube_size, mk(-d.x, -d.y, -d.z), la.w, lc.w);
                    if (v == 0.0f) continue;
                    const float inv = __builtin_amdgcn_rsqf(dot(d, d)), f = (inv * inv) * v;
                    Lo = Lo + hs_radiance(s, d * inv, mk(lc.x * f, lc.y * f, lc.z * f));
                }
            }
            f3 amb = mk(p.ambient * base.x, p.ambient * base.y, p.ambient * base.z);
            if (q.env_tables != nullptr) {   // shadowed hits take it too: never under (1 - shadow)
                const f3 P = hx_env_specular(q.env_tables, a, c.nrm, ns, ro, c.rough);
                amb = hx_env_ambient(q.env_tables, s.n, s.wo, P, base, c.metal, c.rough) * p.ambient;
            }
            if (q.extras != nullptr) amb = amb * ao;   // occlusion: the ambient term only
            color = make_float4(Lo.x * lit + amb.x, Lo.y * lit + amb.y, Lo.z * lit + amb.z, 1.0f);
            if (q.extras != nullptr) { color.x += emis.x; color.y += emis.y; color.z += emis.z; }   // emission: no (1 - shadow), no occlusion
        }
        out[k] = color;   // (a miss: {0, 0, 0, 0} until the loop below says otherwise)
    }
    if (p.env == nullptr) return;
    for (uint64_t k = (uint64_t)blockIdx.x * HIT_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * HIT_THREADS) {
        HitSource s;
        if (hit_source(load_hit(hits, k), p.src, p.n_prims, s) && p.objs[s.object].material != HIT_NO_MATERIAL) continue;   // shaded above
        const rq_f4 rd = reinterpret_cast<const rq_f4 *>(rays + k)[1];   // {direction, t_max}
        const float d[3] = {rd[0], rd[1], rd[2]};
        if (rq_finite(d[0]) && rq_finite(d[1]) && rq_finite(d[2]) && !(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f)) {
            const f3 e = hit_environment(p.env, p.env_w, p.env_h, d);
            out[k] = make_float4(e.x, e.y, e.z, 0.0f);   // this lane's own store above is behind it in program order
        }
    }
}

}  // namespace

hipError_t launch_shade_hits_ext(const void *rays, const void *hits, uint64_t n, const HitShadeExtParams &p, float4 *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    k_shade_hits_ext<<<hit_grid(n), HIT_THREADS, 0, s>>>(static_cast<const RayIn *>(rays), static_cast<const RayOut *>(hits), (uint32_t)n, p, out);
    return hipGetLastError();
}

}  // namespace arctic
