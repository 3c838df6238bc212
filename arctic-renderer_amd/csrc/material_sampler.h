// material_sampler.h -- a material's channels at one texture coordinate: the sampler ps_main uses by default (MIN_MAG_MIP_LINEAR + WRAP at level 0,
// texel centres at +0.5, full fp32 weights, sRGB decoded per texel before filtering), for one pixel at a time and all three image layouts of
// common.h TexDesc.  ONE copy, included by hit_shade.hip (k_shade_hits), hit_shade_ext.hip (k_shade_hits_ext, which also takes the material's
// extras: sample_extras below), compose.hip (k_compose) and gi.hip; every descriptor and texel is a vector load, per lane.  Device compilation only;
// compile with contraction off.
#pragma once
#include "common.h"
#include "ray_query.h"

namespace arctic {

namespace {

// ---- the sampler: MIN_MAG_MIP_LINEAR + WRAP at level 0, texel centres at +0.5, full fp32 weights (the default of ARCTIC_OPT_SAMPLER) ------------
// first texel of the footprint in [-1, n - 1] and the weight of the second.  (The clamp changes no coordinate that is a number: it keeps the
// address of a NaN or infinite one inside the image.)
__device__ __forceinline__ void hs_axis(float u, float nf, int n, int &i0, float &f) {
    const float uw = u - floorf(u);
    const float x = uw * nf - 0.5f;
    const float xf = floorf(x);
    f = x - xf;
    i0 = min(max((int)xf, -1), n - 1);
}
struct Weights { float w00, w10, w01, w11; };
__device__ __forceinline__ Weights hs_weights(float fx, float fy) {
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const Weights w = {gx * gy, fx * gy, gx * fy, fx * fy};
    return w;
}
__device__ __forceinline__ float hs_filter(const Weights &w, float a, float b, float c, float d) { return ((w.w00 * a + w.w10 * b) + w.w01 * c) + w.w11 * d; }
__device__ __forceinline__ float hs_byte(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu); }
// a plain RGBA8 image (a material of unequal image sizes): the four texels of the footprint under WRAP
__device__ __forceinline__ Weights hs_fetch_plain(const TexDesc &d, float u, float v, uint32_t t[4]) {
    int x0, y0;
    float fx, fy;
    const int w = (int)(d.w & ~TEX_INTERLEAVED), h = (int)d.h;
    hs_axis(u, d.wf, w, x0, fx);
    hs_axis(v, d.hf, h, y0, fy);
    const int x1 = x0 + 1 == w ? 0 : x0 + 1, y1 = y0 + 1 == h ? 0 : y0 + 1;
    x0 = x0 < 0 ? w - 1 : x0; y0 = y0 < 0 ? h - 1 : y0;
    t[0] = d.texels[(uint32_t)y0 * (uint32_t)w + (uint32_t)x0]; t[1] = d.texels[(uint32_t)y0 * (uint32_t)w + (uint32_t)x1];
    t[2] = d.texels[(uint32_t)y1 * (uint32_t)w + (uint32_t)x0]; t[3] = d.texels[(uint32_t)y1 * (uint32_t)w + (uint32_t)x1];
    return hs_weights(fx, fy);
}
// a packed image (common.h TexDesc): 8-byte texels with a one-texel WRAP border, row-major or in tiles of 4 x 4 texels; padded texel (X, Y)
__device__ __forceinline__ uint2 hs_packed_texel(const TexDesc &d, uint32_t X, uint32_t Y) {
    const uint32_t o = d.tile_row_bytes ? (Y >> 2) * d.tile_row_bytes + (X >> 2) * 128u + ((Y & 3u) * 4u + (X & 3u)) * 8u : (Y * d.pitch + X) * 8u;
    return *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(d.texels) + o);
}
__device__ __forceinline__ Weights hs_fetch_packed(const TexDesc &d, float u, float v, uint2 t[4]) {
    int x0, y0;
    float fx, fy;
    hs_axis(u, d.wf, (int)(d.w & ~TEX_INTERLEAVED), x0, fx);
    hs_axis(v, d.hf, (int)d.h, y0, fy);
    const uint32_t X = (uint32_t)(x0 + 1), Y = (uint32_t)(y0 + 1);   // the footprint is padded texels (X .. X + 1, Y .. Y + 1): never a wrap test
    t[0] = hs_packed_texel(d, X, Y); t[1] = hs_packed_texel(d, X + 1u, Y);
    t[2] = hs_packed_texel(d, X, Y + 1u); t[3] = hs_packed_texel(d, X + 1u, Y + 1u);
    return hs_weights(fx, fy);
}
// the eight channels ps_main reads (forward.hlsl:98-124): base colour decoded per texel BEFORE filtering, the normal map's rgb on the 0..255
// scale, roughness and metalness (metal-rough .g, .b) on 0..1
struct Channels { float base[3], nrm[3], rough, metal; };
__device__ __forceinline__ TexDesc load_desc(const TexDesc *__restrict__ tex, uint32_t i) {
    const rq_f4 *p = reinterpret_cast<const rq_f4 *>(tex + i);
    const rq_f4 a = p[0], b = p[1];
    TexDesc d;
    d.texels = reinterpret_cast<const uint32_t *>(((unsigned long long)rq_bits(a[1]) << 32) | rq_bits(a[0]));
    d.w = rq_bits(a[2]); d.h = rq_bits(a[3]); d.wf = b[0]; d.hf = b[1]; d.pitch = rq_bits(b[2]); d.tile_row_bytes = rq_bits(b[3]);
    return d;
}
__device__ __forceinline__ Channels sample_material(const TexDesc *__restrict__ tex, const float *__restrict__ lut, uint32_t mat, float u, float v) {
    Channels c;
    const TexDesc d0 = load_desc(tex, 3u * mat);
    if (d0.w & TEX_INTERLEAVED) {
        uint2 t[4];
        const Weights w = hs_fetch_packed(d0, u, v, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) c.base[k] = hs_filter(w, lut[(t[0].x >> (8 * k)) & 0xFFu], lut[(t[1].x >> (8 * k)) & 0xFFu], lut[(t[2].x >> (8 * k)) & 0xFFu], lut[(t[3].x >> (8 * k)) & 0xFFu]);
        c.nrm[0] = hs_filter(w, hs_byte(t[0].x, 3), hs_byte(t[1].x, 3), hs_byte(t[2].x, 3), hs_byte(t[3].x, 3));
        c.nrm[1] = hs_filter(w, hs_byte(t[0].y, 0), hs_byte(t[1].y, 0), hs_byte(t[2].y, 0), hs_byte(t[3].y, 0));
        c.nrm[2] = hs_filter(w, hs_byte(t[0].y, 1), hs_byte(t[1].y, 1), hs_byte(t[2].y, 1), hs_byte(t[3].y, 1));
        c.rough = hs_filter(w, hs_byte(t[0].y, 2), hs_byte(t[1].y, 2), hs_byte(t[2].y, 2), hs_byte(t[3].y, 2)) * (1.0f / 255.0f);
        c.metal = hs_filter(w, hs_byte(t[0].y, 3), hs_byte(t[1].y, 3), hs_byte(t[2].y, 3), hs_byte(t[3].y, 3)) * (1.0f / 255.0f);
    } else {
        uint32_t t[4];
        Weights w = hs_fetch_plain(d0, u, v, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) c.base[k] = hs_filter(w, lut[(t[0] >> (8 * k)) & 0xFFu], lut[(t[1] >> (8 * k)) & 0xFFu], lut[(t[2] >> (8 * k)) & 0xFFu], lut[(t[3] >> (8 * k)) & 0xFFu]);
        w = hs_fetch_plain(load_desc(tex, 3u * mat + 1u), u, v, t);
#pragma unroll
        for (int k = 0; k < 3; ++k) c.nrm[k] = hs_filter(w, hs_byte(t[0], k), hs_byte(t[1], k), hs_byte(t[2], k), hs_byte(t[3], k));
        w = hs_fetch_plain(load_desc(tex, 3u * mat + 2u), u, v, t);
        c.rough = hs_filter(w, hs_byte(t[0], 1), hs_byte(t[1], 1), hs_byte(t[2], 1), hs_byte(t[3], 1)) * (1.0f / 255.0f);
        c.metal = hs_filter(w, hs_byte(t[0], 2), hs_byte(t[1], 2), hs_byte(t[2], 2), hs_byte(t[3], 2)) * (1.0f / 255.0f);
    }
    return c;
}

// ---- glTF material extras at the same coordinate (common.h MaterialExtra, include/arctic_hip.h next to arctic_set_material_extras; k_shade_hits_ext) ----
// records = the descriptors' end, tex + 3 n_materials: record m is four descriptor slots from records + 4 m.  The twelve constants are three
// 16-byte vector loads per lane; the images are taken at level 0 under the sampler above, in both storage layouts:
//   EXTRA_FAST  one image of 4-byte texels {e.r, e.g, e.b, o} with the packed image's one-texel WRAP border, row-major: the footprint's first
//               texel and weights are hs_fetch_packed's on the same sizes, i.e. the material's own at level 0
//   otherwise   two plain RGBA8 images (hs_fetch_plain), each present when its flag bit is set; occlusion is .r
// An absent image reads as 1.  ao = 1 + strength (o - 1);  emis = e * emissive_factor with e sRGB-decoded per texel before filtering
struct ExtraChannels { float base[3], metal, rough, nscale, ao, emis[3]; };
__device__ __forceinline__ ExtraChannels sample_extras(const TexDesc *__restrict__ records, const float *__restrict__ lut, uint32_t mat, float u, float v) {
    const TexDesc *rec = records + EXTRA_SLOTS * mat;
    const rq_f4 *p = reinterpret_cast<const rq_f4 *>(rec);
    const rq_f4 k0 = p[0], k1 = p[1], k2 = p[2];   // base rgb, metallic | roughness, normal scale, occlusion strength, emissive r | emissive g, b, flags
    const uint32_t flags = rq_bits(k2[2]);
    float e[3] = {1.0f, 1.0f, 1.0f}, occ = 1.0f;
    if (flags & EXTRA_FAST) {
        const TexDesc d = load_desc(rec, 2u);
        int x0, y0;
        float fx, fy;
        hs_axis(u, d.wf, (int)(d.w & ~TEX_INTERLEAVED), x0, fx);
        hs_axis(v, d.hf, (int)d.h, y0, fy);
        const uint32_t o = (uint32_t)(y0 + 1) * d.pitch + (uint32_t)(x0 + 1);   // padded texel (x0 + 1, y0 + 1): never a wrap test
        const uint32_t t[4] = {d.texels[o], d.texels[o + 1u], d.texels[o + d.pitch], d.texels[o + d.pitch + 1u]};
        const Weights w = hs_weights(fx, fy);
        if (flags & EXTRA_EMISSIVE) {
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = hs_filter(w, lut[(t[0] >> (8 * k)) & 0xFFu], lut[(t[1] >> (8 * k)) & 0xFFu], lut[(t[2] >> (8 * k)) & 0xFFu], lut[(t[3] >> (8 * k)) & 0xFFu]);
        }
        if (flags & EXTRA_OCCLUSION) occ = hs_filter(w, hs_byte(t[0], 3), hs_byte(t[1], 3), hs_byte(t[2], 3), hs_byte(t[3], 3)) * (1.0f / 255.0f);
    } else {
        uint32_t t[4];
        if (flags & EXTRA_EMISSIVE) {
            const Weights w = hs_fetch_plain(load_desc(rec, 2u), u, v, t);
#pragma unroll
            for (int k = 0; k < 3; ++k) e[k] = hs_filter(w, lut[(t[0] >> (8 * k)) & 0xFFu], lut[(t[1] >> (8 * k)) & 0xFFu], lut[(t[2] >> (8 * k)) & 0xFFu], lut[(t[3] >> (8 * k)) & 0xFFu]);
        }
        if (flags & EXTRA_OCCLUSION) {
            const Weights w = hs_fetch_plain(load_desc(rec, 3u), u, v, t);
            occ = hs_filter(w, hs_byte(t[0], 0), hs_byte(t[1], 0), hs_byte(t[2], 0), hs_byte(t[3], 0)) * (1.0f / 255.0f);
        }
    }
    ExtraChannels x;
    x.base[0] = k0[0]; x.base[1] = k0[1]; x.base[2] = k0[2];
    x.metal = k0[3]; x.rough = k1[0]; x.nscale = k1[1];
    x.ao = __builtin_fmaf(k1[2], occ - 1.0f, 1.0f);
    x.emis[0] = e[0] * k1[3]; x.emis[1] = e[1] * k2[0]; x.emis[2] = e[2] * k2[1];
    return x;
}

}  // namespace

}  // namespace arctic
