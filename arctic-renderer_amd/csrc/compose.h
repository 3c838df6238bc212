// compose.h -- ray-traced occlusion and reflections folded into the shaded frame (include/arctic_hip.h: arctic_compose_planes_device and the text in
// front of it, which is the definition; nothing here restates it, it only carries it out).  ONE copy of the two terms, compiled for the host
// (compose.cpp: the arbiter arctic_compose_pixels) and for the device (compose.hip: k_compose), both with contraction off.  Plain C++ like ray_ao.h,
// whose normalisation (ao_normal: step 1 of the ambient occlusion) it uses unchanged.
#pragma once
#include "ray_ao.h"

namespace arctic {

// == ArcticRayCompose (static_assert in compose.cpp)
struct ComposeDesc { uint32_t flags; float ao_strength, reflection_strength, reflection_bias; uint32_t reserved[4]; };
constexpr uint32_t COMPOSE_AO = 1u, COMPOSE_REFLECTIONS = 2u;   // ARCTIC_COMPOSE_*

RQ_HD float compose_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the occlusion: ps_main's ambient term scaled by ka, as a correction of the colour that already holds it.  ao = 255 or ao_strength = 0: k is +0
RQ_HD void compose_occlusion(float *C, const float *base, float ambient, float ao_strength, uint32_t ao) {
    const float vis = (float)ao / 255.0f;
    const float ka = 1.0f - ao_strength * (1.0f - vis);
    const float k = ka - 1.0f;
    for (int i = 0; i < 3; ++i) C[i] = C[i] + (ambient * base[i]) * k;
}

// is there a reflection to add at all?  (a select: where this is false nothing of the normal or of refl.rgb is looked at; a NaN refl.a is false)
RQ_HD bool compose_reflects(uint32_t flags, float refl_a) { return (flags & COMPOSE_REFLECTIONS) != 0u && refl_a > 0.0f; }

// the reflection of a pixel the occlusion's step 1 covers: m = its unit normal (ao_normal), refl = {rgb, a} with a > 0
RQ_HD void compose_reflection(float *C, const float *base, float metal, float rough, const float *m, const float *world, const float *eye, const float *refl,
                              float reflection_strength) {
    const float d[3] = {eye[0] - world[0], eye[1] - world[1], eye[2] - world[2]};
    const float len = __builtin_sqrtf(compose_dot(d, d));
    const float wo[3] = {d[0] / len, d[1] / len, d[2] / len};
    const float c = rq_max(compose_dot(m, wo), 0.0f);
    const float p = 1.0f - c, p2 = p * p, p5 = (p2 * p2) * p;
    const float q = 1.0f - rough, g = q * q;
    const float s = (reflection_strength * refl[3]) * g;
    for (int i = 0; i < 3; ++i) {
        const float F0 = 0.04f + (base[i] - 0.04f) * metal;
        const float F = F0 + (1.0f - F0) * p5;
        C[i] = C[i] + (s * F) * refl[i];
    }
}

// ---- host side (compose.cpp) -----------------------------------------------------------------------------------------------------------------------
// what the entry points refuse with ARCTIC_E_INVALID, in the header's order: null = nothing; else the reason.  First the block, then the planes
// its flags need (any memory space: only the addresses are looked at; refl_align: the alignment the float plane needs, 16 on the device, 4 in
// the arbiter, which asks only when it has a pixel)
const char *compose_refusal(const ComposeDesc *d);
const char *compose_plane_refusal(const ComposeDesc &d, const void *ao, const void *refl, unsigned refl_align);

#if defined(__HIPCC__)
struct TexDesc;
// compose.hip.  What k_compose reads and writes: G-buffer planes a, b, c, e (common.h) of tiles_x x tiles_y tiles -- the handle's rows x width pixels
// start at row row0_in_tile of the first tile row --, the material table, and the row-major planes of those rows x width pixels: hdr (3 floats),
// ao (a byte; null without COMPOSE_AO), refl (4 floats, 16-byte aligned; null without COMPOSE_REFLECTIONS) in; RGBA8, float LDR and the composed
// HDR (3 floats each) out.  No plane may alias another.
struct ComposeParams {
    const void *plane_a; const float *plane_b; const void *plane_c, *plane_e;
    const TexDesc *tex; const float *srgb_lut;
    const float *hdr; const uint8_t *ao; const void *refl;
    uint32_t *out_rgba8; float *out_ldr, *out_hdr;
    uint32_t tiles_x, tiles_y, width, rows, row0_in_tile, n_materials, flags;
    int32_t tm;
    float ao_strength, reflection_strength, ambient, eye[3], inv_gamma, exposure;
};
// enqueues on `s` and returns the launch error, never synchronises
hipError_t launch_compose(const ComposeParams &p, hipStream_t s);
#endif

}  // namespace arctic
