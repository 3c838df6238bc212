// compose.cpp -- the host side of the composition (include/arctic_hip.h: arctic_compose_planes_device): what the entry points refuse before a
// device is touched, and the arbiter arctic_compose_pixels -- the functions of compose.h that compose.hip runs, on the CPU, on channels the caller
// has sampled already.  No HIP type: it also compiles with a host compiler alone (tests/cpp/compose_sanitize.cpp).
#include "compose.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticRayCompose) == 32 && sizeof(ComposeDesc) == 32, "ArcticRayCompose");
static_assert(offsetof(ArcticRayCompose, ao_strength) == offsetof(ComposeDesc, ao_strength) && offsetof(ArcticRayCompose, reflection_strength) == offsetof(ComposeDesc, reflection_strength) &&
              offsetof(ArcticRayCompose, reflection_bias) == offsetof(ComposeDesc, reflection_bias) && offsetof(ArcticRayCompose, reserved) == offsetof(ComposeDesc, reserved), "the public record is the internal one");
static_assert(ARCTIC_COMPOSE_AO == COMPOSE_AO && ARCTIC_COMPOSE_REFLECTIONS == COMPOSE_REFLECTIONS, "the flags");

const char *compose_refusal(const ComposeDesc *d) {
    if (!d) return "null parameters";
    if (d->flags == 0u || (d->flags & ~(COMPOSE_AO | COMPOSE_REFLECTIONS))) return "flags are 0 or have unknown bits";
    if (!(d->ao_strength >= 0.0f && d->ao_strength <= 1.0f)) return "ao_strength outside [0, 1]";
    if (!(d->reflection_strength >= 0.0f) || !rq_finite(d->reflection_strength)) return "reflection_strength is negative or not finite";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3]) return "reserved not 0";
    return nullptr;
}

const char *compose_plane_refusal(const ComposeDesc &f, const void *ao, const void *refl, unsigned refl_align) {
    const ComposeDesc *d = &f;
    if ((d->flags & COMPOSE_AO) && !ao) return "the occlusion plane is null";
    if ((d->flags & COMPOSE_REFLECTIONS) && (!refl || ((uintptr_t)refl & (uintptr_t)(refl_align - 1u)))) return "the reflection plane is null or misaligned";
    return nullptr;
}

}  // namespace arctic

extern "C" int arctic_compose_pixels(const ArcticRayCompose *compose, const float *eye3, float ambient, uint64_t n, const float *hdr3, const float *base3,
                                     const float *metal, const float *rough, const float *normal3, const float *world3, const uint8_t *ao, const float *refl4,
                                     const uint8_t *geometry, float *out_hdr3) {
    using namespace arctic;
    ComposeDesc d;
    if (compose) std::memcpy(&d, compose, sizeof d);
    if (compose_refusal(compose ? &d : nullptr) || !eye3) return ARCTIC_E_INVALID;
    if (n && (compose_plane_refusal(d, ao, refl4, 4u) || !hdr3 || !base3 || !metal || !rough || !normal3 || !world3 || !geometry || !out_hdr3)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k) {
        float C[3] = {hdr3[3 * k], hdr3[3 * k + 1], hdr3[3 * k + 2]};
        if (geometry[k]) {
            if (d.flags & COMPOSE_AO) compose_occlusion(C, base3 + 3 * k, ambient, d.ao_strength, ao[k]);
            float m[3];
            if (compose_reflects(d.flags, (d.flags & COMPOSE_REFLECTIONS) ? refl4[4 * k + 3] : 0.0f) && ao_normal(normal3[3 * k], normal3[3 * k + 1], normal3[3 * k + 2], m))
                compose_reflection(C, base3 + 3 * k, metal[k], rough[k], m, world3 + 3 * k, eye3, refl4 + 4 * k, d.reflection_strength);
        }
        out_hdr3[3 * k] = C[0]; out_hdr3[3 * k + 1] = C[1]; out_hdr3[3 * k + 2] = C[2];
    }
    return ARCTIC_OK;
}
