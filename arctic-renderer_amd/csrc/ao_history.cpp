// ao_history.cpp -- the host side of the temporal accumulation (include/arctic_hip.h: arctic_accumulate_ambient_occlusion_device): what the entry
// points refuse before a device is touched, and the arbiter arctic_accumulate_pixels -- the functions of ao_history.h that ao_history.hip runs, on
// the CPU, against a previous history given as row-major arrays.  No HIP type: it also compiles with a host compiler alone
// (tests/cpp/ao_history_sanitize.cpp).
#include "ao_history.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticAoHistory) == 32 && sizeof(AoHistoryDesc) == 32, "ArcticAoHistory");
static_assert(offsetof(ArcticAoHistory, max_history) == offsetof(AoHistoryDesc, max_history) && offsetof(ArcticAoHistory, normal_cos) == offsetof(AoHistoryDesc, normal_cos) &&
              offsetof(ArcticAoHistory, plane_dist) == offsetof(AoHistoryDesc, plane_dist) && offsetof(ArcticAoHistory, min_weight) == offsetof(AoHistoryDesc, min_weight) &&
              offsetof(ArcticAoHistory, reserved) == offsetof(AoHistoryDesc, reserved), "the public record is the internal one");

const char *ao_history_refusal(const AoHistoryDesc *d) {
    if (!d) return "null parameters";
    if (!(d->max_history >= 1.0f && d->max_history <= 65536.0f)) return "max_history outside [1, 65536]";
    if (!rq_finite(d->normal_cos)) return "normal_cos is not finite";
    if (!(d->plane_dist >= 0.0f)) return "plane_dist is negative or a NaN";
    if (!(d->min_weight >= 0.0f && d->min_weight < 1.0f)) return "min_weight outside [0, 1)";
    if (d->reserved[0] | d->reserved[1] | d->reserved[2] | d->reserved[3]) return "reserved not 0";
    return nullptr;
}

namespace {
// the previous history as the caller's four row-major arrays
struct RowFetch {
    const float *value, *count, *world3, *normal3;
    uint32_t width;
    void operator()(uint32_t qx, uint32_t qy, AoHistoryEntry &e) const {
        const size_t q = (size_t)qy * width + qx;
        for (int i = 0; i < 3; ++i) { e.world[i] = world3[3 * q + i]; e.m[i] = normal3[3 * q + i]; }
        e.value = value[q]; e.count = count[q];
    }
};
}  // namespace

}  // namespace arctic

extern "C" int arctic_accumulate_pixels(const ArcticAoHistory *hist, uint64_t n, const float *world3, const float *normal3, const uint8_t *geometry, const uint8_t *cur,
                                        const float *prev_proj_view, uint32_t width, uint32_t height, const float *prev_value, const float *prev_count,
                                        const float *prev_world3, const float *prev_normal3, uint8_t *out_u8, float *out_value, float *out_count, float *out_world3,
                                        float *out_normal3) {
    using namespace arctic;
    AoHistoryDesc d;
    if (hist) std::memcpy(&d, hist, sizeof d);
    if (ao_history_refusal(hist ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (prev_proj_view && (!prev_value || !prev_count || !prev_world3 || !prev_normal3)) return ARCTIC_E_INVALID;
    if (n && (!world3 || !normal3 || !geometry || !cur || !out_u8)) return ARCTIC_E_INVALID;
    const RowFetch fetch = {prev_value, prev_count, prev_world3, prev_normal3, width};
    for (uint64_t k = 0; k < n; ++k) {
        AoHistoryEntry h;
        out_u8[k] = (uint8_t)aoh_pixel(geometry[k] != 0, normal3 + 3 * k, world3 + 3 * k, (float)cur[k], prev_proj_view, width, height, d, fetch, h);
        if (out_value) out_value[k] = h.value;
        if (out_count) out_count[k] = h.count;
        for (int i = 0; i < 3; ++i) {
            if (out_world3) out_world3[3 * k + i] = h.world[i];
            if (out_normal3) out_normal3[3 * k + i] = h.m[i];
        }
    }
    return ARCTIC_OK;
}
