// motion.cpp -- the host side of the motion vectors (include/arctic_hip.h: arctic_motion_vectors_device and the accumulation's motion form): the
// arbiters arctic_motion_pixels and arctic_accumulate_pixels_motion -- the functions of motion.h that motion.hip runs, on the CPU, against inputs
// given as plain arrays.  No HIP type: it also compiles with a host compiler alone (tests/cpp/motion_sanitize.cpp).
#include "motion.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {
namespace {
// the previous history as the caller's four row-major arrays (ao_history.cpp's, which keeps its own)
struct RowFetch {
    const float *value, *count, *world3, *normal3;
    uint32_t width;
    void operator()(uint32_t qx, uint32_t qy, AoHistoryEntry &e) const {
        const size_t q = (size_t)qy * width + qx;
        for (int i = 0; i < 3; ++i) { e.world[i] = world3[3 * q + i]; e.m[i] = normal3[3 * q + i]; }
        e.value = value[q]; e.count = count[q];
    }
};
bool frame_size_ok(uint32_t width, uint32_t height) { return width != 0 && height != 0 && width <= 16384u && height <= 16384u; }
}  // namespace
}  // namespace arctic

extern "C" int arctic_motion_pixels(uint64_t n, const float *bary3, const uint32_t *object, const float *prev_pos9, const int32_t *pixel_xy, const float *prev_trs,
                                    uint64_t n_objects, const float *prev_proj_view, uint32_t width, uint32_t height, float *prev_world4, float *velocity2) {
    using namespace arctic;
    if (!frame_size_ok(width, height)) return ARCTIC_E_INVALID;
    if (n && (!bary3 || !object || !prev_pos9 || !pixel_xy || !prev_world4)) return ARCTIC_E_INVALID;
    if (prev_proj_view && n_objects && !prev_trs) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k) {
        const bool has_prev = prev_proj_view != nullptr && object[k] != MOTION_NO_OBJECT && object[k] < n_objects;
        const float *q = prev_pos9 + 9 * k;
        float pw4[4], vel[2];
        mo_pixel(has_prev, has_prev ? prev_trs + 16 * (size_t)object[k] : nullptr, q, q + 3, q + 6, bary3 + 3 * k, prev_proj_view, width, height, pixel_xy[2 * k],
                 pixel_xy[2 * k + 1], pw4, vel);
        std::memcpy(prev_world4 + 4 * k, pw4, sizeof pw4);
        if (velocity2) std::memcpy(velocity2 + 2 * k, vel, sizeof vel);
    }
    return ARCTIC_OK;
}

extern "C" int arctic_accumulate_pixels_motion(const ArcticAoHistory *hist, uint64_t n, const float *world3, const float *prev_world4, const float *normal3,
                                               const uint8_t *geometry, const uint8_t *cur, const float *prev_proj_view, uint32_t width, uint32_t height,
                                               const float *prev_value, const float *prev_count, const float *prev_world3, const float *prev_normal3, uint8_t *out_u8,
                                               float *out_value, float *out_count, float *out_world3, float *out_normal3) {
    using namespace arctic;
    AoHistoryDesc d;
    if (hist) std::memcpy(&d, hist, sizeof d);
    if (ao_history_refusal(hist ? &d : nullptr)) return ARCTIC_E_INVALID;
    if (!frame_size_ok(width, height)) return ARCTIC_E_INVALID;
    if (prev_proj_view && (!prev_value || !prev_count || !prev_world3 || !prev_normal3)) return ARCTIC_E_INVALID;
    if (n && (!world3 || !prev_world4 || !normal3 || !geometry || !cur || !out_u8)) return ARCTIC_E_INVALID;
    const RowFetch fetch = {prev_value, prev_count, prev_world3, prev_normal3, width};
    for (uint64_t k = 0; k < n; ++k) {
        AoHistoryEntry h;
        out_u8[k] = (uint8_t)aoh_pixel_motion(geometry[k] != 0, normal3 + 3 * k, world3 + 3 * k, prev_world4 + 4 * k, (float)cur[k], prev_proj_view, width, height, d, fetch, h);
        if (out_value) out_value[k] = h.value;
        if (out_count) out_count[k] = h.count;
        for (int i = 0; i < 3; ++i) {
            if (out_world3) out_world3[3 * k + i] = h.world[i];
            if (out_normal3) out_normal3[3 * k + i] = h.m[i];
        }
    }
    return ARCTIC_OK;
}
