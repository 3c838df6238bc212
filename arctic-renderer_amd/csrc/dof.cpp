// dof.cpp -- the host side of depth of field (include/arctic_hip.h: arctic_dof_device): what the entry points refuse before a device is
// touched, the arbiters arctic_dof_prepare and arctic_dof_pixels -- the functions of dof.h that dof.hip runs, on the CPU -- and the thin-lens
// helper arctic_dof_coc_scale.  No HIP type: it also compiles with a host compiler alone (tests/cpp/dof_sanitize.cpp).
#include "dof.h"
#include "../../include/arctic_hip.h"

#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticDof) == 32 && sizeof(DofDesc) == 32, "ArcticDof");
static_assert(offsetof(ArcticDof, focus_distance) == offsetof(DofDesc, focus_distance) && offsetof(ArcticDof, coc_scale) == offsetof(DofDesc, coc_scale) &&
              offsetof(ArcticDof, max_radius) == offsetof(DofDesc, max_radius) && offsetof(ArcticDof, samples) == offsetof(DofDesc, samples) &&
              offsetof(ArcticDof, depth_extent) == offsetof(DofDesc, depth_extent) && offsetof(ArcticDof, z_near) == offsetof(DofDesc, z_near) &&
              offsetof(ArcticDof, z_far) == offsetof(DofDesc, z_far), "the public record is the internal one");
static_assert(ARCTIC_DOF_SOURCE_COMPOSED == DOF_SOURCE_COMPOSED && ARCTIC_DOF_SOURCE_TAA == DOF_SOURCE_TAA && ARCTIC_DOF_SOURCE_MOTION_BLUR == DOF_SOURCE_MOTION_BLUR, "the flags");

const char *dof_refusal(const DofDesc *d, bool zero_planes) {
    if (!d) return "null parameters";
    if (d->flags & ~(DOF_SOURCE_COMPOSED | DOF_SOURCE_TAA | DOF_SOURCE_MOTION_BLUR)) return "flags have unknown bits";
    if (d->flags & (d->flags - 1u)) return "the ARCTIC_DOF_SOURCE_* flags exclude each other";
    if (!(d->focus_distance > 0.0f && rq_finite(d->focus_distance))) return "focus_distance not finite and above 0";   // (a NaN fails every comparison)
    if (!(d->coc_scale >= 0.0f && d->coc_scale <= 4096.0f)) return "coc_scale outside [0, 4096]";
    if (!(d->max_radius >= 1.0f && d->max_radius <= 64.0f)) return "max_radius outside [1, 64]";
    if (!(d->samples >= 1u && d->samples <= DOF_MAX_SAMPLES)) return "samples outside 1..64";
    if (!(d->depth_extent > 0.0f && rq_finite(d->depth_extent))) return "depth_extent not finite and above 0";
    if (zero_planes) {
        if (!(d->z_near == 0.0f && d->z_far == 0.0f)) return "z_near and z_far must be 0: the one call takes the scene's camera planes";
    } else {
        if (!(d->z_near > 0.0f)) return "z_near not above 0";
        if (!(d->z_far > d->z_near && rq_finite(d->z_far))) return "z_far not finite and above z_near";
    }
    return nullptr;
}

const char *dof_taps_refusal(const DofDesc *d, const float *taps2) {
    if (!taps2) return "null taps2";
    for (uint32_t i = 0; i < d->samples; ++i) {
        const float x = taps2[2 * i], y = taps2[2 * i + 1];
        if (!(rq_finite(x) && rq_finite(y))) return "a tap is not finite";
        if (!(x * x + y * y <= 1.0f)) return "a tap lies outside the unit disc";
    }
    return nullptr;
}

float dof_view_distance_host(float z_near, float z_far, float depth) { return dof_view_distance(z_near, z_far, depth); }

}  // namespace arctic

extern "C" int arctic_dof_prepare(const ArcticDof *dof, uint32_t width, uint32_t height, const float *depth, float *tile_max, float *neighbour_max, float *prepared2) {
    using namespace arctic;
    DofDesc d;
    if (dof) std::memcpy(&d, dof, sizeof d);
    if (dof_refusal(dof ? &d : nullptr, false)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (!depth || !tile_max || !neighbour_max || !prepared2) return ARCTIC_E_INVALID;
    const uint32_t tiles_x = (width + DOF_TILE - 1) / DOF_TILE, tiles_y = (height + DOF_TILE - 1) / DOF_TILE;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t o = (size_t)y * width + x;
            float s, zv;
            dof_signed_radius(d, depth[o], s, zv);
            prepared2[2 * o] = s; prepared2[2 * o + 1] = zv;
        }
    const auto radius = [&](uint32_t x, uint32_t y) { return __builtin_fabsf(prepared2[2 * ((size_t)y * width + x)]); };
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) tile_max[(size_t)ty * tiles_x + tx] = dof_tile_max(tx, ty, width, height, radius);
    const auto tile = [&](uint32_t tx, uint32_t ty) { return tile_max[(size_t)ty * tiles_x + tx]; };
    for (uint32_t ty = 0; ty < tiles_y; ++ty)
        for (uint32_t tx = 0; tx < tiles_x; ++tx) neighbour_max[(size_t)ty * tiles_x + tx] = dof_neighbour_max(tx, ty, tiles_x, tiles_y, dof_window(d), tile);
    return ARCTIC_OK;
}

extern "C" int arctic_dof_pixels(const ArcticDof *dof, const float *taps2, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height, const float *rgb,
                                 const float *prepared2, const float *neighbour_max, float *out_rgb) {
    using namespace arctic;
    DofDesc d;
    if (dof) std::memcpy(&d, dof, sizeof d);
    if (dof_refusal(dof ? &d : nullptr, false) || dof_taps_refusal(&d, taps2)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u) return ARCTIC_E_INVALID;
    if (n && (!pixel_xy || !rgb || !prepared2 || !neighbour_max || !out_rgb)) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= width || (uint32_t)pixel_xy[2 * k + 1] >= height) return ARCTIC_E_INVALID;
    const uint32_t tiles_x = (width + DOF_TILE - 1) / DOF_TILE;
    const auto color = [&](uint32_t qx, uint32_t qy, float *c) {
        const float *s = rgb + ((size_t)qy * width + qx) * 3;
        c[0] = s[0]; c[1] = s[1]; c[2] = s[2];
    };
    const auto prep = [&](uint32_t qx, uint32_t qy, float &s, float &z) {
        const float *e = prepared2 + ((size_t)qy * width + qx) * 2;
        s = e[0]; z = e[1];
    };
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t px = (uint32_t)pixel_xy[2 * k], py = (uint32_t)pixel_xy[2 * k + 1];
        dof_pixel(px, py, width, height, d, neighbour_max[(size_t)(py / DOF_TILE) * tiles_x + px / DOF_TILE], taps2, color, prep, out_rgb + 3 * k);
    }
    return ARCTIC_OK;
}

extern "C" int arctic_dof_coc_scale(float f_number, float focal_length_mm, float sensor_height_mm, float focus_distance, uint32_t height_px, float *out) {
    using namespace arctic;
    if (!out) return ARCTIC_E_INVALID;
    if (!(f_number > 0.0f && rq_finite(f_number)) || !(focal_length_mm > 0.0f && rq_finite(focal_length_mm)) || !(sensor_height_mm > 0.0f && rq_finite(sensor_height_mm)))
        return ARCTIC_E_INVALID;
    if (height_px == 0 || height_px > 16384u) return ARCTIC_E_INVALID;
    const float fl = focal_length_mm * 0.001f;
    if (!(focus_distance > fl && rq_finite(focus_distance))) return ARCTIC_E_INVALID;   // (a lens focuses no nearer than its focal length)
    const float c = (fl * fl) / (f_number * (focus_distance - fl));
    const float scale = ((0.5f * c) / (sensor_height_mm * 0.001f)) * (float)height_px;
    if (!rq_finite(scale)) return ARCTIC_E_INVALID;
    *out = scale;
    return ARCTIC_OK;
}
