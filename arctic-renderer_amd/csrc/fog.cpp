// fog.cpp -- the host side of volumetric fog (include/arctic_hip.h: arctic_fog_device): what the entry points refuse before a device is
// touched, the arbiter arctic_fog_pixels -- the functions of fog.h that fog.hip runs, on the CPU -- and the binary64 construction of the view
// record behind arctic_fog_view.  No HIP type: it also compiles with a host compiler alone (tests/cpp/fog_sanitize.cpp).
#include "fog.h"
#include "../../include/arctic_hip.h"

#include <cmath>
#include <cstring>

namespace arctic {

static_assert(sizeof(ArcticFog) == 52 && sizeof(FogDesc) == 52, "ArcticFog");
static_assert(sizeof(ArcticFogView) == 128 && sizeof(FogView) == 128, "ArcticFogView");
static_assert(offsetof(ArcticFog, density) == offsetof(FogDesc, density) && offsetof(ArcticFog, anisotropy) == offsetof(FogDesc, anisotropy) &&
              offsetof(ArcticFog, max_distance) == offsetof(FogDesc, max_distance) && offsetof(ArcticFog, steps) == offsetof(FogDesc, steps) &&
              offsetof(ArcticFog, bias) == offsetof(FogDesc, bias) && offsetof(ArcticFog, scatter_color) == offsetof(FogDesc, scatter_color) &&
              offsetof(ArcticFog, ambient_color) == offsetof(FogDesc, ambient_color) && offsetof(ArcticFog, reserved) == offsetof(FogDesc, reserved),
              "the public record is the internal one");
static_assert(offsetof(ArcticFogView, z_near) == offsetof(FogView, z_near) && offsetof(ArcticFogView, ray00) == offsetof(FogView, ray00) &&
              offsetof(ArcticFogView, z_far) == offsetof(FogView, z_far) && offsetof(ArcticFogView, ray_dx) == offsetof(FogView, ray_dx) &&
              offsetof(ArcticFogView, ray_dy) == offsetof(FogView, ray_dy) && offsetof(ArcticFogView, sun_dir) == offsetof(FogView, sun_dir) &&
              offsetof(ArcticFogView, pad2) == offsetof(FogView, pad2) && offsetof(ArcticFogView, light) == offsetof(FogView, light) && offsetof(FogView, light) == 80,
              "the public view record is the internal one");
static_assert(ARCTIC_FOG_SOURCE_COMPOSED == FOG_SOURCE_COMPOSED, "the flags");

const char *fog_refusal(const FogDesc *d) {
    if (!d) return "null parameters";
    if (d->flags & ~FOG_SOURCE_COMPOSED) return "flags have unknown bits";
    if (!(d->density >= 0.0f && d->density <= 64.0f)) return "density outside [0, 64]";   // (a NaN fails every comparison)
    if (!(d->anisotropy >= -0.95f && d->anisotropy <= 0.95f)) return "anisotropy outside [-0.95, 0.95]";
    if (!(d->max_distance > 0.0f && d->max_distance <= 65504.0f)) return "max_distance outside (0, 65504]";
    if (!(d->steps >= 1u && d->steps <= FOG_MAX_STEPS)) return "steps outside 1..128";
    if (!(d->bias >= 0.0f && d->bias <= 1.0f)) return "bias outside [0, 1]";
    for (int c = 0; c < 3; ++c)
        if (!(d->scatter_color[c] >= 0.0f && d->scatter_color[c] <= 65504.0f)) return "scatter_color outside [0, 65504]";
    for (int c = 0; c < 3; ++c)
        if (!(d->ambient_color[c] >= 0.0f && d->ambient_color[c] <= 65504.0f)) return "ambient_color outside [0, 65504]";
    if (d->reserved != 0u) return "reserved != 0";
    return nullptr;
}

const char *fog_view_refusal(const FogView *v) {
    if (!v) return "null view";
    if (rq_bits(v->pad0) | rq_bits(v->pad1) | rq_bits(v->pad2)) return "a pad of the view record is not 0";
    const float *f = reinterpret_cast<const float *>(v);
    for (size_t i = 0; i < sizeof(FogView) / sizeof(float); ++i)
        if (!rq_finite(f[i])) return "a field of the view record is not finite";
    if (!(v->z_near > 0.0f && v->z_near < v->z_far)) return "the view record's z_near is not above 0 and below z_far";
    return nullptr;
}

const char *fog_offsets_refusal(const float *offsets16) {
    if (!offsets16) return nullptr;
    for (uint32_t i = 0; i < FOG_OFFSETS; ++i)
        if (!(offsets16[i] >= 0.0f && offsets16[i] < 1.0f)) return "an offset lies outside [0, 1)";
    return nullptr;
}

namespace {
inline double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline void cross3(const double *x, const double *y, double *o) {
    o[0] = x[1] * y[2] - y[1] * x[2];
    o[1] = x[2] * y[0] - y[2] * x[0];
    o[2] = x[0] * y[1] - y[0] * x[1];
}
inline void normalize3(double *v) {
    const double inv = 1.0 / std::sqrt(dot3(v, v));
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}
// lookAtRH(eye, eye + fwd, +Y): the rows s, u and the unit forward f
inline void basis(const float *fwd, double *s, double *u, double *f) {
    const double up[3] = {0.0, 1.0, 0.0};
    for (int a = 0; a < 3; ++a) f[a] = (double)fwd[a];
    normalize3(f);
    cross3(f, up, s);
    normalize3(s);
    cross3(s, f, u);
}
}  // namespace

void fog_view_build(const float *fwd_cam, const float *fwd_sun, const float *eye, float aspect, float fov_y, float z_near, float z_far, const float *sun_pos, uint32_t width,
                    uint32_t height, FogView *out) {
    FogView v = {};
    double s[3], u[3], f[3];
    basis(fwd_cam, s, u, f);
    const double t = std::tan((double)fov_y * 0.01745329251994329576923690768489 / 2.0), ta = t * (double)aspect;
    for (int a = 0; a < 3; ++a) {
        v.eye[a] = eye[a];
        // D = f + x_ndc * aspect * t * s + y_ndc * t * u with x_ndc = 2 fx / W - 1 and y_ndc = 1 - 2 fy / H
        v.ray00[a] = (float)(f[a] - ta * s[a] + t * u[a]);
        v.ray_dx[a] = (float)((2.0 / (double)width) * ta * s[a]);
        v.ray_dy[a] = (float)(-(2.0 / (double)height) * t * u[a]);
    }
    v.z_near = z_near; v.z_far = z_far;
    // the sun: orthoRH_ZO(-16, 16, -16, 16, 0.1, 50) * lookAtRH(pos, pos + dir, +Y), as sun_proj_view
    double ls[3], lu[3], lf[3];
    basis(fwd_sun, ls, lu, lf);
    const double pos[3] = {(double)sun_pos[0], (double)sun_pos[1], (double)sun_pos[2]};
    const double zn = (double)0.1f, zf = 50.0, sx = 2.0 / 32.0, sy = 2.0 / 32.0, sz = -1.0 / (zf - zn), oz = -zn / (zf - zn);
    // view rows: x = s . (P - pos), y = u . (P - pos), z = -f . (P - pos); clip = {sx x, sy y, sz z + oz}
    for (int a = 0; a < 3; ++a) {
        v.sun_dir[a] = (float)lf[a];
        v.light[0][a] = (float)(0.5 * sx * ls[a]);
        v.light[1][a] = (float)(-0.5 * sy * lu[a]);
        v.light[2][a] = (float)(sz * -lf[a]);
    }
    v.light[0][3] = (float)(0.5 * sx * -dot3(ls, pos) + 0.5);
    v.light[1][3] = (float)(0.5 - 0.5 * sy * -dot3(lu, pos));
    v.light[2][3] = (float)(sz * dot3(lf, pos) + oz);
    *out = v;
}

}  // namespace arctic

extern "C" int arctic_fog_pixels(const ArcticFog *fog, const ArcticFogView *view, const float *offsets16, uint64_t n, const int32_t *pixel_xy, uint32_t width, uint32_t height,
                                 const float *rgb, const float *depth, const float *shadow, uint32_t S, float *out_rgb, float *terms2) {
    using namespace arctic;
    if (!fog || !view) return ARCTIC_E_INVALID;
    FogDesc d;
    FogView v;
    std::memcpy(&d, fog, sizeof d);
    std::memcpy(&v, view, sizeof v);
    if (fog_refusal(&d) || fog_view_refusal(&v) || fog_offsets_refusal(offsets16)) return ARCTIC_E_INVALID;
    if (width == 0 || height == 0 || width > 16384u || height > 16384u || S > 16384u) return ARCTIC_E_INVALID;
    if ((S && !shadow) || (n && (!pixel_xy || !rgb || !out_rgb))) return ARCTIC_E_INVALID;
    for (uint64_t k = 0; k < n; ++k)   // (every pixel is inside the frame before anything is written)
        if (pixel_xy[2 * k] < 0 || pixel_xy[2 * k + 1] < 0 || (uint32_t)pixel_xy[2 * k] >= width || (uint32_t)pixel_xy[2 * k + 1] >= height) return ARCTIC_E_INVALID;
    const auto map = [&](uint32_t tu, uint32_t tv) { return shadow[(size_t)tv * S + tu]; };
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t px = (uint32_t)pixel_xy[2 * k], py = (uint32_t)pixel_xy[2 * k + 1];
        const size_t o = (size_t)py * width + px;
        const float offset = offsets16 ? offsets16[fog_offset_index(px, py)] : 0.5f;
        fog_pixel(px, py, d, v, offset, rgb + o * 3, depth ? depth[o] : 1.0f, S, map, out_rgb + 3 * k, terms2 ? terms2 + 2 * k : nullptr);
    }
    return ARCTIC_OK;
}

extern "C" float arctic_fog_exp2(float x) { return arctic::fog_exp2(x); }

extern "C" int arctic_fog_exp2_poly(uint64_t n, const float *f, float *p) {
    if (n && (!f || !p)) return ARCTIC_E_INVALID;
    for (uint64_t i = 0; i < n; ++i) p[i] = arctic::fog_exp2_poly(f[i]);
    return ARCTIC_OK;
}
