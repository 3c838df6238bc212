// dof_calls.cpp -- the depth of field's calls of the C-ABI (include/arctic_hip.h: arctic_dof_device and the definition in front of it,
// arctic_dof_focus_at; the arithmetic: dof.h; the kernels: dof.hip; the arbiters, the taps and the view distance: dof.cpp).  Of the handle
// (renderer_state.h) it owns ArcticRenderer::Dof and reads the visibility plane (the depth, through the motion blur's mb_depth_plane, and the one
// pixel of arctic_dof_focus_at), and through post_source.cpp the float HDR plane of the latest shading or composition, the anti-aliasing's
// history or the motion blur's output.  Enqueues on r->stream only.
#include <cstdint>
#include <cstring>

#include "renderer_state.h"
#include "dof.h"

extern "C" {

namespace {
// what the calls refuse with ARCTIC_E_INVALID, in the header's order; color, depth, out: the planes the kernels will read and write (null colour,
// output: the handle's own); align: whether they are device planes, whose alignment the loads and stores need; zero_planes: arctic_pass_dof's block
int dof_checks(ArcticRenderer *r, const ArcticSettings *st, const ArcticDof *dof, const void *color, const void *depth, const float *taps2, const void *out, bool align,
               bool zero_planes, DofDesc &d, const char *who) {
    if (!st || !dof) return r->fail(ARCTIC_E_INVALID, "%s: null settings or parameters", who);
    std::memcpy(&d, dof, sizeof d);
    if (const char *why = dof_refusal(&d, zero_planes)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (!depth) return r->fail(ARCTIC_E_INVALID, "%s: null depth", who);
    if (const char *why = dof_taps_refusal(&d, taps2)) return r->fail(ARCTIC_E_INVALID, "%s: %s", who, why);
    if (align && (((uintptr_t)color | (uintptr_t)depth | (uintptr_t)out) & 3u))
        return r->fail(ARCTIC_E_INVALID, "%s: the colour plane, the depth and the output must be 4-byte aligned", who);
    return ARCTIC_OK;
}
// which plane a NULL colour means under the record's flags, and the public name of the flag that says so.  (The history and the composition are
// refused under the motion blur's and the anti-aliasing's names: this stage used to ask those stages' functions, and the texts are part of the
// ABI now)
SourceFlag dof_source(uint32_t flags) {
    if (flags & DOF_SOURCE_MOTION_BLUR) return {HdrSource::MotionBlur, "ARCTIC_DOF_SOURCE_MOTION_BLUR"};
    if (flags & DOF_SOURCE_TAA) return {HdrSource::Taa, "ARCTIC_MB_SOURCE_TAA"};
    return {(flags & DOF_SOURCE_COMPOSED) ? HdrSource::Composed : HdrSource::Shaded, "ARCTIC_TAA_SOURCE_COMPOSED"};
}
// ... and with ARCTIC_E_STATE: no side effect.  own_color: the colour plane is the handle's (d.flags says which)
int dof_states(ArcticRenderer *r, const DofDesc &d, bool own_color, const char *who) {
    if (r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "%s: the gather's taps need the whole frame, this handle owns %u of %u rows (its neighbours' rows are on other shards)", who, r->rows(), r->height);
    return own_color ? source_refusal(r, dof_source(d.flags), who) : ARCTIC_OK;
}
// the handle's buffers, the tap table and the three launches: device pointers throughout but taps2.  d_color: null = the handle's own plane, per
// d.flags; d_out: the caller's RGBA8, or null = the handle's own.  The handle's state moves only behind launches that were enqueued
int dof_planes(ArcticRenderer *r, const ArcticSettings *st, const DofDesc &d, const float *d_color, const float *d_depth, const float *taps2, uint8_t *d_out) {
    ArcticRenderer::Dof &D = r->dof;
    const uint64_t n = std::max<uint64_t>((uint64_t)r->rows() * r->width, 1), tiles = std::max<uint64_t>(r->n_tiles(), 1);
    const size_t table_bytes = DOF_MAX_SAMPLES * 2 * sizeof(float);   // the largest table: the slot and d_taps are made once
    HIPCHECK(r, D.d_prep.ensure(n * 8));
    HIPCHECK(r, D.d_tile.ensure(tiles * 4));
    HIPCHECK(r, D.d_neighbour.ensure(tiles * 4));
    HIPCHECK(r, D.d_hdr.ensure(n * 12));
    if (!d_out) HIPCHECK(r, D.d_rgba8.ensure(n * 4));
    HIPCHECK(r, D.d_ldr.ensure(n * 12));
    HIPCHECK(r, D.d_taps.ensure(table_bytes));
    HIPCHECK(r, D.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, D.written.wait(r->stream));   // (recorded on another stream: arctic_set_stream came in between; on this one: stream order does it)
    if (D.n_taps != d.samples || std::memcmp(D.taps_ring.slot[0].h.p, taps2, (size_t)d.samples * 8) != 0) {   // (n_taps != 0: an empty D holds no table)
        float *h_taps = nullptr;
        HIPCHECK(r, D.taps_ring.stage(table_bytes, &h_taps));
        D.n_taps = 0;
        std::memcpy(h_taps, taps2, (size_t)d.samples * 8);
        HIPCHECK(r, D.taps_ring.send(D.d_taps.p, (size_t)d.samples * 8, r->stream));
        D.n_taps = d.samples;
    }
    SourcePlane source = {d_color, false};
    if (!d_color) { if (int rc = source_plane(r, dof_source(d.flags).source, source)) return rc; }
    DofParams p = {};
    p.color = source.color; p.color_taa = source.color_taa;
    p.depth = d_depth; p.taps = D.d_taps.as<float>();
    p.prep = D.d_prep.p; p.tile_max = D.d_tile.as<float>(); p.neighbour_max = D.d_neighbour.as<float>();
    p.out_hdr = D.d_hdr.as<float>(); p.out_rgba8 = reinterpret_cast<uint32_t *>(d_out ? d_out : D.d_rgba8.as<uint8_t>()); p.out_ldr = D.d_ldr.as<float>();
    p.tiles_x = r->tiles_x; p.tiles_y = r->tiles_y; p.width = r->width; p.rows = r->rows();
    p.tm = st->tm_method; p.inv_gamma = 1.0f / st->gamma; p.exposure = st->exposure;
    p.d = d;
    D.valid = false;   // (until all three are enqueued: a failure between leaves nothing to read, never half this call's)
    HIPCHECK(r, launch_dof_prepare(p, r->stream));
    HIPCHECK(r, launch_dof_neighbour_max(p, r->stream));
    HIPCHECK(r, launch_dof_gather(p, r->stream));
    HIPCHECK(r, D.written.record(r->stream));
    D.valid = true; D.width = r->width; D.height = r->height; D.own_rgba8 = d_out == nullptr;
    ++D.launches; ++D.calls;
    return ARCTIC_OK;
}
}  // namespace

int arctic_dof_device(ArcticRenderer *r, const ArcticSettings *settings, const ArcticDof *dof, const float *d_hdr_rgb32f, const float *d_depth, const float *taps2,
                      uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "dof_device";
    DofDesc d;
    int rc = dof_checks(r, settings, dof, d_hdr_rgb32f, d_depth, taps2, d_out_rgba8, true, false, d, who);
    if (rc || (rc = dof_states(r, d, d_hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    return dof_planes(r, settings, d, d_hdr_rgb32f, d_depth, taps2, d_out_rgba8);
}

int arctic_dof(ArcticRenderer *r, const ArcticSettings *settings, const ArcticDof *dof, const float *hdr_rgb32f, const float *depth, const float *taps2, uint8_t *out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "dof";
    DofDesc d;
    int rc = dof_checks(r, settings, dof, hdr_rgb32f, depth, taps2, out_rgba8, false, false, d, who);
    if (rc || (rc = dof_states(r, d, hdr_rgb32f == nullptr, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Dof &D = r->dof;
    const size_t px = (size_t)r->rows() * r->width;
    if (hdr_rgb32f && (rc = upload_plane(r, D.written, D.d_color, hdr_rgb32f, px, 12)) != ARCTIC_OK) return rc;
    if ((rc = upload_plane(r, D.written, D.d_depth, depth, px, 4)) != ARCTIC_OK) return rc;
    if ((rc = dof_planes(r, settings, d, hdr_rgb32f ? D.d_color.as<float>() : nullptr, D.d_depth.as<float>(), taps2, nullptr)) != ARCTIC_OK) return rc;
    return read_back(r, out_rgba8, D.d_rgba8, px * 4, hdr_rgb32f == nullptr);
}

int arctic_pass_dof(ArcticRenderer *r, const ArcticScene *scene, const ArcticSettings *settings, const ArcticDof *dof, const float *taps2, uint8_t *d_out_rgba8) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "pass_dof";
    alignas(16) static const char own_plane[16] = {};   // (the depth is the handle's own: never null, always aligned)
    DofDesc d;
    int rc = dof_checks(r, settings, dof, nullptr, own_plane, taps2, d_out_rgba8, true, true, d, who);
    if (rc) return rc;
    if (!valid_scene(scene)) return r->fail(ARCTIC_E_INVALID, "%s: null scene", who);
    d.z_near = scene->camera.z_near_far[0]; d.z_far = scene->camera.z_near_far[1];
    if (const char *why = dof_refusal(&d, false)) return r->fail(ARCTIC_E_INVALID, "%s: the scene's camera: %s", who, why);
    // the depth plane's refusal, in front of the first launch
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    if ((rc = dof_states(r, d, true, who)) != ARCTIC_OK || (rc = select_device(r)) != ARCTIC_OK) return rc;
    ArcticRenderer::Dof &D = r->dof;
    const size_t px = std::max<size_t>((size_t)r->rows() * r->width, 1);
    HIPCHECK(r, D.written.ensure(hipEventDisableTiming));
    HIPCHECK(r, D.written.wait(r->stream));   // (the depth below overwrites a plane the previous call read)
    HIPCHECK(r, D.d_depth.ensure(px * 4));
    if ((rc = mb_depth_plane(r, D.d_depth.as<float>())) != ARCTIC_OK) return rc;
    return dof_planes(r, settings, d, nullptr, D.d_depth.as<float>(), taps2, d_out_rgba8);
}

int arctic_read_dof(ArcticRenderer *r, float *ldr_rgb, float *hdr_rgb, uint8_t *rgba8, float *tile_max, float *neighbour_max, float *prepared2) {
    if (!r) return ARCTIC_E_INVALID;
    const ArcticRenderer::Dof &D = r->dof;
    if (!D.holds(*r) || r->rows() != r->height)
        return r->fail(ARCTIC_E_STATE, "read_dof: no depth of field yet, or not since the last resize");
    if (rgba8 && !D.own_rgba8) return r->fail(ARCTIC_E_STATE, "read_dof: the latest call wrote the caller's RGBA8 buffer, not the handle's");
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    const size_t px = (size_t)r->rows() * r->width, tiles = r->n_tiles();
    if (ldr_rgb) HIPCHECK(r, hipMemcpy(ldr_rgb, D.d_ldr.p, px * 12, hipMemcpyDeviceToHost));
    if (hdr_rgb) HIPCHECK(r, hipMemcpy(hdr_rgb, D.d_hdr.p, px * 12, hipMemcpyDeviceToHost));
    if (rgba8) HIPCHECK(r, hipMemcpy(rgba8, D.d_rgba8.p, px * 4, hipMemcpyDeviceToHost));
    if (tile_max) HIPCHECK(r, hipMemcpy(tile_max, D.d_tile.p, tiles * 4, hipMemcpyDeviceToHost));
    if (neighbour_max) HIPCHECK(r, hipMemcpy(neighbour_max, D.d_neighbour.p, tiles * 4, hipMemcpyDeviceToHost));
    if (prepared2) HIPCHECK(r, hipMemcpy(prepared2, D.d_prep.p, px * 8, hipMemcpyDeviceToHost));
    return ARCTIC_OK;
}

int arctic_dof_info(ArcticRenderer *r, uint64_t *out4) {
    if (!r) return ARCTIC_E_INVALID;
    if (!out4) return r->fail(ARCTIC_E_INVALID, "dof_info: null");
    out4[0] = r->dof.device_bytes(); out4[1] = r->dof.launches; out4[2] = r->dof.calls; out4[3] = 0;
    return ARCTIC_OK;
}

int arctic_dof_focus_at(ArcticRenderer *r, float z_near, float z_far, uint32_t px, uint32_t py, float *distance) {
    if (!r) return ARCTIC_E_INVALID;
    const char *who = "dof_focus_at";
    if (!distance) return r->fail(ARCTIC_E_INVALID, "%s: null distance", who);
    if (!(z_near > 0.0f) || !(z_far > z_near && rq_finite(z_far))) return r->fail(ARCTIC_E_INVALID, "%s: z_near not above 0, or z_far not finite and above it", who);
    if (px >= r->width || py >= r->rows()) return r->fail(ARCTIC_E_INVALID, "%s: pixel (%u, %u) is outside the handle's %u x %u pixels", who, px, py, r->width, r->rows());
    if (!r->have_vis) return r->fail(ARCTIC_E_STATE, "%s: no visibility plane (arctic_pass_gbuffer or a frame first; arctic_write_gbuffer leaves none)", who);
    int rc = select_device(r);
    if (rc) return rc;
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    // the plane is tile-major, as k_mb_depth reads it
    const uint32_t yy = py + r->row0_in_tile;
    const size_t at = ((size_t)(yy / 8) * r->tiles_x + px / 8) * 64 + (yy % 8) * 8 + px % 8;
    unsigned long long key = 0;
    HIPCHECK(r, hipMemcpy(&key, r->d_vis().as<unsigned long long>() + at, sizeof key, hipMemcpyDeviceToHost));
    uint32_t bits = (uint32_t)(key >> 32);
    float depth = 1.0f;
    if (key != ~0ull) std::memcpy(&depth, &bits, sizeof depth);
    *distance = dof_view_distance_host(z_near, z_far, depth);
    return ARCTIC_OK;
}

}  // extern "C"
