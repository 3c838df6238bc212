// post_source.cpp -- what the post stages' calls share (renderer_state.h: taa_calls.cpp, motion_blur_calls.cpp, dof_calls.cpp, bloom_calls.cpp,
// exposure_calls.cpp, fog_calls.cpp, taa_upscale_calls.cpp; the composition in ray_calls.cpp asks the same of the shaded plane): which float HDR
// plane a NULL colour pointer means and what refuses it, and the two ends of a host form.  Owns nothing of the handle; of the
// stages it reads what says whether their planes hold a frame of this size, their output planes and their marks.  This is where the stages' names
// meet, so that no stage's unit names a later one.
#include <algorithm>

#include "renderer_state.h"

namespace arctic {

// Every ARCTIC_E_STATE refusal of a source: no side effect.  s.flag: the public name of the flag that chose it (unused for Shaded).
// A stage in front of this one: its planes hold a frame of this size, the condition of its own read call.  Otherwise the float HDR plane: the
// option, a shading under it, the composition where that is the source, no binary16 rounding -- in this order
int source_refusal(ArcticRenderer *r, SourceFlag s, const char *who) {
    switch (s.source) {
    case HdrSource::Taa:
        return r->taa.holds(*r) ? ARCTIC_OK : r->fail(ARCTIC_E_STATE, "%s: %s: the anti-aliasing's history is empty (no resolve yet, or none since the last reset or resize)", who, s.flag);
    case HdrSource::MotionBlur:
        return r->motion_blur.holds(*r) ? ARCTIC_OK : r->fail(ARCTIC_E_STATE, "%s: %s: nothing blurred yet, or not since the last resize", who, s.flag);
    case HdrSource::Dof:
        return r->dof.holds(*r) ? ARCTIC_OK : r->fail(ARCTIC_E_STATE, "%s: %s: no depth of field yet, or not since the last resize", who, s.flag);
    case HdrSource::Bloom:
        return r->bloom.holds(*r) ? ARCTIC_OK : r->fail(ARCTIC_E_STATE, "%s: %s: no bloom yet, or not since the last resize", who, s.flag);
    case HdrSource::Shaded:
    case HdrSource::Composed:
        break;
    }
    if (!r->keep_float) return r->fail(ARCTIC_E_STATE, "%s: the float HDR plane needs ARCTIC_OPT_KEEP_FLOAT_OUTPUT", who);
    if (!r->hdr_valid) return r->fail(ARCTIC_E_STATE, "%s: nothing shaded since ARCTIC_OPT_KEEP_FLOAT_OUTPUT was turned on or since the last resize (arctic_pass_shade or a frame first)", who);
    if (s.source == HdrSource::Composed && (!r->compose.pixels || r->compose.pixels != (uint64_t)r->rows() * r->width))
        return r->fail(ARCTIC_E_STATE, "%s: %s: nothing composed yet, or not since the last resize", who, s.flag);
    if (r->hdr16) return r->fail(ARCTIC_E_STATE, "%s: ARCTIC_OPT_HDR16 = 1: the HDR plane is rounded through binary16", who);
    return ARCTIC_OK;
}

// The plane itself, behind the refusals.  A stage's plane was written on the stream its mark was recorded on: r->stream waits for the mark if
// the handle's stream has changed since.  The shaded and the composed plane were written in the handle's stream order and have no mark
int source_plane(ArcticRenderer *r, HdrSource source, SourcePlane &plane) {
    plane = SourcePlane{nullptr, false};
    switch (source) {
    case HdrSource::Shaded: plane.color = r->d_hdr.p; break;
    case HdrSource::Composed: plane.color = r->compose.d_hdr.p; break;
    case HdrSource::Taa:
        HIPCHECK(r, r->taa.written.wait(r->stream));
        plane = SourcePlane{r->taa.d_t[r->taa.cur].p, true};
        break;
    case HdrSource::MotionBlur:
        HIPCHECK(r, r->motion_blur.written.wait(r->stream));
        plane.color = r->motion_blur.d_hdr.p;
        break;
    case HdrSource::Dof:
        HIPCHECK(r, r->dof.written.wait(r->stream));
        plane.color = r->dof.d_hdr.p;
        break;
    case HdrSource::Bloom:
        HIPCHECK(r, r->bloom.written.wait(r->stream));
        plane.color = r->bloom.d_hdr.p;
        break;
    }
    return ARCTIC_OK;
}

// A host form's head: a caller's plane of px pixels into the stage's buffer d, behind the stage's mark -- the copy overwrites a plane the
// stage's previous call read, perhaps on another stream (arctic_set_stream came in between)
int upload_plane(ArcticRenderer *r, StreamMark &written, DevBuf &d, const void *plane, size_t px, size_t bytes_per_pixel) {
    HIPCHECK(r, written.ensure(hipEventDisableTiming));
    HIPCHECK(r, written.wait(r->stream));
    HIPCHECK(r, d.ensure(std::max<size_t>(px, 1) * bytes_per_pixel));
    HIPCHECK(r, hipMemcpyAsync(d.p, plane, px * bytes_per_pixel, hipMemcpyHostToDevice, r->stream));
    return ARCTIC_OK;
}

// ... and its tail: the result to the caller's memory (out null: nothing to copy), then the stream is drained.  FROM_FRAME: the result was made
// from the G-buffer or the planes of a frame, so the call also reports a rasteriser table that overflowed under that frame (check_item_overflow)
int read_back(ArcticRenderer *r, void *out, const DevBuf &d, size_t bytes, bool from_frame) {
    if (out) HIPCHECK(r, hipMemcpyAsync(out, d.p, bytes, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(r, hipStreamSynchronize(r->stream));
    return from_frame ? check_item_overflow(r) : ARCTIC_OK;
}

}  // namespace arctic
