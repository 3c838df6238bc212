"""The ARCTIC_E_STATE refusals of the seven post stages for a NULL colour plane -- the handle's own HDR source -- by their exact texts (needs an
MI355X, launches no kernel): the temporal anti-aliasing, the motion blur, the depth of field, bloom, auto-exposure, fog and the temporal upscaler,
each with every source flag it accepts, on a fresh 16 x 16 handle and again once ARCTIC_OPT_KEEP_FLOAT_OUTPUT is set; and each stage's whole-frame
refusal on a shard of rows 0..8.  Every refused call leaves the stage's *_info() at zeros.  The texts were copied by hand from the calls' source
as it stood before the source rule was stated once: two stages name another stage's flag, because they reached the refusal through
that stage's function, and that spelling is part of what is pinned."""
import pytest

import fog_reference as G

pytestmark = pytest.mark.gpu
STATE = -4
SETTINGS = (0, 2.2, 1.0)
W = H = 16

KEEP = "the float HDR plane needs ARCTIC_OPT_KEEP_FLOAT_OUTPUT"
SHADED = "nothing shaded since ARCTIC_OPT_KEEP_FLOAT_OUTPUT was turned on or since the last resize (arctic_pass_shade or a frame first)"
NO_TAA = ": the anti-aliasing's history is empty (no resolve yet, or none since the last reset or resize)"
NO_BLUR = ": nothing blurred yet, or not since the last resize"
NO_DOF = ": no depth of field yet, or not since the last resize"
NO_BLOOM = ": no bloom yet, or not since the last resize"
NEIGHBOURS = " need the whole frame, this handle owns 8 of 16 rows (its neighbours' rows are on other shards)"
OTHERS = ", this handle owns 8 of 16 rows (the others are on other shards)"


def own(flags):
    """a source that is the float HDR plane itself or the composition: (flags, text on a fresh handle, text once the option is set)"""
    return (flags, KEEP, SHADED)


def stage_in_front(flags, text):
    """a source that is another stage's plane: the same refusal whatever the option says"""
    return (flags, text, text)


# who: the call's name in its messages; call(r, planes, flags): the device form with a NULL colour plane; whole: the whole-frame refusal on the shard
STAGES = {
    "taa": dict(who="taa_resolve_device", info="taa_info", whole="the history's taps" + NEIGHBOURS,
                call=lambda r, p, f: r.taa_resolve_device(SETTINGS, None, None, None, flags=f),
                sources=(own(0), own(2))),
    "motion_blur": dict(who="motion_blur_device", info="motion_blur_info", whole="the gather's taps" + NEIGHBOURS,
                        call=lambda r, p, f: r.motion_blur_device(SETTINGS, None, p, None, None, flags=f),
                        sources=(own(0), own(2), stage_in_front(4, "ARCTIC_MB_SOURCE_TAA" + NO_TAA))),
    "dof": dict(who="dof_device", info="dof_info", whole="the gather's taps" + NEIGHBOURS,
                call=lambda r, p, f: r.dof_device(SETTINGS, None, p, None, None, flags=f),
                sources=(own(0), own(1), stage_in_front(2, "ARCTIC_MB_SOURCE_TAA" + NO_TAA), stage_in_front(4, "ARCTIC_DOF_SOURCE_MOTION_BLUR" + NO_BLUR))),
    "bloom": dict(who="bloom_device", info="bloom_info", whole="the pyramid's footprints" + NEIGHBOURS,
                  call=lambda r, p, f: r.bloom_device(SETTINGS, None, None, flags=f),
                  sources=(own(0), own(1), stage_in_front(2, "ARCTIC_BLOOM_SOURCE_TAA" + NO_TAA), stage_in_front(4, "ARCTIC_BLOOM_SOURCE_MOTION_BLUR" + NO_BLUR),
                           stage_in_front(8, "ARCTIC_BLOOM_SOURCE_DOF" + NO_DOF))),
    "exposure": dict(who="exposure_device", info="exposure_info", whole="the meter needs the whole frame" + OTHERS,
                     call=lambda r, p, f: r.exposure_device(SETTINGS, None, None, flags=f),
                     sources=(own(0), own(1), stage_in_front(2, "ARCTIC_EXPOSURE_SOURCE_TAA" + NO_TAA), stage_in_front(4, "ARCTIC_EXPOSURE_SOURCE_MOTION_BLUR" + NO_BLUR),
                              stage_in_front(8, "ARCTIC_EXPOSURE_SOURCE_DOF" + NO_DOF), stage_in_front(16, "ARCTIC_EXPOSURE_SOURCE_BLOOM" + NO_BLOOM),
                              own(128), own(1 | 128))),     # ARCTIC_EXPOSURE_HOLD: the source's refusal comes first
    "fog": dict(who="fog_device", info="fog_info", whole="whole frames only" + OTHERS,
                call=lambda r, p, f: r.fog_device(SETTINGS, G.view_record(), None, None, None, None, flags=f),
                sources=(own(0), own(1))),
    "taa_upscale": dict(who="taa_upscale_device", info="taa_upscale_info", whole="the samples' boxes" + NEIGHBOURS,
                        call=lambda r, p, f: r.taa_upscale_device(SETTINGS, (2 * W, 2 * H), None, None, None, flags=f),
                        sources=(own(0), own(2))),
}
CASES = [(name, source) for name, stage in STAGES.items() for source in stage["sources"]]


@pytest.fixture(scope="module")
def plane(hip):
    """a device plane for the velocity or the depth a call insists on: large enough for either, never read by a refused call"""
    import torch
    t = torch.zeros(W * H * 2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t


def refused(hip, r, stage, plane, flags, text):
    with pytest.raises(hip.ArcticError) as e:
        stage["call"](r, plane.data_ptr(), flags)
    message = str(e.value)
    print(repr(message))
    assert e.value.code == STATE, message
    assert message.endswith(stage["who"] + ": " + text), (message, text)
    assert getattr(r, stage["info"])() == (0, 0, 0, 0), message


@pytest.mark.parametrize("name,source", CASES, ids=[f"{n}-{s[0]}" for n, s in CASES])
def test_a_null_colour_is_refused_in_the_stages_words(hip, plane, name, source):
    stage = STAGES[name]
    flags, fresh, kept = source
    r = hip.Renderer(W, H, 64, 16)
    refused(hip, r, stage, plane, flags, fresh)
    r.set_option("keep_float_output", 1)
    refused(hip, r, stage, plane, flags, kept)
    r.close()


@pytest.mark.parametrize("name", list(STAGES))
def test_a_shard_is_refused_in_the_stages_words(hip, plane, name):
    stage = STAGES[name]
    r = hip.Renderer(W, H, 64, 16, row_begin=0, row_end=8)
    refused(hip, r, stage, plane, 0, stage["whole"])
    r.set_option("keep_float_output", 1)
    refused(hip, r, stage, plane, stage["sources"][-1][0], stage["whole"])       # whatever the source: the whole-frame refusal comes first
    r.close()
