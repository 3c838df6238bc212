"""arctic_exposure(_device), arctic_read_exposure, arctic_exposure_reset and arctic_exposure_info on the device (needs an MI355X), against the
numpy definition of tests/exposure_reference.py BY BYTES, no pixel left out: the histogram H, the 32-byte state record and the exposed plane
`out` of the three kernels on synthetic planes (NaN, infinite, negative and huge colours; sizes from 1 x 1 to 136 x 72 and the frame whose pixel
count is the smallest above one full trip of every workgroup of k_exposure_meter; two records, four windows, sentinels behind every caller
plane), the two contention extremes (every lane on one bin; all 256 bins in turn along a row), the tonemapped planes by
test_gpu_bloom.judge_tonemapped's rule, six calls enqueued with nothing read between them, the flags, the host form, warm calls, a resize, the
counters and the refusals; and on the rasterised scene of tests/hit_scenes.py each source flag on a plane of its own, the whole chain render ->
anti-aliasing -> motion blur -> depth of field -> bloom -> exposure, and a handle that never makes these calls."""
import ctypes as C

import numpy as np
import pytest

import exposure_reference as E
import hit_scenes
import test_exposure_reference as TR
import test_gpu_bloom as TB
import test_gpu_compose as TC
import test_gpu_motion as TM
import test_gpu_taa as TT

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SETTINGS = TT.SETTINGS
SIZE = TT.SIZE


def read_all(r):
    """(ldr, out, H, state) of the latest call"""
    ldr, hdr, _, hist, state = r.read_exposure(want=("ldr", "hdr", "hist", "state"))
    return ldr, hdr, hist, state


def got_of(r):
    """(H, state, out) of the latest call"""
    _, out, H, state = read_all(r)
    return H, state, out


def same_call(got, want, what):
    """(H, state, out) by bytes"""
    H, state, out = got
    assert H.dtype == np.uint32 and H.tobytes() == want[0].tobytes(), (what, "H", np.flatnonzero(H != want[0])[:8])
    TR.same_state(state, want[1], what)
    if want[2] is not None:
        TR.same_out(out, want[2], what)


def size_of(size):
    return TR.second_trip_size() if size == "second trip" else size


@pytest.mark.parametrize("size", TR.SMALL_SIZES + ("second trip",), ids=str)
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, size):
    width, height = size_of(size)
    Cp = TR.case(width, height)
    n = width * height
    r = hip.Renderer(width, height, 64, 16)
    assert r.exposure_info() == (0, 0, 0, 0)
    d_c = TT.floats(Cp)
    prev, call = None, 0
    for rec0 in TR.RECORDS:
        for w in TR.windows(width, height):
            rec = dict(rec0, window=w)
            what = (width, height, rec["flags"], w)
            d_o = TT.bytes_on_device(n * 4)
            r.exposure_device(SETTINGS[call % 3], d_c.data_ptr(), d_o.data_ptr(), **rec)
            ldr, out, H, state = read_all(r)
            want = E.exposure(Cp, rec, prev)
            same_call((H, state, out), want, what)
            x0, y0, x1, y1 = E.window_of(rec, width, height)
            assert int(H.astype(np.uint64).sum()) == (x1 - x0) * (y1 - y0)
            prev = want[1]
            got8 = d_o.cpu().numpy()
            assert (got8[n * 4:] == 77).all()                                    # sentinels behind the caller's output
            back = d_c.cpu().numpy()
            assert (back[Cp.size:] == TT.SENTINEL).all() and back[:Cp.size].tobytes() == Cp.tobytes()       # ... and the input is read only
            TB.judge_tonemapped(what, ldr, got8[:n * 4].reshape(height, width, 4), out, SETTINGS[call % 3])
            with pytest.raises(hip.ArcticError):                                 # the RGBA8 went to the caller's buffer
                r.read_exposure(want=("rgba8",))
            call += 1
    info = r.exposure_info()
    lay = pkg.renderer.exposure_layout(width, height)
    assert info[1:] == (call, call, call) and info[0] >= n * (12 + 12) + lay["table_bytes"] + 1024 + 32
    r.close()


@pytest.mark.parametrize("size", ((136, 72), "second trip"), ids=str)
def test_contention_extremes(pkg, hip, size):
    """every lane of every wave on one bin, and all 256 bins in turn along a row: a dropped LDS add, a missed barrier, a lost tail or a stale row
    of the partials table shows here"""
    width, height = size_of(size)
    r = hip.Renderer(width, height, 64, 16)
    prev = None
    for k, plane in enumerate((TR.constant_plane(width, height), TR.cycle_plane(width, height), TR.constant_plane(width, height))):
        rec = TR.RECORDS[k % 2]
        d_c = TT.floats(plane)
        r.exposure_device(SETTINGS[0], d_c.data_ptr(), None, **rec)
        _, out, H, state = read_all(r)
        want = E.exposure(plane, rec, prev)
        same_call((H, state, out), want, (width, height, k))
        assert int(H.astype(np.uint64).sum()) == width * height
        prev = want[1]
    assert int((H != 0).sum()) == 1 and int(H.max()) == width * height           # nothing of the cycle's table is left in the constant plane's
    r.close()


@pytest.mark.parametrize("k", (-3, 1, 5))
def test_property_ii_on_the_device(pkg, hip, k):
    """64 x 32 under the whole band has M = 2048, a power of two: the adapted key shifts by exactly 8k.  40 x 24 and 17 x 9 under narrower bands
    have other M: the key shifts by 8k to the last place of the binary64 division (four spacings of a: the division and the addition of
    888.5 round once each on either side), and L, E and out are exact all the same"""
    wide = dict(min_exposure=2.0 ** -20, max_exposure=65504.0)
    for (width, height), rec, exact in (((64, 32), E.record(flags=E.RESET, low_q16=0, high_q16=65536, **wide), True), ((40, 24), E.record(flags=E.RESET, **wide), False),
                                        ((17, 9), dict(TR.RECORDS[1], flags=E.RESET | E.SKIP_BLACK, **wide), False)):
        C0 = TR.inside_plane(width, height, 40 + width)
        C1 = (C0 * F(2.0 ** k)).astype(F)
        r = hip.Renderer(width, height, 64, 16)
        got = []
        for plane in (C0, C1):
            d_c = TT.floats(plane)
            r.exposure_device(SETTINGS[0], d_c.data_ptr(), None, **rec)
            _, out, H, state = read_all(r)
            same_call((H, state, out), E.exposure(plane, rec), (k, width, height))
            got.append((H, state, out))
        (H0, s0, out0), (H1, s1, out1) = got
        M = int(s0["metered"][0])
        assert (M & (M - 1) == 0) == exact and int(s1["metered"][0]) == M
        shift = float(s1["adapted_key"][0]) - float(s0["adapted_key"][0])
        print(f"k = {k}, {width} x {height}, M = {M}: the adapted key shifts by {shift!r}")
        assert (np.roll(H0, 8 * k) == H1).all()
        assert shift == 8.0 * k if exact else abs(shift - 8.0 * k) <= 4 * np.spacing(float(s0["adapted_key"][0]))
        assert float(s1["luminance"][0]) == float(s0["luminance"][0]) * 2.0 ** k and float(s1["exposure"][0]) == float(s0["exposure"][0]) * 2.0 ** -k
        assert out0.tobytes() == out1.tobytes()
        r.close()


def test_six_calls_enqueued_then_read(pkg, hip):
    """the state lives on the device: six calls over changing frames are enqueued back to back, nothing is read in between, and the sixth's H,
    state and out are numpy's after six -- under rates below 1 they depend on every call since the RESET in the fourth"""
    for width, height in ((17, 9), (40, 24)):
        frames = TR.frames_of_a_sequence(width, height)
        planes = [TT.floats(f) for f in frames]
        for rec0 in TR.RECORDS + (dict(TR.RECORDS[1], window=(1, 1, width - 1, height - 2)),):
            want = TR.sequence_reference(width, height, rec0)
            r = hip.Renderer(width, height, 64, 16)
            for d_c, extra in zip(planes, TR.SEQUENCE_FLAGS):
                r.exposure_device(SETTINGS[1], d_c.data_ptr(), None, **dict(rec0, flags=rec0["flags"] | extra))
            _, out, H, state = read_all(r)
            same_call((H, state, out), want[5], (width, height, rec0["flags"]))
            assert r.exposure_info()[1:] == (6, 6, 6)
            if rec0["flags"] & E.SKIP_BLACK:
                assert int(state["frames"][0]) == 2 and state["adapted_key"].tobytes() != want[3][1]["adapted_key"].tobytes()      # calls 4 and 6 measured; 5 (NaNs) did not
            r.close()


def test_flags_host_form_warm_calls_reset_resize_and_counters(pkg, hip):
    width, height = TR.SMALL_SIZES[4]
    n = width * height
    Cp, dark = TR.case(width, height), (TR.case(width, height, seed=3) * F(2.0 ** -6)).astype(F)
    rec = TR.RECORDS[1]
    r = hip.Renderer(width, height, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_exposure()
    assert e.value.code == STATE                                                 # nothing yet
    with pytest.raises(hip.ArcticError) as e:
        r.exposure(SETTINGS[0], Cp, **dict(rec, flags=rec["flags"] | E.HOLD))
    assert e.value.code == STATE and r.exposure_info() == (0, 0, 0, 0)           # nothing is held
    # METER_ONLY: H and the state, no output plane
    assert r.exposure(SETTINGS[0], Cp, **dict(rec, flags=rec["flags"] | E.METER_ONLY)) is None
    lay = pkg.renderer.exposure_layout(width, height)
    metered = r.exposure_info()
    assert metered[1:] == (0, 1, 1) and lay["table_bytes"] + 1024 + 32 + n * 12 <= metered[0] < lay["table_bytes"] + 1024 + 32 + n * 12 + n * 12      # T, H, state, the host form's colour
    _, _, _, H, state = r.read_exposure(want=("hist", "state"))
    want = E.exposure(Cp, dict(rec, flags=rec["flags"] | E.METER_ONLY))
    same_call((H, state, None), want, "meter only")
    with pytest.raises(hip.ArcticError) as e:
        r.read_exposure(want=("hdr",))
    assert e.value.code == STATE                                                 # no frame was exposed
    # HOLD: the held E on another frame, one launch, the state untouched
    first = r.exposure(SETTINGS[0], dark, **dict(rec, flags=rec["flags"] | E.HOLD))
    ldr, out, H2, state2 = read_all(r)
    TR.same_out(out, E.apply(dark, want[1]["exposure"][0]), "hold")
    assert H2.tobytes() == H.tobytes() and TR.state_bytes(state2) == TR.state_bytes(state) and r.exposure_info()[1:] == (1, 2, 1)
    rgba8 = r.read_exposure(want=("rgba8",))[2]
    assert first.tobytes() == rgba8.tobytes()
    TB.judge_tonemapped("hold", ldr, rgba8, out, SETTINGS[0])
    # the host form adapts from the held state: rates below 1
    assert r.exposure(SETTINGS[1], dark, read=False, **rec) is None
    ldr, out, H3, state3 = read_all(r)
    want3 = E.exposure(dark, rec, want[1])
    same_call((H3, state3, out), want3, "host form")
    assert int(state3["frames"][0]) == 2 and float(state3["adapted_key"][0]) < float(state["adapted_key"][0])
    TB.judge_tonemapped("host form", ldr, r.read_exposure(want=("rgba8",))[2], out, SETTINGS[1])
    held = r.exposure_info()
    assert held[1:] == (2, 3, 2) and held[0] >= metered[0] + n * (12 + 12 + 4)
    # warm calls allocate nothing; the same frame from the same state gives the same bytes on another handle
    r.exposure(SETTINGS[1], dark, **rec)
    assert r.exposure_info() == (held[0], 3, 4, 3)
    want4 = E.exposure(dark, rec, want3[1])
    same_call(got_of(r), want4, "warm")
    # ARCTIC_EXPOSURE_RESET in the record: a = a_t at once
    r.exposure(SETTINGS[1], Cp, **dict(rec, flags=rec["flags"] | E.RESET))
    want5 = E.exposure(Cp, dict(rec, flags=rec["flags"] | E.RESET), want4[1])
    same_call(got_of(r), want5, "RESET")
    assert int(want5[1]["frames"][0]) == 1
    # arctic_exposure_reset: the next call starts from an invalid state, and until then nothing is held
    r.exposure_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.exposure(SETTINGS[0], Cp, **dict(rec, flags=rec["flags"] | E.HOLD))
    assert e.value.code == STATE
    with pytest.raises(hip.ArcticError) as e:
        r.read_exposure(want=("state",))
    assert e.value.code == STATE
    r.exposure(SETTINGS[1], dark, **rec)
    same_call(got_of(r), E.exposure(dark, rec, None), "after the reset")
    # the device form into the handle's own output
    d_c = TT.floats(Cp)
    r.exposure_device(SETTINGS[2], d_c.data_ptr(), None, **TR.RECORDS[0])
    ldr, out, H6, state6 = read_all(r)
    same_call((H6, state6, out), E.exposure(Cp, TR.RECORDS[0], E.exposure(dark, rec, None)[1]), "device form, own output")
    TB.judge_tonemapped("device form, own output", ldr, r.read_exposure(want=("rgba8",))[2], out, SETTINGS[2])
    # resize: nothing to read, nothing held, then the new size from an invalid state
    r.resize(*TR.SMALL_SIZES[3])
    with pytest.raises(hip.ArcticError) as e:
        r.read_exposure()
    assert e.value.code == STATE
    small = TR.case(*TR.SMALL_SIZES[3])
    with pytest.raises(hip.ArcticError) as e:
        r.exposure(SETTINGS[0], small, **dict(rec, flags=rec["flags"] | E.HOLD))
    assert e.value.code == STATE
    r.exposure(SETTINGS[0], small, **rec)
    same_call(got_of(r), E.exposure(small, rec, None), "after the resize")
    r.close()


def test_hold_after_a_call_that_measured_nothing(pkg, hip):
    """HOLD asks whether a metering call has been made, which the host knows, not whether the device state is valid, which it does not: behind an
    all-black frame under SKIP_BLACK the state is invalid and HOLD applies that call's E, the clamped fallback"""
    width, height = TR.SMALL_SIZES[2]
    rec = TR.RECORDS[1]
    Cp = TR.case(width, height)
    r = hip.Renderer(width, height, 64, 16)
    r.exposure(SETTINGS[0], np.zeros_like(Cp), **rec)
    _, _, _, H, state = r.read_exposure(want=("hist", "state"))
    assert int(H[0]) == width * height and int(state["valid"][0]) == 0 and int(state["metered"][0]) == 0 and float(state["exposure"][0]) == 2.0
    r.exposure(SETTINGS[0], Cp, **dict(rec, flags=rec["flags"] | E.HOLD))
    H2, state2, out = got_of(r)
    TR.same_out(out, E.apply(Cp, F(2.0)), "hold behind a call that measured nothing")
    assert H2.tobytes() == H.tobytes() and TR.state_bytes(state2) == TR.state_bytes(state)
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    width, height = TR.SMALL_SIZES[3]
    n = width * height
    Cp = TR.case(width, height)
    r = hip.Renderer(width, height, 64, 16)
    d_c, d_o = TT.floats(Cp), TT.bytes_on_device(n * 4)
    good = TR.RECORDS[0]

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda c=d_c.data_ptr(), o=d_o.data_ptr(), **kw: r.exposure_device(SETTINGS[0], c, o, **dict(good, **kw))
    bads = (dict(flags=512), dict(flags=0x80000000), dict(flags=3), dict(flags=5), dict(flags=6), dict(flags=9), dict(flags=12), dict(flags=17), dict(flags=24), dict(flags=31),
            dict(flags=E.HOLD | E.METER_ONLY), dict(flags=E.HOLD | E.RESET), dict(low_q16=100, high_q16=100), dict(low_q16=200, high_q16=100), dict(high_q16=65537),
            dict(key_value=0.0), dict(key_value=-1.0), dict(key_value=65505.0), dict(key_value=np.nan), dict(key_value=np.inf), dict(min_exposure=0.0), dict(min_exposure=np.nan),
            dict(min_exposure=2.0, max_exposure=1.0), dict(max_exposure=65505.0), dict(max_exposure=np.nan), dict(rate_up=-0.1), dict(rate_up=1.5), dict(rate_up=np.nan),
            dict(rate_down=-0.1), dict(rate_down=1.5), dict(rate_down=np.nan), dict(fallback_exposure=0.0), dict(fallback_exposure=65505.0), dict(fallback_exposure=np.nan),
            dict(window=(0, 0, width + 1, height)), dict(window=(0, 0, width, height + 1)), dict(window=(3, 0, 3, height)), dict(window=(0, 5, width, 4)), dict(window=(0, 0, 0, height)))
    for bad in bads:
        refused(INVALID, lambda: go(**bad))
    reserved = pkg.renderer.exposure_arguments(**good)
    reserved["reserved"] = 1
    refused(INVALID, lambda: r.exposure_device(SETTINGS[0], d_c.data_ptr(), d_o.data_ptr(), exposure=reserved))
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    rec = pkg.renderer.exposure_arguments(**good)
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    assert r.L.arctic_exposure_device(r.h, None, hp(rec), vp(d_c), None) == INVALID
    assert r.L.arctic_exposure_device(r.h, st, None, vp(d_c), None) == INVALID
    assert r.L.arctic_exposure(r.h, None, hp(rec), None, None) == INVALID
    assert r.L.arctic_exposure_info(r.h, None) == INVALID
    # a NULL colour plane is the handle's own: it needs the float HDR plane and a shading, or a composition, a history, a blur, a lens, a bloom
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    for flags in (E.SOURCE_COMPOSED, E.SOURCE_TAA, E.SOURCE_MOTION_BLUR, E.SOURCE_DOF, E.SOURCE_BLOOM):
        refused(STATE, lambda: go(c=None, flags=flags))
        refused(STATE, lambda: r.exposure(SETTINGS[0], None, **dict(good, flags=flags)))
    refused(STATE, lambda: go(flags=E.HOLD))                                     # nothing is held
    refused(INVALID, lambda: go(flags=E.HOLD, key_value=np.nan))                 # ... and ARCTIC_E_INVALID comes first
    assert r.exposure_info() == (0, 0, 0, 0)                                     # a refused call holds nothing
    # a shard is refused: the meter needs the whole frame
    shard = hip.Renderer(width, height, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.exposure_device(SETTINGS[0], d_c.data_ptr(), d_o.data_ptr(), **good)
    assert e.value.code == STATE and shard.exposure_info() == (0, 0, 0, 0)
    with pytest.raises(hip.ArcticError) as e:
        shard.read_exposure()
    assert e.value.code == STATE
    shard.close()
    # the planes and the state are what the last good call left, the caller's buffers were never written by a refused call
    assert (d_o.cpu().numpy() == 77).all()
    go()
    for bad in bads[:3] + bads[12:14] + bads[-2:]:
        refused(INVALID, lambda: go(**bad))
    refused(STATE, lambda: go(c=None))
    assert r.exposure_info()[1:] == (1, 1, 1)
    _, out, H, state = read_all(r)
    same_call((H, state, out), E.exposure(Cp, good), "after the refusals")
    assert (d_o.cpu().numpy()[n * 4:] == 77).all() and (d_c.cpu().numpy()[Cp.size:] == TT.SENTINEL).all()
    r.close()


# ---- the rasterised scene of the hit tests ----------------------------------------------------------------------------------------------------------
KW = E.record(low_q16=6554, high_q16=62259, key_value=0.25, rate_up=0.5, rate_down=0.25)
BLOOM_KW = TB.KW
DOF_KW = TB.DOF_KW


def test_the_chain_and_five_sources(pkg, hip):
    """two frames, each: render, arctic_pass_taa, arctic_pass_motion_blur of the history, arctic_pass_dof of the blur, arctic_bloom_device of the
    lens -- then the shading's plane, the history, the blur's, the lens' and bloom's outputs are five different planes, and the exposure under no
    flag, ARCTIC_EXPOSURE_SOURCE_TAA, _MOTION_BLUR, _DOF and _BLOOM reads each: numpy on the read-back plane, by bytes, the state threaded through
    the five calls.  The last is the whole chain.  Every flag is refused while its plane does not exist, and after a resize; the stages in front
    keep their bytes and their counters"""
    import bloom_reference as B
    import dof_reference as D
    import motion_blur_reference as M
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    zn, zf = (float(x) for x in descs[0].camera["z_near_far"])
    r = TT.lit_handle(pkg, hip)
    r.render_frame(descs[0], SETTINGS[0])
    for flags in (E.SOURCE_TAA, E.SOURCE_MOTION_BLUR, E.SOURCE_DOF, E.SOURCE_BLOOM, E.SOURCE_COMPOSED):
        with pytest.raises(hip.ArcticError) as e:
            r.exposure_device(SETTINGS[0], **dict(KW, flags=flags))
        assert e.value.code == STATE and r.exposure_info() == (0, 0, 0, 0)
    for desc in descs:
        r.render_frame(desc, SETTINGS[0])
        r.pass_taa(desc, SETTINGS[0], max_history=4.0)
        r.pass_motion_blur(desc, SETTINGS[0], flags=M.SOURCE_TAA, shutter=1.0, max_radius=8.0, samples=7, depth_extent=0.05)
        r.pass_dof(desc, SETTINGS[0], flags=D.SOURCE_MOTION_BLUR, read=False, focus_distance=r.dof_focus_at(W // 2, H // 2, zn, zf), **DOF_KW)
        r.bloom_device(SETTINGS[0], flags=B.SOURCE_DOF, **BLOOM_KW)
    shaded, history, blurred = r.read_output(want=("hdr",))[1], r.read_taa(want=("hdr",))[1], r.read_motion_blur(want=("hdr",))[1]
    lens, glow = r.read_dof(want=("hdr",))[1], r.read_bloom(BLOOM_KW["levels"], want=("hdr",))[1]
    assert (shaded != history).any() and (history != blurred).any() and (blurred != lens).any() and (lens != glow).any()
    before = r.motion_info(), r.taa_info(), r.motion_blur_info(), r.dof_info(), r.bloom_info()
    prev = None
    for k, (flags, plane) in enumerate(((0, shaded), (E.SOURCE_TAA, history), (E.SOURCE_MOTION_BLUR, blurred), (E.SOURCE_DOF, lens), (E.SOURCE_BLOOM, glow))):
        rec = dict(KW, flags=flags)
        r.exposure_device(SETTINGS[k % 3], **rec)
        ldr, out, Hh, state = read_all(r)
        want = E.exposure(plane, rec, prev)
        same_call((Hh, state, out), want, ("source", flags))
        prev = want[1]
        TB.judge_tonemapped(("source", flags), ldr, r.read_exposure(want=("rgba8",))[2], out, SETTINGS[k % 3])
        print(f"source {flags}: M = {int(state['metered'][0])}, L = {float(state['luminance'][0]):.4f}, E = {float(state['exposure'][0]):.4f}")
        assert int(state["metered"][0]) > 0 and (out != plane).any()
    host = r.exposure(SETTINGS[0], None, **dict(KW, flags=E.SOURCE_BLOOM))          # the host form of the chain's last step
    assert host.tobytes() == r.read_exposure(want=("rgba8",))[2].tobytes()
    _, out, Hh, state = read_all(r)
    same_call((Hh, state, out), E.exposure(glow, dict(KW, flags=E.SOURCE_BLOOM), prev), "the chain, host form")
    assert (r.motion_info(), r.taa_info(), r.motion_blur_info(), r.dof_info(), r.bloom_info()) == before and r.exposure_info()[1:] == (6, 6, 6)   # it reads the stages in front of it, it moves none
    assert r.read_bloom(BLOOM_KW["levels"], want=("hdr",))[1].tobytes() == glow.tobytes() and r.read_dof(want=("hdr",))[1].tobytes() == lens.tobytes()
    assert r.read_motion_blur(want=("hdr",))[1].tobytes() == blurred.tobytes() and r.read_taa(want=("hdr",))[1].tobytes() == history.tobytes()
    assert r.read_output(want=("hdr",))[1].tobytes() == shaded.tobytes()
    r.resize(W + 8, H)
    for flags in (0, E.SOURCE_TAA, E.SOURCE_MOTION_BLUR, E.SOURCE_DOF, E.SOURCE_BLOOM):
        with pytest.raises(hip.ArcticError) as e:
            r.exposure_device(SETTINGS[0], **dict(KW, flags=flags))
        assert e.value.code == STATE
    r.close()


def test_the_composed_source(pkg, hip):
    """ARCTIC_EXPOSURE_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane, the sixth plane"""
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    with pytest.raises(hip.ArcticError) as e:
        r.exposure_device(TC.SETTINGS, **dict(KW, flags=E.SOURCE_COMPOSED))
    assert e.value.code == STATE and r.exposure_info() == (0, 0, 0, 0)              # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    held = r.compose_info()
    rec = dict(KW, flags=E.SOURCE_COMPOSED)
    r.exposure_device(TC.SETTINGS, **rec)
    ldr, out, H, state = read_all(r)
    want = E.exposure(composed, rec)
    same_call((H, state, out), want, "composed")
    TB.judge_tonemapped("composed source", ldr, r.read_exposure(want=("rgba8",))[2], out, TC.SETTINGS)
    r.exposure_device(TC.SETTINGS, **KW)                                         # ... and without the flag the shading's plane
    _, out, H, state = read_all(r)
    same_call((H, state, out), E.exposure(shaded, KW, want[1]), "shaded")
    assert r.compose_info() == held and r.read_composed(want=("hdr",))[1].tobytes() == composed.tobytes()
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls, which reports zero bytes"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info(), a.dof_info(), a.bloom_info()
    assert a.exposure_info() == (0, 0, 0, 0)
    a.exposure_device(TC.SETTINGS, **KW)
    a.exposure_device(TC.SETTINGS, **KW)
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info(), a.dof_info(), a.bloom_info()) == held
    assert a.exposure_info()[1:] == (2, 2, 2)
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.exposure_info() == (0, 0, 0, 0)
    a.close(); b.close()
