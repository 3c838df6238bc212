"""arctic_bloom(_device), arctic_read_bloom and arctic_bloom_info on the device (needs an MI355X), against the numpy definition of
tests/bloom_reference.py BY BYTES, no pixel left out: the 2 L kernels on synthetic planes (NaN, infinite, negative and huge colours, sizes from
1 x 1 to 136 x 72 -- 5 x 3 workgroups of k_bloom_down_first's 16 x 16 at level 1 and 3 x 2 at level 2 -- at 1, 2, 5 and 8 levels, two records,
sentinels behind every plane), the tonemapped planes against the float64 post_process of the kernel's own `out`, the host form, the handle's
own output, warm calls, a resize, the counters and the refusals; and on the rasterised scene of tests/hit_scenes.py each source flag on a plane
of its own, the whole chain render -> anti-aliasing -> motion blur -> depth of field -> bloom, and a handle that never makes these calls."""
import ctypes as C

import numpy as np
import pytest

import bloom_reference as B
import compose_reference as CR
import hit_scenes
import test_bloom_reference as TR
import test_gpu_compose as TC
import test_gpu_motion as TM
import test_gpu_taa as TT

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SETTINGS = TT.SETTINGS
SIZE = TT.SIZE
GOOD = dict(TR.RECORDS[1], levels=3)


def read_planes(r, levels):
    """(ldr, (out, D, U)) of the latest call"""
    ldr, hdr, _, D, U = r.read_bloom(levels, want=("ldr", "hdr", "down", "up"))
    return ldr, (hdr, D, U)


def judge_tonemapped(what, ldr, rgba8, out, settings):
    """float LDR within the standing 1e-4 of the float64 post_process of the kernel's own `out`, RGBA8 within one step of that reference's
    quantisation, alpha 255: every pixel whose `out` is finite and inside the HDR range the record admits (|x| <= 65504: beyond some 1e19 the
    tonemapper's own fp32 squares overflow, which is no business of this stage)"""
    fine = (np.isfinite(out) & (np.abs(out) <= 65504.0)).all(-1)
    assert (rgba8[..., 3] == 255).all(), what
    if not fine.any():
        return
    want_ldr, want_rgba8 = CR.tonemap(np.where(fine[..., None], out, F(0.0)).astype(np.float64), settings)
    err = np.abs(ldr.astype(np.float64) - want_ldr)[fine].max()
    step = np.abs(rgba8.astype(np.int32) - want_rgba8.astype(np.int32))[fine].max()
    print(f"{what}: ldr {err:.3e}, rgba8 steps {step}, judged {fine.mean():.3f}")
    assert err <= TR.TOL and step <= 1, (what, float(err), int(step))


@pytest.mark.parametrize("width, height", TR.SIZES, ids=lambda v: str(v))
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, width, height):
    Cp = TR.case(width, height)
    n = width * height
    r = hip.Renderer(width, height, 64, 16)
    assert r.bloom_info() == (0, 0, 0, 0)
    d_c = TT.floats(Cp.copy())
    call = 0
    for L in TR.LEVELS:
        for rec in range(len(TR.RECORDS)):
            kw = TR.record_kw(rec, L)
            d_o = TT.bytes_on_device(n * 4)
            r.bloom_device(SETTINGS[call % 3], d_c.data_ptr(), d_o.data_ptr(), **kw)
            ldr, got = read_planes(r, L)
            TR.same_bloom(got, TR.reference(width, height, L, rec), (width, height, L, rec))
            got8 = d_o.cpu().numpy()
            assert (got8[n * 4:] == 77).all()                                    # sentinels behind the caller's output
            back = d_c.cpu().numpy()
            assert (back[Cp.size:] == TT.SENTINEL).all() and back[:Cp.size].tobytes() == Cp.tobytes()       # ... and the input is read only
            judge_tonemapped((width, height, L, rec), ldr, got8[:n * 4].reshape(height, width, 4), got[0], SETTINGS[call % 3])
            with pytest.raises(hip.ArcticError):                                 # the RGBA8 went to the caller's buffer
                r.read_bloom(L, want=("rgba8",))
            call += 1
    info = r.bloom_info()
    lay = pkg.renderer.bloom_layout(width, height, 8)
    assert info[1:] == (call, call, 0) and info[0] >= n * (12 + 12) + 4 * (lay["down_floats"] + lay["up_floats"])
    r.close()


def test_host_form_own_output_warm_calls_resize_and_counters(pkg, hip):
    width, height = TR.SIZES[4]
    Cp = TR.case(width, height)
    r = hip.Renderer(width, height, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_bloom(3)
    assert e.value.code == STATE                                                 # nothing yet
    kw = TR.record_kw(1, 5)
    first = r.bloom(SETTINGS[0], Cp, **kw)
    ldr, got = read_planes(r, 5)
    TR.same_bloom(got, TR.reference(width, height, 5, 1), "host form")
    rgba8 = r.read_bloom(5, want=("rgba8",))[2]
    assert first.tobytes() == rgba8.tobytes()
    judge_tonemapped("host form", ldr, rgba8, got[0], SETTINGS[0])
    assert r.bloom(SETTINGS[1], Cp, read=False, **kw) is None                    # a NULL output stays in the handle
    ldr, got = read_planes(r, 5)
    TR.same_bloom(got, TR.reference(width, height, 5, 1), "host form, own output")
    judge_tonemapped("host form, own output", ldr, r.read_bloom(5, want=("rgba8",))[2], got[0], SETTINGS[1])
    held = r.bloom_info()
    assert held[1:] == (2, 2, 0)
    r.bloom(SETTINGS[0], Cp, **kw)
    assert r.bloom_info() == (held[0], 3, 3, 0)                                  # a warm call allocates nothing
    r.bloom(SETTINGS[0], Cp, **TR.record_kw(0, 8))                               # ... nor does a second record: the pyramids are made for 8 levels
    assert r.bloom_info() == (held[0], 4, 4, 0)
    TR.same_bloom(read_planes(r, 8)[1], TR.reference(width, height, 8, 0), "a second record")
    r.bloom(SETTINGS[0], Cp, **TR.record_kw(0, 1))
    assert r.bloom_info() == (held[0], 5, 5, 0)
    TR.same_bloom(read_planes(r, 1)[1], TR.reference(width, height, 1, 0), "one level")
    # the device form into the handle's own output
    d_c = TT.floats(Cp.copy())
    r.bloom_device(SETTINGS[2], d_c.data_ptr(), None, **kw)
    ldr, got = read_planes(r, 5)
    TR.same_bloom(got, TR.reference(width, height, 5, 1), "device form, own output")
    judge_tonemapped("device form, own output", ldr, r.read_bloom(5, want=("rgba8",))[2], got[0], SETTINGS[2])
    # resize: nothing to read, then the new size
    r.resize(*TR.SIZES[3])
    with pytest.raises(hip.ArcticError) as e:
        r.read_bloom(5)
    assert e.value.code == STATE
    r.bloom(SETTINGS[0], TR.case(*TR.SIZES[3]), **kw)
    TR.same_bloom(read_planes(r, 5)[1], TR.reference(*TR.SIZES[3], 5, 1), "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    width, height = TR.SIZES[4]
    n = width * height
    Cp = TR.case(width, height)
    r = hip.Renderer(width, height, 64, 16)
    d_c, d_o = TT.floats(Cp.copy()), TT.bytes_on_device(n * 4)

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda c=d_c.data_ptr(), o=d_o.data_ptr(), **kw: r.bloom_device(SETTINGS[0], c, o, **dict(GOOD, **kw))
    for bad in (dict(flags=16), dict(flags=0x80000000), dict(flags=3), dict(flags=5), dict(flags=6), dict(flags=9), dict(flags=12), dict(flags=15), dict(threshold=-0.1),
                dict(threshold=65505.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(soft_knee=-0.1), dict(soft_knee=1.5), dict(soft_knee=np.nan), dict(clamp_max=0.0),
                dict(clamp_max=-1.0), dict(clamp_max=65505.0), dict(clamp_max=np.nan), dict(clamp_max=np.inf), dict(intensity=-0.1), dict(intensity=16.5), dict(intensity=np.nan),
                dict(spread=-0.1), dict(spread=1.5), dict(spread=np.nan), dict(levels=0), dict(levels=9)):
        refused(INVALID, lambda: go(**bad))
    reserved = pkg.renderer._bloom_arguments(0, 1.0, 0.5, 65504.0, 0.5, 1.0, 3)
    reserved["reserved"] = 1
    refused(INVALID, lambda: r.bloom_device(SETTINGS[0], d_c.data_ptr(), d_o.data_ptr(), bloom=reserved))
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer._bloom_arguments(0, 1.0, 0.5, 65504.0, 0.5, 1.0, 3)
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    assert r.L.arctic_bloom_device(r.h, None, hp(good), vp(d_c), None) == INVALID
    assert r.L.arctic_bloom_device(r.h, st, None, vp(d_c), None) == INVALID
    assert r.L.arctic_bloom(r.h, None, hp(good), None, None) == INVALID
    assert r.L.arctic_bloom_info(r.h, None) == INVALID
    # a NULL colour plane is the handle's own: it needs the float HDR plane and a shading, or a composition, a history, a blur, a lens
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    for flags in (B.SOURCE_COMPOSED, B.SOURCE_TAA, B.SOURCE_MOTION_BLUR, B.SOURCE_DOF):
        refused(STATE, lambda: go(c=None, flags=flags))
        refused(STATE, lambda: r.bloom(SETTINGS[0], None, **dict(GOOD, flags=flags)))
    assert r.bloom_info() == (0, 0, 0, 0)                                        # a refused call holds nothing
    # a shard is refused: the footprints' rows are elsewhere
    shard = hip.Renderer(width, height, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.bloom_device(SETTINGS[0], d_c.data_ptr(), d_o.data_ptr(), **GOOD)
    assert e.value.code == STATE and shard.bloom_info() == (0, 0, 0, 0)
    with pytest.raises(hip.ArcticError) as e:
        shard.read_bloom(3)
    assert e.value.code == STATE
    shard.close()
    # the planes are what the last good call left, the caller's buffers were never written by a refused call
    assert (d_o.cpu().numpy() == 77).all()
    go()
    refused(INVALID, lambda: go(levels=0))
    refused(INVALID, lambda: go(flags=3))
    refused(STATE, lambda: go(c=None))
    assert r.bloom_info()[1:] == (1, 1, 0)
    TR.same_bloom(read_planes(r, 3)[1], B.bloom(Cp, **GOOD), "after the refusals")
    assert (d_o.cpu().numpy()[n * 4:] == 77).all() and (d_c.cpu().numpy()[Cp.size:] == TT.SENTINEL).all()
    r.close()


# ---- the rasterised scene of the hit tests ----------------------------------------------------------------------------------------------------------
KW = dict(threshold=0.25, soft_knee=0.5, clamp_max=65504.0, intensity=0.8, spread=0.75, levels=4)
DOF_KW = dict(coc_scale=12.0, max_radius=8.0, samples=16, depth_extent=0.5)


def test_the_chain_and_four_sources(pkg, hip):
    """two frames, each: render, arctic_pass_taa, arctic_pass_motion_blur of the history, arctic_pass_dof of the blur -- then the shading's plane,
    the history, the blur's and the lens' outputs are four different planes, and bloom under no flag, ARCTIC_BLOOM_SOURCE_TAA, _MOTION_BLUR and
    _DOF reads each: numpy on the read-back plane, by bytes.  The last is the whole chain.  Every flag is refused while its plane does not exist,
    and after a resize; the stages in front keep their bytes and their counters"""
    import dof_reference as D
    import motion_blur_reference as M
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    zn, zf = (float(x) for x in descs[0].camera["z_near_far"])
    r = TT.lit_handle(pkg, hip)
    r.render_frame(descs[0], SETTINGS[0])
    for flags in (B.SOURCE_TAA, B.SOURCE_MOTION_BLUR, B.SOURCE_DOF, B.SOURCE_COMPOSED):
        with pytest.raises(hip.ArcticError) as e:
            r.bloom_device(SETTINGS[0], flags=flags, **KW)
        assert e.value.code == STATE and r.bloom_info() == (0, 0, 0, 0)
    for desc in descs:
        r.render_frame(desc, SETTINGS[0])
        r.pass_taa(desc, SETTINGS[0], max_history=4.0)
        r.pass_motion_blur(desc, SETTINGS[0], flags=M.SOURCE_TAA, shutter=1.0, max_radius=8.0, samples=7, depth_extent=0.05)
        r.pass_dof(desc, SETTINGS[0], flags=D.SOURCE_MOTION_BLUR, read=False, focus_distance=r.dof_focus_at(W // 2, H // 2, zn, zf), **DOF_KW)
    shaded, history, blurred = r.read_output(want=("hdr",))[1], r.read_taa(want=("hdr",))[1], r.read_motion_blur(want=("hdr",))[1]
    lens = r.read_dof(want=("hdr",))[1]
    assert (shaded != history).any() and (history != blurred).any() and (blurred != lens).any()
    before = r.motion_info(), r.taa_info(), r.motion_blur_info(), r.dof_info()
    for k, (flags, plane) in enumerate(((0, shaded), (B.SOURCE_TAA, history), (B.SOURCE_MOTION_BLUR, blurred), (B.SOURCE_DOF, lens))):
        r.bloom_device(SETTINGS[k % 3], flags=flags, **KW)
        ldr, got = read_planes(r, KW["levels"])
        TR.same_bloom(got, B.bloom(plane, **KW), ("source", flags))
        judge_tonemapped(("source", flags), ldr, r.read_bloom(KW["levels"], want=("rgba8",))[2], got[0], SETTINGS[k % 3])
        changed = (got[0] != plane).any(-1)
        print(f"source {flags}: {int(changed.sum())} of {W * H} pixels changed, the plane's largest value is {float(np.nanmax(plane)):.3f}")
        assert changed.sum() >= 50
    host = r.bloom(SETTINGS[0], None, flags=B.SOURCE_DOF, **KW)                   # the host form of the chain's last step
    assert host.tobytes() == r.read_bloom(KW["levels"], want=("rgba8",))[2].tobytes()
    TR.same_bloom(read_planes(r, KW["levels"])[1], B.bloom(lens, **KW), "the chain, host form")
    assert (r.motion_info(), r.taa_info(), r.motion_blur_info(), r.dof_info()) == before and r.bloom_info()[1:] == (5, 5, 0)    # it reads the stages in front of it, it moves none
    assert r.read_dof(want=("hdr",))[1].tobytes() == lens.tobytes() and r.read_motion_blur(want=("hdr",))[1].tobytes() == blurred.tobytes()
    assert r.read_taa(want=("hdr",))[1].tobytes() == history.tobytes() and r.read_output(want=("hdr",))[1].tobytes() == shaded.tobytes()
    r.resize(W + 8, H)
    for flags in (0, B.SOURCE_TAA, B.SOURCE_MOTION_BLUR, B.SOURCE_DOF):
        with pytest.raises(hip.ArcticError) as e:
            r.bloom_device(SETTINGS[0], flags=flags, **KW)
        assert e.value.code == STATE
    r.close()


def test_the_composed_source(pkg, hip):
    """ARCTIC_BLOOM_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane, the fifth plane"""
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    with pytest.raises(hip.ArcticError) as e:
        r.bloom_device(TC.SETTINGS, flags=B.SOURCE_COMPOSED, **KW)
    assert e.value.code == STATE and r.bloom_info() == (0, 0, 0, 0)              # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    held = r.compose_info()
    r.bloom_device(TC.SETTINGS, flags=B.SOURCE_COMPOSED, **KW)
    ldr, got = read_planes(r, KW["levels"])
    TR.same_bloom(got, B.bloom(composed, **KW), "composed")
    judge_tonemapped("composed source", ldr, r.read_bloom(KW["levels"], want=("rgba8",))[2], got[0], TC.SETTINGS)
    r.bloom_device(TC.SETTINGS, **KW)                                            # ... and without the flag the shading's plane
    TR.same_bloom(read_planes(r, KW["levels"])[1], B.bloom(shaded, **KW), "shaded")
    assert r.compose_info() == held and r.read_composed(want=("hdr",))[1].tobytes() == composed.tobytes()
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls, which reports zero bytes"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info(), a.dof_info()
    assert a.bloom_info() == (0, 0, 0, 0)
    a.bloom_device(TC.SETTINGS, **KW)
    a.bloom_device(TC.SETTINGS, **KW)
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info(), a.dof_info()) == held
    assert a.bloom_info()[1:] == (2, 2, 0)
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.bloom_info() == (0, 0, 0, 0)
    a.close(); b.close()
