"""arctic_dof(_device), arctic_pass_dof, arctic_read_dof, arctic_dof_info and arctic_dof_focus_at on the device (needs an MI355X), against the
numpy definition of tests/dof_reference.py BY BYTES, no pixel left out: the three kernels on synthetic planes (depths 0, 1.0, beyond 1 and NaN,
regions of one depth each, a focus plane inside the scene, NaN colours, coc_scale = 0, sentinels behind every plane), the tonemapped planes
against the float64 post_process of the kernel's own `out`, the host form, resize, the counters and the refusals; and on the rasterised scene of
tests/hit_scenes.py the one call against the calls by hand and against numpy, the autofocus against the read-back depth, each of the three
source flags, and a handle that never makes these calls."""
import ctypes as C

import numpy as np
import pytest

import dof_reference as D
import hit_scenes
import test_dof_reference as TR
import test_gpu_compose as TC
import test_gpu_motion as TM
import test_gpu_taa as TT

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SETTINGS = TT.SETTINGS
SIZE = TT.SIZE
PLANES = ("hdr", "tile_max", "neighbour_max", "P")
BLOCKS = (dict(TR.CAMERA), dict(TR.CAMERA, max_radius=6.5, coc_scale=20.0, depth_extent=0.05))


def read_planes(r):
    """(ldr, (out, tile_max, neighbour_max, P)) of the latest call"""
    ldr, hdr, _, tile, near, P = r.read_dof(want=("ldr", "hdr", "tile_max", "neighbour_max", "prepared"))
    return ldr, (hdr, tile, near, P)


def same_planes(got, want, what):
    for g, w, name in zip(got, want, PLANES):
        TR.same(g, w, (what, name))


@pytest.mark.parametrize("width, height", TR.SIZES, ids=lambda v: str(v))
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, width, height):
    rng = np.random.default_rng(9700 + width)
    Cp, z = TR.random_planes(rng, width, height)
    n = width * height
    r = hip.Renderer(width, height, 64, 16)
    assert r.dof_info() == (0, 0, 0, 0)
    d_c, d_z = TT.floats(Cp), TT.floats(z)
    call = 0
    for block in BLOCKS:
        for samples in (1, 16, 48):
            kw = dict(block, samples=samples)
            d_o = TT.bytes_on_device(n * 4)
            r.dof_device(SETTINGS[call % 3], d_c.data_ptr(), d_z.data_ptr(), None, d_o.data_ptr(), **kw)
            ldr, got = read_planes(r)
            same_planes(got, D.dof(Cp, z, **kw), (width, height, kw))
            got8 = d_o.cpu().numpy()
            assert (got8[n * 4:] == 77).all()                                    # sentinels behind every plane of the caller's
            for d, host in ((d_c, Cp), (d_z, z)):
                back = d.cpu().numpy()
                assert (back[host.size:] == TT.SENTINEL).all() and back[:host.size].tobytes() == host.tobytes()   # ... and the inputs are read only
            TT.judge_tonemapped((width, height, kw), ldr, got8[:n * 4].reshape(height, width, 4), got[0], SETTINGS[call % 3], least=0.75)
            with pytest.raises(hip.ArcticError):                                 # the RGBA8 went to the caller's buffer
                r.read_dof(want=("rgba8",))
            call += 1
    # coc_scale = 0: a copy; and a table of the caller's
    r.dof_device(SETTINGS[0], d_c.data_ptr(), d_z.data_ptr(), None, None, **dict(TR.CAMERA, coc_scale=0.0))
    same_planes(read_planes(r)[1], D.dof(Cp, z, **dict(TR.CAMERA, coc_scale=0.0)), "coc_scale 0")
    assert np.nan_to_num(read_planes(r)[1][0], nan=-1.0).tobytes() == np.nan_to_num(Cp, nan=-1.0).tobytes()
    taps2 = rng.uniform(-0.7, 0.7, (7, 2)).astype(F)
    r.dof_device(SETTINGS[0], d_c.data_ptr(), d_z.data_ptr(), taps2, None, samples=7, **TR.CAMERA)
    same_planes(read_planes(r)[1], D.dof(Cp, z, taps2, samples=7, **TR.CAMERA), "the caller's table")
    info = r.dof_info()
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    assert info[1:] == (8, 8, 0) and info[0] >= n * (8 + 12 + 12) + 2 * tiles * 4 + 64 * 8
    r.close()


def test_host_form_own_output_resize_and_counters(pkg, hip):
    width, height = TR.SIZES[1]
    rng = np.random.default_rng(9800)
    Cp, z = TR.random_planes(rng, width, height)
    kw = dict(TR.CAMERA, samples=16, max_radius=8.0)
    r = hip.Renderer(width, height, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_dof()
    assert e.value.code == STATE                                                 # nothing yet
    first = r.dof(SETTINGS[0], Cp, z, **kw)
    ldr, got = read_planes(r)
    same_planes(got, D.dof(Cp, z, **kw), "host form")
    rgba8 = r.read_dof(want=("rgba8",))[2]
    assert first.tobytes() == rgba8.tobytes()
    TT.judge_tonemapped("host form", ldr, rgba8, got[0], SETTINGS[0], least=0.75)
    assert r.dof(SETTINGS[1], Cp, z, read=False, **kw) is None                   # a NULL output stays in the handle
    ldr, got = read_planes(r)
    same_planes(got, D.dof(Cp, z, **kw), "host form, own output")
    TT.judge_tonemapped("host form, own output", ldr, r.read_dof(want=("rgba8",))[2], got[0], SETTINGS[1], least=0.75)
    held = r.dof_info()
    assert held[1:] == (2, 2, 0)
    r.dof(SETTINGS[0], Cp, z, **kw)
    assert r.dof_info() == (held[0], 3, 3, 0)                                    # a warm call allocates nothing
    r.dof(SETTINGS[0], Cp, z, **dict(kw, samples=48))                            # ... nor does another table: the slot is made for the largest
    assert r.dof_info() == (held[0], 4, 4, 0)
    same_planes(read_planes(r)[1], D.dof(Cp, z, **dict(kw, samples=48)), "another table")
    # resize: nothing to read, then the new size
    r.resize(*TR.SIZES[0])
    with pytest.raises(hip.ArcticError) as e:
        r.read_dof()
    assert e.value.code == STATE
    Cp, z = TR.random_planes(rng, *TR.SIZES[0])
    r.dof(SETTINGS[0], Cp, z, **kw)
    same_planes(read_planes(r)[1], D.dof(Cp, z, **kw), "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    width, height = TR.SIZES[1]
    n = width * height
    rng = np.random.default_rng(9900)
    cur, z = TR.random_planes(rng, width, height)
    r = hip.Renderer(width, height, 64, 16)
    d_c, d_z, d_o = TT.floats(cur), TT.floats(z), TT.bytes_on_device(n * 4)

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda c=d_c.data_ptr(), zz=d_z.data_ptr(), o=d_o.data_ptr(), taps=None, **kw: r.dof_device(SETTINGS[0], c, zz, taps, o, **dict(TR.CAMERA, **kw))
    for bad in (dict(flags=8), dict(flags=0x80000000), dict(flags=3), dict(flags=5), dict(flags=6), dict(flags=7), dict(focus_distance=0.0), dict(focus_distance=np.nan),
                dict(focus_distance=np.inf), dict(coc_scale=-0.1), dict(coc_scale=4096.5), dict(coc_scale=np.nan), dict(max_radius=0.5), dict(max_radius=64.5), dict(max_radius=np.nan),
                dict(samples=0), dict(samples=65), dict(depth_extent=0.0), dict(depth_extent=-1.0), dict(depth_extent=np.nan), dict(depth_extent=np.inf), dict(z_near=0.0),
                dict(z_near=np.nan), dict(z_far=0.25), dict(z_far=np.inf), dict(z_near=0.0, z_far=0.0)):
        refused(INVALID, lambda: go(**bad))
    refused(INVALID, lambda: go(zz=None))                                        # the depth is required
    for taps in ([[np.nan, 0.0]], [[0.0, -np.inf]], [[0.8, 0.8]]):
        refused(INVALID, lambda: go(taps=taps, samples=1))
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(zz=d_z.data_ptr() + 2))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer._dof_arguments(0, 5.0, 8.0, 16.0, 16, 0.5, 0.5, 50.0)
    table = pkg.renderer.dof_taps(16)
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    assert r.L.arctic_dof_device(r.h, None, hp(good), vp(d_c), vp(d_z), hp(table), None) == INVALID
    assert r.L.arctic_dof_device(r.h, st, None, vp(d_c), vp(d_z), hp(table), None) == INVALID
    assert r.L.arctic_dof_device(r.h, st, hp(good), vp(d_c), vp(d_z), None, None) == INVALID          # a null table
    assert r.L.arctic_dof(r.h, st, hp(good), None, None, hp(table), None) == INVALID
    out = C.c_float(-7.0)
    assert r.L.arctic_dof_focus_at(r.h, 0.5, 50.0, 0, 0, None) == INVALID
    assert r.L.arctic_dof_focus_at(r.h, 0.0, 50.0, 0, 0, C.byref(out)) == INVALID and r.L.arctic_dof_focus_at(r.h, 0.5, 0.5, 0, 0, C.byref(out)) == INVALID
    assert r.L.arctic_dof_focus_at(r.h, 0.5, 50.0, width, 0, C.byref(out)) == INVALID and r.L.arctic_dof_focus_at(r.h, 0.5, 50.0, 0, height, C.byref(out)) == INVALID
    assert r.L.arctic_dof_focus_at(r.h, 0.5, 50.0, 0, 0, C.byref(out)) == STATE and out.value == -7.0  # no visibility plane
    # a NULL colour plane is the handle's own: it needs the float HDR plane and a shading, or a composition, a history, a blur
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    refused(STATE, lambda: go(c=None, flags=D.SOURCE_COMPOSED))
    refused(STATE, lambda: go(c=None, flags=D.SOURCE_TAA))                       # T is empty
    refused(STATE, lambda: go(c=None, flags=D.SOURCE_MOTION_BLUR))               # nothing blurred
    desc = TC.scene(pkg, width, height)
    refused(STATE, lambda: r.pass_dof(desc, SETTINGS[0]))                        # no visibility plane either
    refused(INVALID, lambda: r.pass_dof(desc, SETTINGS[0], dof=pkg.renderer._dof_arguments(0, 5.0, 8.0, 16.0, 16, 0.5, 0.5, 50.0)))   # the one call takes the scene's planes
    assert r.dof_info() == (0, 0, 0, 0)                                          # a refused call holds nothing
    # a shard is refused: the taps' rows are elsewhere
    shard = hip.Renderer(width, height, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.dof_device(SETTINGS[0], d_c.data_ptr(), d_z.data_ptr(), None, d_o.data_ptr(), **TR.CAMERA)
    assert e.value.code == STATE and shard.dof_info() == (0, 0, 0, 0)
    shard.close()
    # the planes are what the last good call left, the caller's buffers were never written by a refused call
    assert (d_o.cpu().numpy() == 77).all()
    go(samples=16)
    refused(INVALID, lambda: go(samples=0))
    refused(INVALID, lambda: go(taps=[[0.8, 0.8]], samples=1))
    refused(STATE, lambda: go(c=None))
    assert r.dof_info()[1:] == (1, 1, 0)
    same_planes(read_planes(r)[1], D.dof(cur, z, samples=16, **TR.CAMERA), "after the refusals")
    assert (d_o.cpu().numpy()[n * 4:] == 77).all() and (d_z.cpu().numpy()[n:] == TT.SENTINEL).all()
    r.close()


# ---- the rasterised scene of the hit tests ----------------------------------------------------------------------------------------------------------
KW = dict(coc_scale=12.0, max_radius=8.0, samples=16, depth_extent=0.5)


def test_the_one_call_the_calls_by_hand_numpy_and_the_autofocus(pkg, hip):
    """a frame through arctic_pass_dof on one handle and through depth plane + gather by hand on a second: byte for byte the same planes, and
    numpy on the read-back HDR frame and depth under the scene's camera planes; arctic_dof_focus_at equals step 1's zv of the read-back depth,
    on geometry and on the sky; focused on the middle of the frame the scene has pixels in front of the focus plane and behind it"""
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    desc = TM.hit_desc(pkg, g.objects, SIZE)
    zn, zf = (float(x) for x in desc.camera["z_near_far"])
    one, hand = TT.lit_handle(pkg, hip), TT.lit_handle(pkg, hip)
    d_z = TT.floats(np.zeros((H, W), F))
    for r in (one, hand):
        r.render_frame(desc, SETTINGS[0])
    depth = hand.read_gbuffer(want=("depth",))[2]
    assert (depth == 1.0).any() and (depth < 1.0).sum() >= 300
    zv = D.view_distance(depth, zn, zf)
    sky, solid = np.argwhere(depth == 1.0)[0], np.argwhere(depth < 1.0)
    for y, x in [tuple(sky), (H // 2, W // 2), (0, 0), (H - 1, W - 1)] + [tuple(p) for p in solid[:: max(len(solid) // 6, 1)]]:
        assert F(hand.dof_focus_at(x, y, zn, zf)) == zv[y, x], (x, y)
    forward = zf / (zf - zn) * (1.0 - zn / zv.astype(np.float64))                # the camera's projection, forward: the header's inverse inverts it
    assert np.abs(forward - depth)[depth < 1.0].max() <= 1e-6
    # ... and zv IS the distance along the view axis of what the camera drew: the G-buffer's world position of every pixel against the eye and
    # the forward axis, in float64.  The depth's rounding, 2^-24 * (zf - zn) against den = zn * zf / zv, is 6e-7 * zv relative here, and the
    # world position is fp32 as well: some 1e-5 at these distances.  1e-3 is far above that and far below a wrong projection
    world = hand.read_gbuffer(want=("attrs",))[0][..., 11:14].astype(np.float64)
    xr, yr = np.radians(np.asarray(desc.camera["rotation"], np.float64))
    axis = np.array([np.cos(xr) * np.cos(yr), np.sin(xr), np.cos(xr) * np.sin(yr)])
    along = (world - np.asarray(desc.camera["eye"], np.float64)) @ axis
    rel = (np.abs(zv - along) / along)[depth < 1.0]
    print(f"view distance against the drawn geometry: the largest relative difference is {rel.max():.2e}, distances {along[depth < 1.0].min():.2f} to {along[depth < 1.0].max():.2f}")
    assert rel.max() <= 1e-3
    focus = hand.dof_focus_at(W // 2, H // 2, zn, zf)
    kw = dict(KW, focus_distance=focus)
    rgba8 = one.pass_dof(desc, SETTINGS[0], **kw)
    hand.depth_plane_device(d_z.data_ptr())
    hand.dof_device(SETTINGS[0], None, d_z.data_ptr(), None, None, z_near=zn, z_far=zf, **kw)
    got, want = one.read_dof(), hand.read_dof()
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes(), int((a != b).sum())
    assert rgba8.tobytes() == want[2].tobytes()
    back = d_z.cpu().numpy()
    assert back[:W * H].tobytes() == depth.tobytes() and (back[W * H:] == TT.SENTINEL).all()
    hdr = hand.read_output(want=("hdr",))[1]
    same_planes((got[1], got[3], got[4], got[5]), D.dof(hdr, depth, z_near=zn, z_far=zf, **kw), "numpy")
    TT.judge_tonemapped("the one call", got[0], got[2], got[1], SETTINGS[0])
    s = got[5][..., 0]
    changed = (got[1] != hdr).any(-1)
    print(f"focus at {focus:.3f}: {int((s < -0.5).sum())} pixels in front of the focus plane by more than half a pixel, {int((s > 0.5).sum())} behind, {int(changed.sum())} changed")
    assert (s > 0.5).sum() >= 50 and changed.sum() >= 50 and s[H // 2, W // 2] == 0.0
    assert one.dof_info()[1:] == (1, 1, 0)
    one.close(); hand.close()


def test_the_three_source_flags(pkg, hip):
    """two frames, each: render, arctic_pass_taa, arctic_pass_motion_blur of the history -- then the shading's plane, the history and the blur's
    output are three different planes, and arctic_pass_dof under no flag, ARCTIC_DOF_SOURCE_TAA and ARCTIC_DOF_SOURCE_MOTION_BLUR gathers each;
    each flag is refused while its plane does not exist, and the blur's after a resize"""
    import motion_blur_reference as M
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    zn, zf = (float(x) for x in descs[0].camera["z_near_far"])
    r = TT.lit_handle(pkg, hip)
    r.render_frame(descs[0], SETTINGS[0])
    for flags in (D.SOURCE_TAA, D.SOURCE_MOTION_BLUR, D.SOURCE_COMPOSED):
        with pytest.raises(hip.ArcticError) as e:
            r.pass_dof(descs[0], SETTINGS[0], flags=flags, **KW)
        assert e.value.code == STATE and r.dof_info() == (0, 0, 0, 0)
    for desc in descs:
        r.render_frame(desc, SETTINGS[0])
        r.pass_taa(desc, SETTINGS[0], max_history=4.0)
        r.pass_motion_blur(desc, SETTINGS[0], flags=M.SOURCE_TAA, shutter=1.0, max_radius=8.0, samples=7, depth_extent=0.05)
    shaded, history, blurred = r.read_output(want=("hdr",))[1], r.read_taa(want=("hdr",))[1], r.read_motion_blur(want=("hdr",))[1]
    assert (shaded != history).any() and (history != blurred).any()
    depth = r.read_gbuffer(want=("depth",))[2]
    kw = dict(KW, focus_distance=r.dof_focus_at(W // 2, H // 2, zn, zf))
    before = r.motion_info(), r.taa_info(), r.motion_blur_info()
    for flags, plane in ((0, shaded), (D.SOURCE_TAA, history), (D.SOURCE_MOTION_BLUR, blurred)):
        r.pass_dof(descs[1], SETTINGS[0], flags=flags, read=False, **kw)
        ldr, got = read_planes(r)
        same_planes(got, D.dof(plane, depth, z_near=zn, z_far=zf, **kw), ("source", flags))
        TT.judge_tonemapped(("source", flags), ldr, r.read_dof(want=("rgba8",))[2], got[0], SETTINGS[0])
        assert (got[0] != plane).any()
    assert (r.motion_info(), r.taa_info(), r.motion_blur_info()) == before and r.dof_info()[1:] == (3, 3, 0)   # it reads the stages in front of it, it moves none
    assert r.read_motion_blur(want=("hdr",))[1].tobytes() == blurred.tobytes()
    r.resize(W + 8, H)
    with pytest.raises(hip.ArcticError) as e:
        r.pass_dof(descs[1], SETTINGS[0], flags=D.SOURCE_MOTION_BLUR, **kw)
    assert e.value.code == STATE
    r.close()


def test_the_composed_source(pkg, hip):
    """ARCTIC_DOF_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane"""
    desc = TC.scene(pkg)
    zn, zf = (float(x) for x in desc.camera["z_near_far"])
    r = TC.handle(pkg, hip, TC.images())
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    kw = dict(KW, focus_distance=r.dof_focus_at(r.width // 2, r.rows // 2, zn, zf))
    with pytest.raises(hip.ArcticError) as e:
        r.pass_dof(desc, TC.SETTINGS, flags=D.SOURCE_COMPOSED, **kw)
    assert e.value.code == STATE and r.dof_info() == (0, 0, 0, 0)                # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    depth = r.read_gbuffer(want=("depth",))[2]
    r.pass_dof(desc, TC.SETTINGS, flags=D.SOURCE_COMPOSED, read=False, **kw)
    ldr, got = read_planes(r)
    same_planes(got, D.dof(composed, depth, z_near=zn, z_far=zf, **kw), "composed")
    TT.judge_tonemapped("composed source", ldr, r.read_dof(want=("rgba8",))[2], got[0], TC.SETTINGS)
    r.pass_dof(desc, TC.SETTINGS, read=False, **kw)                              # ... and without the flag the shading's plane
    same_planes(read_planes(r)[1], D.dof(shaded, depth, z_near=zn, z_far=zf, **kw), "shaded")
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls, which reports zero bytes"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info()
    assert a.dof_info() == (0, 0, 0, 0)
    a.pass_dof(desc, TC.SETTINGS, **KW)
    a.pass_dof(desc, TC.SETTINGS, **KW)
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info(), a.motion_blur_info(), a.motion_info()) == held and a.dof_info()[1:] == (2, 2, 0)
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.dof_info() == (0, 0, 0, 0)
    a.close(); b.close()
