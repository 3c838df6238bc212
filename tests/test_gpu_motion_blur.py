"""arctic_motion_blur(_device), arctic_depth_plane_device, arctic_pass_motion_blur, arctic_read_motion_blur and arctic_motion_blur_info on the
device (needs an MI355X), against the numpy definition of tests/motion_blur_reference.py BY BYTES, no pixel left out: the four kernels on
synthetic planes (velocities that are zero, below a pixel, beyond max_radius, NaN or infinite, NaN colours and depths, sentinels behind every
plane), the tonemapped planes against the float64 post_process of the kernel's own `out`, the host form, resize, the counters and the refusals;
and on the rasterised scene of tests/hit_scenes.py the depth plane, the one call against the calls by hand and against numpy, a moved box, the
composed source, the anti-aliasing's history as the source, and a handle that never makes these calls."""
import numpy as np
import pytest

import hit_scenes
import motion_blur_reference as M
import test_gpu_compose as TC
import test_gpu_motion as TM
import test_gpu_taa as TT
import test_motion_blur_reference as TR

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SETTINGS = TT.SETTINGS
SIZE = TT.SIZE
PLANES = ("hdr", "tile_max2", "neighbour_max2", "P")


def read_planes(r):
    """(ldr, (out, tile_max2, neighbour_max2, P)) of the latest call"""
    ldr, hdr, _, tile, near, P = r.read_motion_blur(want=("ldr", "hdr", "tile_max", "neighbour_max", "prepared"))
    return ldr, (hdr, tile, near, P)


def same_planes(got, want, what):
    for g, w, name in zip(got, want, PLANES):
        TR.same(g, w, (what, name))


@pytest.mark.parametrize("width, height", TR.SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "no depth"])
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, width, height, with_depth):
    rng = np.random.default_rng(9200 + width)
    C, v, z = TR.random_planes(rng, width, height)
    n = width * height
    r = hip.Renderer(width, height, 64, 16)
    assert r.motion_blur_info() == (0, 0, 0, 0)
    d_c, d_v, d_z = TT.floats(C), TT.floats(v), TT.floats(z)
    call = 0
    for flags in (0, M.DITHER):
        for samples in (1, 7, 15):
            kw = dict(samples=samples, flags=flags, max_radius=6.5 if samples == 7 else 16.0, shutter=0.5 if samples == 7 else 1.0, depth_extent=0.01 if flags else 0.05)
            d_o = TT.bytes_on_device(n * 4)
            r.motion_blur_device(SETTINGS[call % 3], d_c.data_ptr(), d_v.data_ptr(), d_z.data_ptr() if with_depth else None, d_o.data_ptr(), **kw)
            ldr, got = read_planes(r)
            want = M.blur(C, v, z if with_depth else None, **kw)
            same_planes(got, want, (width, height, with_depth, kw))
            got8 = d_o.cpu().numpy()
            assert (got8[n * 4:] == 77).all()                                    # sentinels behind every plane of the caller's
            for d, host in ((d_c, C), (d_v, v), (d_z, z)):
                back = d.cpu().numpy()
                assert (back[host.size:] == TT.SENTINEL).all() and back[:host.size].tobytes() == host.tobytes()   # ... and the inputs are read only
            TT.judge_tonemapped((width, height, with_depth, samples, flags), ldr, got8[:n * 4].reshape(height, width, 4), got[0], SETTINGS[call % 3], least=0.75)
            with pytest.raises(hip.ArcticError):                                 # the RGBA8 went to the caller's buffer
                r.read_motion_blur(want=("rgba8",))
            call += 1
    info = r.motion_blur_info()
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    assert info[1:] == (6, 6, 0) and info[0] >= n * (8 + 12 + 12) + 2 * tiles * 8
    r.close()


def test_host_form_own_output_resize_and_counters(pkg, hip):
    width, height = TR.SIZES[1]
    rng = np.random.default_rng(9300)
    C, v, z = TR.random_planes(rng, width, height)
    kw = dict(samples=7, max_radius=8.0)
    r = hip.Renderer(width, height, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_motion_blur()
    assert e.value.code == STATE                                                 # nothing blurred yet
    first = r.motion_blur(SETTINGS[0], C, v, z, **kw)
    ldr, got = read_planes(r)
    same_planes(got, M.blur(C, v, z, **kw), "host form")
    rgba8 = r.read_motion_blur(want=("rgba8",))[2]
    assert first.tobytes() == rgba8.tobytes()
    TT.judge_tonemapped("host form", ldr, rgba8, got[0], SETTINGS[0], least=0.75)
    assert r.motion_blur(SETTINGS[1], C, v, None, read=False, **kw) is None      # a NULL depth is 0 everywhere, a NULL output stays in the handle
    ldr, got = read_planes(r)
    same_planes(got, M.blur(C, v, None, **kw), "host form, no depth")
    TT.judge_tonemapped("host form, no depth", ldr, r.read_motion_blur(want=("rgba8",))[2], got[0], SETTINGS[1], least=0.75)
    held = r.motion_blur_info()
    assert held[1:] == (2, 2, 0)
    r.motion_blur(SETTINGS[0], C, v, z, **kw)
    assert r.motion_blur_info() == (held[0], 3, 3, 0)                            # a warm call allocates nothing
    # resize: nothing to read, then the new size
    r.resize(*TR.SIZES[0])
    with pytest.raises(hip.ArcticError) as e:
        r.read_motion_blur()
    assert e.value.code == STATE
    C, v, z = TR.random_planes(rng, *TR.SIZES[0])
    r.motion_blur(SETTINGS[0], C, v, z, **kw)
    same_planes(read_planes(r)[1], M.blur(C, v, z, **kw), "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    import ctypes as C
    width, height = TR.SIZES[1]
    n = width * height
    rng = np.random.default_rng(9400)
    cur, vel, z = TR.random_planes(rng, width, height)
    r = hip.Renderer(width, height, 64, 16)
    d_c, d_v, d_z, d_o = TT.floats(cur), TT.floats(vel), TT.floats(z), TT.bytes_on_device(n * 4)

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda c=d_c.data_ptr(), v=d_v.data_ptr(), zz=d_z.data_ptr(), o=d_o.data_ptr(), **kw: r.motion_blur_device(SETTINGS[0], c, v, zz, o, **kw)
    for bad in (dict(flags=8), dict(flags=0x80000000), dict(flags=M.SOURCE_COMPOSED | M.SOURCE_TAA), dict(shutter=-0.1), dict(shutter=4.5), dict(shutter=np.nan), dict(shutter=np.inf),
                dict(max_radius=0.5), dict(max_radius=64.5), dict(max_radius=np.nan), dict(samples=0), dict(samples=65), dict(depth_extent=0.0), dict(depth_extent=-1.0),
                dict(depth_extent=np.nan), dict(depth_extent=np.inf)):
        refused(INVALID, lambda: go(**bad))
    m = pkg.renderer._motion_blur_arguments(0, 1.0, 16.0, 15, 0.05)
    m["reserved"][0, 2] = 1
    refused(INVALID, lambda: go(mb=m))
    refused(INVALID, lambda: go(v=None))                                         # velocity2 is required
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(v=d_v.data_ptr() + 4))
    refused(INVALID, lambda: go(zz=d_z.data_ptr() + 2))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    refused(INVALID, lambda: r.depth_plane_device(None))
    refused(INVALID, lambda: r.depth_plane_device(d_z.data_ptr() + 2))
    refused(STATE, lambda: r.depth_plane_device(d_z.data_ptr()))                 # no visibility plane
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer._motion_blur_arguments(0, 1.0, 16.0, 15, 0.05)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert r.L.arctic_motion_blur_device(r.h, None, C.c_void_p(good.ctypes.data), vp(d_c), vp(d_v), None, None) == INVALID
    assert r.L.arctic_motion_blur_device(r.h, st, None, vp(d_c), vp(d_v), None, None) == INVALID
    assert r.L.arctic_motion_blur(r.h, st, C.c_void_p(good.ctypes.data), None, None, None, None) == INVALID
    # a NULL colour plane is the handle's own: it needs the float HDR plane and a shading, or a composition, or a history
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    refused(STATE, lambda: go(c=None, flags=M.SOURCE_COMPOSED))
    refused(STATE, lambda: go(c=None, flags=M.SOURCE_TAA))                       # T is empty
    refused(STATE, lambda: r.pass_motion_blur(TC.scene(pkg, width, height), SETTINGS[0]))   # no visibility plane either
    assert r.motion_blur_info() == (0, 0, 0, 0)                                  # a refused call holds nothing
    # a shard is refused: the taps' rows are elsewhere
    shard = hip.Renderer(width, height, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.motion_blur_device(SETTINGS[0], d_c.data_ptr(), d_v.data_ptr(), None, d_o.data_ptr())
    assert e.value.code == STATE and shard.motion_blur_info() == (0, 0, 0, 0)
    shard.close()
    # the planes are what the last good call left, the caller's buffers were never written
    go(samples=7)
    refused(INVALID, lambda: go(samples=0))
    refused(STATE, lambda: go(c=None))
    assert r.motion_blur_info()[1:] == (1, 1, 0)
    same_planes(read_planes(r)[1], M.blur(cur, vel, z, samples=7), "after the refusals")
    assert (d_o.cpu().numpy()[n * 4:] == 77).all() and (d_z.cpu().numpy()[n:] == TT.SENTINEL).all()
    r.close()


# ---- the rasterised scene of the hit tests --------------------------------------------------------------------------------------------------------
KW = dict(shutter=1.0, max_radius=8.0, samples=7, depth_extent=0.05)


def test_the_depth_plane_the_one_call_the_calls_by_hand_and_numpy(pkg, hip):
    """two frames -- the scene, then the scene with a box moved -- through arctic_pass_motion_blur on one handle and through motion vectors +
    depth plane + blur by hand on a second: byte for byte the same planes, and numpy on the read-back HDR frame, velocity and depth; the moved
    box's pixels change; on a still scene (a third frame) the HDR plane is copied"""
    import torch
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    one, hand = TT.lit_handle(pkg, hip), TT.lit_handle(pkg, hip)
    d_pw = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    d_vel = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda")
    d_z = TT.floats(np.zeros((H, W), F))
    torch.cuda.synchronize()
    for k, desc in enumerate(descs):
        for r in (one, hand):
            r.render_frame(desc, SETTINGS[0])
        rgba8 = one.pass_motion_blur(desc, SETTINGS[0], **KW)
        hand.motion_vectors_device(desc, d_pw.data_ptr(), d_vel.data_ptr())
        hand.depth_plane_device(d_z.data_ptr())
        hand.motion_blur_device(SETTINGS[0], None, d_vel.data_ptr(), d_z.data_ptr(), None, **KW)
        got, want = one.read_motion_blur(), hand.read_motion_blur()
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), (k, int((a != b).sum()))
        assert rgba8.tobytes() == want[2].tobytes()
        depth = hand.read_gbuffer(want=("depth",))[2]
        back = d_z.cpu().numpy()
        assert back[:W * H].tobytes() == depth.tobytes() and (back[W * H:] == TT.SENTINEL).all()      # arctic_read_gbuffer's depth by bytes
        assert (depth == 1.0).any() and (depth < 1.0).sum() >= 300
        hdr, vel = hand.read_output(want=("hdr",))[1], d_vel.cpu().numpy()
        ref = M.blur(hdr, vel, depth, **KW)
        same_planes((got[1], got[3], got[4], got[5]), ref, ("numpy", k))
        TT.judge_tonemapped(("chain", k), got[0], got[2], got[1], SETTINGS[0])
        moving = np.abs(vel).max(-1) > 0.5
        changed = (got[1] != hdr).any(-1)
        print(f"frame {k}: {int(moving.sum())} pixels move by more than half a pixel, {int(changed.sum())} pixels changed")
        if k == 1:
            assert moving.sum() >= 50 and changed[moving].mean() >= 0.5           # the moved box is smeared
        else:
            assert not moving.any() and got[1].tobytes() == hdr.tobytes()        # a still scene is copied, bit for bit
    assert one.motion_blur_info()[1:] == (3, 3, 0) and one.motion_info()[1:] == (3, 0, 3)
    one.close(); hand.close()


def test_the_composed_source(pkg, hip):
    """ARCTIC_MB_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane"""
    import torch
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    H, W = r.rows, r.width
    vel = np.zeros((H, W, 2), F)
    vel[:, : W // 2] = (7.0, -3.0)
    d_v = TT.floats(vel)
    with pytest.raises(hip.ArcticError) as e:
        r.motion_blur_device(TC.SETTINGS, None, d_v.data_ptr(), flags=M.SOURCE_COMPOSED, **KW)
    assert e.value.code == STATE and r.motion_blur_info() == (0, 0, 0, 0)        # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    r.motion_blur_device(TC.SETTINGS, None, d_v.data_ptr(), flags=M.SOURCE_COMPOSED, **KW)
    ldr, got = read_planes(r)
    same_planes(got, M.blur(composed, vel, None, **KW), "composed")
    TT.judge_tonemapped("composed source", ldr, r.read_motion_blur(want=("rgba8",))[2], got[0], TC.SETTINGS)
    r.motion_blur_device(TC.SETTINGS, None, d_v.data_ptr(), **KW)                 # ... and without the flag the shading's plane
    same_planes(read_planes(r)[1], M.blur(shaded, vel, None, **KW), "shaded")
    r.close()


def test_the_history_as_the_source_behind_pass_taa(pkg, hip):
    """render, arctic_pass_taa, arctic_pass_motion_blur with ARCTIC_MB_SOURCE_TAA: no second motion call, C is T, the velocity is the one
    arctic_pass_taa left; refused after a resolve made by hand, after a reset and without any resolve"""
    import torch
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    r, hand = TT.lit_handle(pkg, hip), TT.lit_handle(pkg, hip)
    d_pw = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    d_vel = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(flags=M.SOURCE_TAA, **KW)
    r.render_frame(descs[0], SETTINGS[0])
    with pytest.raises(hip.ArcticError) as e:
        r.pass_motion_blur(descs[0], SETTINGS[0], **kw)
    assert e.value.code == STATE and r.motion_blur_info() == (0, 0, 0, 0)        # T is empty
    for k, desc in enumerate(descs):
        for x in (r, hand):
            x.render_frame(desc, SETTINGS[0])
        r.pass_taa(desc, SETTINGS[0], max_history=4.0)
        hand.motion_vectors_device(desc, d_pw.data_ptr(), d_vel.data_ptr())      # the same velocity, on a handle whose planes can be read
        before = r.motion_info()
        r.pass_motion_blur(desc, SETTINGS[0], **kw)
        assert r.motion_info() == before                                         # no motion call
        _, t, _, _ = r.read_taa(want=("hdr",))
        vel, depth = d_vel.cpu().numpy(), r.read_gbuffer(want=("depth",))[2]
        ldr, got = read_planes(r)
        same_planes(got, M.blur(t, vel, depth, **KW), ("history", k))
        TT.judge_tonemapped(("history", k), ldr, r.read_motion_blur(want=("rgba8",))[2], got[0], SETTINGS[0])
    assert (np.abs(vel).max(-1) > 0.5).sum() >= 50 and (got[0] != t).any()
    held = r.motion_blur_info()
    # the device form takes T with a velocity of the caller's
    r.motion_blur_device(SETTINGS[0], None, d_vel.data_ptr(), None, None, **kw)
    same_planes(read_planes(r)[1], M.blur(t, vel, None, **KW), "history, by hand")
    # a resolve made by hand leaves no velocity of this frame in the handle
    r.taa_resolve_device(SETTINGS[0], None, d_vel.data_ptr(), None, max_history=4.0)
    with pytest.raises(hip.ArcticError) as e:
        r.pass_motion_blur(descs[1], SETTINGS[0], **kw)
    assert e.value.code == STATE
    r.pass_taa(descs[1], SETTINGS[0], max_history=4.0)
    r.pass_motion_blur(descs[1], SETTINGS[0], **kw)
    r.taa_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.pass_motion_blur(descs[1], SETTINGS[0], **kw)
    assert e.value.code == STATE and r.motion_blur_info() == (held[0], held[1] + 2, held[2] + 2, 0)
    r.close(); hand.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls, which reports zero bytes"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info()
    assert a.motion_blur_info() == (0, 0, 0, 0)
    a.pass_motion_blur(desc, TC.SETTINGS, **KW)
    a.pass_motion_blur(desc, TC.SETTINGS, **KW)
    assert a.read_motion_blur(want=("hdr",))[1].tobytes() == a.read_output(want=("hdr",))[1].tobytes()      # a still scene: copied
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.taa_info()) == held and a.motion_blur_info()[1:] == (2, 2, 0)
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.motion_blur_info() == (0, 0, 0, 0)
    a.close(); b.close()
