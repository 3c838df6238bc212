"""arctic_set_camera_jitter, arctic_taa_resolve(_device), arctic_pass_taa, arctic_taa_reset / _info and arctic_read_taa on the device (needs an
MI355X), against the numpy definition of tests/taa_reference.py BY BYTES, no pixel left out: k_taa_resolve on synthetic planes (velocities that
point outside the frame or are not finite, NaN colours, sentinels behind every plane), its tonemapped planes against the float64 post_process of
its own `out`, the host form, reset, resize, the counters and the refusals; the jitter on the rasterised scene of tests/hit_scenes.py; and the
whole chain: eight jittered frames through arctic_pass_taa against the calls by hand and against numpy on the read-back planes, a moved box with
and without velocity2, the composed source, and a handle that never makes these calls."""
import numpy as np
import pytest

import compose_reference as CR
import hit_scenes
import taa_reference as T
import test_gpu_compose as TC
import test_gpu_extended_shading as G
import test_gpu_motion as TM

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SENTINEL = F(-77.0)
PAD = 16
SIZES = ((8, 8), (17, 9), (40, 24))              # (width, height): one tile, a ragged frame of 3 x 2 tiles, 5 x 3 tiles
SETTINGS = ((0, 2.2, 1.0), (1, 2.2, 1.5), (2, 2.4, 1.0))
SIZE = (40, 24)


def floats(plane, pad=PAD):
    return TM.floats_on_device(np.asarray(plane, F), pad)


def bytes_on_device(n, pad=PAD):
    import torch
    t = torch.full((n + pad,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def same_t(hdr, count, want, what):
    """{out, N} against numpy: the same bytes, no pixel left out -- where a value is a NaN, a NaN (its payload is no part of the definition)"""
    got = np.concatenate([hdr, count[..., None]], -1)
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaNs elsewhere", int((np.isnan(got) != nan).sum()))
    TM.same(np.where(nan, F(0.0), got), np.where(nan, F(0.0), want), what)


def judge_tonemapped(what, ldr, rgba8, out, settings, least=0.9):
    """float LDR within the standing 1e-4 of the float64 post_process of the kernel's own `out`, RGBA8 within one step of that reference's
    quantisation (tests/test_gpu_compose.py's bar), alpha 255: every pixel whose `out` is finite"""
    fine = np.isfinite(out).all(-1)
    want_ldr, want_rgba8 = CR.tonemap(out.astype(np.float64), settings)
    err = np.abs(ldr.astype(np.float64) - want_ldr)[fine].max()
    step = np.abs(rgba8.astype(np.int32) - want_rgba8.astype(np.int32))[fine].max()
    print(f"{what}: ldr {err:.3e}, rgba8 steps {step}, finite {fine.mean():.3f}")
    assert fine.mean() >= least and err <= G.TOL and step <= 1 and (rgba8[..., 3] == 255).all(), (what, float(err), int(step))


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("flags", [0, T.LUMA_WEIGHT], ids=["plain", "luma"])
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, width, height, flags):
    import test_taa_reference as TR
    rng = np.random.default_rng(8000 + width)
    frames, vels, jitters = TR.random_frames(rng, width, height, 5, nan_calls=(3,))      # (a NaN colour stays in the history it enters)
    n = width * height
    kw = dict(max_history=3.0, min_weight=0.1, flags=flags)
    r = hip.Renderer(width, height, 64, 16)
    assert r.taa_info() == (0, 0, 0, 0)
    prev = None
    for call in range(5):                                                        # sequences of 1, 2 and 5 calls are this one's prefixes
        d_c, d_v, d_o = floats(frames[call]), floats(vels[call]), bytes_on_device(n * 4)
        r.taa_resolve_device(SETTINGS[call % 3], d_c.data_ptr(), d_v.data_ptr(), d_o.data_ptr(), jitter=jitters[call], **kw)
        ldr, hdr, count, _ = r.read_taa(want=("ldr", "hdr", "count"))
        want = T.resolve(frames[call], vels[call], prev, jitter=jitters[call], **kw)
        same_t(hdr, count, want, (width, height, flags, call))
        got8 = d_o.cpu().numpy()
        assert (got8[n * 4:] == 77).all() and (d_c.cpu().numpy()[n * 3:] == SENTINEL).all() and (d_v.cpu().numpy()[n * 2:] == SENTINEL).all()
        assert d_c.cpu().numpy()[:n * 3].tobytes() == frames[call].tobytes()      # the inputs are read only
        judge_tonemapped((width, height, flags, call), ldr, got8[:n * 4].reshape(height, width, 4), hdr, SETTINGS[call % 3], least=0.75)
        with pytest.raises(hip.ArcticError):                                     # the RGBA8 went to the caller's buffer
            r.read_taa(want=("rgba8",))
        prev = want
    assert width * height < 64 or (prev[..., 3].max() == 3.0 and (prev[..., 3] == 1.0).any())
    info = r.taa_info()
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    assert info[1:] == (5, 5, 0) and info[0] >= 2 * tiles * 64 * 16 + n * 12
    r.close()


def test_host_form_own_output_reset_resize_and_counters(pkg, hip):
    import test_taa_reference as TR
    width, height = SIZES[1]
    rng = np.random.default_rng(8100)
    frames, vels, jitters = TR.random_frames(rng, width, height, 3, nan_calls=())
    kw = dict(max_history=8.0, min_weight=0.0)
    r = hip.Renderer(width, height, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa()
    assert e.value.code == STATE                                                 # T is empty
    first = r.taa_resolve(SETTINGS[0], frames[0], vels[0], jitter=jitters[0], **kw)
    ldr, hdr, count, rgba8 = r.read_taa()
    assert hdr.tobytes() == frames[0].tobytes() and (count == 1).all() and first.tobytes() == rgba8.tobytes()
    second = r.taa_resolve(SETTINGS[0], frames[1], None, jitter=jitters[1], read=False, **kw)      # a NULL velocity is zero, a NULL output stays in the handle
    assert second is None
    ldr, hdr, count, rgba8 = r.read_taa()
    want = T.resolve(frames[1], None, T.resolve(frames[0]), jitter=jitters[1], **kw)
    same_t(hdr, count, want, "host form, second call")
    judge_tonemapped("host form", ldr, rgba8, hdr, SETTINGS[0])
    assert r.taa_info()[1:] == (2, 2, 0)
    held = r.taa_info()[0]
    # reset: the next call is a first call; nothing is freed, the launches go on counting
    r.taa_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa()
    assert e.value.code == STATE and r.taa_info() == (held, 2, 0, 0)
    r.taa_resolve(SETTINGS[0], frames[2], vels[2], jitter=jitters[2], **kw)
    _, hdr, count, _ = r.read_taa(want=("hdr", "count"))
    assert hdr.tobytes() == frames[2].tobytes() and (count == 1).all() and r.taa_info() == (held, 3, 1, 0)      # a warm call allocates nothing
    # resize: T is empty again, at the new size
    r.resize(*SIZES[0])
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa()
    assert e.value.code == STATE
    small = rng.uniform(0, 4, (SIZES[0][1], SIZES[0][0], 3)).astype(F)
    r.taa_resolve(SETTINGS[0], small, None, **kw)
    r.taa_resolve(SETTINGS[0], small * F(0.5), None, **kw)
    _, hdr, count, _ = r.read_taa(want=("hdr", "count"))
    want = T.resolve(small * F(0.5), None, T.resolve(small), **kw)
    same_t(hdr, count, want, "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    import ctypes as C
    width, height = SIZES[1]
    n = width * height
    rng = np.random.default_rng(8200)
    cur = rng.uniform(0, 4, (height, width, 3)).astype(F)
    r = hip.Renderer(width, height, 64, 16)
    d_c, d_v, d_o = floats(cur), floats(np.zeros((height, width, 2), F)), bytes_on_device(n * 4)

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda c=d_c.data_ptr(), v=d_v.data_ptr(), o=d_o.data_ptr(), **kw: r.taa_resolve_device(SETTINGS[0], c, v, o, **kw)
    for bad in (dict(flags=4), dict(flags=0x80000000), dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=np.nan), dict(max_history=np.inf),
                dict(min_weight=-0.1), dict(min_weight=1.0), dict(min_weight=np.nan), dict(jitter=(1.5, 0.0)), dict(jitter=(0.0, np.nan)), dict(jitter=(-np.inf, 0.0))):
        refused(INVALID, lambda: go(**bad))
    t = pkg.renderer._taa_arguments(0, 8.0, 0.0, (0.0, 0.0))
    t["reserved"][0, 1] = 1
    refused(INVALID, lambda: go(taa=t))
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(v=d_v.data_ptr() + 4))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer._taa_arguments(0, 8.0, 0.0, (0.0, 0.0))
    assert r.L.arctic_taa_resolve_device(r.h, None, C.c_void_p(good.ctypes.data), C.c_void_p(d_c.data_ptr()), None, None) == INVALID
    assert r.L.arctic_taa_resolve_device(r.h, st, None, C.c_void_p(d_c.data_ptr()), None, None) == INVALID
    assert r.L.arctic_taa_resolve(r.h, st, None, None, None, None) == INVALID
    for bad in ((1.5, 0.0), (0.0, -1.001), (np.nan, 0.0), (0.0, np.inf)):
        refused(INVALID, lambda: r.set_camera_jitter(*bad))
    # a NULL colour plane is the handle's own: it needs the float HDR plane, and a shading
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    refused(STATE, lambda: r.pass_taa(TC.scene(pkg, width, height), SETTINGS[0]))   # no visibility plane either
    assert r.taa_info() == (0, 0, 0, 0)                                          # a refused call holds nothing
    # a shard is refused: the taps' rows are elsewhere
    shard = hip.Renderer(width, height, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.taa_resolve_device(SETTINGS[0], d_c.data_ptr(), None, d_o.data_ptr())
    assert e.value.code == STATE and shard.taa_info() == (0, 0, 0, 0)
    shard.close()
    # the state is what the last good call left
    go(max_history=8.0)
    refused(INVALID, lambda: go(max_history=0.0))
    refused(STATE, lambda: go(c=None))
    r.flush()
    assert r.taa_info()[1:] == (1, 1, 0)
    go(max_history=8.0)
    _, hdr, count, _ = r.read_taa(want=("hdr", "count"))
    want = T.resolve(cur, None, T.resolve(cur), max_history=8.0)
    same_t(hdr, count, want, "after the refusals")
    assert (count == 2).all() and (d_o.cpu().numpy()[n * 4:] == 77).all()
    r.close()


# ---- the jitter on the rasterised scene of the hit tests ------------------------------------------------------------------------------------------
def lit_handle(pkg, hip, size=SIZE, keep_float=True):
    """test_gpu_motion.hit_handle with lights and an environment, so that a frame can be shaded"""
    r = TM.hit_handle(pkg, hip, size)
    r.update_lights(pkg.scenes.random_lights(np.random.default_rng(64), 5, (-3, 0.5, -3), (3, 3, 3), intensity=6.0))
    r.create_hdri(pkg.scenes.synthetic_hdri(64, 32))
    if keep_float:
        r.set_option("keep_float_output", 1)
    return r


def drawn(r, desc):
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, SETTINGS[0])
    return r.read_gbuffer() + (r.read_output(want=("rgba8",))[2],)


def distance_to_sample(pkg, desc, attrs, material, jitter):
    """per covered pixel: how far the float64 projection of the G-buffer's world through the UNJITTERED proj_view lies from p + 0.5 - j, pixels"""
    W, H = SIZE
    M = pkg.renderer.frame_constants(desc)[0].astype(np.float64)                  # [col][row]
    covered = material != 0xFFFFFFFF
    w = np.concatenate([attrs[..., 11:14].astype(np.float64), np.ones(attrs.shape[:2] + (1,))], -1)
    clip = w @ M
    sx, sy = (clip[..., 0] / clip[..., 3] + 1.0) * (0.5 * W), (1.0 - clip[..., 1] / clip[..., 3]) * (0.5 * H)
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.hypot(sx - (xs + 0.5 - jitter[0]), sy - (ys + 0.5 - jitter[1]))
    return d[covered], covered


def test_camera_jitter_moves_the_samples_and_zero_changes_nothing(pkg, hip):
    """The bound for the jittered frame is 4 x the largest distance of the unjittered frame of the same run (the parent's path); the margin covers
    the two extra roundings per matrix row.  Measured when this was written, 555 covered pixels: 2.38e-3 px with j = 0, 2.34e-3 px with
    j = (0.4, -0.3); both are printed"""
    g = hit_scenes.geometry(pkg)
    desc = TM.hit_desc(pkg, g.objects, SIZE)
    never, zero, moved = lit_handle(pkg, hip), lit_handle(pkg, hip), lit_handle(pkg, hip)
    zero.set_camera_jitter(0.0, 0.0)
    j = (0.4, -0.3)
    moved.set_camera_jitter(*j)
    a, b, c = drawn(never, desc), drawn(zero, desc), drawn(moved, desc)
    for x, y in zip(a, b):                                                       # attributes, material, depth, triangle, RGBA8
        assert x.tobytes() == y.tobytes()
    assert (a[3] != c[3]).any() and (a[1] != 0xFFFFFFFF).sum() >= 300
    d0, _ = distance_to_sample(pkg, desc, a[0], a[1], (0.0, 0.0))
    dj, covered = distance_to_sample(pkg, desc, c[0], c[1], j)
    wrong, _ = distance_to_sample(pkg, desc, c[0], c[1], (0.0, 0.0))
    print(f"distance to the sample position: j = 0 {d0.max():.3e} px, j = {j} {dj.max():.3e} px over {int(covered.sum())} pixels; bound {4 * d0.max():.3e}")
    assert dj.max() <= 4 * d0.max(), (float(dj.max()), float(d0.max()))
    assert wrong.min() > 0.4                                                     # and the samples have moved by j, not stayed
    # a resize keeps the jitter; the shadow map and arctic_frame_constants do not see it
    assert never.read_shadow_map().tobytes() == moved.read_shadow_map().tobytes()
    moved.resize(*SIZE)
    again = drawn(moved, desc)
    assert again[3].tobytes() == c[3].tobytes() and again[4].tobytes() == c[4].tobytes()
    moved.set_camera_jitter(0.0, 0.0)
    assert drawn(moved, desc)[4].tobytes() == a[4].tobytes()
    assert never.taa_info() == (0, 0, 0, 0) and moved.taa_info() == (0, 0, 0, 0)
    never.close(); zero.close(); moved.close()


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, T.LUMA_WEIGHT], ids=["plain", "luma"])
def test_eight_jittered_frames_one_call_by_hand_and_numpy(pkg, hip, flags):
    """arctic_render_frame + arctic_pass_taa over eight jittered frames of the still scene, against render + motion vectors + resolve by hand on a
    second handle (byte for byte) and against numpy on the read-back HDR frames and velocities (byte for byte); then the anti-aliasing condition
    against the mean of the eight frames.  The figures are printed; when this was written, on the 578 pixels that differ between the frames: one
    frame 0.0654, the resolve 0.0090 (ratio 0.14) without the luma weight and 0.0136 (0.21) with it; the condition is 0.5"""
    import torch
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    desc = TM.hit_desc(pkg, g.objects, SIZE)
    one, hand = lit_handle(pkg, hip), lit_handle(pkg, hip)
    d_pw = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    d_vel = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(max_history=8.0, min_weight=0.0, flags=flags)
    frames, prev = [], None
    for k in range(8):
        j = pkg.renderer.taa_jitter(k)
        for r in (one, hand):
            r.set_camera_jitter(*j)
            r.render_frame(desc, SETTINGS[0])
        rgba8 = one.pass_taa(desc, SETTINGS[0], jitter=j, **kw)
        hand.motion_vectors_device(desc, d_pw.data_ptr(), d_vel.data_ptr())
        hand.taa_resolve_device(SETTINGS[0], None, d_vel.data_ptr(), None, jitter=j, **kw)
        got, want = one.read_taa(), hand.read_taa()
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), (k, int((a != b).sum()))
        assert rgba8.tobytes() == want[3].tobytes()
        hdr = hand.read_output(want=("hdr",))[1]
        vel = d_vel.cpu().numpy()
        prev = T.resolve(hdr, vel, prev, jitter=j, **kw)
        same_t(got[1], got[2], prev, ("numpy", flags, k))
        covered = hand.read_gbuffer(want=("material",))[1] != 0xFFFFFFFF
        if k:
            assert np.abs(vel[covered] + F(j)).max() <= 1.0 / 64, float(np.abs(vel[covered] + F(j)).max())   # a still scene: velocity2 = -j
        frames.append(hdr)
    judge_tonemapped(("chain", flags), got[0], got[3], got[1], SETTINGS[0])
    differ = np.zeros((H, W), bool)
    for f in frames[1:]:
        differ |= (f != frames[0]).any(-1)
    mean = np.stack(frames).astype(np.float64).mean(0)
    single = np.abs(T.reinhard(frames[-1]) - T.reinhard(mean))[differ].mean()
    resolved = np.abs(T.reinhard(got[1]) - T.reinhard(mean))[differ].mean()
    print(f"flags {flags}: {int(differ.sum())} pixels differ between the frames; against the mean of the 8: one frame {single:.4e}, resolved {resolved:.4e}, ratio {resolved / single:.3f}; "
          f"N in [{got[2].min()}, {got[2].max()}]")
    assert differ.sum() >= 100 and resolved <= 0.5 * single, (flags, float(resolved), float(single))
    assert one.taa_info()[1:] == (8, 8, 0) and one.motion_info()[1:] == (8, 0, 8)
    one.close(); hand.close()


def test_a_moved_box_with_and_without_velocity2(pkg, hip):
    import torch
    W, H = SIZE
    g = hit_scenes.geometry(pkg)
    descs = [TM.hit_desc(pkg, g.objects, SIZE), TM.hit_desc(pkg, g.moved, SIZE)]
    with_v, without = lit_handle(pkg, hip), lit_handle(pkg, hip)
    d_pw = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
    d_vel = torch.full((H, W, 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(max_history=8.0, min_weight=0.05)
    prev_v = prev_0 = None
    for k, desc in enumerate(descs):
        for r in (with_v, without):
            r.render_frame(desc, SETTINGS[0])
        with_v.motion_vectors_device(desc, d_pw.data_ptr(), d_vel.data_ptr())
        with_v.taa_resolve_device(SETTINGS[0], None, d_vel.data_ptr(), None, **kw)
        without.taa_resolve_device(SETTINGS[0], None, None, None, **kw)
        hdr, vel = with_v.read_output(want=("hdr",))[1], d_vel.cpu().numpy()
        prev_v, prev_0 = T.resolve(hdr, vel, prev_v, **kw), T.resolve(hdr, None, prev_0, **kw)
        for r, want in ((with_v, prev_v), (without, prev_0)):
            _, got, count, _ = r.read_taa(want=("hdr", "count"))
            same_t(got, count, want, ("moved box", k, r is with_v))
    assert (np.abs(vel).max(-1) > 0.5).sum() >= 50 and prev_v.tobytes() != prev_0.tobytes()   # the box has moved on the screen, and the velocity matters
    with_v.close(); without.close()


def test_the_composed_source(pkg, hip):
    """ARCTIC_TAA_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane"""
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    with pytest.raises(hip.ArcticError) as e:
        r.taa_resolve_device(TC.SETTINGS, flags=T.SOURCE_COMPOSED)
    assert e.value.code == STATE and r.taa_info() == (0, 0, 0, 0)                  # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    r.taa_resolve_device(TC.SETTINGS, flags=T.SOURCE_COMPOSED)
    _, hdr, count, _ = r.read_taa(want=("hdr", "count"))
    assert hdr.tobytes() == composed.tobytes() and (count == 1).all()
    r.taa_resolve_device(TC.SETTINGS)                                             # ... and without the flag the shading's plane, blended into that history
    ldr, hdr, count, rgba8 = r.read_taa()
    want = T.resolve(shaded, None, T.resolve(composed), max_history=8.0)
    same_t(hdr, count, want, "composed, then shaded")
    judge_tonemapped("composed source", ldr, rgba8, hdr, TC.SETTINGS)
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls; arctic_taa_info is
    zeros until the first call"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.motion_info()
    assert a.taa_info() == (0, 0, 0, 0)
    a.taa_resolve_device(TC.SETTINGS)
    a.taa_resolve_device(TC.SETTINGS)
    _, hdr, count, _ = a.read_taa(want=("hdr", "count"))
    assert hdr.tobytes() == a.read_output(want=("hdr",))[1].tobytes() and (count == 2).all()      # the same frame twice: its own mean
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info(), a.motion_info()) == held
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.taa_info() == (0, 0, 0, 0)
    a.close(); b.close()
