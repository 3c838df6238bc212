"""arctic_taa_upscale(_device), arctic_pass_taa_upscale, arctic_taa_upscale_reset / _info and arctic_read_taa_upscale on the device (needs an
MI355X), against the numpy definition of tests/taa_upscale_reference.py BY BYTES, no pixel left out: k_taa_upscale on synthetic planes at every
size pair (output sizes that are no multiple of 8, a ratio of 4, unequal ratios on the two axes, a 1x1 input; velocities that point outside the
frame or are not finite, NaN colours, sentinels behind every plane, each flag and both blend forms), its tonemapped planes against the float64
post_process of its own `out`, the device form against the host form and a caller's buffer against the handle's own, P1 against
arctic_taa_resolve on the same handle, the state's life (reset, resize, a changed output size, the counters, a handle that never calls), the
refusals, and the whole chain: a half-size handle under the exact four-phase jitter through arctic_pass_taa_upscale against a handle that
renders the output size directly."""
import json
import os

import numpy as np
import pytest

import taa_reference as T
import taa_upscale_reference as U
import test_gpu_compose as TC
import test_gpu_taa as TG

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITY = os.path.join(ROOT, "profiles", "taa_upscale_quality.json")
PAIRS = U.PAIRS + (((37, 23), (55, 34)), ((37, 23), (74, 46)))
SETTINGS = TG.SETTINGS
# the chain's configuration (tools/taa_upscale_quality.py --gpu measures it with chain() below and writes QUALITY)
CHAIN = dict(scale=0.25, rounds=2)


def same_planes(a, b, what):
    """two read-backs: the same bytes, a NaN where the other has one (its payload is no part of the definition)"""
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, what
        if x.dtype == F:
            nan = np.isnan(y)
            assert (np.isnan(x) == nan).all(), (what, "NaNs elsewhere")
            x, y = np.where(nan, F(0.0), x), np.where(nan, F(0.0), y)
        assert x.tobytes() == y.tobytes(), (what, int((x != y).sum()))


def read_u(r):
    ldr, hdr, count, _ = r.read_taa_upscale(want=("ldr", "hdr", "count"))
    return ldr, hdr, count


@pytest.mark.parametrize("in_size, out_size", PAIRS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("blend", [0, U.LUMA_WEIGHT], ids=["plain", "luma"])
def test_six_frames_equal_numpy_by_bytes_device_and_host_form(pkg, hip, in_size, out_size, blend):
    """six calls on synthetic planes: the device form into a caller's RGBA8 buffer on one handle, the host form into the handle's own on another;
    {out, N} of both equals numpy by bytes every frame, the tonemapped planes hold the standing bar, and the two handles' planes are the same"""
    import test_taa_upscale_reference as TR
    (w, h), (W, H) = in_size, out_size
    rng = np.random.default_rng(9600 + w + W)
    frames, vels, jitters = TR.random_frames(rng, in_size, out_size, 6, nan_calls=(3,))
    n = W * H
    dev, host = hip.Renderer(w, h, 64, 16), hip.Renderer(w, h, 64, 16)
    assert dev.taa_upscale_info() == (0, 0, 0, 0)
    prev = None
    for call in range(6):                                                        # sequences of 1, 2 and 6 calls are this one's prefixes
        kw = dict(jitter=jitters[call], max_history=3.0, min_weight=0.1, sharpness=(0.0, 0.7, 2.0)[call % 3], confidence_floor=0.05,
                  flags=blend | (U.NO_CLAMP if call in (2, 4) else 0))
        d_c, d_v, d_o = TG.floats(frames[call]), TG.floats(vels[call]), TG.bytes_on_device(n * 4)
        dev.taa_upscale_device(SETTINGS[call % 3], out_size, d_c.data_ptr(), d_v.data_ptr(), d_o.data_ptr(), **kw)
        ldr, hdr, count = read_u(dev)
        want = U.upscale(frames[call], out_size, vels[call], prev, **kw)
        TG.same_t(hdr, count, want, (in_size, out_size, blend, call))
        got8 = d_o.cpu().numpy()
        assert (got8[n * 4:] == 77).all() and (d_c.cpu().numpy()[w * h * 3:] == TG.SENTINEL).all() and (d_v.cpu().numpy()[w * h * 2:] == TG.SENTINEL).all()
        assert d_c.cpu().numpy()[:w * h * 3].tobytes() == frames[call].tobytes()  # the inputs are read only
        TG.judge_tonemapped((in_size, out_size, blend, call), ldr, got8[:n * 4].reshape(H, W, 4), hdr, SETTINGS[call % 3], least=0.7)
        with pytest.raises(hip.ArcticError):                                     # the RGBA8 went to the caller's buffer
            dev.read_taa_upscale(want=("rgba8",))
        first = host.taa_upscale(SETTINGS[call % 3], out_size, frames[call], vels[call], **kw)
        h_ldr, h_hdr, h_count, h_rgba8 = host.read_taa_upscale()
        assert h_ldr.tobytes() == ldr.tobytes() and h_hdr.tobytes() == hdr.tobytes() and h_count.tobytes() == count.tobytes()
        assert h_rgba8.tobytes() == got8[:n * 4].tobytes() == first.tobytes()    # the handle's own buffer holds what the caller's does
        prev = want
    assert n < 64 or (np.nanmax(prev[..., 3]) == 3.0 and (prev[..., 3] < 1.0).any())
    info = dev.taa_upscale_info()
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert info[1:] == (6, 6, W | H << 32) and 2 * 16 * 64 * tiles + n * 12 <= info[0] <= 2 * 16 * 64 * tiles + (n * 12) * 5 // 4 + 256
    assert dev.taa_info() == (0, 0, 0, 0)                                        # the resolve's state is another
    dev.close(); host.close()


@pytest.mark.parametrize("width, height", ((1, 1), (17, 9), (40, 24)))
@pytest.mark.parametrize("flags", [0, T.LUMA_WEIGHT], ids=["plain", "luma"])
def test_p1_at_ratio_one_it_is_the_resolve_on_the_device(pkg, hip, width, height, flags):
    """the same handle runs arctic_taa_resolve and the upscaler at W = w, H = h, sharpness 0: {out, N}, float LDR and RGBA8 are the same bytes
    through five calls (NaN for NaN), whatever confidence_floor says"""
    import test_taa_reference as TR
    rng = np.random.default_rng(9700 + width)
    frames, vels, jitters = TR.random_frames(rng, width, height, 5)
    jitters[3] = (0.499, -0.499)
    r = hip.Renderer(width, height, 64, 16)
    for call in range(5):
        kw = dict(jitter=jitters[call], max_history=3.0, min_weight=0.1, flags=flags)
        a8 = r.taa_resolve(SETTINGS[call % 3], frames[call], vels[call], **kw)
        b8 = r.taa_upscale(SETTINGS[call % 3], (width, height), frames[call], vels[call], sharpness=0.0, confidence_floor=(1.0, 0.3, 2.0 ** -30)[call % 3], **kw)
        same_planes(r.read_taa(), r.read_taa_upscale(), (width, height, flags, call))
        assert a8.tobytes() == b8.tobytes()
    assert r.taa_info()[1:3] == (5, 5) and r.taa_upscale_info()[1:3] == (5, 5)
    r.close()


def test_reset_resize_a_changed_output_size_and_the_counters(pkg, hip):
    import test_taa_upscale_reference as TR
    in_size, out_size, other = (17, 9), (29, 14), (34, 18)
    rng = np.random.default_rng(9800)
    frames, vels, jitters = TR.random_frames(rng, in_size, out_size, 4, nan_calls=())
    kw = dict(max_history=8.0, sharpness=0.5, confidence_floor=0.1)
    r = hip.Renderer(*in_size, 64, 16)
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa_upscale()
    assert e.value.code == STATE                                                 # U is empty
    first_call = lambda k, size=out_size: U.upscale(frames[k], size, vels[k], None, jitter=jitters[k], **kw)
    r.taa_upscale(SETTINGS[0], out_size, frames[0], vels[0], jitter=jitters[0], **kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, first_call(0), "first call")
    r.taa_upscale(SETTINGS[0], out_size, frames[1], None, jitter=jitters[1], read=False, **kw)       # a NULL velocity is zero, a NULL output stays in the handle
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, U.upscale(frames[1], out_size, None, first_call(0), jitter=jitters[1], **kw), "second call")
    tiles = lambda s: ((s[0] + 7) // 8) * ((s[1] + 7) // 8)
    held = r.taa_upscale_info()
    assert held[1:] == (2, 2, out_size[0] | out_size[1] << 32) and held[0] >= 2 * 16 * 64 * tiles(out_size)
    # reset: the next call is a first call; nothing is freed, the launches go on counting
    r.taa_upscale_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa_upscale()
    assert e.value.code == STATE and r.taa_upscale_info() == (held[0], 2, 0, held[3])
    r.taa_upscale(SETTINGS[0], out_size, frames[2], vels[2], jitter=jitters[2], **kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, first_call(2), "after the reset")
    assert r.taa_upscale_info() == (held[0], 3, 1, held[3])                      # a warm call allocates nothing
    # a changed output size: U is re-allocated, 32 bytes per output pixel of whole tiles, and empty
    r.taa_upscale(SETTINGS[0], other, frames[3], vels[3], jitter=jitters[3], **kw)
    _, hdr, count = read_u(r)
    assert hdr.shape == (other[1], other[0], 3)
    TG.same_t(hdr, count, first_call(3, other), "after the output size changed")
    info = r.taa_upscale_info()
    assert info[3] == other[0] | other[1] << 32 and info[0] - held[0] >= 2 * 16 * 64 * (tiles(other) - tiles(out_size))
    r.taa_upscale(SETTINGS[0], other, frames[0], vels[0], jitter=jitters[0], **kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, U.upscale(frames[0], other, vels[0], first_call(3, other), jitter=jitters[0], **kw), "the second call at the new size")
    # resize: U is empty again, at the new input size
    r.resize(8, 8)
    with pytest.raises(hip.ArcticError) as e:
        r.read_taa_upscale()
    assert e.value.code == STATE
    small = rng.uniform(0, 4, (8, 8, 3)).astype(F)
    r.taa_upscale(SETTINGS[0], (16, 16), small, None, **kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, U.upscale(small, (16, 16), **kw), "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_u_as_it_was(pkg, hip):
    import ctypes as C
    in_size, out_size = (17, 9), (29, 14)
    (w, h), (W, H) = in_size, out_size
    rng = np.random.default_rng(9900)
    cur = rng.uniform(0, 4, (h, w, 3)).astype(F)
    r = hip.Renderer(w, h, 64, 16)
    d_c, d_v, d_o = TG.floats(cur), TG.floats(np.zeros((h, w, 2), F)), TG.bytes_on_device(W * H * 4)

    def refused(code, fn, word=None):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code and (word is None or word in str(e.value)), e.value
    go = lambda c=d_c.data_ptr(), v=d_v.data_ptr(), o=d_o.data_ptr(), size=out_size, **kw: r.taa_upscale_device(SETTINGS[0], size, c, v, o, **kw)
    for bad in (dict(flags=8), dict(flags=0x80000000), dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=np.nan), dict(min_weight=-0.1), dict(min_weight=1.0),
                dict(jitter=(1.5, 0.0)), dict(jitter=(0.0, np.nan)), dict(sharpness=-1.0), dict(sharpness=np.inf), dict(sharpness=np.nan), dict(confidence_floor=0.0),
                dict(confidence_floor=1.5), dict(confidence_floor=np.nan), dict(size=(16, 14)), dict(size=(29, 37)), dict(size=(69, 14)), dict(size=(0, 14))):
        refused(INVALID, lambda: go(**bad))
    # the header's order: of two faults the earlier one is named
    refused(INVALID, lambda: go(flags=8, max_history=0.5), "flags")
    refused(INVALID, lambda: go(max_history=0.5, sharpness=-1.0), "max_history")
    refused(INVALID, lambda: go(sharpness=-1.0, size=(16, 14)), "sharpness")
    refused(INVALID, lambda: go(size=(16, 14), c=d_c.data_ptr() + 2), "output size")
    t = pkg.renderer.taa_upscale_arguments(out_size)
    t["reserved"][0, 1] = 1
    refused(INVALID, lambda: go(upscale=t))
    refused(INVALID, lambda: go(c=d_c.data_ptr() + 2))
    refused(INVALID, lambda: go(v=d_v.data_ptr() + 4))
    refused(INVALID, lambda: go(o=d_o.data_ptr() + 2))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer.taa_upscale_arguments(out_size)
    assert r.L.arctic_taa_upscale_device(r.h, None, C.c_void_p(good.ctypes.data), C.c_void_p(d_c.data_ptr()), None, None) == INVALID
    assert r.L.arctic_taa_upscale_device(r.h, st, None, C.c_void_p(d_c.data_ptr()), None, None) == INVALID
    assert r.L.arctic_taa_upscale(r.h, st, None, None, None, None) == INVALID
    # a NULL colour plane is the handle's own: it needs the float HDR plane, and a shading
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    refused(INVALID, lambda: go(c=None, flags=8))                                # ... and INVALID comes first
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    refused(STATE, lambda: r.pass_taa_upscale(TC.scene(pkg, w, h), SETTINGS[0], out_size))   # no visibility plane either
    refused(STATE, lambda: r.taa_upscale_hdr_device(d_c.data_ptr()))             # U is empty
    refused(INVALID, lambda: r.taa_upscale_hdr_device(None))
    refused(INVALID, lambda: r.taa_upscale_hdr_device(d_c.data_ptr() + 2))
    assert r.taa_upscale_info() == (0, 0, 0, 0)                                  # a refused call holds nothing
    # a shard is refused
    shard = hip.Renderer(w, h, 64, 16, row_begin=0, row_end=8)
    with pytest.raises(hip.ArcticError) as e:
        shard.taa_upscale_device(SETTINGS[0], out_size, d_c.data_ptr(), None, d_o.data_ptr())
    assert e.value.code == STATE and shard.taa_upscale_info() == (0, 0, 0, 0)
    shard.close()
    # U is what the last good call left
    kw = dict(max_history=8.0, sharpness=0.5)
    go(**kw)
    refused(INVALID, lambda: go(max_history=0.0))
    refused(INVALID, lambda: go(size=(30, 14), flags=8))
    refused(STATE, lambda: go(c=None))
    r.flush()
    assert r.taa_upscale_info()[1:3] == (1, 1)
    go(**kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, U.upscale(cur, out_size, None, U.upscale(cur, out_size, **kw), **kw), "after the refusals")
    assert (d_o.cpu().numpy()[W * H * 4:] == 77).all()
    r.close()


def test_the_composed_source_and_nothing_else_moved(pkg, hip):
    """ARCTIC_TAA_UPSCALE_SOURCE_COMPOSED after arctic_pass_ray_effects: C is the composition's HDR plane; and a frame's RGBA8, arctic_stats and
    the other stages' counters are the same before the first call, after it, and on a handle that never calls"""
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    size = (2 * r.width, 2 * r.rows)
    first = r.render_frame(desc, TC.SETTINGS).copy()
    before = r.stats().copy()
    held = r.compose_info(), r.hit_shading_info(), r.ao_history_info(), r.motion_info(), r.taa_info()
    with pytest.raises(hip.ArcticError) as e:
        r.taa_upscale_device(TC.SETTINGS, size, flags=U.SOURCE_COMPOSED)
    assert e.value.code == STATE and r.taa_upscale_info() == (0, 0, 0, 0)       # nothing composed yet
    shaded = r.read_output(want=("hdr",))[1]
    kw = dict(sharpness=1.0, confidence_floor=0.25)
    r.taa_upscale_device(TC.SETTINGS, size, **kw)
    _, hdr, count = read_u(r)
    TG.same_t(hdr, count, U.upscale(shaded, size, **kw), "the shading's plane")
    assert (r.compose_info(), r.hit_shading_info(), r.ao_history_info(), r.motion_info(), r.taa_info()) == held
    after = r.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (r.stats()[:2] == before[:2]).all()
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed = r.read_composed(want=("hdr",))[1]
    assert (composed != shaded).any(-1).mean() >= 0.05
    r.taa_upscale_device(TC.SETTINGS, size, flags=U.SOURCE_COMPOSED, **kw)
    ldr, hdr, count, rgba8 = r.read_taa_upscale()
    TG.same_t(hdr, count, U.upscale(composed, size, None, U.upscale(shaded, size, **kw), flags=U.SOURCE_COMPOSED, **kw), "composed, behind shaded")
    TG.judge_tonemapped("composed source", ldr, rgba8, hdr, TC.SETTINGS)
    never = TC.handle(pkg, hip, TC.images(), keep_float=False)                                # a handle that never makes the calls
    assert never.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (never.stats()[:8] == before[:8]).all() and never.taa_upscale_info() == (0, 0, 0, 0)
    r.close(); never.close()


def chain(pkg, hip, scale, rounds):
    """The smallest BASELINE configuration's scene (config 1) on a half-size handle under the exact four-phase jitter, `rounds` times round,
    through arctic_pass_taa_upscale, next to the calls by hand on a second half-size handle and to a third handle that renders the output
    size directly.  -> the figures, and the planes of the last frame"""
    import torch
    sc = pkg.scenes.config1(scale=scale)
    out_size, in_size = (sc.width, sc.height), (sc.width // 2, sc.height // 2)
    make = lambda size: sc.upload(hip.Renderer(size[0], size[1], sc.shadow_size, sc.max_lights))
    one, hand, full = make(in_size), make(in_size), make(out_size)
    for r in (one, hand, full):
        r.set_option("keep_float_output", 1)
    full.render_frame(sc.desc, sc.settings)
    direct = full.read_output(want=("ldr",))[0]
    one.render_frame(sc.desc, sc.settings)                                       # one half-size frame, no jitter, stretched
    stretched = U.stretch_bilinear(one.read_output(want=("ldr",))[0], out_size)
    d_pw = torch.full((in_size[1], in_size[0], 4), -7.0, dtype=torch.float32, device="cuda")
    d_vel = torch.full((in_size[1], in_size[0], 2), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(max_history=float(rounds), sharpness=1.0, confidence_floor=2.0 ** -25, flags=U.NO_CLAMP)
    prev = None
    for k in range(4 * rounds):
        j = pkg.renderer.taa_upscale_jitter(k, in_size, out_size, exact=True)
        for r in (one, hand):
            r.set_camera_jitter(*j)
            r.render_frame(sc.desc, sc.settings)
        rgba8 = one.pass_taa_upscale(sc.desc, sc.settings, out_size, jitter=j, **kw)
        hand.motion_vectors_device(sc.desc, d_pw.data_ptr(), d_vel.data_ptr())
        hand.taa_upscale_device(sc.settings, out_size, None, d_vel.data_ptr(), None, jitter=j, **kw)
        got, want = one.read_taa_upscale(), hand.read_taa_upscale()
        same_planes(got, want, ("the one call against the two by hand", k))
        assert rgba8.tobytes() == want[3].tobytes()
        prev = U.upscale(hand.read_output(want=("hdr",))[1], out_size, d_vel.cpu().numpy(), prev, jitter=j, **kw)
        TG.same_t(got[1], got[2], prev, ("numpy", k))
    # behind the upscaler: U's colour as a row-major device plane is the explicit colour argument of the output-size handle's stages
    n = out_size[0] * out_size[1]
    d_hdr = torch.full((n * 3 + 16,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    one.taa_upscale_hdr_device(d_hdr.data_ptr())
    one.flush()
    plane = d_hdr.cpu().numpy()
    assert plane[:n * 3].tobytes() == got[1].tobytes() and (plane[n * 3:] == -77.0).all()
    full.bloom_device(sc.settings, d_hdr.data_ptr(), levels=3)
    chained = full.read_bloom(3, want=("hdr", "rgba8"))
    full.bloom(sc.settings, got[1], levels=3, read=False)
    by_host = full.read_bloom(3, want=("hdr", "rgba8"))
    assert chained[1].tobytes() == by_host[1].tobytes() and chained[2].tobytes() == by_host[2].tobytes() and np.isfinite(chained[1]).all()
    assert one.taa_upscale_info()[1:3] == (4 * rounds, 4 * rounds)                # the plane is no call and no launch of the counters
    covered = full.read_gbuffer(want=("material",))[1] != 0xFFFFFFFF
    launches = one.taa_upscale_info()[1], one.motion_info()[1], one.taa_info()
    for r in (one, hand, full):
        r.close()
    up = float(np.abs(got[0].astype(np.float64) - direct).mean())
    st = float(np.abs(stretched - direct).mean())
    return dict(scale=scale, rounds=rounds, in_size=list(in_size), out_size=list(out_size), covered_fraction=float(covered.mean()), mad_upscaled=up, mad_single_stretched=st,
                ratio_vs_single=up / st), dict(ldr=got[0], hdr=got[1], count=got[2], rgba8=got[3], settings=sc.settings, launches=launches, covered=covered)


def test_the_chain_half_size_frames_against_the_direct_render(pkg, hip):
    """Every frame of the chain: the one call equals the two calls by hand byte for byte and numpy on the read-back planes byte for byte.  Then
    what the feature is for: the upscaled float LDR's mean absolute difference from the handle that renders 128 x 128 directly lies below that
    of one 64 x 64 frame stretched bilinearly.  Bit equality with the direct render is NOT expected: the rasteriser snaps vertices to 1/256
    pixel, and a 64 x 64 frame's snapping grid is not the 128 x 128 frame's, so the two sample slightly different positions.  The ratio was
    measured on an MI355X and recorded in profiles/taa_upscale_quality.json under "gpu"; the bound is halfway between the recorded ratio and 1."""
    recorded = json.load(open(QUALITY))["gpu"]
    assert recorded["scale"] == CHAIN["scale"] and recorded["rounds"] == CHAIN["rounds"] and recorded["ratio_vs_single"] < 1.0
    fig, planes = chain(pkg, hip, **CHAIN)
    print(fig)
    assert planes["launches"] == (4 * CHAIN["rounds"], 4 * CHAIN["rounds"], (0, 0, 0, 0))   # one motion call per frame, and the resolve's state untouched
    # N is the number of rounds where there is geometry, up to the 1/64 pixel by which the rasterised velocity2 differs from -j (which makes
    # the four taps' weights (1 - e, e, ...) instead of (1, 0, 0, 0)); a pixel without geometry has velocity2 = 0 and fetches half a pixel aside
    near = np.abs(planes["count"][planes["covered"]] - CHAIN["rounds"]) < 0.25
    print(f"N within 0.25 of {CHAIN['rounds']} on {near.mean():.3f} of the covered pixels")
    assert near.mean() > 0.8
    TG.judge_tonemapped("chain", planes["ldr"], planes["rgba8"], planes["hdr"], planes["settings"])
    assert fig["covered_fraction"] > 0.1 and fig["mad_upscaled"] < fig["mad_single_stretched"]
    assert fig["ratio_vs_single"] <= 0.5 * (recorded["ratio_vs_single"] + 1.0), fig
