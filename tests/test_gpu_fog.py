"""arctic_fog(_device), arctic_pass_fog, arctic_read_fog and arctic_fog_info on the device (needs an MI355X), against the numpy definition of
tests/fog_reference.py BY BYTES, no pixel left out: k_fog_march on the shapes of the CPU test (frames of one tile, partial tiles and 8 x 5
tiles; maps of side 0, 16 and 64 injected with arctic_write_shadow_map; 1, 7, 32 and 128 steps; depths 0, 1.0, beyond 1 and NaN; NaN, infinite
and negative colours; rows that send every sample off the map, and rows that send samples off each side and beyond depth 1 alone; density 0
and 64; max_distance nearer than the surface; a caller's offset table; sentinels behind every caller plane), the
tonemapped planes against the float64 post_process of the kernel's own `out`, the host form, resize, the counters and the refusals; and on a
rasterised scene the one call against the calls by hand and against numpy with the composed source, the fog's caller-owned output fed as the
explicit colour of arctic_taa_resolve_device, and a handle that never makes these calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import fog_reference as G
import taa_reference as T
import test_fog_reference as TR
import test_gpu_compose as TC
import test_gpu_taa as TT

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SETTINGS = TT.SETTINGS
VIEWS = (G.view_record(), G.view_record(**TR.HOSTILE))


@functools.lru_cache(maxsize=None)
def reference(width, height, S, steps, vi):
    """numpy's (out, T, I) of a case, computed once and left unchanged"""
    Cp, z = TR.planes(width, height)
    offsets = TR.table(steps) if steps in (7, 128) else None
    out = G.fog(Cp, z, TR.shadow_map(S), VIEWS[vi], offsets, **dict(TR.RECORD, steps=steps))[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_case(width, height, name, S, steps):
    """test_fog_reference.edge_case with numpy's `out` alone kept, computed once and left unchanged"""
    C, z, m, view, offsets, kw, want = TR.edge_case(width, height, name, S, steps)
    want[0].setflags(write=False)
    return C, z, m, view, offsets, kw, want[0]


@pytest.mark.parametrize("width, height", TR.SIZES, ids=lambda v: str(v))
def test_synthetic_planes_equal_numpy_by_bytes(pkg, hip, width, height):
    Cp, z = TR.planes(width, height)
    n = width * height
    d_c, d_z = TT.floats(Cp), TT.floats(z)
    call = 0
    for S in TR.MAPS:
        r = hip.Renderer(width, height, S, 16)
        assert r.fog_info() == (0, 0, 0, 0)
        if S:
            r.write_shadow_map(TR.shadow_map(S))
        for steps in TR.STEPS:
            for vi, view in enumerate(VIEWS):
                kw = dict(TR.RECORD, steps=steps)
                offsets = TR.table(steps) if steps in (7, 128) else None
                d_h, d_o = TT.floats(np.zeros((height, width, 3), F)), TT.bytes_on_device(n * 4)
                r.fog_device(SETTINGS[call % 3], view, d_c.data_ptr(), d_z.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), offsets, **kw)
                ldr = r.read_fog(want=("ldr",))[0]
                got, got8 = d_h.cpu().numpy(), d_o.cpu().numpy()
                out = got[:n * 3].reshape(height, width, 3)
                G.same(out, reference(width, height, S, steps, vi), (width, height, S, steps, vi))
                assert (got8[n * 4:] == 77).all() and (got[n * 3:] == TT.SENTINEL).all()                # sentinels behind every plane of the caller's
                for d, host in ((d_c, Cp), (d_z, z)):
                    back = d.cpu().numpy()
                    assert (back[host.size:] == TT.SENTINEL).all() and back[:host.size].tobytes() == host.tobytes()   # ... and the inputs are read only
                rgba8 = got8[:n * 4].reshape(height, width, 4)
                if vi == 0:                                                      # (the hostile view's rays overflow: every pixel's phase is a NaN)
                    TT.judge_tonemapped((width, height, S, steps, vi), ldr, rgba8, out, SETTINGS[call % 3], least=0.75)
                assert (rgba8[..., 3] == 255).all()
                for want in ("hdr", "rgba8"):
                    with pytest.raises(hip.ArcticError):                         # both went to the caller's planes
                        r.read_fog(want=(want,))
                call += 1
        # the samples that leave the map by each clause of the inside test alone (test_fog_reference.edge_case asserts that they exist)
        for name, Se, steps in TR.EDGE_CASES:
            if Se != S:
                continue
            _, _, _, view, offsets, kw, want = edge_case(width, height, name, S, steps)
            r.fog_device(SETTINGS[0], view, d_c.data_ptr(), d_z.data_ptr(), None, None, offsets, **kw)
            G.same(r.read_fog(want=("hdr",))[1], want, (width, height, name, S, steps))
        # max_distance nearer than every surface, and the largest density
        for kw in (dict(TR.RECORD, max_distance=0.75, steps=32), dict(TR.RECORD, density=64.0, steps=128)):
            r.fog_device(SETTINGS[0], VIEWS[0], d_c.data_ptr(), d_z.data_ptr(), None, None, TR.table(3), **kw)
            G.same(r.read_fog(want=("hdr",))[1], G.fog(Cp, z, TR.shadow_map(S), VIEWS[0], TR.table(3), **kw)[0], (width, height, S, kw))
        # density 0: the input by bits; no depth plane; the handle's own outputs
        r.fog_device(SETTINGS[0], VIEWS[0], d_c.data_ptr(), d_z.data_ptr(), None, None, **dict(TR.RECORD, density=0.0, steps=7))
        G.same(r.read_fog(want=("hdr",))[1], Cp, "density 0")
        kw = dict(TR.RECORD, steps=32)
        r.fog_device(SETTINGS[0], VIEWS[0], d_c.data_ptr(), None, None, None, TR.table(3), **kw)
        ldr, hdr, rgba8 = r.read_fog()
        G.same(hdr, G.fog(Cp, None, TR.shadow_map(S), VIEWS[0], TR.table(3), **kw)[0], "no depth plane")
        TT.judge_tonemapped("own planes", ldr, rgba8, hdr, SETTINGS[0], least=0.75)
        info = r.fog_info()
        calls = len(TR.STEPS) * 2 + 2 + 2 + sum(1 for _, Se, _ in TR.EDGE_CASES if Se == S)
        assert info[1:3] == (calls, calls) and info[0] >= n * (12 + 12 + 4) + 64
        r.close()


def test_host_form_own_output_resize_and_counters(pkg, hip):
    width, height = TR.SIZES[1]
    Cp, z = TR.planes(width, height)
    m = TR.shadow_map(16)
    kw = dict(TR.RECORD, steps=7)
    r = hip.Renderer(width, height, 16, 16)
    r.write_shadow_map(m)
    with pytest.raises(hip.ArcticError) as e:
        r.read_fog()
    assert e.value.code == STATE                                                 # nothing yet
    hdr, rgba8 = r.fog(SETTINGS[0], VIEWS[0], Cp, z, **kw)
    want = G.fog(Cp, z, m, VIEWS[0], **kw)[0]
    G.same(hdr, want, "host form")
    ldr, own_hdr, own8 = r.read_fog()
    assert own_hdr.tobytes() == hdr.tobytes() and own8.tobytes() == rgba8.tobytes()
    TT.judge_tonemapped("host form", ldr, rgba8, hdr, SETTINGS[0], least=0.75)
    assert r.fog(SETTINGS[1], VIEWS[0], Cp, z, read=False, **kw) is None         # NULL outputs stay in the handle
    ldr, own_hdr, own8 = r.read_fog()
    G.same(own_hdr, want, "host form, own output")
    TT.judge_tonemapped("host form, own output", ldr, own8, own_hdr, SETTINGS[1], least=0.75)
    held = r.fog_info()
    assert held[1:] == (2, 2, 1)                                                 # one table sent: both calls used the default
    r.fog(SETTINGS[0], VIEWS[0], Cp, z, **kw)
    assert r.fog_info() == (held[0], 3, 3, 1)                                    # a warm call allocates nothing and sends nothing
    r.fog(SETTINGS[0], VIEWS[0], Cp, z, TR.table(1), **dict(kw, steps=128))
    assert r.fog_info() == (held[0], 4, 4, 2)                                    # another table travels, nothing is allocated for it
    G.same(r.read_fog(want=("hdr",))[1], G.fog(Cp, z, m, VIEWS[0], TR.table(1), **dict(kw, steps=128))[0], "another table")
    # a new map is the one the next call reads
    m2 = TR.shadow_map(16, seed=5)
    r.write_shadow_map(m2)
    r.fog(SETTINGS[0], VIEWS[0], Cp, z, **kw)
    G.same(r.read_fog(want=("hdr",))[1], G.fog(Cp, z, m2, VIEWS[0], **kw)[0], "a new map")
    # resize: nothing to read, then the new size
    r.resize(*TR.SIZES[0])
    with pytest.raises(hip.ArcticError) as e:
        r.read_fog()
    assert e.value.code == STATE
    Cp, z = TR.planes(*TR.SIZES[0])
    r.fog(SETTINGS[0], VIEWS[0], Cp, z, **kw)
    G.same(r.read_fog(want=("hdr",))[1], G.fog(Cp, z, m2, VIEWS[0], **kw)[0], "after the resize")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    width, height = TR.SIZES[1]
    n = width * height
    Cp, z = TR.planes(width, height)
    m = TR.shadow_map(16)
    r = hip.Renderer(width, height, 16, 16)
    d_c, d_z, d_h, d_o = TT.floats(Cp), TT.floats(z), TT.floats(np.zeros((height, width, 3), F)), TT.bytes_on_device(n * 4)
    zeros = d_h.cpu().numpy().copy()

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    base = dict(TR.RECORD, steps=7)
    go = lambda c=d_c.data_ptr(), zz=d_z.data_ptr(), h=d_h.data_ptr(), o=d_o.data_ptr(), view=VIEWS[0], offsets=None, **kw: r.fog_device(
        SETTINGS[0], view, c, zz, h, o, offsets, **dict(base, **kw))
    refused(STATE, go)                                                           # the sun's map was never drawn or written
    assert r.fog_info() == (0, 0, 0, 0)
    r.write_shadow_map(m)
    for bad in (dict(flags=2), dict(flags=0x80000000), dict(density=-0.1), dict(density=65.0), dict(density=np.nan), dict(anisotropy=0.99), dict(anisotropy=np.nan),
                dict(max_distance=0.0), dict(max_distance=1e6), dict(max_distance=np.nan), dict(steps=0), dict(steps=129), dict(bias=-0.5), dict(bias=2.0), dict(bias=np.nan),
                dict(scatter_color=(-1.0, 0.0, 0.0)), dict(scatter_color=(0.0, np.nan, 0.0)), dict(ambient_color=(0.0, 0.0, 1e6)), dict(ambient_color=(np.inf, 0.0, 0.0))):
        refused(INVALID, lambda: go(**bad))
    reserved = pkg.renderer.fog_arguments(**base)
    reserved["reserved"] = 1
    refused(INVALID, lambda: r.fog_device(SETTINGS[0], VIEWS[0], d_c.data_ptr(), d_z.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), fog=reserved))
    for change in (dict(pad0=1.0), dict(pad2=np.nan), dict(z_near=0.0), dict(z_near=50.0), dict(z_far=np.inf)):
        v = G.view_record()
        for k, x in change.items():
            v[k] = x
        refused(INVALID, lambda: go(view=v))
    v = G.view_record()
    v["ray_dy"][0][2] = np.nan
    refused(INVALID, lambda: go(view=v))
    for x in (1.0, -0.5, np.nan):
        refused(INVALID, lambda: go(offsets=[0.5] * 15 + [x]))
    for which in ("c", "zz", "h", "o"):
        refused(INVALID, lambda: go(**{which: dict(c=d_c, zz=d_z, h=d_h, o=d_o)[which].data_ptr() + 2}))
    st = C.byref(pkg.scene.CSettings(0, 2.2, 1.0))
    good = pkg.renderer.fog_arguments(**base)
    vp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    assert r.L.arctic_fog_device(r.h, None, hp(good), hp(VIEWS[0]), None, vp(d_c), vp(d_z), vp(d_h), vp(d_o)) == INVALID
    assert r.L.arctic_fog_device(r.h, st, None, hp(VIEWS[0]), None, vp(d_c), vp(d_z), vp(d_h), vp(d_o)) == INVALID
    assert r.L.arctic_fog_device(r.h, st, hp(good), None, None, vp(d_c), vp(d_z), vp(d_h), vp(d_o)) == INVALID
    assert r.L.arctic_fog(r.h, st, hp(good), None, None, None, None, None, None) == INVALID
    # a NULL colour plane is the handle's own: it needs the float HDR plane and a shading, or a composition
    refused(STATE, lambda: go(c=None))                                           # ARCTIC_OPT_KEEP_FLOAT_OUTPUT is off
    r.set_option("keep_float_output", 1)
    refused(STATE, lambda: go(c=None))                                           # nothing shaded since
    refused(STATE, lambda: go(c=None, flags=G.SOURCE_COMPOSED))
    desc = TC.scene(pkg, width, height)
    refused(STATE, lambda: r.pass_fog(desc, SETTINGS[0], **base))                # no visibility plane either
    refused(INVALID, lambda: r.pass_fog(desc, SETTINGS[0], **dict(base, steps=0)))
    assert r.fog_info() == (0, 0, 0, 0)                                          # a refused call holds nothing
    # a shard is refused
    shard = hip.Renderer(width, height, 16, 16, row_begin=0, row_end=8)
    shard.write_shadow_map(m)
    with pytest.raises(hip.ArcticError) as e:
        shard.fog_device(SETTINGS[0], VIEWS[0], d_c.data_ptr(), d_z.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), **base)
    assert e.value.code == STATE and shard.fog_info() == (0, 0, 0, 0)
    shard.close()
    # the caller's planes were never written by a refused call; the planes are what the last good call left
    assert (d_o.cpu().numpy() == 77).all() and d_h.cpu().numpy().tobytes() == zeros.tobytes()
    go(h=None, o=None)
    refused(INVALID, lambda: go(steps=0))
    refused(INVALID, lambda: go(offsets=[1.0] * 16))
    refused(STATE, lambda: go(c=None))
    assert r.fog_info()[1:] == (1, 1, 1)
    G.same(r.read_fog(want=("hdr",))[1], G.fog(Cp, z, m, VIEWS[0], **base)[0], "after the refusals")
    assert (d_o.cpu().numpy() == 77).all() and (d_z.cpu().numpy()[n:] == TT.SENTINEL).all()
    r.close()


# ---- the rasterised scene ------------------------------------------------------------------------------------------------------------------------------------
KW = dict(density=0.08, anisotropy=0.4, max_distance=30.0, steps=32, bias=0.003, scatter_color=(2.0, 1.8, 1.5), ambient_color=(0.02, 0.03, 0.05))


def test_the_one_call_the_calls_by_hand_numpy_and_the_next_stage(pkg, hip):
    """a frame and its composition, then arctic_pass_fog under ARCTIC_FOG_SOURCE_COMPOSED against arctic_fog_view + arctic_depth_plane_device +
    arctic_fog_device by hand: byte for byte the same planes, and numpy on the read-back composition, depth and sun map; without the flag the
    shading's plane; then the fog's caller-owned output as the explicit colour of arctic_taa_resolve_device"""
    desc = TC.scene(pkg)
    r = TC.handle(pkg, hip, TC.images())
    W, H = r.width, r.rows
    dirs = pkg.renderer.ao_directions(TC.AO_KW["n_rays"], TC.AO_KW["pattern"], seed=3)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, TC.SETTINGS)
    with pytest.raises(hip.ArcticError) as e:
        r.pass_fog(desc, TC.SETTINGS, flags=G.SOURCE_COMPOSED, **KW)
    assert e.value.code == STATE and r.fog_info() == (0, 0, 0, 0)                # nothing composed yet
    r.pass_ray_effects(desc, TC.SETTINGS, dirs=dirs, reflection_bias=TC.BIAS, **TC.AO_KW)
    composed, shaded = r.read_composed(want=("hdr",))[1], r.read_output(want=("hdr",))[1]
    depth, sun_map = r.read_gbuffer(want=("depth",))[2], r.read_shadow_map()
    view = pkg.renderer.fog_view(desc, W, H)
    offsets = pkg.renderer.fog_offsets(7)
    rgba8 = r.pass_fog(desc, TC.SETTINGS, offsets=offsets, flags=G.SOURCE_COMPOSED, **KW)
    one = r.read_fog()
    d_z = TT.floats(np.zeros((H, W), F))
    r.depth_plane_device(d_z.data_ptr())
    r.fog_device(TC.SETTINGS, view, None, d_z.data_ptr(), None, None, offsets, flags=G.SOURCE_COMPOSED, **KW)
    hand = r.read_fog()
    for a, b in zip(one, hand):
        assert a.tobytes() == b.tobytes(), int((a != b).sum())
    assert rgba8.tobytes() == hand[2].tobytes()
    back = d_z.cpu().numpy()
    assert back[:W * H].tobytes() == depth.tobytes() and (back[W * H:] == TT.SENTINEL).all()
    want, Tn, In, reads, _ = G.fog(composed, depth, sun_map, view, offsets, **KW)
    G.same(one[1], want, "numpy, composed")
    TT.judge_tonemapped("the one call", one[0], one[2], one[1], TC.SETTINGS)
    changed = (one[1] != composed).any(-1)
    dark = In < (1.0 - Tn) - 1e-4
    print(f"fog on the scene: {changed.mean():.3f} of the pixels changed, {dark.mean():.3f} have a shadowed sample, {reads} lookups read the map, T from {Tn.min():.3f} to {Tn.max():.3f}")
    assert changed.mean() >= 0.9 and reads > 0
    r.pass_fog(desc, TC.SETTINGS, offsets=offsets, read=False, **KW)             # ... and without the flag the shading's plane
    G.same(r.read_fog(want=("hdr",))[1], G.fog(shaded, depth, sun_map, view, offsets, **KW)[0], "numpy, shaded")
    assert r.fog_info()[1:3] == (3, 3)
    # the next stage takes the fog's caller-owned plane through its explicit colour argument
    d_h = TT.floats(np.zeros((H, W, 3), F))
    r.fog_device(TC.SETTINGS, view, None, d_z.data_ptr(), d_h.data_ptr(), None, offsets, flags=G.SOURCE_COMPOSED, **KW)
    r.taa_resolve_device(TC.SETTINGS, d_h.data_ptr(), None, None, max_history=4.0)
    _, hdr, count, _ = r.read_taa(want=("hdr", "count"))
    TT.same_t(hdr, count, T.resolve(want, None, None, max_history=4.0), "the anti-aliasing behind the fog")
    got = d_h.cpu().numpy()
    assert got[:W * H * 3].tobytes() == want.tobytes() and (got[W * H * 3:] == TT.SENTINEL).all()
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls, which reports zeros"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.taa_info(), a.motion_blur_info(), a.dof_info(), a.bloom_info(), a.exposure_info()
    assert a.fog_info() == (0, 0, 0, 0)
    a.pass_fog(desc, TC.SETTINGS, **KW)
    a.pass_fog(desc, TC.SETTINGS, **KW)
    assert (a.compose_info(), a.taa_info(), a.motion_blur_info(), a.dof_info(), a.bloom_info(), a.exposure_info()) == held and a.fog_info()[1:] == (2, 2, 1)
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.fog_info() == (0, 0, 0, 0)
    a.close(); b.close()
