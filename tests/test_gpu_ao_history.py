"""arctic_accumulate_ambient_occlusion_device, its host form, arctic_read_ao_history, arctic_ao_history_reset / _info and
arctic_pass_ray_effects_temporal on the device (needs an MI355X): k_ao_accumulate on the analytic G-buffers of tests/ao_history_scenes.py, injected
with arctic_write_gbuffer, against the numpy definition of tests/ao_history_reference.py BY BYTES -- the output plane and all four history planes,
every call of sequences of 1, 2 and 5 calls under each camera path, frames of 96 x 64 and of 61 x 37, NO pixel left out.  Then in place against
out of place, the first call after a reset and after a resize, max_history = 1, degenerate normals and NaN positions, the ragged frame's last
byte, the refusals (which write nothing and leave the history as it was), shards, the one call against the public calls made by hand on a
rasterised scene, and that a handle which never makes these calls is what it was."""
import numpy as np
import pytest

import ao_history_reference as HR
import ao_history_scenes as HS
import test_gpu_compose as TC

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SENTINEL, PAD = 0xA5, 64
PLANES = ("value", "count", "world", "normal")


def handle(hip, size, **kw):
    return hip.Renderer(size[0], size[1], 64, 16, **kw)


def on_device(plane, pad=PAD):
    """the byte plane on the device, with `pad` sentinel bytes behind it"""
    import torch
    t = torch.full((plane.size + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    t[:plane.size] = torch.from_numpy(np.ascontiguousarray(plane).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


def call(r, c, k, hist=HR.HIST, in_place=False):
    """call k of a case on the device -> (bytes (H, W), the pad behind them, (value, count, world, normal))"""
    import torch
    attrs, material, _ = c["frames"][k]
    r.write_gbuffer(attrs, material)
    d_in = on_device(c["planes"][k])
    d_out = d_in if in_place else torch.full_like(d_in, SENTINEL)
    torch.cuda.synchronize()
    r.accumulate_ambient_occlusion_device(c["descs"][k], d_in.data_ptr(), d_out.data_ptr(), **hist)
    r.flush()
    host = d_out.cpu().numpy()
    n = material.size
    if not in_place:
        assert d_in.cpu().numpy()[:n].tobytes() == c["planes"][k].tobytes()      # the input plane is only read
    return host[:n].reshape(material.shape), host[n:], r.read_ao_history()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(got.shape[0], got.shape[1], -1) != want.view(np.uint8).reshape(got.shape[0], got.shape[1], -1)).any(-1))
        raise AssertionError((what, len(bad[0]), [(int(y), int(x)) for y, x in zip(bad[0][:5], bad[1][:5])]))


def judge(step, want, what):
    byte, pad, planes = step
    want_byte, state, _ = want
    same(byte, want_byte, what + ("bytes",))
    assert (pad == SENTINEL).all(), what                                         # nothing past the last pixel
    for name, plane in zip(PLANES, planes):
        same(plane, state[name], what + (name,))


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("move", HS.MOVES)
def test_sequences_equal_numpy_by_bytes(pkg, hip, move, size):
    c = HS.case(pkg, move, *size)
    want = HR.run_sequence(c["frames"], c["planes"])
    r = handle(hip, size)
    for n in HS.CALLS:
        r.ao_history_reset()
        for k in range(n):
            judge(call(r, c, k), want[k], (move, size, n, k))
    assert want[-1][0].tobytes() != c["planes"][4].tobytes()
    if move != "still":                                                          # the frames hold every class the definition names
        HS.check_classes(pkg, *size)
    r.close()


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_and_the_host_form_equal_out_of_place(pkg, hip, size):
    c = HS.case(pkg, "translated", *size)
    want = HR.run_sequence(c["frames"], c["planes"])
    r = handle(hip, size)
    for k in range(3):
        judge(call(r, c, k, in_place=True), want[k], ("in place", size, k))
    r.ao_history_reset()
    for k in range(3):
        attrs, material, _ = c["frames"][k]
        r.write_gbuffer(attrs, material)
        same(r.accumulate_ambient_occlusion(c["descs"][k], c["planes"][k], **HR.HIST), want[k][0], ("host form", size, k))
        for name, plane in zip(PLANES, r.read_ao_history()):
            same(plane, want[k][1][name], ("host form", size, k, name))
    r.close()


def test_first_call_after_a_reset_and_after_a_resize_and_max_history_one(pkg, hip):
    big, small = HS.SIZES
    c, cs = HS.case(pkg, "rotated", *big), HS.case(pkg, "rotated", *small)
    r = handle(hip, big)

    def is_first(step, c, k):
        byte, _, (value, count, _, _) = step
        covered = HR.accumulate_frame(*c["frames"][k][:2], c["planes"][k], None, c["frames"][k][2])[2] > HR.NOT_COVERED
        assert covered.sum() >= 1000 and (~covered).sum() >= 100
        assert (byte[covered] == c["planes"][k][covered]).all() and (byte[~covered] == 255).all()
        assert (count[covered] == 1).all() and (count[~covered] == 0).all() and (value[covered] == c["planes"][k][covered]).all()
    is_first(call(r, c, 0), c, 0)
    second = call(r, c, 1)
    assert (second[2][1] > 1).sum() >= 1000                                      # the second call blends
    r.ao_history_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.read_ao_history()
    assert e.value.code == STATE
    is_first(call(r, c, 2), c, 2)
    call(r, c, 3)
    r.resize(*small)
    with pytest.raises(hip.ArcticError) as e:
        r.read_ao_history()
    assert e.value.code == STATE
    is_first(call(r, cs, 1), cs, 1)
    r.resize(*big)                                                               # and back to a size the planes were made for
    is_first(call(r, c, 4), c, 4)
    # max_history = 1: every call returns its input bytes, whatever the history holds
    one = dict(HR.HIST, max_history=1.0)
    want = HR.run_sequence(c["frames"], c["planes"], one)
    r.ao_history_reset()
    for k in range(3):
        step = call(r, c, k, hist=one)
        judge(step, want[k], ("max_history 1", k))
        covered = want[k][2] > HR.NOT_COVERED
        assert (step[0][covered] == c["planes"][k][covered]).all() and (step[2][1][covered] == 1).all()
    r.close()


def test_degenerate_normals_and_nan_positions_stay_where_they_are(pkg, hip):
    """the scenes carry test_gpu_compose's four kinds of degenerate normals; here NaN and infinite world positions come on top, in the frame that
    is read as history and in the frame that reads it: no fault, the reference's bytes, and no NaN in any value or count"""
    size = HS.SIZES[0]
    base = HS.case(pkg, "translated", *size)
    rng = np.random.default_rng(77)
    frames = []
    for attrs, material, P in base["frames"][:3]:
        attrs = attrs.copy()
        flat = attrs.reshape(-1, 18)
        covered = np.nonzero(material.reshape(-1) != HR.NO_MATERIAL)[0]
        px = rng.choice(covered, 90, replace=False)
        flat[px[:30], 11] = np.nan
        flat[px[30:60], 12] = np.inf
        flat[px[60:], 11:14] = (np.nan, -np.inf, 3e38)
        frames.append((attrs, material, P))
    c = dict(base, frames=frames)
    want = HR.run_sequence(c["frames"], c["planes"])
    r = handle(hip, size)
    for k in range(3):
        step = call(r, c, k)
        judge(step, want[k], ("nan positions", k))
        assert np.isfinite(step[2][0]).all() and np.isfinite(step[2][1]).all()
        assert (want[k][2] == HR.NOT_COVERED).sum() >= 40
    assert (want[2][2] == HR.BEHIND).sum() >= 60                                 # a position that is not finite projects to nothing
    r.close()


def test_refusals_write_nothing_and_leave_the_history(pkg, hip):
    import ctypes as C
    import torch
    size = HS.SIZES[0]
    c = HS.case(pkg, "still", *size)
    r = handle(hip, size)
    d_in, d_out = on_device(c["planes"][0]), on_device(np.full(size[::-1], SENTINEL, np.uint8))
    desc = c["descs"][0]

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    go = lambda **kw: r.accumulate_ambient_occlusion_device(desc, d_in.data_ptr(), d_out.data_ptr(), **dict(HR.HIST, **kw))
    assert r.ao_history_info() == (0, 0, 0, 0)
    refused(STATE, go)                                                           # no G-buffer
    refused(STATE, lambda: r.accumulate_ambient_occlusion(desc, c["planes"][0], **HR.HIST))
    refused(STATE, r.read_ao_history)
    assert r.ao_history_info() == (0, 0, 0, 0)                                   # a refused call holds nothing
    first = call(r, c, 0)
    bad = (dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=np.nan), dict(max_history=np.inf), dict(normal_cos=np.inf), dict(normal_cos=np.nan),
           dict(plane_dist=-1e-6), dict(plane_dist=np.nan), dict(min_weight=-0.1), dict(min_weight=1.0), dict(min_weight=np.nan))
    for kw in bad:
        refused(INVALID, lambda: go(**kw))
    refused(INVALID, lambda: r.accumulate_ambient_occlusion_device(desc, None, d_out.data_ptr(), **HR.HIST))
    refused(INVALID, lambda: r.accumulate_ambient_occlusion_device(desc, d_in.data_ptr(), None, **HR.HIST))
    h = pkg.renderer._ao_history_arguments(**HR.HIST)
    h["reserved"][0, 2] = 1
    refused(INVALID, lambda: r.accumulate_ambient_occlusion_device(desc, d_in.data_ptr(), d_out.data_ptr(), hist=h))
    s, vp = desc.fill(pkg.scene.CScene()), C.c_void_p
    h["reserved"] = 0
    assert r.L.arctic_accumulate_ambient_occlusion_device(r.h, None, vp(h.ctypes.data), vp(d_in.data_ptr()), vp(d_out.data_ptr())) == INVALID
    assert r.L.arctic_accumulate_ambient_occlusion_device(r.h, C.byref(s), None, vp(d_in.data_ptr()), vp(d_out.data_ptr())) == INVALID
    assert r.L.arctic_accumulate_ambient_occlusion(r.h, C.byref(s), vp(h.ctypes.data), None, None) == INVALID
    # the one call: without ARCTIC_COMPOSE_AO, with a bad history block, and in a state the composition refuses (no float HDR plane)
    dirs = pkg.renderer.ao_directions(1, 2, seed=0)
    refused(INVALID, lambda: r.pass_ray_effects_temporal(desc, TC.SETTINGS, None, reflection_bias=1e-3))
    refused(INVALID, lambda: r.pass_ray_effects_temporal(desc, TC.SETTINGS, dirs, max_history=0.0))
    refused(STATE, lambda: r.pass_ray_effects_temporal(desc, TC.SETTINGS, dirs))
    r.flush()
    assert (d_out.cpu().numpy() == SENTINEL).all()                               # a refused call writes nothing ...
    for a, b in zip(r.read_ao_history(), first[2]):
        assert a.tobytes() == b.tobytes()                                        # ... and the history is what the last good call wrote
    assert r.ao_history_info()[1:] == (1, 1, 0)
    want = HR.run_sequence(c["frames"], c["planes"])
    judge(call(r, c, 1), want[1], ("after the refusals", 1))                     # the next call blends into it as if nothing had been tried
    r.close()


@pytest.mark.parametrize("sharding", list(TC.SHARDS))
def test_a_row_range_and_a_band_shard_are_refused(pkg, hip, sharding):
    import torch
    size = HS.SIZES[0]
    c = HS.case(pkg, "still", *size)
    for shard in TC.SHARDS[sharding]:
        r = handle(hip, size, **shard)
        rows = TC.S.owned(pkg, size[1], shard)
        r.write_gbuffer(c["frames"][0][0][rows], c["frames"][0][1][rows])
        d = torch.full((len(rows) * size[0],), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(hip.ArcticError) as e:
            r.accumulate_ambient_occlusion_device(c["descs"][0], d.data_ptr(), d.data_ptr(), **HR.HIST)
        assert e.value.code == STATE and "whole frame" in str(e.value)
        r.flush()
        assert (d.cpu().numpy() == SENTINEL).all() and r.ao_history_info() == (0, 0, 0, 0)
        r.close()


def test_the_one_call_equals_the_public_calls_by_hand_over_two_frames(pkg, hip):
    """arctic_pass_ray_effects_temporal on ao_scenes.raster_scene under a camera that moves between two frames, against trace + accumulate +
    reflections + compose made by hand on a second handle: RGBA8, float LDR, composed HDR and the history, byte for byte"""
    import torch
    imgs = TC.images()
    desc0 = TC.scene(pkg)
    cam = dict(desc0.camera)
    cam["eye"], cam["rotation"] = (cam["eye"][0] + 0.15, cam["eye"][1], cam["eye"][2] - 0.1), (cam["rotation"][0] - 1.0, cam["rotation"][1] + 2.5)
    desc1 = pkg.scenes.SceneDesc(camera=cam, ambient=desc0.ambient, sun=desc0.sun, objects=desc0.objects)
    one, hand = TC.handle(pkg, hip, imgs), TC.handle(pkg, hip, imgs)
    kw = dict(ao_strength=0.9, reflection_strength=1.2)
    ao_kw = dict(n_rays=1, pattern=2, radius=0.75, bias=1e-3, filter=True)
    hist = dict(max_history=16.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.05)
    d_ao = torch.full((TC.HEIGHT, TC.WIDTH), 77, dtype=torch.uint8, device="cuda")
    d_refl = torch.full((TC.HEIGHT, TC.WIDTH, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    results = []
    for frame, desc in enumerate((desc0, desc1)):
        dirs = pkg.renderer.ao_directions(1, 2, seed=frame)
        for r in (one, hand):
            r.pass_shadow_map(desc)
            r.pass_gbuffer(desc)
            r.pass_shade(desc, TC.SETTINGS)
        rgba8 = one.pass_ray_effects_temporal(desc, TC.SETTINGS, dirs, reflection_bias=TC.BIAS, **kw, **ao_kw, max_history=hist["max_history"],
                                              history_normal_cos=hist["normal_cos"], history_plane_dist=hist["plane_dist"], min_weight=hist["min_weight"])
        hand.trace_ambient_occlusion_device(desc, dirs, d_ao.data_ptr(), **ao_kw)
        traced = d_ao.cpu().numpy().copy()
        hand.accumulate_ambient_occlusion_device(desc, d_ao.data_ptr(), d_ao.data_ptr(), **hist)
        hand.trace_reflections_device(desc, TC.BIAS, d_refl.data_ptr())
        hand.compose_planes_device(desc, TC.SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), **kw)
        want = hand.read_composed()
        for a, b in zip(one.read_composed(), want):
            assert a.tobytes() == b.tobytes(), (frame, int((a != b).sum()))
        assert rgba8.tobytes() == want[2].tobytes()
        for a, b in zip(one.read_ao_history(), hand.read_ao_history()):
            assert a.tobytes() == b.tobytes(), frame
        results.append((traced, d_ao.cpu().numpy().copy(), hand.read_ao_history()[1]))
    assert results[0][0].tobytes() == results[0][1].tobytes()                     # the first frame: the traced plane as it is
    changed = results[1][0] != results[1][1]
    assert changed.mean() >= 0.1 and (results[1][2] == 2).sum() >= 1000          # the second: blended with the first, through the first camera
    assert one.ao_history_info()[1:] == (2, 2, 0) and one.compose_info()[2] == 2
    one.close(); hand.close()


def test_nothing_else_moved_and_the_info(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls; arctic_ao_history_info is
    zeros before the first call, holds the two history sets after it (exactly 64 bytes per pixel of the tile-padded frame) and the same
    bytes after the second"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    compose_before, hit_before = a.compose_info(), a.hit_shading_info()
    assert a.ao_history_info() == (0, 0, 0, 0)
    plane = np.full((TC.HEIGHT, TC.WIDTH), 200, np.uint8)
    out = a.accumulate_ambient_occlusion(desc, plane, **HR.HIST)                 # (the G-buffer is resolved on demand behind the frame)
    assert out.shape == plane.shape and set(np.unique(out)) <= {200, 255}
    held = a.ao_history_info()
    tiles = ((TC.WIDTH + 7) // 8) * ((TC.HEIGHT + 7) // 8)
    need = tiles * 64 * 16
    assert held == (4 * need, 1, 1, 0), (held, need)                             # exactly 64 bytes per pixel of the tile-padded frame
    a.accumulate_ambient_occlusion(desc, plane, **HR.HIST)
    assert a.ao_history_info() == (held[0], 2, 2, 0)
    a.ao_history_reset()
    assert a.ao_history_info() == (held[0], 2, 0, 0)                             # a reset frees nothing
    a.accumulate_ambient_occlusion(desc, plane, **HR.HIST)
    assert a.ao_history_info() == (held[0], 3, 1, 0)
    assert a.compose_info() == compose_before and a.hit_shading_info() == hit_before
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.ao_history_info() == (0, 0, 0, 0)
    a.close(); b.close()
