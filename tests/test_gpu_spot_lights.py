"""Spot lights on the device (arctic_update_spot_lights, kernels k_spotlit / k_spotlit_vis): an omnidirectional spot light adds the bits
of a point light, cones and ranges against an independent float64 evaluation, every path and shard agreeing bit for bit, the environment
term combining linearly, and the list's bookkeeping (clear, cap, invalid lights, options that do not apply)."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's standing bar on float LDR
W, H, S = 96, 64, 64
PI_F = np.float32(np.pi)


def _spots(pkg, positions, directions, colors, outer, inner, ranges):
    a = np.zeros(len(positions), pkg.scene.SPOT_LIGHT_DTYPE)
    a["position"], a["direction"], a["color"] = positions, directions, colors
    a["outer_cone_angle"], a["inner_cone_angle"], a["range"] = outer, inner, ranges
    return a


def _omni_of(pkg, points):
    n = len(points)
    return _spots(pkg, points["position"], np.tile([0.0, -1.0, 0.0], (n, 1)), points["color"], np.full(n, PI_F), np.zeros(n), np.zeros(n))


def _gbuffer_handle(pkg, hip, sc, attrs, mat, shadow, max_lights=16):
    r = hip.Renderer(W, H, S, max_lights)
    for d, n, m in sc.materials:
        r.create_material(d, n, m)
    r.write_gbuffer(attrs, mat)
    r.write_shadow_map(shadow)
    r.set_option("keep_float_output", 1)
    return r


def _random_inputs(pkg, sc, seed):
    rng = np.random.default_rng(seed)
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, len(sc.materials), coverage=0.9)
    shadow = rng.random((S, S), dtype=np.float32) * 0.6 + 0.3
    return rng, attrs, mat, shadow


def test_omni_spot_equals_point_light_bit_for_bit(pkg, hip):
    """k omnidirectional spot lights (outer = pi, no range) against the same k point lights, scalar light loop: HDR, LDR and RGBA8 equal,
    over a random G-buffer with a shadow map (arctic_pass_shade) and over whole frames of config 3 (arctic_render_frame)"""
    sc = pkg.scenes.config3(scale=0.1)
    rng, attrs, mat, shadow = _random_inputs(pkg, sc, 21)
    for k in (1, 5, 12):
        pts = pkg.scenes.random_lights(rng, k, (-15, 0, -7), (15, 12, 7))
        a = _gbuffer_handle(pkg, hip, sc, attrs, mat, shadow)
        b = _gbuffer_handle(pkg, hip, sc, attrs, mat, shadow)
        for r in (a, b):
            r.set_option("light_path", 1)
        a.update_lights(pts)
        b.update_lights(pts[:0])
        b.update_spot_lights(_omni_of(pkg, pts))
        for culling in (1, 0):
            a.set_option("culling", culling); b.set_option("culling", culling)
            a.pass_shade(sc.desc, sc.settings); b.pass_shade(sc.desc, sc.settings)
            oa, ob = a.read_output(), b.read_output()
            for x, y in zip(oa, ob):
                np.testing.assert_array_equal(x, y)
            assert oa[1].max() > 0
        a.close(); b.close()
    # whole frames: the config's own point lights (the first 8) as omnidirectional spot lights
    pts = sc.lights[:8]
    a = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    b = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    for r in (a, b):
        r.set_option("light_path", 1); r.set_option("keep_float_output", 1)
    a.update_lights(pts)
    b.update_lights(pts[:0])
    b.update_spot_lights(_omni_of(pkg, pts))
    fa, fb = a.render_frame(sc.desc, sc.settings), b.render_frame(sc.desc, sc.settings)
    np.testing.assert_array_equal(fa, fb)
    for x, y in zip(a.read_output(), b.read_output()):
        np.testing.assert_array_equal(x, y)
    a.close(); b.close()


def _att_window(consts, world):
    """f = att * window per light and pixel in float64 from the fp32-rounded constants (12 floats per light) and the world positions;
    also cd and cos(outer) for the hard-cone mask"""
    out, cds = [], []
    for c in consts.astype(np.float64):
        d = c[0:3] - world
        d2 = (d * d).sum(-1)
        cd = -(d * c[4:7]).sum(-1) / np.sqrt(d2)
        att = np.clip(cd * c[3] + c[7], 0, 1) ** 2
        win = np.clip(1 - (d2 * c[11]) ** 2, 0, 1)
        out.append(att * win); cds.append(cd)
    return out, cds


def test_cones_and_ranges_against_float64(pkg, hip, oracle):
    sc = pkg.scenes.config3(scale=0.1)
    rng, attrs, mat, shadow = _random_inputs(pkg, sc, 22)
    n = 7
    pos = rng.uniform((-14, 1, -6), (14, 11, 6), (n, 3))
    target = rng.uniform((-15, 0, -7), (15, 12, 7), (n, 3))
    outer = rng.uniform(0.3, 1.2, n)
    inner = outer * rng.uniform(0, 0.9, n)
    inner[0] = outer[0]                                   # a hard cone (scale 1000)
    ranges = np.where(np.arange(n) % 2 == 0, rng.uniform(4, 12, n), 0.0)   # ranges cutting through the scene, and none
    colors = rng.uniform(5, 30, (n, 3))
    spots = _spots(pkg, pos, target - pos, colors, outer, inner, ranges)
    spots[n - 1]["position"] = (0.0, 13.0, 0.0)           # above the ceiling pointing up: behind every surface's light
    spots[n - 1]["direction"] = (0.0, 1.0, 0.0)
    from importlib import import_module
    L = import_module("arctic_renderer_amd.binding").lib()
    consts = np.zeros((n, 12), np.float32)
    assert L.arctic_spot_light_constants(spots.ctypes.data, n, consts.ctypes.data) == 0
    tm, gamma, exposure = sc.settings
    desc = copy.deepcopy(sc.desc)
    r = _gbuffer_handle(pkg, hip, sc, attrs, mat, shadow)
    r.update_lights(sc.lights[:0])
    r.update_spot_lights(spots)
    r.pass_shade(desc, sc.settings)
    ldr, hdr, _ = r.read_output()
    world = r.read_gbuffer(want=("attrs",))[0][..., 11:14].astype(np.float64)
    # the oracle: point-light handles -- the sun and ambient part without local lights, then each light alone with sun and ambient off
    o = _gbuffer_handle(pkg, hip, sc, attrs, mat, shadow)
    o.update_lights(sc.lights[:0])
    o.pass_shade(desc, sc.settings)
    base_hdr = o.read_output(want=("hdr",))[1]
    want = base_hdr.astype(np.float64)
    dark = copy.deepcopy(desc)
    dark.ambient = 0.0
    dark.sun = dict(dark.sun, color=(0.0, 0.0, 0.0))
    f, cds = _att_window(consts, world)
    ok = mat != 0xFFFFFFFF
    cos_o = np.cos(np.float64(np.float32(outer[0])))
    ok &= (cds[0] < cos_o - 1e-5) | (cds[0] > cos_o + 1e-3 + 1e-5)   # the hard cone: only where att is exactly 0 or exactly 1 (its whole
    #                                                                     ramp lies within 1e-3 of cos(outer), where fp32 cd * 1000 is ill-conditioned)
    for i in range(n):
        o.update_lights(pkg.scene.make_lights(spots["position"][i:i + 1], spots["color"][i:i + 1]))
        o.pass_shade(dark, sc.settings)
        term = o.read_output(want=("hdr",))[1].astype(np.float64)    # (1 - shadow) term_i
        want += term * f[i][..., None]
    assert ok.mean() > 0.8
    for i in range(n):     # the cases are there: each light lights some pixels and leaves others dark
        if i < n - 1:
            assert (f[i][ok] > 0).any() and (f[i][ok] == 0).any(), i
    assert (f[n - 1] == 0).all()
    ys, xs = np.nonzero(ok)
    exp = np.array([oracle.tonemap(tm, gamma, exposure, want[y, x])[1] for y, x in zip(ys, xs)])
    err = np.abs(ldr[ys, xs] - exp)
    assert err.max() <= TOL, (err.max(), ys[np.argmax(err.max(-1))], xs[np.argmax(err.max(-1))])
    assert np.abs(hdr - base_hdr).max() > 0.01   # the spot lights are seen
    r.close(); o.close()


def _frame_handle(pkg, hip, sc, spots, **kw):
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    r.update_spot_lights(spots)
    return r


@pytest.mark.parametrize("cfg,scale", [(3, 0.1), (2, 0.25)])
def test_paths_and_shards_agree_bit_for_bit(pkg, hip, cfg, scale):
    from arctic_renderer_amd import sharding as sh
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    spots = pkg.scenes.spot_lights(6, seed=cfg)
    r = _frame_handle(pkg, hip, sc, spots)
    ref = r.render_frame(sc.desc, sc.settings)
    plain = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    assert not np.array_equal(ref, plain.render_frame(sc.desc, sc.settings))   # the lights are seen
    plain.close()
    # the G-buffer path
    r.set_option("visbuffer", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], ref)
    r.set_option("visbuffer", 1)
    # culling off: every covered pixel evaluates every light
    r.set_option("culling", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.set_option("culling", 1)
    # the dispatch-order hint is ignored
    r.set_option("tile_order", 1)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    for fif in (1, 2):
        r.set_option("frames_in_flight", fif)
        for _ in range(2):
            np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.set_option("frames_in_flight", 0)
    # light paths 1 and 2 differ only in the order of the point sums
    r.set_option("keep_float_output", 1)
    out = {}
    for lp in (1, 2):
        r.set_option("light_path", lp)
        r.render_frame(sc.desc, sc.settings)
        out[lp] = r.read_output(want=("ldr",))[0]
    assert np.abs(out[1] - out[2]).max() <= 1e-6
    r.set_option("light_path", 0)
    # shards: an unaligned row cut, an interleaved band shard
    cut = sc.height // 3 + 3
    rs = _frame_handle(pkg, hip, sc, spots, row_begin=cut, row_end=sc.height)
    np.testing.assert_array_equal(rs.render_frame(sc.desc, sc.settings), ref[cut:])
    rb = _frame_handle(pkg, hip, sc, spots, band_rows=16, shard=(1, 3))
    np.testing.assert_array_equal(rb.render_frame(sc.desc, sc.settings), ref[sh.owned_rows(sc.height, 1, 3, 16)])
    rs.close(); rb.close(); r.close()


def test_env_lighting_combines_linearly(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    env = np.ones((32, 64, 4), np.float32)
    env[..., :3] = np.linspace(0.8, 1.2, 64, dtype=np.float32)[None, :, None] * np.float32([0.5, 0.6, 0.7])
    sc.environment = env
    spots = pkg.scenes.spot_lights(5, seed=7)
    hdr = {}
    for env_on in (0, 1):
        r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
        r.set_option("keep_float_output", 1)
        r.set_option("env_lighting", env_on)
        for k, s in ((0, spots[:0]), (1, spots)):
            r.update_spot_lights(s)
            r.render_frame(sc.desc, sc.settings)
            hdr[env_on, k] = r.read_output(want=("hdr",))[1].astype(np.float64)
        r.close()
    d_env, d_plain = hdr[1, 1] - hdr[1, 0], hdr[0, 1] - hdr[0, 0]
    assert np.abs(d_plain).max() > 1e-3   # (config 3 is mostly in the sun's shadow, where spot lights do not light)
    scale = np.maximum(np.abs(hdr[1, 1]), np.abs(hdr[0, 1])) + 1e-30
    assert (np.abs(d_env - d_plain) <= 4 * np.finfo(np.float32).eps * scale).all(), np.abs(d_env - d_plain).max()


def test_clear_cap_invalid_and_options(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    never = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    ref0 = never.render_frame(sc.desc, sc.settings)
    never.close()
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    spots = pkg.scenes.spot_lights(4)
    r.update_spot_lights(spots)
    with_spots = r.render_frame(sc.desc, sc.settings)
    assert not np.array_equal(with_spots, ref0)
    # an invalid light: ARCTIC_E_INVALID, the previous list stays
    bad = spots.copy()
    bad[2]["inner_cone_angle"] = bad[2]["outer_cone_angle"] + 0.1
    for b in (bad, np.concatenate([spots[:1], spots[:1]])):
        if b is not bad:
            b[1]["direction"] = (0, 0, 0)
        with pytest.raises(hip.ArcticError) as e:
            r.update_spot_lights(b)
        assert e.value.code == -1
        np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), with_spots)
    # statistics and the tile trace do not apply with spot lights
    for opt in ("count_light_evals", "tile_trace"):
        r.set_option(opt, 1)
        with pytest.raises(hip.ArcticError) as e:
            r.render_frame(sc.desc, sc.settings)
        assert e.value.code == -4
        r.set_option(opt, 0)
    # cleared: the frame of a handle that never had spot lights, bit for bit; the options apply again
    r.update_spot_lights(spots[:0])
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref0)
    r.set_option("count_light_evals", 1)
    r.render_frame(sc.desc, sc.settings)
    r.set_option("count_light_evals", 0)
    r.close()
    # the cap: max_lights spot lights are kept, the rest dropped
    cap = 4
    many = pkg.scenes.spot_lights(7, seed=3)
    a = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, cap))
    b = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, cap))
    a.update_spot_lights(many)
    b.update_spot_lights(many[:cap])
    np.testing.assert_array_equal(a.render_frame(sc.desc, sc.settings), b.render_frame(sc.desc, sc.settings))
    a.close(); b.close()


def test_gltf_spot_lights_render(pkg, hip, tmp_path):
    """a glTF file's KHR_lights_punctual spot light, loaded and handed to update_spot_lights, lights the file's geometry"""
    import json
    from importlib import import_module
    from test_gltf_loader import write_scene
    gltf = import_module("arctic_renderer_amd.gltf")
    gltf.build()
    path, _, _ = write_scene(str(tmp_path))
    doc = json.load(open(path))
    doc["extensions"] = {"KHR_lights_punctual": {"lights": [
        {"type": "spot", "color": [1.0, 0.9, 0.8], "intensity": 40.0, "range": 30.0, "spot": {"innerConeAngle": 0.2, "outerConeAngle": 0.7}}]}}
    # (a node "matrix" with the offset in its bottom row: assimp_to_mat4's transpose makes it the light's position, (0, 0, 4))
    doc["nodes"].append({"name": "lamp", "matrix": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4, 0, 0, 0, 1],
                         "extensions": {"KHR_lights_punctual": {"light": 0}}})
    doc["scenes"][0]["nodes"].append(4)
    json.dump(doc, open(path, "w"))
    g = gltf.load(path)
    assert len(g.spot_lights) == 1
    np.testing.assert_array_equal(g.spot_lights[0]["position"], [0, 0, 4])
    np.testing.assert_array_equal(g.spot_lights[0]["direction"], [0, 0, -1])
    objs = g.objects.copy()
    objs["trs"] = np.eye(4, dtype=np.float32).reshape(16)   # as test_gltf_loader renders the file
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0.3, 0.4, 4.0), rotation=(0.0, -90.0), aspect=1.5, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.2, sun=dict(position=(2, 10, 6), rotation=(-55.0, -110.0), color=(8, 8, 8)), objects=objs)
    frames = []
    for spots in (g.spot_lights[:0], g.spot_lights):
        r = g.upload(hip.Renderer(192, 128, 256, 16))
        r.update_lights(g.point_lights)
        r.update_spot_lights(spots)
        frames.append(r.render_frame(desc, (2, 2.2, 1.0)))
        r.close()
    assert not np.array_equal(frames[0], frames[1])
    assert frames[1].astype(int).sum() > frames[0].astype(int).sum()
