"""ARCTIC_OPT_ENV_LIGHTING on the device: the precomputed tables against the float64 numpy reference (tests/env_reference.py), the
per-pixel term against the reference evaluated with the device's own tables, the paths and shards agreeing bit for bit, and nothing
else moving."""
import copy

import numpy as np
import pytest

import env_reference as ER

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's standing bar on float LDR


def _constant_map(w, h, c):
    env = np.ones((h, w, 4), np.float32)
    env[..., :3] = c
    return env


def _tables(hip, env):
    r = hip.Renderer(16, 8, 0, 16)
    r.create_hdri(env)
    r.set_option("env_lighting", 1)
    out = r.read_env_lighting()
    r.close()
    return out


def test_brdf_table_matches_reference(pkg, hip):
    _, lut, _ = _tables(hip, pkg.scenes.synthetic_hdri(64, 32))
    np.testing.assert_allclose(lut, ER.brdf_lut(), atol=1e-5, rtol=0)


@pytest.mark.parametrize("size", [(128, 64), (97, 41)])
def test_sh_coefficients_match_reference(pkg, hip, size):
    env = pkg.scenes.synthetic_hdri(*size)
    sh, _, levels = _tables(hip, env)
    want = ER.sh_project(env)
    assert np.abs(sh - want).max() <= 1e-6 * np.abs(want[0]).max(), np.abs(sh - want).max()
    np.testing.assert_array_equal(levels[0], env)   # level 0 is the map itself


def test_prefiltered_levels_match_reference(pkg, hip):
    env = pkg.scenes.synthetic_hdri(64, 32)
    _, _, levels = _tables(hip, env)
    assert len(levels) == ER.LEVELS
    for k in range(1, ER.LEVELS):
        want = ER.prefilter_level(env, k)
        got = levels[k][..., :3]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=0, err_msg=f"level {k}")
    c = np.array([0.3, 1.5, 7.0], np.float32)
    _, _, levels = _tables(hip, _constant_map(64, 32, c))
    for k in range(1, ER.LEVELS):
        np.testing.assert_allclose(levels[k][..., :3], np.broadcast_to(c, levels[k][..., :3].shape), rtol=1e-6)


def _material(base_rgb, normal_rgb, rough, metal, side):
    d = np.zeros((side, side, 4), np.uint8); d[..., :3] = base_rgb; d[..., 3] = 255
    n = np.zeros((side, side, 4), np.uint8); n[..., :3] = normal_rgb; n[..., 3] = 255
    m = np.zeros((side, side, 4), np.uint8); m[..., 1] = rough; m[..., 2] = metal; m[..., 3] = 255
    return d, n, m


def test_per_pixel_term_matches_reference(pkg, hip):
    """HDR(mode 1) - HDR(mode 0) = ambient (IBL - base) from the reference evaluated with the device's tables, in every tonemapper,
    with and without the binary16 target; the materials are 1x1 / 2x2 constant images, so n, base, metal and rough are known"""
    rng = np.random.default_rng(11)
    W, H, S = 96, 64, 64
    sc = pkg.scenes.config2(scale=0.05)
    r = hip.Renderer(W, H, S, 16)
    mats = []
    for i, rough in enumerate([0, 26, 51, 77, 128, 179, 204, 230, 255, 13]):
        metal = 255 if i % 2 else 0
        base = rng.integers(20, 255, 3)
        nrm = np.array([rng.integers(100, 156), rng.integers(100, 156), rng.integers(200, 256)])
        mats.append((base, nrm, rough, metal))
        r.create_material(*_material(base, nrm, rough, metal, 1 + i % 2))
    r.update_lights(pkg.scenes.random_lights(rng, 4, (-15, 0, -7), (15, 12, 7)))
    env = pkg.scenes.synthetic_hdri(128, 64)
    r.create_hdri(env)
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, len(mats), coverage=0.9)
    r.write_gbuffer(attrs, mat)
    r.write_shadow_map(rng.random((S, S), dtype=np.float32) * 0.6 + 0.3)
    r.set_option("keep_float_output", 1)
    r.set_option("env_lighting", 1)
    sh, lut, levels = r.read_env_lighting()
    # n, wo, base, metal, rough of every covered pixel, in float64
    cov = mat != 0xFFFFFFFF
    m = np.where(cov, mat, 0)
    P = np.array([x[0] for x in mats], np.float64)[m]
    base = ER.srgb_to_linear(P)
    nb = np.array([x[1] for x in mats], np.float64)[m]
    ts = np.stack([nb[..., 0] * 2 / 255 - 1, -(nb[..., 1] * 2 / 255 - 1), nb[..., 2] * 2 / 255 - 1], -1)
    a = attrs.astype(np.float64)
    n = a[..., 2:5] * ts[..., :1] + a[..., 5:8] * ts[..., 1:2] + a[..., 8:11] * ts[..., 2:3]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    rough = np.array([x[2] for x in mats], np.float64)[m] / 255
    metal = np.array([x[3] for x in mats], np.float64)[m] / 255
    for ambient in (0.1, 1.0):
        desc = copy.deepcopy(sc.desc)
        desc.ambient = ambient
        eye = np.array(desc.camera["eye"], np.float64)
        wo = eye - a[..., 11:14]
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        ibl = ER.ibl(n, wo, base, metal, rough, sh, lut, levels)
        for tm in (0, 1, 2):
            settings = (tm, 2.2, 1.0)
            r.set_option("hdr16", 0)
            r.set_option("env_lighting", 0)
            r.pass_shade(desc, settings)
            _, hdr0, _ = r.read_output()
            want_hdr = hdr0.astype(np.float64) + ambient * (ibl - base)
            for hdr16 in (0, 1):
                r.set_option("hdr16", hdr16)
                r.set_option("env_lighting", 1)
                r.pass_shade(desc, settings)
                ldr1, hdr1, _ = r.read_output()
                want = want_hdr.astype(np.float16).astype(np.float64) if hdr16 else want_hdr
                err = np.abs(ldr1 - ER.tonemap(tm, want))[cov]
                if hdr16:   # the binary16 rounding is a discontinuity: test_reference_quantised_mode's bar
                    assert np.quantile(err, 0.999) <= TOL and err.max() <= 1e-3, (ambient, tm, err.max())
                else:
                    assert err.max() <= TOL, (ambient, tm, err.max(), np.unravel_index(np.argmax(np.where(cov, np.abs(ldr1 - ER.tonemap(tm, want)).max(-1), 0)), cov.shape))
                    assert np.all(hdr1[~cov] == hdr0[~cov])   # pixels without geometry: untouched
    r.close()


def _scene(pkg, cfg, scale):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    sc.environment = pkg.scenes.synthetic_hdri(128, 64)
    return sc


def _handle(pkg, hip, sc, env_lighting=1, **kw):
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    r.set_option("env_lighting", env_lighting)
    return r


@pytest.mark.parametrize("cfg,scale", [(2, 0.25), (3, 0.1)])
def test_paths_and_shards_agree_bit_for_bit(pkg, hip, cfg, scale):
    from arctic_renderer_amd import sharding as sh
    sc = _scene(pkg, cfg, scale)
    r = _handle(pkg, hip, sc)
    ref = r.render_frame(sc.desc, sc.settings)
    base_handle = _handle(pkg, hip, sc, env_lighting=0)
    assert not np.array_equal(ref, base_handle.render_frame(sc.desc, sc.settings))   # the mode is not a no-op
    base_handle.close()
    # the G-buffer path
    r.set_option("visbuffer", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], ref)
    r.set_option("visbuffer", 1)
    for fif in (1, 2, 3):
        r.set_option("frames_in_flight", fif)
        for _ in range(2):
            np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.set_option("frames_in_flight", 0)
    # shards: an unaligned row cut, an interleaved band shard
    cut = sc.height // 3 + 3
    rs = _handle(pkg, hip, sc, row_begin=cut, row_end=sc.height)
    np.testing.assert_array_equal(rs.render_frame(sc.desc, sc.settings), ref[cut:])
    rb = _handle(pkg, hip, sc, band_rows=16, shard=(1, 3))
    np.testing.assert_array_equal(rb.render_frame(sc.desc, sc.settings), ref[sh.owned_rows(sc.height, 1, 3, 16)])
    # two handles given the same map hold the same tables
    a, b = r.read_env_lighting(), rb.read_env_lighting()
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        np.testing.assert_array_equal(x, y)
    rs.close(); rb.close(); r.close()


def test_nothing_else_moves(pkg, hip):
    sc = pkg.scenes.config2(scale=0.25)
    plain = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    ref0 = plain.render_frame(sc.desc, sc.settings)
    # mode 1 without a map = mode 0, bit for bit; no tables to read
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_option("env_lighting", 1)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref0)
    with pytest.raises(hip.ArcticError) as e:
        r.read_env_lighting()
    assert e.value.code == -4
    # a map: sky pixels take it in both modes, identically; set and unset = never set
    env = pkg.scenes.synthetic_hdri(128, 64)
    plain.create_hdri(env)
    sky0 = plain.render_frame(sc.desc, sc.settings)
    r.create_hdri(env)
    img1 = r.render_frame(sc.desc, sc.settings)
    _, mat, _, _ = r.read_gbuffer(want=("material",))
    sky = mat == 0xFFFFFFFF
    assert sky.any() and (~sky).any()
    np.testing.assert_array_equal(img1[sky], sky0[sky])
    assert not np.array_equal(img1[~sky], sky0[~sky])
    r.set_option("env_lighting", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), sky0)
    # the statistics and the tile trace do not apply in mode 1
    r.set_option("env_lighting", 1)
    r.set_option("count_light_evals", 1)
    with pytest.raises(hip.ArcticError) as e:
        r.render_frame(sc.desc, sc.settings)
    assert e.value.code == -4
    r.set_option("count_light_evals", 0)
    # a second map rebuilds the tables
    sh1, _, lv1 = r.read_env_lighting()
    env2 = pkg.scenes.synthetic_hdri(96, 48, seed=5, sun_peak=20.0)
    r.create_hdri(env2)
    sh2, _, lv2 = r.read_env_lighting()
    np.testing.assert_allclose(sh2, ER.sh_project(env2), rtol=0, atol=1e-6 * np.abs(sh2[0]).max())
    assert lv2[0].shape == env2.shape and not np.array_equal(sh1, sh2)
    # resize keeps them
    r.resize(sc.width // 2, sc.height // 2)
    np.testing.assert_array_equal(r.read_env_lighting()[0], sh2)
    plain.close(); r.close()


def test_full_size_frame_is_finite(pkg, hip):
    sc = pkg.scenes.config3()
    sc.environment = pkg.scenes.synthetic_hdri(2048, 1024)
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_option("keep_float_output", 1)
    ref0 = r.render_frame(sc.desc, sc.settings)
    r.set_option("env_lighting", 1)
    img1 = r.render_frame(sc.desc, sc.settings)
    _, hdr1, _ = r.read_output()
    assert np.isfinite(hdr1).all()
    assert not np.array_equal(img1, ref0)
    # 2048 x 1024: eight trips per thread in k_env_sh_rows, four in k_env_sh_final
    sh = r.read_env_lighting(level=ER.LEVELS - 1)[0]
    want = ER.sh_project(sc.environment)
    assert np.abs(sh - want).max() <= 1e-6 * np.abs(want[0]).max(), np.abs(sh - want).max()
    r.set_option("env_lighting", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref0)
    r.close()
