"""ARCTIC_OPT_ENV_LIGHTING at the shapes where its kernels' loops, grids and clamps do something: the tables of env_light.hip against
the float64 numpy reference (tests/env_reference.py) on the maps of tests/env_shapes.py, and the per-pixel lookup of shade.hip
(env_ambient / env_level) on a crafted G-buffer whose pixels sit on its wraps and clamps, against the reference evaluated with the
device's own tables.  tests/test_env_lighting.py pins, on the CPU, that the reference can see a fault at each of these shapes.
The tolerances are those of tests/test_gpu_env_lighting.py."""
import copy
import functools

import numpy as np
import pytest

import env_reference as ER
import env_shapes as ES

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's standing bar on float LDR


def _tables(hip, env):
    r = hip.Renderer(16, 8, 0, 16)
    r.create_hdri(env)
    r.set_option("env_lighting", 1)
    out = r.read_env_lighting()
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _lut_reference():
    return ER.brdf_lut()


def _check_tables(name, env, sh, lut, levels):
    W, H, _ = ES.MAPS[name]
    want = ER.sh_project(env)
    err = np.abs(sh - want).max()
    print(f"{name}: SH max error {err:.3e} of {np.abs(want[0]).max():.3e}")
    assert err <= 1e-6 * np.abs(want[0]).max(), err
    np.testing.assert_allclose(lut, _lut_reference(), atol=1e-5, rtol=0)
    assert len(levels) == ER.LEVELS
    np.testing.assert_array_equal(levels[0], env)   # level 0 is the map itself
    for k in range(1, ER.LEVELS):
        w, h = ER.level_size(W, H, k)
        assert levels[k].shape == (h, w, 4), (k, levels[k].shape)
        texels = ES.level_texels(name, k)
        want = ER.prefilter_level(env, k, texels=texels)
        got = levels[k][..., :3]
        if texels is not None:
            rc = np.array(texels)
            got = got[rc[:, 0], rc[:, 1]]
        print(f"{name}: level {k} ({w} x {h}, {want.shape[0] if texels is not None else w * h} texels) max relative error {(np.abs(got - want) / want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=0, err_msg=f"{name} level {k}")
        np.testing.assert_array_equal(levels[k][..., 3], 1.0)


@pytest.mark.parametrize("name", ["odd", "wide", "tall", "big"])
def test_tables_match_reference_at_shape(pkg, hip, name):
    """SH, the BRDF table, level 0 and the five prefiltered levels of one map per path (sizes: env_shapes.MAPS):
    odd  97 x 41: odd-sided mip levels (97, 41, 5 and 3 wide or high): k_env_mip's floor rule drops their last column / row.  All whole.
    wide 300 x 20: the second, ragged trip of k_env_sh_rows (300 = 256 + 44); level 1 is 300 wide, so k_env_prefilter runs a second,
         ragged x-block (blockIdx.x = 1, 44 threads live).  Its mip level 1 is 150 wide: k_env_mip stays in one block here (that is
         `big`'s).  All whole.
    tall 40 x 300: the second, ragged trip of k_env_sh_final (threads 0..43 sum two rows); min(H, 256) of env_level_size.  Levels above
         1000 texels on env_shapes.level_texels' subset.
    big  1040 x 520: both clamps of env_level_size (levels 512 x 256 ... 32 x 16); up to five trips per thread in k_env_sh_rows and three
         in k_env_sh_final; blockIdx.x = 1 of k_env_prefilter at level 1 (full) and blockIdx.x = 1, 2 of k_env_mip (mip level 1 is 520 wide,
         ragged); an 11-level chain with the odd side 65.  Levels 1 and 2 on the subset (corners, last row and column, columns 255 - 257),
         levels 3 to 5 whole."""
    env = ES.make_map(pkg.scenes, name)
    assert env[..., :3].min() > 0   # atol = 0 is sound
    _check_tables(name, env, *_tables(hip, env))


@pytest.mark.parametrize("name", ["1x1", "2x1", "1x7", "3x5"])
def test_tables_of_tiny_maps(pkg, hip, name):
    """maps below the levels' 8 x 4 floor (levels 2 to 5 are 8 x 4; level 1 is 8 x max(4, H)), all compared whole.  1 x 1: a one-entry mip
    chain -- every sample of k_env_prefilter takes sample_lod's lod >= top branch -- and a one-texel wrap64 on both axes: its levels equal
    its one texel, which needs no reference.  2 x 1, 1 x 7, 3 x 5: one-texel wraps on one axis, chains 2, 3 and 3 levels long."""
    env = ES.make_map(pkg.scenes, name)
    sh, lut, levels = _tables(hip, env)
    _check_tables(name, env, sh, lut, levels)
    if name == "1x1":
        for k in range(1, ER.LEVELS):
            np.testing.assert_allclose(levels[k][..., :3], np.broadcast_to(env[0, 0, :3], levels[k][..., :3].shape), rtol=1e-6)


def test_two_handles_hold_the_same_tables_of_a_large_map(pkg, hip):
    """1040 x 520: threads of both SH kernels make several trips, so the sums' fixed order is what keeps two handles' bytes equal"""
    env = ES.make_map(pkg.scenes, "big")
    a, b = _tables(hip, env), _tables(hip, env)
    np.testing.assert_array_equal(a[0], b[0]); np.testing.assert_array_equal(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        np.testing.assert_array_equal(x, y)


def _material(base_rgb, normal_rgb, rough, metal, side):
    d = np.zeros((side, side, 4), np.uint8); d[..., :3] = base_rgb; d[..., 3] = 255
    n = np.zeros((side, side, 4), np.uint8); n[..., :3] = normal_rgb; n[..., 3] = 255
    m = np.zeros((side, side, 4), np.uint8); m[..., 1] = rough; m[..., 2] = metal; m[..., 3] = 255
    return d, n, m


def _lookup_errors(pkg, hip, env, attrs, mat, mats):
    """the float-LDR error of every pixel of mode 1 against HDR(mode 0) + ambient (IBL - base), IBL from ER.ibl with the device's tables:
    {(ambient, tonemapper): (rows, width) max over the channels}, and the coverage mask"""
    rng = np.random.default_rng(3)
    H, W = mat.shape
    S = 64
    sc = pkg.scenes.config2(scale=0.05)
    assert tuple(sc.desc.camera["eye"]) == ES.EYE
    r = hip.Renderer(W, H, S, 16)
    for i, (base, nrm, rough, metal) in enumerate(mats):
        r.create_material(*_material(base, nrm, rough, metal, ES.material_side(i)))
    r.update_lights(pkg.scenes.random_lights(rng, 4, (-15, 0, -7), (15, 12, 7)))
    r.create_hdri(env)
    r.write_gbuffer(attrs, mat)
    r.write_shadow_map(rng.random((S, S), dtype=np.float32) * 0.6 + 0.3)
    r.set_option("keep_float_output", 1)
    r.set_option("hdr16", 0)
    r.set_option("env_lighting", 1)
    sh, lut, levels = r.read_env_lighting()
    n, wo, base, metal, rough, cov = ES.pixel_inputs(attrs, mat, mats)
    ibl = ER.ibl(n, wo, base, metal, rough, sh, lut, levels)
    out = {}
    for ambient in (0.1, 1.0):
        desc = copy.deepcopy(sc.desc)
        desc.ambient = ambient
        for tm in (0, 1, 2):
            settings = (tm, 2.2, 1.0)
            r.set_option("env_lighting", 0)
            r.pass_shade(desc, settings)
            _, hdr0, _ = r.read_output()
            r.set_option("env_lighting", 1)
            r.pass_shade(desc, settings)
            ldr1, hdr1, _ = r.read_output()
            want = hdr0.astype(np.float64) + ambient * (ibl - base)
            out[(ambient, tm)] = np.where(cov, np.abs(ldr1 - ER.tonemap(tm, want)).max(-1), 0.0)
            assert np.all(hdr1[~cov] == hdr0[~cov])   # pixels without geometry: untouched
    r.close()
    return out, cov


def _report(label, errs, cov, kind):
    worst = 0.0
    for key, e in errs.items():
        at = np.unravel_index(np.argmax(e), e.shape)
        print(f"{label} ambient {key[0]} tonemapper {key[1]}: max error {e.max():.3e} at {at} (kind {kind[at]}), "
              f"share of covered pixels above 1e-5: {(e[cov] > 1e-5).mean():.4f}, above 1e-4: {(e[cov] > 1e-4).mean():.5f}")
        worst = max(worst, e.max())
    return worst


@pytest.mark.parametrize("size", [(128, 64), (97, 41)])
def test_lookup_at_its_wraps_and_clamps(pkg, hip, size):
    """env_ambient / env_level on env_shapes.crafted_gbuffer, every covered pixel at the 1e-4 bar, tonemappers 0 to 2, ambient 0.1 and 1:
    - the u seam: R = (-1, 0, +-e), e from 0.05 to 24 texels of level 0 on both sides (x0 = w - 1, x1 = 0 in wrap_axis), and the v wrap
      across each pole, 0.05 to 5 texels away (y0 = h - 1, y1 = 0), each direction with every roughness byte;
    - the roughness bytes 0, 1, 50, 51, 52, 101, 102, 153, 204, 254, 255: t = 5 r on and beside every level boundary, and k1's clamp
      min(k0 + 1, 5) at 255 together with the LUT's last row.  The term is continuous across a boundary (f = 0 at level k equals f = 1 at
      level k - 1), so floor(t) may land on either side in fp32 and in float64: the bar absorbs the difference;
    - n.wo = 1, 0.5, 1/64, 1e-4, 0 to rounding, -0.2, -0.9: the LUT's last and first columns, p5 = 1, and R built from the raw negative dot
      while the LUT and Fresnel take the clamped one;
    - 97 x 41: odd level sizes (97 x 41, 48 x 20, 24 x 10, 12 x 5) in env_level.
    Materials are mixed within the tiles; tile (3, 5) holds one material.  Before the device is asked, the fans must reach the wraps.
    Measured, worst of the six settings: 2.2e-4 (128 x 64) and 1.1e-4 (97 x 41) with the fp32 lookup coordinates this test found, all
    of it in the pole fans (asinf and an fp32 R lose the direction there); 2.4e-6 and 3.6e-6 with binary64 coordinates."""
    w0, h0 = size
    env = pkg.scenes.synthetic_hdri(w0, h0)
    attrs, mat, mats, kind = ES.crafted_gbuffer(w0, h0, ES.ROUGH_EDGES)
    assert min(ES.wrap_counts(attrs, mat, mats, kind, w0, h0)) >= 32
    assert len(set(mat[24:32, 40:48].ravel())) == 1 and all(len(set(mat[y:y + 8, x:x + 8].ravel())) > 1 for y, x in ((0, 0), (8, 16), (56, 88)))
    errs, cov = _lookup_errors(pkg, hip, env, attrs, mat, mats)
    worst = _report(f"{w0} x {h0}", errs, cov, kind)
    assert worst <= TOL, worst


def test_level0_lookup_precision_at_a_real_map_size(pkg, hip):
    """the lookup where fp32 coordinates are coarsest against the texel: a 2048 x 1024 map whose neighbouring texels differ by up to a
    factor 16, roughness bytes 0, 13, 26, 38, 50 (level 0, the raw map, weighs in), dielectrics and metals; the seam and pole fans in this
    map's texels plus random pixels (coverage 0.9).  Every covered pixel at the 1e-4 bar.
    Measured, worst of the six settings (ambient 1, ACES): with fp32 coordinates the largest error was 4.6e-2, 6.4 % of the covered pixels
    above 1e-4 and 15 % above 1e-5, all of the former in the pole fans; with binary64 coordinates (shade.hip env_reflection) 6.1e-5, none
    above 1e-4 and 0.05 % above 1e-5, the largest at a random pixel."""
    w0, h0 = 2048, 1024
    env = ES.contrast_map(pkg.scenes, w0, h0)
    attrs, mat, mats, kind = ES.crafted_gbuffer(w0, h0, ES.ROUGH_LEVEL0, angles=False)
    assert min(ES.wrap_counts(attrs, mat, mats, kind, w0, h0)) >= 32
    errs, cov = _lookup_errors(pkg, hip, env, attrs, mat, mats)
    worst = _report("2048 x 1024, contrast 16", errs, cov, kind)
    assert worst <= TOL, worst
