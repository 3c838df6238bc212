"""The third branch of shadow_coords (shadow_coords.h: `lsx / lsw` for a general w) on the device (needs an MI355X).

No rasterised frame takes it (the sun is orthographic) and scenes.random_gbuffer writes w = 1.0, so nothing in the suite ran it; it is the branch
of every G-buffer a host hands over through arctic_write_gbuffer with a perspective light, and of any tile in which one lane holds an
exactly-zero coordinate.  tests/shadow_w_inputs.py builds one 96 x 64 G-buffer per 8 x 8 tile -- w in [0.5, 2], negative, 2^-20 and 2^20, within
the near-one domain with ONE zero coordinate in the tile, one ulp-step outside that domain, exactly 1 (the control), and all of them mixed lane
by lane -- over a 256^2 map with a noise half (the 25 taps decide) and a smooth half (the min/max table decides).  The inputs are held to their
conditions on the CPU with the oracle's calculate_shadow alone (at least 500 penumbra pixels, 200 fully lit, 200 fully shadowed among the general-w
tiles) before any device result is looked at; tests/test_shadow_w_inputs.py does the same without a device.

Checked: the base kernel against the CPU oracle at the suite's standing bars (float LDR within TOL of test_gpu_parity.py, RGBA8 within one step,
no pixel left out), with 0 and 16 point lights and with nothing but the sun (ambient 0: the colour is (1 - shadow) Lo, so ONE misplaced tap is a
step of Lo / 25); k_envlit, k_spotlit, k_cubelit, k_miplit and k_pbrlit through the harnesses of test_gpu_extended_shading.py and
test_gpu_material_extras.py at their bars; and that the control tiles are the same bytes whatever the other tiles' w is.

What this does NOT try: a quotient one ulp off.  The operands, the lanes and the choice of branch are checked at parity level;
tests/test_gpu_division.py enumerates the near-one quotient, and the general one is the compiler's IEEE division.
"""
import copy

import numpy as np
import pytest

import shadow_w_inputs as SW
import test_gpu_extended_shading as G
import test_gpu_material_extras as X
from test_gpu_parity import TOL

W, H, S = SW.W, SW.H, SW.S
NO_MAT = SW.NO_MAT
EXTENDED = {"env": "k_envlit", "spot": "k_spotlit", "cube": "k_cubelit", "mip": "k_miplit"}


# ---- inputs (no device; tests/test_shadow_w_inputs.py runs these builders on the CPU) ------------------------------------------------------
def base_inputs(pkg):
    """the base kernel's frame: config 3's materials and lights at its smallest scale, scenes.random_gbuffer with the light-space positions replaced"""
    sc = pkg.scenes.config3(scale=0.05)
    rng = np.random.default_rng(SW.SEED + 3)
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, len(sc.materials), coverage=0.9)
    smap = SW.shadow_map()
    ls, tile_cls, lane_cls, _, _ = SW.light_space(mat=mat, smap=smap)
    attrs[..., 14:18] = ls
    return sc, attrs, mat, smap, tile_cls


def extended_case(feature):
    return G.Case(f"general-w-{feature}", frozenset([feature]) if feature != "pbr" else frozenset(), n_points=5, seed=900 + list(EXTENDED).index(feature) if feature != "pbr" else 904)


def extended_inputs(pkg, feature):
    """one case of test_gpu_extended_shading's (or, for k_pbrlit, test_gpu_material_extras') builders with attrs[..., 14:18] and the map replaced"""
    case = extended_case(feature)
    I = (X if feature == "pbr" else G).build_inputs(pkg, case)
    I.shadow = SW.shadow_map()
    ls, I.tile_cls, _, _, _ = SW.light_space(mat=I.mat, smap=I.shadow)
    I.attrs[..., 14:18] = ls
    return case, I


def conditions(oracle, smap, attrs, mat, tile_cls):
    """the input conditions, by the CPU oracle alone; returns 1 - shadow per pixel (1 where nothing is covered), as sun_lit does"""
    f = SW.shadow_factors(oracle, smap, attrs[..., 14:18], mat)
    counts = SW.check_input_conditions(f, tile_cls, mat)
    return np.where(np.isnan(f), 1.0, 1.0 - f), counts


pytestmark = pytest.mark.gpu


# ---- the base kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base(pkg, oracle):
    sc, attrs, mat, smap, tile_cls = base_inputs(pkg)
    lit, counts = conditions(oracle, smap, attrs, mat, tile_cls)
    print("base frame, covered pixels of the general-w tiles:", counts)
    o = sc.upload(oracle.Oracle(W, H, S, sc.max_lights))
    o.write_shadow_map(smap)
    return sc, attrs, mat, smap, tile_cls, lit, o


def _desc(sc, ambient):
    d = copy.deepcopy(sc.desc)
    d.ambient = float(ambient)
    d.camera["aspect"] = W / H
    return d


@pytest.mark.parametrize("n_lights,ambient", [(0, 0.1), (16, 0.1), (0, 0.0)], ids=["no-point-lights", "16-point-lights", "sun-alone"])
def test_base_kernel_against_the_oracle(pkg, oracle, hip, base, n_lights, ambient):
    sc, attrs, mat, smap, tile_cls, lit, o = base
    desc = _desc(sc, ambient)
    r = sc.upload(hip.Renderer(W, H, S, sc.max_lights))
    r.set_option("keep_float_output", 1)
    r.update_lights(sc.lights[:n_lights]); o.update_lights(sc.lights[:n_lights])
    r.write_shadow_map(smap)
    r.write_gbuffer(attrs, mat)
    r.pass_shade(desc, sc.settings)
    ldr, hdr, rgba = [x.copy() for x in r.read_output()]
    ref = o.shade_gbuffer(desc, sc.settings, attrs, mat, threads=oracle.hardware_threads(), want=("hdr", "ldr", "rgba8"))
    err = np.abs(ldr.astype(np.float64) - ref["ldr"])
    step = np.abs(rgba.astype(np.int16) - ref["rgba8"].astype(np.int16))
    cov = mat != NO_MAT
    for c in SW.CLASSES:
        sel = cov & (tile_cls == c)
        print(f"{n_lights} lights, ambient {ambient}, tiles {c}: {int(sel.sum())} covered pixels, max |ldr - oracle| = {err[sel].max():.3e}, RGBA8 steps {int(step[sel].max())}")
    if ambient == 0.0:      # the shadow factor is visible: where the oracle's pixel is fully shadowed the colour is exactly black, where it is not it is not
        dark = cov & (lit == 0)
        assert dark.sum() >= 200 and (hdr[dark] == 0).all()
        assert (ref["hdr"][cov & (lit > 0)].max(-1) > 0).mean() > 0.2      # (about half of the random normals face the sun)
    y, x, _ = np.unravel_index(err.argmax(), err.shape)
    assert err.max() <= TOL, f"max err {err.max():.3e} at {(y, x)}: tile class {tile_cls[y, x]}, ls {attrs[y, x, 14:18]}, 1 - shadow {lit[y, x]}"
    assert step.max() <= 1
    r.close()


def test_control_tiles_do_not_depend_on_the_other_tiles(pkg, hip, base):
    """the w == 1 tiles are the same bytes whether the other tiles carry a general w or w = 1.0 as well (a second G-buffer, everything else
    unchanged); and the other tiles are NOT the same, i.e. their w was read"""
    sc, attrs, mat, smap, tile_cls, _, _ = base
    desc = _desc(sc, 0.1)
    r = sc.upload(hip.Renderer(W, H, S, sc.max_lights))
    r.set_option("keep_float_output", 1)
    r.update_lights(sc.lights[:16])
    r.write_shadow_map(smap)
    out = []
    second = attrs.copy()
    second[..., 14:18] = SW.with_w_one(attrs[..., 14:18], tile_cls)
    for a in (attrs, second):
        r.write_gbuffer(a, mat)
        r.pass_shade(desc, sc.settings)
        out.append([x.copy() for x in r.read_output()])
    e = tile_cls == "e"
    assert (e & (mat != NO_MAT)).sum() > 500
    for a, b in zip(*out):
        np.testing.assert_array_equal(a[e].view(np.uint8), b[e].view(np.uint8))
    assert (out[0][1] != out[1][1]).any(-1)[~e].mean() > 0.03
    r.close()


# ---- the extended kernels ----------------------------------------------------------------------------------------------------------------
def _handle(hip, case, I):
    """test_gpu_extended_shading._injected_handle with this file's map size"""
    r = hip.Renderer(case.width, case.frame_rows, S, 16)
    r.set_option("texture_mips", int("mip" in case.features))
    for d, n, m in I.images:
        r.create_material(d, n, m)
    r.create_hdri(I.env_map)
    r.update_lights(I.points)
    r.write_gbuffer(I.attrs, I.mat)
    r.write_shadow_map(I.shadow)
    for opt, v in (("keep_float_output", 1), ("point_shadow_size", G.F), ("sampler", case.sampler), ("hdr16", case.hdr16), ("culling", case.culling),
                   ("light_path", case.light_path)):
        r.set_option(opt, v)
    return r


@pytest.mark.parametrize("feature", list(EXTENDED) + ["pbr"])
def test_extended_kernels(pkg, oracle, hip, feature):
    case, I = extended_inputs(pkg, feature)
    _, counts = conditions(oracle, I.shadow, I.attrs, I.mat, I.tile_cls)
    print(f"{case.name}: covered pixels of the general-w tiles: {counts}")
    r = _handle(hip, case, I)
    G._configure(r, I, case.features)
    if feature == "pbr":
        X._apply(r, I.extras)
    ldr, hdr, rgba = G._shade(r, I)
    attrs = r.read_gbuffer(want=("attrs",))[0]                   # the G-buffer the kernels read (an input, read back)
    cov = I.mat != NO_MAT
    np.testing.assert_array_equal(attrs[cov].view(np.uint32), I.attrs[cov].view(np.uint32))
    env_tables = r.read_env_lighting() if "env" in case.features else None
    materials = G._device_materials(r, I.images, chains="mip" in case.features)
    lit = G.sun_lit(oracle, I.shadow, attrs, I.mat)
    if feature == "pbr":
        ref = X.reference_for(case, I, lit, materials, env_tables, attrs=attrs)
    else:
        ref = G.reference_for(case, I, lit, materials, env_tables, attrs=attrs)
        _configure_off = case.features - {feature}                # it did not fall back to the base kernel: the feature switched off moves the judged pixels
        G._configure(r, I, _configure_off)
        off = G._shade(r, I)
        assert np.abs(off[1] - hdr)[ref["judged"]].max() > 1e-3
    r.close()
    left_out = 1 - ref["judged"].sum() / ref["covered"].sum()
    print(f"{case.name}: {left_out:.4f} of the covered pixels left out")
    assert left_out <= 0.10                                       # (the mask's standing limit: test_visibility_path)
    (X if feature == "pbr" else G).judge(case.name, ref, ldr, hdr)
