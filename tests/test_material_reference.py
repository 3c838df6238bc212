"""tests/material_reference.py pinned on the CPU: by hand on 1 x 1 constant materials (closed forms, each term alone and all together), exactly
equal to tests/shading_reference.py when every material is neutral, and -- for the inputs of every GPU case of
tests/test_gpu_material_extras.py -- able to tell each deliberate defect of material_reference.MUTATIONS from the truth, with the project's
standing constants (tests/test_shading_reference.py: a defect moves at least MOVED_SHARE of the judged pixels by more than 10 x TOL, the mask
leaves out at most LEFT_OUT of the covered pixels).  These are conditions on the INPUTS: a case that misses one gets other inputs, not another bar.
"""
import numpy as np
import pytest

import material_reference as XR
import mip_reference as MR
import shading_reference as SR
import test_gpu_extended_shading as G
import test_gpu_material_extras as GX
from test_shading_reference import LEFT_OUT, MOVED_BY, MOVED_SHARE

assert (MOVED_BY, MOVED_SHARE, LEFT_OUT) == (10 * G.TOL, 0.01, 0.10)
assert (XR.LDR_BAR, XR.HDR_BAR) == (G.TOL, G.HDR_REL)
T = MR.srgb_table().astype(np.float64)


# ---- by hand -----------------------------------------------------------------------------------------------------------------------------
def _pixel(normal=(0.0, 1.0, 0.0), world=(0.0, 0.0, 0.0)):
    """one covered pixel: tangent frame T = +x, B = +z, N = `normal`'s axis frame, at `world`"""
    a = np.zeros((1, 1, 18))
    a[0, 0, 0:2] = (0.3, 0.6)
    a[0, 0, 2:5], a[0, 0, 5:8], a[0, 0, 8:11] = (1, 0, 0), (0, 0, 1), normal
    a[0, 0, 11:14] = world
    return a, np.zeros((1, 1), np.uint32)


def _constant(diffuse=(200, 120, 60), normal=(128, 128, 255), rough=128, metal=0):
    """one material: a chain of one 1 x 1 level"""
    px = lambda *c: np.array([[list(c) + [255]]], np.uint8)
    return [MR.pack(px(*diffuse), px(*normal), px(255, rough, metal))]


ARGS = dict(eye=(0.0, 5.0, 0.0), sun_rotation=(-60.0, 30.0), sun_color=(3.0, 2.5, 2.0), ambient=0.25, settings=(1, 2.2, 1.0))


def _shade(extras, lit=1.0, materials=None, mutate=(), **kw):
    attrs, mat = _pixel()
    materials = materials or _constant()
    ch = SR.material_channels([materials], attrs, mat)
    args = dict(ARGS, **kw)
    return XR.shade(attrs, mat, ch, np.full((1, 1), lit), args["eye"], args["sun_rotation"], args["sun_color"], args["ambient"], args["settings"],
                    [extras], mutate=mutate), ch


def _params(**kw):
    p = {f: np.asarray(v, np.float32) for f, v in XR.NEUTRAL.items()}
    p.update({k: np.asarray(v, np.float32) for k, v in kw.items()})
    return p


def _image(r, g, b, w=1, h=1):
    a = np.zeros((h, w, 4), np.uint8)
    a[...] = (r, g, b, 255)
    return a


def test_neutral_is_shading_reference_exactly():
    attrs, mat = _pixel()
    ch = SR.material_channels([_constant()], attrs, mat)
    want = SR.shade(attrs, mat, ch, np.full((1, 1), 0.4), ARGS["eye"], ARGS["sun_rotation"], ARGS["sun_color"], ARGS["ambient"], ARGS["settings"])
    for x in (None, XR.extras(), XR.extras(_params())):
        assert XR.is_neutral(x)
        got, _ = _shade(x, lit=0.4)
        np.testing.assert_array_equal(got["hdr"], want["hdr"])
        np.testing.assert_array_equal(got["ldr"], want["ldr"])
    assert not XR.is_neutral(XR.extras(_params(normal_scale=2.0))) and not XR.is_neutral(XR.extras(None, _image(1, 2, 3)))


def test_fully_shadowed_pixel_closed_forms():
    """lit = 0: color = ambient base' ao + E, each term alone and all together"""
    base = T[[200, 120, 60]]
    amb = float(np.float32(0.25))
    # base colour factor alone
    got, _ = _shade(XR.extras(_params(base_color_factor=(0.5, 0.25, 1.0))), lit=0.0)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base * np.float32([0.5, 0.25, 1.0]).astype(np.float64), rtol=1e-15)
    # emissive factor without an image: e = 1
    got, _ = _shade(XR.extras(_params(emissive_factor=(0.5, 4.0, 0.125))), lit=0.0)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base + [0.5, 4.0, 0.125], rtol=1e-15)
    np.testing.assert_array_equal(got["E"][0, 0], [0.5, 4.0, 0.125])
    # emissive image: decoded per texel
    got, _ = _shade(XR.extras(_params(emissive_factor=(1.0, 2.0, 0.5)), emissive=_image(255, 128, 10)), lit=0.0)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base + T[[255, 128, 10]] * [1.0, 2.0, 0.5], rtol=1e-15)
    # occlusion: R channel, linear; ao = 1 + strength (o - 1)
    got, _ = _shade(XR.extras(_params(occlusion_strength=0.5), occlusion=_image(51, 7, 9)), lit=0.0)
    assert got["ao"][0, 0] == pytest.approx(1 + float(np.float32(0.5)) * (51 / 255 - 1), rel=1e-15) == pytest.approx(0.6, rel=1e-12)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base * 0.6, rtol=1e-12)
    # occlusion strength without an image does nothing (o = 1)
    got, _ = _shade(XR.extras(_params(occlusion_strength=0.25)), lit=0.0)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base, rtol=1e-15)
    # all together; metallic, roughness and the normal scale do not reach a shadowed pixel without ENV
    x = XR.extras(_params(base_color_factor=(0.5, 0.25, 1.0), metallic_factor=0.3, roughness_factor=0.6, normal_scale=1.9, occlusion_strength=0.5,
                          emissive_factor=(1.0, 2.0, 0.5)), emissive=_image(255, 128, 10), occlusion=_image(51, 0, 0))
    got, _ = _shade(x, lit=0.0)
    np.testing.assert_allclose(got["hdr"][0, 0], amb * base * [0.5, 0.25, 1.0] * 0.6 + T[[255, 128, 10]] * [1.0, 2.0, 0.5], rtol=1e-12)
    np.testing.assert_allclose((got["A"] * got["ao"][..., None] + got["E"])[0, 0], got["hdr"][0, 0], rtol=1e-15)


def test_bilinear_wrap_of_the_two_images():
    """a 2 x 1 occlusion image at u = 0.5: texel centres at 0.25 and 0.75, so u = 0.5 is half of each; u = 0 wraps: half of each again;
    u = 0.25: texel 0 alone"""
    occ = np.zeros((1, 2, 4), np.uint8)
    occ[0, 0, 0], occ[0, 1, 0] = 255, 51
    attrs, mat = _pixel()
    for u, want in ((0.5, 0.6), (0.0, 0.6), (0.25, 1.0), (0.75, 0.2), (0.375, 0.8)):
        attrs[0, 0, 0] = u
        X = XR.extra_channels([XR.extras(None, None, occ)], attrs, mat)
        assert X["o"][0, 0] == pytest.approx(want, rel=1e-12), u


def test_lit_pixel_factors_reach_the_brdf():
    """lit = 1, no emission, no occlusion: the result is shading_reference's on hand-modified channels"""
    attrs, mat = _pixel()
    materials = _constant(normal=(168, 108, 240), rough=200, metal=255)
    ch = SR.material_channels([materials], attrs, mat)
    s = 1.5
    p = _params(base_color_factor=(0.5, 0.75, 1.0), metallic_factor=0.5, roughness_factor=0.25, normal_scale=s)
    got, _ = _shade(XR.extras(p), materials=materials)
    by_hand = ch.copy()
    by_hand[..., 0:3] *= [0.5, 0.75, 1.0]
    by_hand[..., 6] *= 0.25
    by_hand[..., 7] *= 0.5
    # the normal: t = (168 * 2 / 255 - 1, -(108 * 2 / 255 - 1), 240 * 2 / 255 - 1); n' = normalize(T t.x s + B t.y s + N t.z), T = x, B = z, N = y
    t = np.array([168 * 2 / 255 - 1, -(108 * 2 / 255 - 1), 240 * 2 / 255 - 1])
    n = np.array([t[0] * s, t[2], t[1] * s])
    n /= np.linalg.norm(n)
    np.testing.assert_allclose(SR.surface_normal(attrs, got["ch"])[0, 0], n, rtol=1e-13)
    by_hand[..., 3] = (t[0] * s + 1) * 255 / 2
    by_hand[..., 4] = (-t[1] * s + 1) * 255 / 2
    want = SR.shade(attrs, mat, by_hand, np.ones((1, 1)), ARGS["eye"], ARGS["sun_rotation"], ARGS["sun_color"], ARGS["ambient"], ARGS["settings"])
    np.testing.assert_allclose(got["hdr"], want["hdr"], rtol=1e-12)
    assert got["rough"][0, 0] == pytest.approx(200 / 255 * 0.25, rel=1e-12) and got["metal"][0, 0] == pytest.approx(0.5, rel=1e-12)
    # Lo (1 - shadow) and A come apart: half the light, the same ambient
    half, _ = _shade(XR.extras(p), materials=materials, lit=0.5)
    np.testing.assert_allclose(half["lo_lit"], 0.5 * got["lo_lit"], rtol=1e-13)
    np.testing.assert_allclose(half["A"], got["A"], rtol=1e-12)
    np.testing.assert_allclose(got["A"][0, 0], float(np.float32(0.25)) * by_hand[0, 0, 0:3], rtol=1e-12)


def test_all_terms_together_and_binary16():
    materials = _constant(normal=(150, 120, 250), rough=180, metal=0)
    x = XR.extras(_params(base_color_factor=(0.9, 0.8, 0.7), roughness_factor=0.5, occlusion_strength=0.75, emissive_factor=(0.5, 0.25, 2.0)),
                  emissive=_image(40, 200, 90), occlusion=_image(102, 0, 0))
    got, _ = _shade(x, materials=materials, lit=0.6)
    ao = 1 + 0.75 * (102 / 255 - 1)
    E = T[[40, 200, 90]] * [0.5, 0.25, 2.0]
    np.testing.assert_allclose(got["hdr"][0, 0], got["lo_lit"][0, 0] + got["A"][0, 0] * ao + E, rtol=1e-13)
    assert (got["lo_lit"][0, 0] > 0).all()
    # the mutations, each by its closed form
    lit = 0.6
    m = lambda name: _shade(x, materials=materials, lit=lit, mutate=(name,))[0]
    np.testing.assert_allclose(m("ao_on_direct")["hdr"][0, 0], (got["lo_lit"][0, 0] + got["A"][0, 0]) * ao + E, rtol=1e-13)
    np.testing.assert_allclose(m("emissive_times_lit")["hdr"][0, 0], got["lo_lit"][0, 0] + got["A"][0, 0] * ao + E * lit, rtol=1e-13)
    np.testing.assert_allclose(m("emissive_not_decoded")["hdr"][0, 0], got["lo_lit"][0, 0] + got["A"][0, 0] * ao + np.array([40, 200, 90]) / 255 * [0.5, 0.25, 2.0], rtol=1e-13)
    np.testing.assert_allclose(m("strength_ignored")["hdr"][0, 0], got["lo_lit"][0, 0] + got["A"][0, 0] * 0.4 + E, rtol=1e-12)
    assert m("metal_rough_factors_swapped")["rough"][0, 0] == pytest.approx(180 / 255) and m("metal_rough_factors_swapped")["metal"][0, 0] == 0
    y = XR.extras(_params(normal_scale=3.0))
    truth, plain = _shade(y, materials=materials)[0], _shade(None, materials=materials)[0]
    zed = _shade(y, materials=materials, mutate=("scale_on_z",))[0]
    assert np.abs(truth["hdr"] - plain["hdr"]).max() > 1e-3
    np.testing.assert_allclose(zed["hdr"], plain["hdr"], rtol=1e-9)          # a scale on all three components cancels in the normalisation
    # binary16 before the tonemapper
    attrs, mat = _pixel()
    ch = SR.material_channels([materials], attrs, mat)
    q = XR.shade(attrs, mat, ch, np.full((1, 1), lit), ARGS["eye"], ARGS["sun_rotation"], ARGS["sun_color"], ARGS["ambient"], ARGS["settings"], [x], hdr16=True)
    np.testing.assert_array_equal(q["hdr"], got["hdr"])
    import env_reference as ER
    np.testing.assert_array_equal(q["ldr"], ER.tonemap(1, got["hdr"].astype(np.float16).astype(np.float64), float(np.float32(2.2)), 1.0))
    assert np.abs(q["ldr"] - got["ldr"]).max() > 0


def test_tonemap_moved_by_hand():
    """Reinhard at c = 1 in closed form; under ACES a grey is judged on LDR and a saturated blue whose red output cancels to 6e-6 is not"""
    g = float(np.float32(2.2))
    slope = (1 / g) * 0.5 ** (1 / g - 1) * 0.25                                  # d/dc (c / (c + 1))^(1 / g) at c = 1
    np.testing.assert_allclose(XR.tonemap_moved((0, 2.2, 1.0), np.ones((1, 1, 3))), 3 * slope * XR.HDR_BAR * 1.001, rtol=1e-3)
    assert XR.tonemap_moved((2, 2.2, 1.0), np.full((1, 1, 3), 0.5))[0, 0] < XR.LDR_BAR
    blue = np.array([[[0.03325381, 0.11907961, 0.64210604]]])
    import env_reference as ER
    assert 0 < ER.tonemap(2, blue, g, 1.0)[0, 0, 0] ** g < 1e-5 and XR.tonemap_moved((2, 2.2, 1.0), blue)[0, 0] > XR.LDR_BAR
    # ... and shade() keeps such a pixel for the HDR bar: an emissive of that colour on a black, unlit, fully shadowed material
    x = XR.extras(_params(emissive_factor=blue[0, 0], base_color_factor=(0, 0, 0)))
    got, _ = _shade(x, lit=0.0, settings=(2, 2.2, 1.0))
    assert got["judged_hdr"].all() and not got["judged"].any() and got["reasons"]["tonemap"].all()
    got, _ = _shade(XR.extras(_params(emissive_factor=(0.5, 0.5, 0.5))), lit=0.0, settings=(2, 2.2, 1.0))
    assert got["judged_hdr"].all() and got["judged"].all()


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GX.CASES, ids=repr)
def test_gpu_case_inputs_are_sensitive_and_mostly_judged(pkg, oracle, case):
    I = GX.build_inputs(pkg, case)
    lit = G.sun_lit(oracle, I.shadow, I.attrs, I.mat)
    cov = I.mat != SR.NO_MAT
    materials = G.host_materials(I.images, "mip" in case.features)
    env = G.host_env_tables(I.env_map) if "env" in case.features else None
    truth = GX.reference_for(case, I, lit, materials, env)
    # the inputs' own conditions: rough' at or above 13 / 255, no grazing view under the scaled normal, every kind of material under the frame
    assert truth["rough"][cov].min() >= 13 / 255 - 1e-12
    n = SR.surface_normal(I.attrs, truth["ch"])
    wo = SR.f32(I.eye) - I.attrs[..., 11:14].astype(np.float64)
    wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
    assert np.abs((n * wo).sum(-1))[cov].min() >= G.GRAZING
    assert all((I.mat == m).sum() > 128 for m in range(4))
    assert I.extras[1] is None and I.extras[0][1].shape[:2] == I.images[0][0].shape[:2] and I.extras[2][1].shape[:2] == (4, 8) and I.extras[3][2].shape[:2] == (3, 5)
    left_out = 1 - truth["judged"].sum() / cov.sum()
    j = truth["judged"]
    shares = {m: float((np.abs(GX.reference_for(case, I, lit, materials, env, mutate=(m,))["ldr"] - truth["ldr"]).max(-1)[j] > MOVED_BY).mean()) for m in XR.MUTATIONS}
    print(f"{case.name}: left out {left_out:.4f} (of which the tonemapper's clip {truth['reasons']['tonemap'].sum() / cov.sum():.4f}); moved by more than {MOVED_BY:g}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert left_out <= LEFT_OUT, (case.name, left_out)
    for k, v in shares.items():
        assert v >= MOVED_SHARE, (case.name, k, v)
    # each extended material is seen at all: the GPU case asserts the same of the device
    for m in (0, 2, 3):
        off = GX.reference_for(case, I, lit, materials, env, extras=[None if k == m else x for k, x in enumerate(I.extras)])
        assert np.abs(off["hdr"] - truth["hdr"])[j & (I.mat == m)].max() > 1e-3, (case.name, m)
    if case.half_shadow:
        left = slice(0, case.width // 2)
        assert (lit[:, left][cov[:, left]] == 0).all() and (truth["lo_lit"][:, left][j[:, left]] == 0).all()


def test_cases_cover_what_the_issue_lists():
    names = {c.name for c in GX.CASES}
    for t in ("none", "env", "mip", "spot+cube", "all"):
        assert {f"extras-{t}-path1", f"extras-{t}-path2"} <= names
    for t in ("none", "all"):
        assert {f"extras-{t}-{e}" for e in ("points0", "points13", "culling0", "100x70", "rows13to77", "sampler1", "hdr16", "half-shadowed")} <= names
    assert len(set(XR.MUTATIONS)) >= 6
