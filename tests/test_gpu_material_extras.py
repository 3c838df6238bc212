"""glTF material factors, emissive and occlusion (arctic_set_material_extras, the k_pbrlit / k_pbrlit_vis kernels) against the float64 pixel
of tests/material_reference.py, on the injected frames of tests/test_gpu_extended_shading.py (its builders, imported).

The four materials of that file get extras (material_extras below): 0 takes the fast path (emissive + occlusion of its own size), 1 stays
neutral, 2 (images of unequal sizes) an 8 x 4 emissive, 3 (1 x 1, packed) a 5 x 3 occlusion -- the cold path on a packed material.  Each case
asserts: parity at the standing bars (judge below); the pixels of the neutral material and the pixels without geometry bit-equal to the same handle with
every material reset; that reset handle bit-equal to a fresh one that never had extras; each extended material seen; and, in the
half-shadowed case, the shadowed half equal to A ao + E.

The builders (CASES, build_inputs, reference_for) need no device: tests/test_material_reference.py shows on the CPU that each case's inputs
tell the deliberate defects of material_reference.MUTATIONS from the truth.
"""
import numpy as np
import pytest

import material_reference as XR
import shading_reference as SR
import test_gpu_extended_shading as G

pytestmark = pytest.mark.gpu
NO_MAT = G.NO_MAT
SETS = {"none": frozenset(), "env": frozenset(["env"]), "mip": frozenset(["mip"]), "spot+cube": frozenset(["spot", "cube"]), "all": G.ALL}


def _cases():
    out = [G.Case(f"extras-{t}-path{lp}", fs, light_path=lp, n_points=5, seed=300 + 2 * k + lp) for k, (t, fs) in enumerate(SETS.items()) for lp in (1, 2)]
    for k, t in enumerate(("none", "all")):
        fs, s = SETS[t], 340 + 20 * k
        out += [G.Case(f"extras-{t}-points0", fs, n_points=0, tm=0, seed=s),
                G.Case(f"extras-{t}-points13", fs, n_points=13, tm=1, seed=s + 1),           # automatic switch to the packed loop, odd tail
                G.Case(f"extras-{t}-culling0", fs, culling=0, light_path=2, seed=s + 2),
                G.Case(f"extras-{t}-100x70", fs, width=100, rows=70, tm=0, seed=s + 3),      # ragged right and bottom tiles
                G.Case(f"extras-{t}-rows13to77", fs, row_begin=13, frame_rows=96, tm=1, seed=s + 4),   # a shard cut inside a tile row
                G.Case(f"extras-{t}-sampler1", fs, sampler=1, seed=s + 5),
                G.Case(f"extras-{t}-hdr16", fs, hdr16=1, seed=s + 6),
                G.Case(f"extras-{t}-half-shadowed", fs, half_shadow=True, n_points=13, seed=s + 7)]
    return out


CASES = _cases()


# ---- inputs (no device) ------------------------------------------------------------------------------------------------------------
def _params(pkg, **kw):
    p = pkg.scene.neutral_material_params()
    for k, v in kw.items():
        p[k] = v
    return p[0]


def material_extras(pkg, rng, images):
    """the extras of the four materials: (params record, emissive, occlusion) or None"""
    h0, w0 = images[0][0].shape[:2]
    img = lambda w, h: G._random_images(rng, w, h)[0]
    return [(_params(pkg, base_color_factor=(0.8, 0.6, 0.9), metallic_factor=0.4, roughness_factor=0.8, normal_scale=1.7, occlusion_strength=0.8,
                     emissive_factor=(2.0, 1.0, 0.5)), img(w0, h0), img(w0, h0)),
            None,
            (_params(pkg, base_color_factor=(0.5, 0.9, 0.7), metallic_factor=0.9, roughness_factor=0.6, emissive_factor=(0.7, 0.9, 1.2)), img(8, 4), None),
            (_params(pkg, occlusion_strength=0.5, emissive_factor=(0.3, 0.2, 0.4)), None, img(5, 3))]


def reference_extras(extras):
    return [None if x is None else XR.extras(*x) for x in extras]


def _steer_clear_of_grazing_views(rng, case, I):
    """test_gpu_extended_shading._steer_clear_of_grazing_views with the normal the extras give (normal_scale tilts it): redraw the world position
    of the pixels whose |n'.wo| is below GRAZING"""
    materials = G.host_materials(I.images, "mip" in case.features)
    ch = SR.material_channels(materials, I.attrs, I.mat, lod=I.lod if "mip" in case.features else None, q8=bool(case.sampler & 1))
    X = XR.extra_channels(reference_extras(I.extras), I.attrs, I.mat, q8=bool(case.sampler & 1))
    n = SR.surface_normal(I.attrs, XR.apply_factors(ch, X))
    lo, hi = np.asarray(G.BOX_LO, np.float32), np.asarray(G.BOX_HI, np.float32)
    for _ in range(100):
        wo = SR.f32(I.eye) - I.attrs[..., 11:14].astype(np.float64)
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        bad = (I.mat != NO_MAT) & (np.abs((n * wo).sum(-1)) < G.GRAZING)
        if not bad.any():
            return
        I.attrs[bad, 11:14] = lo + rng.random((int(bad.sum()), 3), dtype=np.float32) * (hi - lo)
    raise AssertionError("grazing views left")


def build_inputs(pkg, case):
    """test_gpu_extended_shading.build_inputs plus the extras; roughness bytes of the materials whose roughness_factor is below 1 raised to 26 and
    above, so that rough' stays at or above 13 / 255 (the smallest roughness the existing cases carry: below it the NDF is ill-conditioned in fp32)"""
    I = G.build_inputs(pkg, case)
    rng = np.random.default_rng(9000 + case.seed)
    I.extras = material_extras(pkg, rng, I.images)
    images = []
    for (d, n, m), x in zip(I.images, I.extras):
        if x is not None and x[0]["roughness_factor"] < 1:
            assert x[0]["roughness_factor"] >= 0.5
            m = m.copy()
            m[..., 1] = np.maximum(m[..., 1], 26)
        images.append((d, n, m))
    I.images = images
    _steer_clear_of_grazing_views(rng, case, I)
    return I


def reference_for(case, I, lit, materials, env_tables, attrs=None, extras=None, mutate=()):
    attrs = I.attrs if attrs is None else attrs
    on, q8 = case.features, bool(case.sampler & 1)
    ch = SR.material_channels(materials, attrs, I.mat, lod=I.lod if "mip" in on else None, q8=q8)
    return XR.shade(attrs, I.mat, ch, lit, I.eye, I.sun["rotation"], I.sun["color"], I.ambient, I.settings,
                    reference_extras(I.extras if extras is None else extras), q8=q8, hdr16=bool(case.hdr16), mutate=mutate, points=I.points,
                    spots=I.spots if "spot" in on else (), cubes=I.cubes if "cube" in on else (), faces=I.faces if "cube" in on else (),
                    env=env_tables if "env" in on else None)


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def judge(name, ref, ldr, hdr, hdr16=False):
    """test_gpu_extended_shading.judge (both bars) on the judged pixels, and the HDR bar on the pixels material_reference.tonemap_moved keeps
    from the LDR bar as well (`judged_hdr`): nothing escapes the HDR bar.  Under ARCTIC_OPT_HDR16 the stored colour is the binary16 rounding
    of one within the bar: half an ulp, 2^-11 of the value, on top."""
    j = ref["judged_hdr"]
    rel = float((np.abs(hdr.astype(np.float64) - ref["hdr"]) / (np.abs(ref["hdr"]) + 1e-3))[j].max())
    bar = G.HDR_REL + 2.0 ** -11 * (1 + G.HDR_REL) if hdr16 else G.HDR_REL
    print(f"{name}: hdr_rel over all {int(j.sum())} pixels = {rel:.3e} (bar {bar:.3e}), {int(ref['reasons']['tonemap'].sum())} left to the HDR bar alone")
    rec = G.judge(name, ref, ldr, hdr, hdr16=hdr16)
    assert rel <= bar, (name, rel)
    return rec


def _apply(r, extras, only=None):
    for m, x in enumerate(extras):
        if only is None or m == only:
            r.set_material_extras(m, *(x or (None, None, None)))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_injected_extras(pkg, oracle, hip, case):
    I = build_inputs(pkg, case)
    r = G._injected_handle(hip, case, I)
    G._configure(r, I, case.features)
    _apply(r, I.extras)
    ldr, hdr, rgba = G._shade(r, I)
    attrs = r.read_gbuffer(want=("attrs",))[0]                   # the G-buffer the kernels read (an input, read back)
    cov = I.mat != NO_MAT
    np.testing.assert_array_equal(attrs[cov], I.attrs[cov])
    env_tables = r.read_env_lighting() if "env" in case.features else None
    materials = G._device_materials(r, I.images, chains="mip" in case.features)
    lit = G.sun_lit(oracle, I.shadow, attrs, I.mat)
    ref = reference_for(case, I, lit, materials, env_tables, attrs=attrs)
    # 4. each ingredient is seen: one material reset alone moves its judged pixels
    for m in (0, 2, 3):
        r.set_material_extras(m)
        off = G._shade(r, I)
        sel = ref["judged"] & (I.mat == m)
        assert sel.any() and np.abs(off[1] - hdr)[sel].max() > 1e-3, (case.name, m)
        _apply(r, I.extras, only=m)
    again = G._shade(r, I)
    for a, b in zip((ldr, hdr, rgba), again):
        np.testing.assert_array_equal(a, b)
    # 2. the pixels of the neutral material and the pixels without geometry: the bits of the same handle with every material reset
    for m in range(len(I.extras)):
        r.set_material_extras(m)
    reset = G._shade(r, I)
    neutral = (I.mat == 1) | ~cov
    assert (I.mat == 1).sum() > 128
    for a, b in zip((ldr, hdr, rgba), reset):
        np.testing.assert_array_equal(a[neutral], b[neutral])
    r.close()
    # 3. ... and that is a handle that never had extras: it fell back to today's kernels
    fresh = G._injected_handle(hip, case, I)
    G._configure(fresh, I, case.features)
    never = G._shade(fresh, I)
    fresh.close()
    for a, b in zip(reset, never):
        np.testing.assert_array_equal(a, b)
    # 5. the fully shadowed half is A ao + E: emission survives the sun's shadow, direct light does not
    if case.half_shadow:
        left = np.zeros(cov.shape, bool)
        left[:, : case.width // 2] = True
        sel = left & ref["judged"]
        assert (lit[left & cov] == 0).all() and (ref["lo_lit"][sel] == 0).all() and (ref["E"][sel].max(-1) > 0.05).mean() > 0.3
        want = (ref["A"] * ref["ao"][..., None] + ref["E"])[sel]
        rel = np.abs(hdr[sel].astype(np.float64) - want) / (np.abs(want) + 1e-3)
        print(f"{case.name}: shadowed half against A ao + E: relative HDR {rel.max():.3e}")
        assert rel.max() <= G.HDR_REL, (case.name, rel.max())
    # 1. parity
    judge(case.name, ref, ldr, hdr, hdr16=bool(case.hdr16))


@pytest.mark.parametrize("cfg,scale", [(2, 0.25), (3, 0.1)])
def test_visibility_path_with_extras(pkg, oracle, hip, cfg, scale):
    """render_frame through k_pbrlit_vis = pass_gbuffer + pass_shade through k_pbrlit bit for bit, mips on and off, and the latter against the
    reference built from what the handle itself holds.  Material 0 gets images of its own size (the fast path), material 5 a differently
    sized emissive (the cold path on a packed material).

    The new images are smooth, as the scenes' own textures are (scenes.make_material_textures; a periodic wave for the 24 x 12 one, so that
    WRAP has no seam).  The scenes tile their materials (uv up to 7.5), and the fp32 footprint -- the same one for all of a material's images
    -- carries a bilinear weight to about half an ulp of the texel coordinate: 4e-6 at the 102 texels of config 3 here, 3e-5 at config 2's 512.
    A weight error dw moves a filtered value by dw x (the step between the two texels).  Per-texel noise has steps of the order of the value
    range, i.e. 3e-6 ... 2e-5 absolute on an emission of 0.01 ... 1, which is the HDR bar's 1e-4 (|c| + 1e-3) and more: config 3's floor showed
    1.7e-4 that way.  Between neighbours that differ by a fraction of their value the same dw is a few 1e-6 of the value.  The injected cases
    keep their noise images: 64 texels and uv below 4 there."""
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    r = hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
    r.set_option("texture_mips", 1)
    sc.upload(r)
    r.set_option("keep_float_output", 1)
    rng = np.random.default_rng(50 + cfg)
    h0, w0 = sc.materials[0][0].shape[:2]
    assert h0 == w0
    smooth = lambda: pkg.scenes.make_material_textures(rng, w0)[0]
    y, x = np.mgrid[0:12, 0:24] + 0.5
    wave = np.full((12, 24, 4), 255, np.uint8)
    for c, phase in enumerate((0.0, 2.1, 4.2)):   # bytes 90 ... 210, periodic in both directions
        wave[..., c] = np.rint(150 + 60 * np.sin(2 * np.pi * x / 24 + phase) * np.cos(2 * np.pi * y / 12))
    extras = [None] * len(sc.materials)
    extras[0] = (_params(pkg, base_color_factor=(0.9, 0.7, 0.8), metallic_factor=0.5, normal_scale=1.25, occlusion_strength=0.7,
                         emissive_factor=(0.6, 0.4, 0.8)), smooth(), smooth())
    extras[5] = (_params(pkg, base_color_factor=(0.6, 0.9, 0.8), emissive_factor=(0.5, 0.8, 0.3)), wave, None)
    _apply(r, extras)
    I = G._frame_inputs(sc, (), ())
    materials = G._device_materials(r, sc.materials, chains=True)   # (the chains the handle holds, read back while the option is on)
    for mips in (1, 0):
        r.set_option("texture_mips", mips)
        r.set_option("visbuffer", 1)
        img_out = r.render_frame(sc.desc, sc.settings)
        vis = [x.copy() for x in r.read_output()]
        np.testing.assert_array_equal(img_out, vis[2])
        r.pass_gbuffer(sc.desc)
        r.pass_shade(sc.desc, sc.settings)
        gb = [x.copy() for x in r.read_output()]
        for a, b in zip(vis, gb):
            np.testing.assert_array_equal(a, b)
        attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
        assert (mat == 0).sum() > 64
        lod = r.read_lod() if mips else None
        smap = r.read_shadow_map() if r.shadow_size else None
        ch = SR.material_channels(materials, attrs, mat, lod=lod)
        ref = XR.shade(attrs, mat, ch, G.sun_lit(oracle, smap, attrs, mat), I.eye, I.sun["rotation"], I.sun["color"], I.ambient, I.settings,
                       reference_extras(extras), points=I.points)
        judge(f"extras-visibility-config{cfg}-mips{mips}", ref, gb[0], gb[1])
        assert 1 - ref["judged"].sum() / ref["covered"].sum() <= 0.10    # (the mask's standing limit, as test_visibility_path asserts it)
        if mips == 0:   # the extras are seen in the frame
            for m in range(len(extras)):
                r.set_material_extras(m)
            r.pass_shade(sc.desc, sc.settings)
            plain = r.read_output()[1]
            assert np.abs(plain - gb[1])[ref["judged"] & (mat == 0)].max() > 1e-3
    r.close()
