"""The pixel with glTF material factors, emissive and occlusion in float64 numpy, written from include/arctic_hip.h (the text next to
arctic_set_material_extras) alone, on top of tests/shading_reference.py:

    base'  = base * base_color_factor          metal' = metal * metallic_factor          rough' = rough * roughness_factor
    n'     = normalize(T t.x s + B t.y s + N t.z),  t = today's tangent-space normal, s = normal_scale
    ao     = 1 + occlusion_strength (o - 1)     E = e * emissive_factor                   (o, e: bilinear + WRAP at level 0; no image: 1)
    color  = Lo(base', metal', rough', n') (1 - shadow) + A ao + E,   A = ambient * base'  or  ambient * ibl(n', wo, base', metal', rough')

It never calls the product library.  The factors and the normal scale go into the `ch` array shading_reference.shade already takes (the
normal re-encoded onto the 0..255 scale in float64), Lo (1 - shadow) and A are taken apart by evaluating that function at the scene's
ambient and at ambient 0, and the colour is formed as  full + A (ao - 1) + E  -- the same number as the formula above, and exactly
shading_reference's when every material is neutral.  tests/test_material_reference.py pins it by hand on constant materials.

`shade(..., mutate={...})` evaluates a deliberately WRONG variant (MUTATIONS), as shading_reference does: the CPU tests show that the inputs
of the GPU cases tell each of them from the truth.
"""
import numpy as np

import env_reference as ER
import mip_reference as MR
import shading_reference as SR

NO_MAT = SR.NO_MAT
FIELDS = ("base_color_factor", "metallic_factor", "roughness_factor", "normal_scale", "occlusion_strength", "emissive_factor")
NEUTRAL = dict(base_color_factor=(1.0, 1.0, 1.0), metallic_factor=1.0, roughness_factor=1.0, normal_scale=1.0, occlusion_strength=1.0,
               emissive_factor=(0.0, 0.0, 0.0))
MUTATIONS = ("ao_on_direct",                  # occlusion scales the lights as well
             "emissive_times_lit",            # emission carries (1 - shadow)
             "emissive_not_decoded",          # the emissive image filtered as linear bytes
             "scale_on_z",                    # the normal scale on all three components (it cancels in the normalisation)
             "metal_rough_factors_swapped",
             "strength_ignored")              # ao = o


def extras(params=None, emissive=None, occlusion=None):
    """one material's extras: params = a record / dict with FIELDS (None: neutral), images (h, w, 4) uint8 or None"""
    p = dict(NEUTRAL)
    if params is not None:
        for f in FIELDS:
            p[f] = np.asarray(params[f], np.float32).astype(np.float64).reshape(-1)   # the fp32 values the library is handed
            p[f] = p[f] if len(p[f]) == 3 else float(p[f][0])
    return dict(params=p, emissive=None if emissive is None else np.asarray(emissive, np.uint8),
                occlusion=None if occlusion is None else np.asarray(occlusion, np.uint8))


def is_neutral(x):
    return x is None or (x["emissive"] is None and x["occlusion"] is None and
                         all(np.array_equal(np.asarray(x["params"][f], np.float64).reshape(-1), np.asarray(NEUTRAL[f], np.float64).reshape(-1)) for f in FIELDS))


def extra_channels(material_extras, attrs, mat, q8=False, mutate=()):
    """per pixel: the factors, o and e (the two images bilinear + WRAP at level 0 at the pixel's uv)"""
    shape = np.asarray(mat).shape
    out = dict(base=np.ones(shape + (3,)), metal=np.ones(shape), rough=np.ones(shape), scale=np.ones(shape), strength=np.ones(shape),
               factor=np.zeros(shape + (3,)), e=np.ones(shape + (3,)), o=np.ones(shape))
    u, v = np.asarray(attrs)[..., 0], np.asarray(attrs)[..., 1]
    for m in np.unique(mat[mat != NO_MAT]):
        x = material_extras[int(m)] if int(m) < len(material_extras) else None
        if x is None:
            continue
        p, P = mat == m, x["params"]
        out["base"][p], out["metal"][p], out["rough"][p] = P["base_color_factor"], P["metallic_factor"], P["roughness_factor"]
        out["scale"][p], out["strength"][p], out["factor"][p] = P["normal_scale"], P["occlusion_strength"], P["emissive_factor"]
        if x["emissive"] is not None:
            img = x["emissive"]
            f = MR.bilinear(MR.pack(img, img, img), u[p], v[p], q8)   # channels 0..2: decoded per texel, 3..5: the bytes
            out["e"][p] = f[..., 3:6] / 255.0 if "emissive_not_decoded" in mutate else f[..., 0:3]
        if x["occlusion"] is not None:
            img = x["occlusion"]
            out["o"][p] = MR.bilinear(MR.pack(img, img, img), u[p], v[p], q8)[..., 3] / 255.0   # R, linear
    return out


def apply_factors(ch, X, mutate=()):
    """the `ch` array of shading_reference with base', rough', metal' and the normal-map bytes whose tangent-space x and y are scaled"""
    c = np.array(ch, np.float64)
    c[..., 0:3] *= X["base"]
    rf, mf = (X["metal"], X["rough"]) if "metal_rough_factors_swapped" in mutate else (X["rough"], X["metal"])
    c[..., 6] *= rf
    c[..., 7] *= mf
    s = X["scale"]
    for k in (3, 4) + ((5,) if "scale_on_z" in mutate else ()):
        c[..., k] = ((c[..., k] * 2 / 255 - 1) * s + 1) * 255 / 2   # t.k * s back onto the 0..255 scale (the sign of t.y is its own)
    return c


LDR_BAR = 1e-4      # the two standing bars of tests/test_gpu_extended_shading.py (TOL, HDR_REL): |ldr - want| and |hdr - want| / (|want| + 1e-3)
HDR_BAR = 1e-4


def tonemap_moved(settings, hdr):
    """How far an HDR error AT the HDR bar moves the LDR value: per pixel, the sum over the three HDR channels of the largest LDR change
    that moving that channel alone by +-HDR_BAR (|c| + 1e-3) causes.

    Where this exceeds LDR_BAR the two bars contradict each other: a device colour the HDR bar accepts lands outside the LDR one.  That is
    the ACES fit's clip at 0 followed by the gamma root.  Its output matrix has negative entries, so a saturated colour -- an emissive
    texel is one; the scenes' lit surfaces are not -- gives a channel t = 1.60 f(r) - 0.53 f(g) - 0.07 f(b) that cancels to a few 1e-6 of
    terms near 0.1, and d(t^(1/gamma))/dt = t^(1/gamma) / (gamma t) is unbounded towards the clip: at t = 6e-6 a relative error of 3e-6 in
    the terms (fp32 carries 6e-8 per operation) is 1e-4 of LDR.  Such a pixel is left to the HDR bar alone (`judged_hdr`)."""
    tm, gamma, exposure = int(settings[0]), float(np.float32(settings[1])), float(np.float32(settings[2]))
    hdr = np.asarray(hdr, np.float64)
    at = ER.tonemap(tm, hdr, gamma, exposure)
    moved = np.zeros(hdr.shape[:-1])
    for j in range(3):
        step = np.zeros(hdr.shape)
        step[..., j] = HDR_BAR * (np.abs(hdr[..., j]) + 1e-3)
        moved += np.maximum(np.abs(ER.tonemap(tm, hdr + step, gamma, exposure) - at).max(-1), np.abs(ER.tonemap(tm, hdr - step, gamma, exposure) - at).max(-1))
    return moved


def shade(attrs, mat, ch, lit, eye, sun_rotation, sun_color, ambient, settings, material_extras, q8=False, hdr16=False, mutate=(), **lights):
    """shading_reference.shade's arguments plus material_extras[i] = extras(...) or None per material; lights: points, spots, cubes, faces,
    env.  Returns its dict (hdr before any binary16 rounding, ldr, covered, judged, ...) plus A, ao, E and lo_lit = Lo (1 - shadow);
    judged_hdr = shading_reference's judged pixels, judged = those of them whose LDR is well-conditioned as well (tonemap_moved)."""
    mutate = frozenset(mutate)
    assert mutate <= set(MUTATIONS), mutate - set(MUTATIONS)
    X = extra_channels(material_extras, attrs, mat, q8, mutate)
    c = apply_factors(ch, X, mutate)
    memo = {}
    full = SR.shade(attrs, mat, c, lit, eye, sun_rotation, sun_color, ambient, settings, memo=memo, **lights)
    dark = SR.shade(attrs, mat, c, lit, eye, sun_rotation, sun_color, 0.0, settings, memo=memo, **lights)
    covered = full["covered"]
    lo_lit = dark["hdr"]
    A = full["hdr"] - lo_lit
    ao = X["o"] if "strength_ignored" in mutate else 1 + X["strength"] * (X["o"] - 1)
    E = X["e"] * X["factor"]
    if "emissive_times_lit" in mutate:
        E = E * np.asarray(lit, np.float64)[..., None]
    if "ao_on_direct" in mutate:
        color = (lo_lit + A) * ao[..., None] + E
    else:
        color = full["hdr"] + A * (ao[..., None] - 1) + E
    color = np.where(covered[..., None], color, 0.0)
    with np.errstate(over="ignore"):
        hdr = color.astype(np.float16).astype(np.float64) if hdr16 else color
    tm, gamma, exposure = settings
    ldr = ER.tonemap(int(tm), hdr, float(np.float32(gamma)), float(np.float32(exposure)))
    out = dict(full)
    clip = covered & (tonemap_moved(settings, hdr) > LDR_BAR)
    out.update(judged_hdr=full["judged"], judged=full["judged"] & ~clip, reasons=dict(full["reasons"], tonemap=clip))
    out.update(hdr=color, ldr=np.where(covered[..., None], ldr, 0.0), A=A, ao=ao, E=np.where(covered[..., None], E, 0.0), lo_lit=lo_lit, ch=c)
    return out
