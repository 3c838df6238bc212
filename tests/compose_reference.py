"""The composition of include/arctic_hip.h (arctic_compose_planes_device and the definition in front of it) in float64 numpy: the occlusion's
correction of the ambient term, the mirror reflection under Schlick's Fresnel and the (1 - rough)^2 gate, and the tonemapper of
tests/env_reference.py behind them.  Independent of the library: nothing here calls it.  The material's channels come from
tests/shading_reference.py (material_channels) where a G-buffer is composed, or from the caller where pixels are.

Only ONE decision is taken in fp32, as the definition takes it: whether the occlusion's step 1 covers a pixel (ao_reference.normal -- a normal of
3e19 overflows its own length in fp32 and is NOT COVERED, which float64 would not notice).

MUTATIONS: deliberate defects of the composition, for the tests that show the bar would notice each of them."""
import numpy as np

import ao_reference as A
import env_reference as ER
import shading_reference as SR

AO, REFLECTIONS = 1, 2
NO_MAT = SR.NO_MAT
MUTATIONS = {   # name -> the flag whose term it breaks
    "occlusion_on_whole_colour": AO, "vis_for_one_minus_vis": AO,
    "fresnel_left_out": REFLECTIONS, "roughness_gate_left_out": REFLECTIONS, "alpha_ignored": REFLECTIONS, "normal_mapped_normal": REFLECTIONS,
}


def compose(hdr, base, metal, rough, normal, world, geometry, eye, ambient, ao=None, refl=None, flags=None, ao_strength=1.0, reflection_strength=1.0,
            mutate=(), mapped_normal=None):
    """-> the composed HDR colour (N, 3) float64.  hdr, base, normal, world (N, 3), metal, rough (N,), geometry (N,) bool, ao (N,) uint8, refl (N, 4);
    eye, ambient and the strengths are rounded to fp32 first, as the library receives them.  mapped_normal: (N, 3) unit normals for the defect
    "normal_mapped_normal\""""
    mutate = frozenset(mutate)
    assert mutate <= set(MUTATIONS), mutate - set(MUTATIONS)
    f64 = lambda x, k: np.asarray(x, np.float32).astype(np.float64).reshape((-1, k) if k > 1 else (-1,))
    hdr, base, metal, rough, world = f64(hdr, 3), f64(base, 3), f64(metal, 1)[:, None], f64(rough, 1)[:, None], f64(world, 3)
    geometry = np.asarray(geometry, bool).ravel()
    if flags is None:
        flags = (AO if ao is not None else 0) | (REFLECTIONS if refl is not None else 0)
    ambient, ks, kr = (float(np.float32(x)) for x in (ambient, ao_strength, reflection_strength))
    C = hdr.copy()
    if flags & AO:
        vis = np.asarray(ao, np.uint8).ravel().astype(np.float64)[:, None] / 255.0
        ka = 1.0 - ks * (vis if "vis_for_one_minus_vis" in mutate else 1.0 - vis)
        with np.errstate(invalid="ignore", over="ignore"):
            term = hdr * (ka - 1.0) if "occlusion_on_whole_colour" in mutate else (ambient * base) * (ka - 1.0)
        C = np.where(geometry[:, None], C + term, C)
    if flags & REFLECTIONS:
        refl = np.asarray(refl, np.float32).reshape(-1, 4)
        _, covered = A.normal(normal)
        n64 = np.asarray(normal, np.float32).astype(np.float64).reshape(-1, 3)
        with np.errstate(all="ignore"):
            alpha = refl[:, 3].astype(np.float64)
            present = geometry & covered & (refl[:, 3] > 0)
            if "alpha_ignored" in mutate:
                present, alpha = geometry & covered & np.isfinite(refl[:, :3]).all(1), np.ones(len(refl))
            m = n64 / np.linalg.norm(n64, axis=1, keepdims=True)
            if "normal_mapped_normal" in mutate:
                m = np.asarray(mapped_normal, np.float64).reshape(-1, 3)
            wo = np.asarray(eye, np.float32).astype(np.float64) - world
            wo = wo / np.linalg.norm(wo, axis=1, keepdims=True)
            c = np.maximum((m * wo).sum(1, keepdims=True), 0.0)
            F0 = 0.04 + (base - 0.04) * metal
            F = np.ones_like(F0) if "fresnel_left_out" in mutate else F0 + (1.0 - F0) * (1.0 - c) ** 5
            g = 1.0 if "roughness_gate_left_out" in mutate else (1.0 - rough) ** 2
            term = kr * alpha[:, None] * g * F * refl[:, :3].astype(np.float64)
        C = np.where(present[:, None], C + term, C)      # a select: NaNs of the pixels without a reflection stay out
    return C


def tonemap(C, settings):
    """float LDR (float64) and the RGBA8 the store makes of it: saturate, * 255, + 0.5, truncate; a = 255"""
    tm, gamma, exposure = settings
    ldr = ER.tonemap(int(tm), C, float(np.float32(gamma)), float(np.float32(exposure)))
    q = np.floor(np.clip(np.nan_to_num(ldr, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    return ldr, np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)


def compose_gbuffer(materials, attrs, mat, hdr, eye, ambient, settings, ao=None, refl=None, **kw):
    """a whole G-buffer: attrs (rows, width, 18), mat (rows, width), hdr (rows, width, 3), ao (rows, width), refl (rows, width, 4); materials as
    shading_reference.material_channels takes them.  -> dict(hdr, ldr, rgba8) shaped like the frame"""
    rows, width = mat.shape
    ch = SR.material_channels(materials, attrs, mat)
    flat = np.asarray(attrs, np.float32).reshape(-1, 18)
    if "normal_mapped_normal" in kw.get("mutate", ()):
        kw["mapped_normal"] = SR.surface_normal(flat, ch.reshape(-1, 8))
    C = compose(hdr, ch[..., 0:3], ch[..., 7], ch[..., 6], flat[:, 8:11], flat[:, 11:14], mat.reshape(-1) != NO_MAT, eye, ambient,
                None if ao is None else np.asarray(ao).reshape(-1), None if refl is None else np.asarray(refl).reshape(-1, 4), **kw)
    ldr, rgba8 = tonemap(C, settings)
    return dict(hdr=C.reshape(rows, width, 3), ldr=ldr.reshape(rows, width, 3), rgba8=rgba8.reshape(rows, width, 4))


def rel_err(got, want):
    """the HDR bar's measure: |got - want| / (|want| + 1e-3)"""
    return np.abs(np.asarray(got, np.float64) - want) / (np.abs(want) + 1e-3)
