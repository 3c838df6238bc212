"""What the tests of ARCTIC_OPT_HIT_MODEL = 1 (tests/test_hit_model_reference.py on the CPU, tests/test_gpu_hit_model.py on the device) add to the
scene of tests/hit_scenes.py, made once from the reference alone and never changed: 4 spot lights (one re-aimed at the middle of the floor, so that
its cone's edge crosses it), 2 shadow-casting point lights inside the scene whose faces (32 x 32) are TRACED on the host -- the 6 F^2 texel-centre
rays per light through arctic_trace_triangles, pz of the hit stored --, and material extras: material 0 with every factor off neutral and both
images at the packed size (the fast layout), material 1 with images of unequal sizes, material 2 with an emissive image alone, material 3 neutral.

The float64 pixel is tests/material_reference.py on tests/shading_reference.py, per origin group with eye = the group's origin; nothing here calls
the product library except the host arbiter of the ray queries, which makes inputs."""
from types import SimpleNamespace

import numpy as np

import env_reference as ER
import hit_reference as HR
import hit_scenes as HS
import material_reference as XR
import ray_reference as R
import shading_reference as SR
import test_gpu_extended_shading as G

F32 = np.float32
FACE = 32                                                   # F: ARCTIC_OPT_POINT_SHADOW_SIZE of the tests
FEATURES = ("extras", "spot", "cube", "env")
SETS = {"extras": ("extras",), "spot": ("spot",), "cube": ("cube",), "env": ("env",), "all": FEATURES}
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)   # faces +X, -X, +Y, -Y, +Z, -Z
_made = {}


def spots(pkg):
    a = pkg.scenes.spot_lights(4, lo=(-3, 0.5, -3), hi=(3, 3, 3), intensity=10.0)
    p = a[0]["position"].astype(np.float64)
    t = np.array([0.4, 0.0, -0.3])                         # the middle of the floor: the whole rim of the cone lies on it
    a[0]["direction"], a[0]["range"] = t - p, 1.5 * np.linalg.norm(t - p) + 2.0
    a[0]["inner_cone_angle"] = a[0]["outer_cone_angle"]     # ... and a hard one (the clamped scale 1000): its ramp is the reason "hard cone ramp" leaves out
    return a


def rim_on_the_floor(I, attrs, mat):
    """floor hits inside and outside the re-aimed spot's cone, and the point where its axis meets the floor: -> (inside, outside, axis point)"""
    c = SR.spot_constants(I.spots[:1])[0]
    obj, _, _ = HR.prim_sources(I.c.g.objects, I.c.g.meshes)
    ok = (mat != HR.NO_MATERIAL) & np.isfinite(attrs).all(1)
    floor = np.zeros(len(mat), bool)
    floor[ok] = obj[I.c.hits["prim"][ok]] == 3
    _, _, _, cd = SR.spot_factor(c, attrs[floor, 11:14].astype(np.float64))
    p, s = c["p"], c["s"]
    return int((cd > c["cos_outer"]).sum()), int((cd < c["cos_outer"]).sum()), p + s * (-p[1] / s[1])


def cubes(pkg):
    """low above the floor, below the boxes.  The floor is a plane perpendicular to the -Y face's axis: every texel of that face holds the pz of
    the floor itself, a compare nobody decides (there is no bias in the definition).  A light at height h sees the floor through that face within
    the radius h only; beyond it through the side faces, at a slope, where texel centre and hit differ by far more than the margin"""
    return pkg.scenes.point_shadow_lights(2, seed=3, lo=(-2.2, 0.25, -2.2), hi=(2.2, 0.5, 2.2), intensity=8.0, z_near=0.1, z_far=12.0)


def cubes_above(pkg):
    """for the faces the handle draws itself: above the boxes.  The pass culls front faces, so the floor seen from above is not in its maps (nothing
    coplanar to compare with) and what hides a hit is a box's far side: the lights hang where the boxes shadow the floor"""
    return pkg.scenes.point_shadow_lights(2, seed=3, lo=(-2.2, 2.2, -2.2), hi=(2.2, 2.8, 2.2), intensity=8.0, z_near=0.1, z_far=12.0)


def traced_faces(pkg, g, lights, size=FACE):
    """per light (6, F, F) float32: pz = zf / (zf - zn) (1 - zn / m) of the closest hit along the ray through each texel's centre, m = the hit's
    distance along the face's axis; 1 where nothing is hit or the hit lies beyond the far plane.  Row 0 at clip y = +1, the header's lookAt rows"""
    c = (np.arange(size) + 0.5) / size * 2 - 1
    x, y = np.meshgrid(c, -c)                               # x[j, i] of column i, y[j, i] of row j
    d = AXES[:, None, None, :] + x[None, ..., None] * SR.S_ROWS[:, None, None, :] + y[None, ..., None] * SR.U_ROWS[:, None, None, :]
    out = []
    for L in lights:
        rays = R.make_rays(np.broadcast_to(L["position"], (6 * size * size, 3)), d.reshape(-1, 3))
        hits = pkg.renderer.trace_triangles(g.tris, rays)
        zn, zf = float(L["z_near"]), float(L["z_far"])
        m = hits["t"].astype(np.float64)                    # the direction's component along the axis is 1: t is m
        with np.errstate(all="ignore"):
            pz = np.where(hits["prim"] != HR.NO_PRIM, zf / (zf - zn) * (1 - zn / m), 1.0)
        out.append(np.ascontiguousarray(np.clip(pz, 0.0, 1.0).reshape(6, size, size), F32))
    return out


def _params(pkg, **kw):
    p = pkg.scene.neutral_material_params()
    for k, v in kw.items():
        p[k] = v
    return p[0]


def material_extras(pkg, images):
    """(params record, emissive, occlusion) or None per material of hit_scenes"""
    rng = np.random.default_rng(63001)
    h0, w0 = images[0][0].shape[:2]
    img = lambda w, h: G._random_images(rng, w, h)[0]
    return [(_params(pkg, base_color_factor=(0.8, 0.6, 0.9), metallic_factor=0.4, roughness_factor=0.9, normal_scale=1.4, occlusion_strength=0.8,
                     emissive_factor=(2.0, 1.0, 0.5)), img(w0, h0), img(w0, h0)),
            (_params(pkg, base_color_factor=(0.5, 0.9, 0.7), metallic_factor=0.7, roughness_factor=0.95, normal_scale=0.7, occlusion_strength=0.6,
                     emissive_factor=(0.7, 0.9, 1.2)), img(8, 4), img(5, 3)),
            (_params(pkg, occlusion_strength=0.5, emissive_factor=(0.3, 0.2, 0.4)), img(8, 4), None),
            None]


def inputs(pkg, assignment):
    """-> Case(c = hit_scenes.scene, spots, cubes, faces, extras, extras_ref)"""
    if assignment not in _made:
        c = HS.scene(pkg, assignment)
        if "lights" not in _made:
            cb = cubes(pkg)
            _made["lights"] = (spots(pkg), cb, traced_faces(pkg, c.g, cb))
        sp, cb, faces = _made["lights"]
        ex = material_extras(pkg, c.images)
        _made[assignment] = SimpleNamespace(c=c, spots=sp, cubes=cb, faces=faces, extras=ex, extras_ref=[None if x is None else XR.extras(*x) for x in ex])
    return _made[assignment]


def host_env(c):
    """the tables of ARCTIC_OPT_ENV_LIGHTING from tests/env_reference.py, for the CPU test (the GPU test reads the handle's own back)"""
    return G.host_env_tables(c.env_map)


def reference(I, attrs, mat, lit, on, env=None, faces=None, mutate=(), sr_mutate=()):
    """the float64 pixel per hit under the features `on`, and the environment along every other ray.  -> Case(rgba, covered, judged, left_out,
    sky, invalid, E, reasons).  mutate: material_reference's defects; sr_mutate: shading_reference's (evaluated without extras: `on` must not
    hold them).  A covered hit whose attributes are not finite is shaded by nobody and judged by nobody."""
    c = I.c
    n = len(c.rays)
    on = frozenset(on)
    assert not (sr_mutate and "extras" in on)
    finite = np.isfinite(attrs).all(1)
    covered = mat != HR.NO_MATERIAL
    ask = np.where(finite, mat, HR.NO_MATERIAL)
    ch = SR.material_channels(c.materials, attrs, ask)
    extras = I.extras_ref if "extras" in on else [None] * len(c.materials)
    lights = dict(points=c.lights, spots=I.spots if "spot" in on else (), cubes=I.cubes if "cube" in on else (),
                  faces=(I.faces if faces is None else faces) if "cube" in on else (), env=env if "env" in on else None)
    assert "env" not in on or env is not None
    rgba, judged, E = np.zeros((n, 4)), np.zeros(n, bool), np.zeros((n, 3))
    reasons = {}
    sun = c.desc.sun
    for k in range(HS.N_ORIGINS):
        sel = np.nonzero((c.origin_of == k) & covered & finite)[0]
        args = (attrs[sel], ask[sel], ch[sel], lit[sel], c.origins[k], sun["rotation"], sun["color"], c.desc.ambient, HS.SETTINGS)
        if sr_mutate:
            ref = SR.shade(*args, mutate=sr_mutate, **lights)
            ref["judged_hdr"] = ref["judged"]
        else:
            ref = XR.shade(*args, extras, mutate=mutate, **lights)
            E[sel] = ref["E"]
        rgba[sel, :3], rgba[sel, 3] = ref["hdr"], 1.0
        judged[sel] = ref["judged_hdr"]
        for why, mask in ref["reasons"].items():
            if why != "tonemap":                            # the LDR's conditioning: only the HDR colour is compared here
                reasons.setdefault(why, np.zeros(n, bool))[sel] = mask
    d = c.rays["direction"].astype(np.float64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(d).all(1) & (d != 0).any(1)
    sky = ~covered & valid
    if sky.any():
        u, v = ER.dir_uv(d[sky])
        rgba[sky, :3] = ER.sample_uv(c.env_map, u, v)
    graze = grazing(I, attrs, ask, ch, "extras" in on)
    reasons["grazing"], reasons["not finite"] = graze, covered & ~finite
    judged &= ~graze
    return SimpleNamespace(rgba=rgba, covered=covered, judged=judged, left_out=int((covered & ~judged).sum()), sky=sky, invalid=~covered & ~valid, E=E,
                           reasons={k: int(v.sum()) for k, v in reasons.items()})


def grazing(I, attrs, mat, ch, with_extras):
    """hit_scenes.grazing with the normal the extras give (normal_scale tilts it)"""
    c = I.c
    if with_extras:
        ch = XR.apply_factors(ch, XR.extra_channels(I.extras_ref, attrs, mat))
    with np.errstate(all="ignore"):
        n = SR.surface_normal(attrs, ch)
        wo = c.rays["origin"].astype(np.float64) - attrs[:, 11:14].astype(np.float64)
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        ndwo = np.abs((n * wo).sum(-1))
    return (mat != HR.NO_MATERIAL) & ~(ndwo >= G.GRAZING)


def cube_terms(I, attrs, mat, lit, faces=None):
    """per hit: a cube light in front of the surface reaches it with 0 < v, and one is wholly hidden (v = 0); hits the sun's map leaves lit only"""
    c = I.c
    ok = (mat != HR.NO_MATERIAL) & np.isfinite(attrs).all(1) & (lit > 0)
    a = np.where(ok[:, None], attrs, SR._NO_GEOMETRY).astype(np.float64)
    ch = SR.material_channels(c.materials, attrs, np.where(ok, mat, HR.NO_MATERIAL))
    with np.errstate(all="ignore"):
        n = SR.surface_normal(a, ch)
    some, none = np.zeros(len(mat), bool), np.zeros(len(mat), bool)
    for L, fc in zip(I.cubes, I.faces if faces is None else faces):
        p = SR.f32(L["position"])
        v, _ = SR.cube_visibility(fc, a[:, 11:14], p, float(L["z_near"]), float(L["z_far"]))
        front = ((p - a[:, 11:14]) * n).sum(-1) > 0
        some |= ok & front & (v > 0)
        none |= ok & front & (v == 0)
    return some, none


def rel_err(got, want):
    return np.abs(np.asarray(got, np.float64) - want) / (np.abs(want) + 1e-3)
