"""The whole extended pixel in float64 numpy, written from include/arctic_hip.h alone:

    color = Lo * (1 - shadow) + ambient * (ENV ? ibl(n, wo, base, metal, rough) : base)
    Lo    = sun + sum(point) + sum(spot: color * att * window / d2) + sum(cube: color * v / d2)

then the tonemapper and gamma, optionally through binary16.  It never calls the product library and takes no value from a HIP handle other
than inputs the caller read back (G-buffer, maps, faces, chains, lambda, environment tables).  tests/test_shading_reference.py pins it on
the CPU (against the C++ oracle where the two overlap, by hand where they do not); tests/test_gpu_extended_shading.py compares the
k_envlit / k_spotlit / k_cubelit / k_miplit kernels with it.

`shade(..., mutate={...})` evaluates a deliberately WRONG variant (MUTATIONS): the CPU tests use them to show that the inputs of the GPU
cases can tell each such defect from the truth.
"""
import numpy as np

import env_reference as ER
import mip_reference as MR

NO_MAT = 0xFFFFFFFF
EPS = 1e-5          # distance to a cube compare or face-selection decision below which a pixel is not judged (tests/test_gpu_point_shadows.py)
HARD_RAMP = 1e-3    # a cone with cos(inner) - cos(outer) below this has the clamped scale 1000: its whole ramp is not judged (tests/test_gpu_spot_lights.py)
PI_HLSL = 3.14159265   # forward.hlsl's PI

# the cube's lookAt rows per face (+X, -X, +Y, -Y, +Z, -Z), from the header's table
S_ROWS = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
U_ROWS = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)

# attributes standing in for the pixels without geometry (their value is 0 whatever they hold): a unit frame, one unit in front of the eye
_NO_GEOMETRY = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1], np.float64)

MUTATIONS = {   # name -> the feature whose term it breaks (a case is asked to notice it when its feature set holds that feature)
    "drop_window": "spot", "offset_wrong_sign": "spot", "cone_not_squared": "spot", "spot_missing_d2": "spot",
    "cube_u_row_negated": "cube", "cube_faces_swapped": "cube", "pcf_fx_fy_swapped": "cube", "cube_ignores_sun_shadow": "cube",
    "trilinear_floor_only": "mip", "env_times_sun_shadow": "env", "odd_last_light_dropped": "point",
}


def f32(x):
    """rounded once to fp32, carried on in float64"""
    return np.asarray(x, np.float32).astype(np.float64)


def sun_direction(rotation_deg):
    """DirectionalLight::direction(): (cos x cos y, sin x, cos x sin y) of the rotation in degrees (x = pitch, y = yaw), in fp32 like the host
    code that hands it to the kernels (scene.cpp:9-19 is glm in fp32): a mirror-like highlight moves by 1e-5 of itself with the last bit of it"""
    f = np.float32
    xr, yr = f(rotation_deg[0]) * f(np.pi / 180), f(rotation_deg[1]) * f(np.pi / 180)
    return np.array([f(np.cos(xr) * np.cos(yr)), np.sin(xr), f(np.cos(xr) * np.sin(yr))], np.float32).astype(np.float64)


# ---- materials ---------------------------------------------------------------------------------------------------------------------
def material_channels(materials, attrs, mat, lod=None, q8=False, mutate=()):
    """the eight filtered channels per pixel (base rgb decoded, normal rgb on the 0..255 scale, roughness, metalness).
    materials[i] is a list of (h, w, 8) uint8 levels (a chain, or one level) or a tuple (diffuse, normal, metal_rough) of RGBA8 images of
    unequal sizes (one level each, sampled at level 0 in every mode).  lod None = MIP off: bilinear at level 0."""
    ch = np.zeros(mat.shape + (8,))
    u, v = attrs[..., 0], attrs[..., 1]
    for m in np.unique(mat[mat != NO_MAT]):
        p = mat == m
        M = materials[int(m)]
        if isinstance(M, tuple):
            d, n, r = (np.asarray(x, np.uint8) for x in M)
            ch[p, 0:3] = MR.bilinear(MR.pack(d, d, d), u[p], v[p], q8)[..., 0:3]
            ch[p, 3:6] = MR.bilinear(MR.pack(n, n, n), u[p], v[p], q8)[..., 3:6]
            ch[p, 6:8] = MR.bilinear(MR.pack(r, r, r), u[p], v[p], q8)[..., 6:8]
        elif lod is None or len(M) == 1:
            ch[p] = MR.bilinear(M[0], u[p], v[p], q8)
        else:
            lam = np.asarray(lod, np.float64)[p]
            if "trilinear_floor_only" in mutate:
                lam = np.floor(lam)
            ch[p] = MR.trilinear(M, u[p], v[p], lam, q8)
    return ch


# ---- spot lights ---------------------------------------------------------------------------------------------------------------------
def spot_constants(spots):
    """per light, in binary64, each rounded once to fp32: position, scale, s, offset, color, ir2, and (binary64) cos(outer), hard"""
    out = []
    for L in spots:
        d = np.asarray(L["direction"], np.float64)
        s = f32(d / np.sqrt((d * d).sum()))
        outer, inner, rng = float(np.float32(L["outer_cone_angle"])), float(np.float32(L["inner_cone_angle"])), float(np.float32(L["range"]))
        co, ci = np.cos(outer), np.cos(inner)
        if np.float32(outer) == np.float32(np.pi):
            scale, offset, hard = 0.0, 1.0, False
        else:
            scale = 1.0 / max(1e-3, ci - co)
            offset = -co * scale
            hard = (ci - co) < HARD_RAMP
        ir2 = 1.0 / (rng * rng) if rng > 0 else 0.0
        out.append(dict(p=f32(L["position"]), s=s, scale=float(f32(scale)), offset=float(f32(offset)), color=f32(L["color"]), ir2=float(f32(ir2)),
                        cos_outer=co, hard=hard))
    return out


def spot_factor(c, world, mutate=()):
    """(att * window, d, d2, cd) of one light's constants over the pixels"""
    d = c["p"] - world
    d2 = (d * d).sum(-1)
    inv = 1.0 / np.sqrt(d2)
    cd = -(d * c["s"]).sum(-1) * inv
    offset = -c["offset"] if "offset_wrong_sign" in mutate else c["offset"]
    att = np.clip(cd * c["scale"] + offset, 0, 1)
    if "cone_not_squared" not in mutate:
        att = att * att
    q = d2 * c["ir2"]
    window = np.ones_like(d2) if "drop_window" in mutate else np.clip(1 - q * q, 0, 1)
    return att * window, d, d2, cd


# ---- shadow-casting point lights --------------------------------------------------------------------------------------------------
def cube_face(d):
    """the face of d = world - p: the axis of max |d| (ties x, then y, then z) and its sign; also m and the gap to the runner-up"""
    ad = np.abs(d)
    m = ad.max(-1)
    axis = np.where((ad[..., 0] >= ad[..., 1]) & (ad[..., 0] >= ad[..., 2]), 0, np.where(ad[..., 1] >= ad[..., 2], 1, 2))
    sign = np.take_along_axis(d, axis[..., None], -1)[..., 0] >= 0
    srt = np.sort(ad, -1)
    return 2 * axis + np.where(sign, 0, 1), m, srt[..., 2] - srt[..., 1]


def cube_lookup(d, F, zn, zf):
    """face, texel coordinates x = px F - 0.5, y = py F - 0.5, pz, m of d = world - p"""
    face, m, gap = cube_face(d)
    mm = np.where(m > 0, m, 1.0)
    px = 0.5 + 0.5 * (S_ROWS[face] * d).sum(-1) / mm
    py = 0.5 - 0.5 * (U_ROWS[face] * d).sum(-1) / mm
    pz = zf / (zf - zn) * (1 - zn / mm)
    return face, px * F - 0.5, py * F - 0.5, pz, m, gap


def cube_visibility(faces, world, p, zn, zf, mutate=()):
    """v per pixel and whether the pixel is farther than EPS from every decision of the lookup (depth compares, face selection, the near
    and the far plane)"""
    faces = np.asarray(faces)
    F = faces.shape[-1]
    d = world - np.asarray(p, np.float64)
    face, x, y, pz, m, gap = cube_lookup(d, F, zn, zf)
    if "cube_u_row_negated" in mutate:      # the u row of face 0 (+X) negated
        y = np.where(face == 0, (F - 1) - y, y)
    if "cube_faces_swapped" in mutate:
        face = face ^ 1
    ok = gap > EPS * np.maximum(m, 1.0)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    if "pcf_fx_fy_swapped" in mutate:
        fx, fy = fy, fx
    c0, c1 = np.clip(x0, 0, F - 1).astype(int), np.clip(x0 + 1, 0, F - 1).astype(int)
    r0, r1 = np.clip(y0, 0, F - 1).astype(int), np.clip(y0 + 1, 0, F - 1).astype(int)
    t = [faces[face, r, c].astype(np.float64) for r, c in ((r0, c0), (r0, c1), (r1, c0), (r1, c1))]
    s = [(pz > ti).astype(np.float64) for ti in t]
    outside = (m <= zn) | (pz > 1)
    near_compare = np.zeros(m.shape, bool)
    for ti in t:
        near_compare |= np.abs(pz - ti) <= EPS
    ok &= ~(near_compare & ~outside)
    top, bottom = s[0] + (s[1] - s[0]) * fx, s[2] + (s[3] - s[2]) * fx
    v = 1 - (top + (bottom - top) * fy)
    ok &= (np.abs(m - zn) > EPS) & (np.abs(pz - 1) > EPS)
    return np.where(outside, 1.0, v), ok


def surface_normal(attrs, ch):
    """get_normal (forward.hlsl:104-111): the filtered normal-map rgb (0..255 scale) with g -> 1 - g, * 2 - 1, through the tangent frame, normalised"""
    a = np.asarray(attrs, np.float64)
    ts = np.stack([ch[..., 3] * 2 / 255 - 1, -(ch[..., 4] * 2 / 255 - 1), ch[..., 5] * 2 / 255 - 1], -1)
    n = a[..., 2:5] * ts[..., :1] + a[..., 5:8] * ts[..., 1:2] + a[..., 8:11] * ts[..., 2:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        return n / np.linalg.norm(n, axis=-1, keepdims=True)


# ---- the pixel ---------------------------------------------------------------------------------------------------------------------
def shade(attrs, mat, ch, lit, eye, sun_rotation, sun_color, ambient, settings, points=(), spots=(), cubes=(), faces=(), env=None,
          hdr16=False, mutate=(), memo=None):
    """attrs (..., 18) G-buffer floats, mat (...) material ids, ch (..., 8) from material_channels, lit = 1 - shadow per pixel.
    points / spots / cubes: the light records as the caller handed them to the library; faces[i] = (6, F, F) of cube light i;
    env = (sh (9, 3), lut, levels) from read_env_lighting, or None = flat ambient; settings = (tonemapper, gamma, exposure).
    Returns dict(hdr, ldr, covered, judged, reasons): hdr / ldr are float64 (uncovered pixels 0), judged = the covered pixels no float64
    decision of which is closer than the existing tests' margins to flipping in fp32, reasons = {why: mask of the pixels left out}.
    memo: a dict the caller keeps between calls that share attrs, mat, ch, eye, the sun and the light lists (whole frames shaded under
    several feature sets): the sums of each light list and the environment bracket are then evaluated once."""
    mutate = frozenset(mutate)
    assert memo is None or not mutate
    memo = {} if memo is None else memo
    assert mutate <= set(MUTATIONS), mutate - set(MUTATIONS)
    covered = np.asarray(mat) != NO_MAT
    a = np.where(covered[..., None], np.asarray(attrs, np.float64), _NO_GEOMETRY + np.concatenate([np.zeros(11), f32(eye), np.zeros(4)]))
    lit = np.asarray(lit, np.float64)
    base, rough, metal = ch[..., :3], ch[..., 6:7], ch[..., 7:8]
    n = surface_normal(a, ch)
    world = a[..., 11:14]
    wo = f32(eye) - world
    wo = wo / np.linalg.norm(wo, axis=-1, keepdims=True)
    F0 = 0.04 + (base - 0.04) * metal
    a2 = (rough * rough) ** 2
    k = (rough + 1) ** 2 / 8
    ndwo = np.maximum((n * wo).sum(-1, keepdims=True), 0)

    def radiance(wi, Li):   # calculate_outgoing_radiance, forward.hlsl:126-193
        h = wo + wi
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        Fr = F0 + (1 - F0) * (1 - np.maximum((h * wo).sum(-1, keepdims=True), 0)) ** 5
        ndh = np.maximum((n * h).sum(-1, keepdims=True), 0)
        ndwi = np.maximum((n * wi).sum(-1, keepdims=True), 0)
        D = a2 / (PI_HLSL * (ndh * ndh * (a2 - 1) + 1) ** 2)
        G = (ndwo / (ndwo * (1 - k) + k)) * (ndwi / (ndwi * (1 - k) + k))
        spec = D * G * Fr / (4 * ndwo * ndwi + 1e-4)
        return ((1 - Fr) * (1 - metal) * base / PI_HLSL + spec) * Li * ndwi

    def point_term(p, color):
        d = f32(p) - world
        d2 = (d * d).sum(-1, keepdims=True)
        return radiance(d / np.sqrt(d2), f32(color) / d2), d, d2

    def once(key, fn):
        if key not in memo:
            memo[key] = fn()
        return memo[key]

    def sun_and_points():
        Lo = radiance(np.broadcast_to(-sun_direction(sun_rotation), world.shape), f32(sun_color))
        pts = list(points)
        if "odd_last_light_dropped" in mutate and len(pts) % 2:
            pts = pts[:-1]
        for L in pts:
            Lo = Lo + point_term(L["position"], L["color"])[0]
        return Lo

    def spot_sum():
        Lo, ramp = np.zeros(world.shape), np.zeros(covered.shape, bool)
        for c in spot_constants(spots):
            f, d, d2, cd = spot_factor(c, world, mutate)
            d2 = d2[..., None]
            Li = c["color"] * f[..., None] / (1.0 if "spot_missing_d2" in mutate else d2)
            Lo = Lo + radiance(d / np.sqrt(d2), Li)
            if c["hard"]:   # only exactly 0 or exactly 1 is judged: the ramp lies within HARD_RAMP of cos(outer), where fp32 cd * 1000 is ill-conditioned
                facing = (n * d).sum(-1) > 0
                ramp |= facing & ~((cd < c["cos_outer"] - EPS) | (cd > c["cos_outer"] + HARD_RAMP + EPS))
        return Lo, ramp

    def cube_sum():
        assert len(cubes) == len(faces)
        Lo, undecided = np.zeros(world.shape), np.zeros(covered.shape, bool)
        for L, fc in zip(cubes, faces):
            zn, zf = float(np.float32(L["z_near"])), float(np.float32(L["z_far"]))
            v, ok = cube_visibility(fc, world, f32(L["position"]), zn, zf, mutate)
            term, d, _ = point_term(L["position"], L["color"])
            Lo = Lo + term * v[..., None]
            undecided |= ((n * d).sum(-1) > 0) & ~ok   # behind the surface the term is zero whatever v is
        return Lo, undecided

    reasons = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        Lo = once("sun_and_points", sun_and_points)
        cube_Lo = 0.0
        sunlit = covered & (lit != 0)   # where the sun's map covers everything no light's term is seen
        if len(spots):
            spot_Lo, ramp = once("spots", spot_sum)
            Lo = Lo + spot_Lo
            reasons["hard cone ramp"] = sunlit & ramp
        if len(cubes):
            cube_Lo, undecided = once("cubes", cube_sum)
            reasons["cube decision"] = (covered if "cube_ignores_sun_shadow" in mutate else sunlit) & undecided
        if env is not None:
            sh, lut, levels = env
            amb = once("env", lambda: ER.ibl(n, wo, base, metal[..., 0], rough[..., 0], sh, lut, levels))
        else:
            amb = base
        amb = amb * float(np.float32(ambient))
        if "env_times_sun_shadow" in mutate and env is not None:
            amb = amb * lit[..., None]
        if "cube_ignores_sun_shadow" in mutate:
            color = Lo * lit[..., None] + cube_Lo + amb
        else:
            color = (Lo + cube_Lo) * lit[..., None] + amb
    color = np.where(covered[..., None], color, 0.0)
    hdr = color.astype(np.float16).astype(np.float64) if hdr16 else color
    tm, gamma, exposure = settings
    ldr = ER.tonemap(int(tm), hdr, float(np.float32(gamma)), float(np.float32(exposure)))
    judged = covered.copy()
    for r in reasons.values():
        judged &= ~r
    return dict(hdr=color, ldr=np.where(covered[..., None], ldr, 0.0), covered=covered, judged=judged, reasons=reasons,
                rough=rough[..., 0], metal=metal[..., 0], lit=lit)   # (the last three: for a failing pixel's report)
