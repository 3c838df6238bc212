"""The inputs of the environment-lighting shape tests, shared by the GPU tests (tests/test_gpu_env_shapes.py) and the CPU tests that pin
what those inputs can see (tests/test_env_lighting.py): the maps, the fixed texel subsets of the large prefiltered levels, and the crafted
G-buffer whose pixels sit on the wraps and clamps of the per-pixel lookup.  Plain numpy; never calls the library."""
import numpy as np

import env_reference as ER

# name: (W, H, seed of scenes.synthetic_hdri).  The smallest maps that take each path of env_light.hip (level sizes: ER.level_size):
MAPS = {
    "odd": (97, 41, 21),       # mip chain 97x41, 48x20, 24x10, 12x5, 6x2, 3x1, 1x1: the odd sides 97, 41, 5, 3 drop their last column / row
    "wide": (300, 20, 22),     # SH rows: 1 or 2 trips, ragged (300 = 256 + 44); level 1 is 300 wide: a second, ragged x-block of k_env_prefilter
    "tall": (40, 300, 23),     # SH final: 300 rows, threads 0..43 make two trips; levels have min(H, 256) = 256 rows
    "big": (1040, 520, 24),    # above both clamps of env_level_size; mip level 1 (520 wide) is three x-blocks of k_env_mip; 11 mip levels
    "1x1": (1, 1, 25),         # a one-entry mip chain: every sample takes the lod >= top branch; a one-texel wrap
    "2x1": (2, 1, 26),
    "1x7": (1, 7, 27),
    "3x5": (3, 5, 28),
}
SUBSET_CAP = 1000              # texels compared of a level whose whole reference is too slow on the CPU
SUBSET_LEVELS = {("tall", k) for k in range(1, ER.LEVELS)} | {("big", 1), ("big", 2)}
EYE = (-3.2, 2.2, 4.2)         # scenes.config2's camera
EYE32 = np.asarray(EYE, np.float32).astype(np.float64)   # ... as the library is given it (ArcticCamera::eye is float[3])


def make_map(scenes, name):
    W, H, seed = MAPS[name]
    return scenes.synthetic_hdri(W, H, seed=seed)


def contrast_map(scenes, W=2048, H=1024, seed=31):
    """synthetic_hdri with its RGB multiplied per texel by exp2(U(-2, 2)): neighbouring texels differ by up to a factor 16"""
    env = scenes.synthetic_hdri(W, H)
    rng = np.random.default_rng(seed)
    env[..., :3] *= np.exp2(rng.uniform(-2.0, 2.0, (H, W, 1))).astype(np.float32)
    return env


def level_texels(name, k):
    """the (row, column) pairs of level k of map `name` that the tests compare: None = the whole level.  A fixed set per level: the four
    corners, 128 texels of the last row, 64 of the last column and of each of the columns 255, 256 and 257 where the level has them (the
    boundary between the first two x-blocks of a 256-thread row), and a seeded random rest, SUBSET_CAP in all."""
    W, H, _ = MAPS[name]
    w, h = ER.level_size(W, H, k)
    if (name, k) not in SUBSET_LEVELS or w * h <= SUBSET_CAP:
        return None
    rng = np.random.default_rng(1000 * MAPS[name][2] + k)
    picked = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    picked |= {(h - 1, int(c)) for c in rng.choice(w, min(w, 128), replace=False)}
    for col in (w - 1, 255, 256, 257):
        if col < w:
            picked |= {(int(r), col) for r in rng.choice(h, min(h, 64), replace=False)}
    while len(picked) < SUBSET_CAP:
        picked.add((int(rng.integers(h)), int(rng.integers(w))))
    return sorted(picked)


# ---- the crafted G-buffer of the per-pixel lookup ---------------------------------------------------------------------------------
ROUGH_EDGES = (0, 1, 50, 51, 52, 101, 102, 153, 204, 254, 255)   # t = 5 r on, and just to either side of, every level boundary; k1's clamp at 255
ROUGH_LEVEL0 = (0, 13, 26, 38, 50)                               # level 0 weighs in
NORMAL_TEXEL = (128, 128, 255)                                   # the one normal-map texel of every material
COSINES = (1.0, 0.5, 1.0 / 64, 1e-4, 0.0, -0.2, -0.9)            # n.wo: the LUT's last and first columns, p5 = 1, R from a negative dot


def materials(rough_bytes, seed=5):
    """(base rgb bytes, normal rgb bytes, rough byte, metal byte) per material: every roughness byte as a dielectric and as a metal"""
    rng = np.random.default_rng(seed)
    return [(rng.integers(20, 255, 3), np.array(NORMAL_TEXEL), int(rb), metal) for rb in rough_bytes for metal in (0, 255)]


def material_side(i):
    """material i's images are 1 x 1 or 2 x 2"""
    return 1 + i % 2


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def fan_dirs(w0, h0):
    """unit directions around the u seam and the two poles of a w0 x h0 equirect, the angles in its texels.
    Seam: azimuth pi - e and -pi + e (direction (-1, 0, +-e)), e = 0.05 .. 24 texels, at elevations 0 and +-0.3 rad.
    Poles: 0.05 .. 5 texels away from (0, +-1, 0), at six azimuths.  Returns (seam (120, 3), poles (144, 3))."""
    du, dv = 1.0 / (ER.C_U * w0), 1.0 / (ER.C_V * h0)       # radians per texel
    eps = np.geomspace(0.05, 24.0, 20) * du
    seam = []
    for sign in (1.0, -1.0):
        for el in (0.0, 0.3, -0.3):
            phi = sign * (np.pi - eps)
            seam.append(np.stack([np.cos(el) * np.cos(phi), np.sin(el) * np.ones_like(phi), np.cos(el) * np.sin(phi)], -1))
    th = np.geomspace(0.05, 5.0, 12) * dv
    poles = []
    for sign in (1.0, -1.0):
        for az in 0.3 + np.arange(6) * np.pi / 3:
            poles.append(np.stack([np.sin(th) * np.cos(az), sign * np.cos(th), np.sin(th) * np.sin(az)], -1))
    return np.concatenate(seam), np.concatenate(poles)


def _tangent_space(nrm_bytes):
    b = np.asarray(nrm_bytes, np.float64)
    return np.array([b[0] * 2 / 255 - 1, -(b[1] * 2 / 255 - 1), b[2] * 2 / 255 - 1])


def frames_for(n):
    """tangent frames (t, b, g), each (N, 3), whose shading normal t ts.x + b ts.y + g ts.z -- ts the tangent-space value of NORMAL_TEXEL --
    points along the unit vectors n (N, 3): the rotation that takes ts / |ts| to n"""
    m = _unit(_tangent_space(NORMAL_TEXEL))
    e1 = _unit(np.cross(m, [0.0, 1.0, 0.0]))
    e2 = np.cross(m, e1)
    up = np.where((np.abs(n[:, 1]) < 0.9)[:, None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    a = _unit(np.cross(up, n))
    c = np.cross(n, a)
    F = a[:, :, None] * e1[None, None, :] + c[:, :, None] * e2[None, None, :] + n[:, :, None] * m[None, None, :]   # F m = n
    return F[:, :, 0], F[:, :, 1], F[:, :, 2]


def crafted_gbuffer(w0, h0, rough_bytes, rows=64, width=96, angles=True, seed=17):
    """(attrs (rows, width, 18) float32, material (rows, width) uint32, mats, kind (rows, width) int) in scenes.random_gbuffer's layout, for
    the camera at EYE and materials(rough_bytes).  kind: 1 = a seam-fan pixel, 2 = a pole-fan pixel, 3 = an angle pixel, 4 = the tile of
    one material, 0 = a random pixel (one in ten of those has no geometry).
    Fan pixels have n = wo = a direction d of fan_dirs(w0, h0), through world = EYE - s d, so R = wo = d: every direction with every
    roughness byte.  Angle pixels (angles=True) have n.wo = each of COSINES, the frame rotated about an axis across wo, with every material,
    along four view directions.  The tile (3, 5) is covered by one material; everywhere else the materials are mixed within the tiles."""
    rng = np.random.default_rng(seed)
    mats = materials(rough_bytes)
    eye = EYE32
    seam, poles = fan_dirs(w0, h0)
    d, n, m, kind = [], [], [], []
    nr = len(rough_bytes)
    for code, fan in ((1, seam), (2, poles)):
        for di, v in enumerate(fan):
            for ri in range(nr):
                d.append(v); n.append(None); m.append(2 * ri + ((di + ri) & 1)); kind.append(code)
    if angles:
        views = _unit(np.array([[0.3, 0.5, 0.8], [-0.7, 0.2, -0.4], [0.1, -0.9, 0.3], [0.6, 0.6, -0.5]]))
        for v in views:
            p = _unit(np.cross(v, [0.2, 0.3, -0.9]))
            for c in COSINES:
                ang = np.arccos(c)
                for mi in range(len(mats)):
                    d.append(v); n.append(np.cos(ang) * v + np.sin(ang) * p); m.append(mi); kind.append(3)
    ty, tx = 3, 5
    for _ in range(64):
        v = _unit(rng.standard_normal(3))
        d.append(v); n.append(_unit(v + 0.5 * _unit(rng.standard_normal(3)))); m.append(7 % len(mats)); kind.append(4)
    N = len(d)
    assert N <= rows * width - 64
    d = np.array(d)
    world = (eye - rng.uniform(3.0, 12.0, (N, 1)) * d).astype(np.float32)
    wo = _unit(eye - world.astype(np.float64))                     # what a pixel at the stored position sees
    nn = np.array([wo[i] if n[i] is None else n[i] for i in range(N)])
    t, b, g = frames_for(nn)
    # the rest of the frame: random_gbuffer's kind of pixel
    a = np.empty((rows, width, 18), np.float32)
    a[..., 0:2] = rng.random((rows, width, 2), dtype=np.float32) * 4.0
    g0 = _unit(rng.standard_normal((rows, width, 3)))
    t0 = _unit(np.cross(g0, _unit(rng.standard_normal((rows, width, 3)))))
    a[..., 2:5], a[..., 5:8], a[..., 8:11] = t0, np.cross(g0, t0), g0
    a[..., 11:14] = np.array([-15.0, 0, -7]) + rng.random((rows, width, 3)) * np.array([30.0, 12, 14])
    a[..., 14:16] = rng.random((rows, width, 2), dtype=np.float32) * 2.2 - 1.1
    a[..., 16] = rng.random((rows, width), dtype=np.float32) * 1.1
    a[..., 17] = 1.0
    mat = rng.integers(0, len(mats), (rows, width), dtype=np.uint32)
    mat[rng.random((rows, width)) >= 0.9] = 0xFFFFFFFF
    kd = np.zeros((rows, width), np.int64)
    # where the crafted pixels go: the tile's 64 places, then a seeded shuffle of all the others
    in_tile = np.zeros((rows, width), bool)
    in_tile[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = True
    tile_pos = np.argwhere(in_tile)
    other = np.argwhere(~in_tile)
    other = other[rng.permutation(len(other))][:N - 64]
    pos = np.concatenate([other, tile_pos])
    y, x = pos[:, 0], pos[:, 1]
    a[y, x, 2:5], a[y, x, 5:8], a[y, x, 8:11], a[y, x, 11:14] = t, b, g, world
    mat[y, x] = np.array(m, np.uint32)
    # The crafted pixels sample their material at a texel centre, where the bilinear weights are (1, 0, 0, 0) and the fp32 sampler returns
    # the constant exactly.  Elsewhere its weights need not sum to 1, and the filtered normal byte can be one ulp (8e-6) off 128.  The
    # reference takes the constant: within a tenth of a texel of a pole of a 2048 x 1024 map that ulp turns R's azimuth by a tenth of a
    # texel (measured on the CPU: 8 % of the level-0 sample), which would be the sampler's rounding, not the lookup's.
    a[y, x, 0] = a[y, x, 1] = np.where(np.array([material_side(i) for i in m]) == 1, 0.5, 0.25).astype(np.float32)
    kd[y, x] = kind
    return a, mat, mats, kd


def pixel_inputs(attrs, mat, mats, eye=EYE32):
    """n, wo, base, metal, rough of every pixel in float64 from the G-buffer and the eye as stored (fp32: within a texel of a pole of a
    2048 x 1024 map, the 5e-8 between -3.2 and float(-3.2) turns R's azimuth by a tenth of a texel), and the coverage mask"""
    cov = mat != 0xFFFFFFFF
    m = np.where(cov, mat, 0)
    base = ER.srgb_to_linear(np.array([x[0] for x in mats], np.float64)[m])
    nb = np.array([x[1] for x in mats], np.float64)[m]
    ts = np.stack([nb[..., 0] * 2 / 255 - 1, -(nb[..., 1] * 2 / 255 - 1), nb[..., 2] * 2 / 255 - 1], -1)
    a = attrs.astype(np.float64)
    n = a[..., 2:5] * ts[..., :1] + a[..., 5:8] * ts[..., 1:2] + a[..., 8:11] * ts[..., 2:3]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    rough = np.array([x[2] for x in mats], np.float64)[m] / 255
    metal = np.array([x[3] for x in mats], np.float64)[m] / 255
    wo = np.asarray(eye, np.float64) - a[..., 11:14]
    wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
    return n, wo, base, metal, rough, cov


def wrap_counts(attrs, mat, mats, kind, w0, h0):
    """how many pixels with roughness below 0.2 (level 0 weighs in) take each wrap of a w0 x h0 level 0, from the reference's own _wrap:
    (seam: x0 = w0 - 1 and x1 = 0; north pole, south pole: y0 = h0 - 1 and y1 = 0)"""
    n, wo, _, _, rough, cov = pixel_inputs(attrs, mat, mats)
    R = 2 * np.sum(n * wo, -1)[..., None] * n - wo
    u, v = ER.dir_uv(R)
    x0, x1, _ = ER._wrap(u, w0)
    y0, y1, _ = ER._wrap(v, h0)
    lvl0 = cov & (rough < 0.2)
    seam = lvl0 & (kind == 1) & (x0 == w0 - 1) & (x1 == 0)
    ywrap = lvl0 & (kind == 2) & (y0 == h0 - 1) & (y1 == 0)
    return int(seam.sum()), int((ywrap & (R[..., 1] > 0)).sum()), int((ywrap & (R[..., 1] < 0)).sum())
