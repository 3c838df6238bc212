"""Inputs of the indirect-light tests that need no device (tests/test_gi_reference.py) and of those that do (tests/test_gpu_gi.py): made once,
never changed.

  hostile_points()    points {world3, normal3} whose normals and positions are what stage 1 has to survive: m2 = -0.0, zero and non-finite
                      normals, normals that overflow or underflow the length, non-finite world positions
  hostile_gbuffer()   the same edits on a G-buffer's pixels (attributes and materials as arctic_read_gbuffer gives them), in place on a copy
  synthetic_frame()   a small G-buffer of two planes that meet in an edge, pixels without geometry and hostile pixels, with rounds of ray records
                      and of colours that hold NaN, infinities, negatives and values above the clamp
"""
from types import SimpleNamespace

import numpy as np

import gi_reference as GI

F = np.float32
NO_MATERIAL = 0xFFFFFFFF
HOSTILE_NORMALS = [(0.0, 1.0, -0.0), (0.6, 0.8, -0.0), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (0.0, np.inf, 0.0), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0.0),
                   (0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (-0.0, -0.0, -0.0), (1e-20, 1.0, 1e-20)]
HOSTILE_WORLDS = [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (-np.inf, 1.0, 2.0)]
_made = {}


def hostile_points(n_random=200, seed=71001):
    """-> (points (N, 6) float32, kinds (N,): 0 random, 1 + k hostile normal k, 100 + k hostile world k)"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.uniform(-3, 3, (n_random, 3)), rng.normal(size=(n_random, 3)) * rng.uniform(0.2, 3.0, (n_random, 1))], 1).astype(F)
    kinds = np.zeros(n_random, np.int64)
    extra, extra_kinds = [], []
    for k, n in enumerate(HOSTILE_NORMALS):
        for _ in range(3):
            extra.append(np.concatenate([rng.uniform(-3, 3, 3), n]))
            extra_kinds.append(1 + k)
    for k, w in enumerate(HOSTILE_WORLDS):
        for _ in range(3):
            extra.append(np.concatenate([w, rng.normal(size=3)]))
            extra_kinds.append(100 + k)
    return np.concatenate([pts, np.array(extra, F)]).astype(F), np.concatenate([kinds, extra_kinds])


def hostile_gbuffer(attrs, material, seed=71002):
    """-> (attrs, material, marks {name: flat pixel indices}): copies with hostile normals and worlds over covered pixels and a block without geometry"""
    attrs, material = attrs.copy(), material.copy()
    rng = np.random.default_rng(seed)
    flat, mat = attrs.reshape(-1, 18), material.reshape(-1)
    cov = np.nonzero(mat != NO_MATERIAL)[0]
    per = 4
    pick = rng.choice(cov, per * (len(HOSTILE_NORMALS) + len(HOSTILE_WORLDS)) + 12, replace=False)
    marks = {}
    for k, n in enumerate(HOSTILE_NORMALS):
        px = pick[per * k:per * (k + 1)]
        flat[px, 8:11] = np.array(n, F)
        marks["normal %d" % k] = px
    base = per * len(HOSTILE_NORMALS)
    for k, w in enumerate(HOSTILE_WORLDS):
        px = pick[base + per * k:base + per * (k + 1)]
        flat[px, 11:14] = np.array(w, F)
        marks["world %d" % k] = px
    holes = pick[-12:]
    mat[holes] = NO_MATERIAL
    marks["holes"] = holes
    return attrs, material, marks


def synthetic_frame(width=21, height=13, n_rays=3, P=4, seed=71003):
    """-> Case(attrs, material, dirs, rays (n_rays, h, w), colors (n_rays, h, w, 4), clamp_max, ...): a wall x = 0 on the left, a floor y = 0 on
    the right, so that the filter's windows across the edge reject; the wall's colours are +inf, sanitised to clamp_max = 3e38, and three of them
    sum to +inf in S: what a rejected pixel holds must not reach its neighbour, not even multiplied by zero (inf * 0 is a NaN)"""
    key = (width, height, n_rays, P, seed)
    if key in _made:
        return _made[key]
    rng = np.random.default_rng(seed)
    attrs = np.zeros((height, width, 18), F)
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    wall = x < width // 2                                                         # on the LEFT: every window (offsets -1..0 for P = 2) of the floor's first columns reaches it
    attrs[..., 11] = np.where(wall, 0.0, (x - width // 2) * 0.25)
    attrs[..., 12] = np.where(wall, (width // 2 - x) * 0.25, 0.0)
    attrs[..., 13] = y * 0.25
    attrs[..., 8:11] = np.where(wall[..., None], (1.7, 0.0, 0.0), (0.0, 2.3, 0.0))
    attrs[..., 8:11] += rng.normal(size=(height, width, 3)).astype(F) * F(0.02)
    attrs[..., 11:14] += rng.normal(size=(height, width, 3)).astype(F) * F(0.002)
    material = np.zeros((height, width), np.uint32)
    attrs, material, marks = hostile_gbuffer(attrs, material, seed + 1)
    dirs = cosine_table(n_rays, P, seed + 2)
    rays = np.stack([GI.image_rays(attrs, material, dirs, n_rays, P, k, 50.0, 1e-3)[0] for k in range(n_rays)])
    colors = rng.uniform(0.0, 4.0, (n_rays, height, width, 4)).astype(F)
    colors[..., 3] = rng.integers(0, 2, colors.shape[:-1])
    colors[:, wall, 0:3] = np.inf                                                 # radiance that a rejected neighbour must keep to itself
    floor_w = width - width // 2
    odd = rng.choice(height * floor_w, 40, replace=False).reshape(4, 10)          # on the floor: NaN, -inf, negative, a large value
    fy, fx = odd // floor_w, odd % floor_w + width // 2
    for k, v in enumerate([np.nan, -np.inf, -2.5, 1e30]):
        colors[k % n_rays, fy[k], fx[k], k % 3] = v
    c = SimpleNamespace(attrs=attrs, material=material, marks=marks, dirs=dirs, rays=rays, colors=colors, wall=wall, n_rays=n_rays, P=P, odd=(fy, fx),
                        clamp_max=3e38, normal_cos=0.9, plane_dist=0.05, width=width, height=height)
    _made[key] = c
    return c


def cosine_table(n_rays, P, seed=0):
    """a table for the tests: (P * P, n_rays, 3) float32 unit directions, cosine-weighted over z > 0, each set drawn on its own"""
    rng = np.random.default_rng([seed, n_rays, P])
    u, phi = rng.random((P * P, n_rays)), rng.random((P * P, n_rays)) * 2.0 * np.pi
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(1.0 - u, 0.0))], -1).astype(F)
