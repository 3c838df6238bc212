"""Light-space positions with a general w, for the third branch of shadow_coords (shadow_coords.h: `lsx / lsw`), and a shadow map to test them
against.  No device: tests/test_shadow_w_inputs.py checks on the CPU that the inputs are what they are meant to be, tests/test_gpu_shadow_w.py
injects them through arctic_write_gbuffer.

A rasterised frame never takes that branch (the sun is orthographic: w is 1 at every vertex and within a few ulps of 1 after interpolation),
and scenes.random_gbuffer writes w = 1.0 exactly.  A wave takes it when ANY of its 64 lanes (one 8 x 8 tile) has a w outside 1 -+ 6 ulp-steps,
or a coordinate that is exactly zero beside a w that is not exactly 1.  So the frame is built per tile, one class per tile in a fixed pattern:

  a  w uniform in [0.5, 2]
  b  w negative, -[0.5, 2], and about one lane in eight with |w| = 2^-20 or 2^20
  c  w = 1 -+ 1..6 ulp-steps in every lane (the near-one domain), and ONE covered lane with x, y or z exactly 0.0 or -0.0: the whole tile leaves
     the near-one quotient for the general one
  d  w = 1 -+ 7 ulp-steps: just outside the near-one domain
  e  w == 1 in every lane: the control, the first branch
  m  every lane draws its class from a..e

In every class xyz = fl32(w q) with q in the usual ranges of scenes.random_gbuffer (x, y in [-1.1, 1.1], z in [0, 1.1]), so the quotients cover the
map, its borders and the outside.  The map (S x S) has a random half (columns below S / 2, i.e. quotients x < 0: per-texel noise, the 25 taps
decide) and a smooth half (the min/max table decides).
"""
import numpy as np

W, H, S = 96, 64, 256
TILE = 8
NO_MAT = 0xFFFFFFFF
CLASSES = "abcdem"
SEED = 20261


def tile_classes(rows=H, width=W):
    """(rows / 8, width / 8) array of class letters: a diagonal pattern, sixteen tiles of each class at 96 x 64"""
    ty, tx = np.mgrid[0:rows // TILE, 0:width // TILE]
    return np.array(list(CLASSES))[(tx + 5 * ty) % len(CLASSES)]


def one_plus_steps(k):
    """1.0 moved by k steps of its bit pattern (what near_one_divisible counts): k = -6 .. 6 is the near-one domain"""
    return (np.uint32(0x3F800000) + np.asarray(k, np.int64)).astype(np.uint32).view(np.float32)


def _w_of(rng, cls):
    """w per pixel from its class letter"""
    n = cls.shape
    sign = np.where(rng.random(n) < 0.5, -1, 1)
    general = (0.5 + 1.5 * rng.random(n)).astype(np.float32)
    extreme = np.where(rng.random(n) < 0.5, np.float32(2.0 ** -20), np.float32(2.0 ** 20)) * sign.astype(np.float32)
    negative = np.where(rng.random(n) < 0.125, extreme, -general).astype(np.float32)
    near = one_plus_steps(sign * rng.integers(1, 7, n))
    outside = one_plus_steps(sign * 7)
    w = np.ones(n, np.float32)
    for letter, values in (("a", general), ("b", negative), ("c", near), ("d", outside)):
        w = np.where(cls == letter, values, w)
    return w.astype(np.float32)


def _bilinear(m, u, v):
    """the map at (u, v) in [0, 1]^2, texel centres at (i + 0.5) / S (float64; only to place depths NEAR the surface)"""
    n = m.shape[0]
    x, y = u * n - 0.5, v * n - 0.5
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = x - x0, y - y0
    at = lambda yy, xx: m[np.clip(yy, 0, n - 1), np.clip(xx, 0, n - 1)].astype(np.float64)
    return (at(y0, x0) * (1 - fx) + at(y0, x0 + 1) * fx) * (1 - fy) + (at(y0 + 1, x0) * (1 - fx) + at(y0 + 1, x0 + 1) * fx) * fy


def light_space(seed=SEED, mat=None, smap=None, rows=H, width=W):
    """(ls (rows, width, 4) float32, tile class per pixel, lane class per pixel, q (rows, width, 3): the quotients the positions were made from,
    zero lanes: [(y, x, component)]).  mat, if given, is edited in place so that the zero lane of each c tile is covered; with smap, the depth of
    nearly half of the pixels inside the map is the map's own there -+ 0.015 (still within [0, 1.1]): penumbra where the map is noise."""
    rng = np.random.default_rng(seed)
    tiles = tile_classes(rows, width)
    tile_cls = np.repeat(np.repeat(tiles, TILE, 0), TILE, 1)
    lane_cls = np.where(tile_cls == "m", np.array(list("abcde"))[rng.integers(0, 5, tile_cls.shape)], tile_cls)
    q = np.empty((rows, width, 3), np.float32)
    q[..., :2] = rng.random((rows, width, 2), dtype=np.float32) * 2.2 - 1.1
    q[..., 2] = rng.random((rows, width), dtype=np.float32) * 1.1
    if smap is not None:   # a uniform depth meets the 25 taps' spread (a twentieth of a texel) once in thirty pixels: steer nearly half of the pixels onto the map's surface
        near = (rng.random((rows, width)) < 0.45) & (np.abs(q[..., :2]) <= 1).all(-1)
        surface = _bilinear(smap, q[..., 0] * 0.5 + 0.5, 1.0 - (q[..., 1] * 0.5 + 0.5))
        q[..., 2] = np.where(near, np.clip(surface + rng.uniform(-0.015, 0.015, (rows, width)), 0.0, 1.1), q[..., 2]).astype(np.float32)
    w = _w_of(rng, lane_cls)
    ls = np.empty((rows, width, 4), np.float32)
    ls[..., :3] = q * w[..., None]                     # fl32(w q): each product rounds once
    ls[..., 3] = w
    zero_lanes = []
    for k, (ty, tx) in enumerate(zip(*np.nonzero(tiles == "c"))):
        y, x, comp = ty * TILE + int(rng.integers(0, TILE)), tx * TILE + int(rng.integers(0, TILE)), k % 3
        ls[y, x, comp] = np.float32(-0.0) if (k // 3) % 2 else np.float32(0.0)
        zero_lanes.append((y, x, comp))
        if mat is not None and mat[y, x] == NO_MAT:
            mat[y, x] = 0
    return ls, tile_cls, lane_cls, q, zero_lanes


def shadow_map(seed=SEED, size=S):
    rng = np.random.default_rng(seed + 1)
    m = np.empty((size, size), np.float32)
    m[:, :size // 2] = 0.2 + 0.7 * rng.random((size, size // 2), dtype=np.float32)
    yy, xx = np.mgrid[0:size, size // 2:size]
    m[:, size // 2:] = 0.5 + 0.2 * np.sin(xx / 17.0) * np.cos(yy / 23.0)
    return m


def with_w_one(ls, tile_cls):
    """the second G-buffer of the A/B check: w = 1.0 in every lane of every tile, everything else as it is.  The e tiles are the same bytes in both."""
    out = ls.copy()
    out[..., 3] = 1.0
    assert np.array_equal(out[tile_cls == "e"].view(np.uint32), ls[tile_cls == "e"].view(np.uint32))
    return out


def shadow_factors(oracle, smap, ls, mat):
    """calculate_shadow of the CPU oracle per covered pixel (NaN elsewhere)"""
    out = np.full(mat.shape, np.nan)
    ls = np.ascontiguousarray(ls, np.float32)
    smap = np.ascontiguousarray(smap, np.float32)
    for y, x in zip(*np.nonzero(mat != NO_MAT)):
        out[y, x] = oracle.calculate_shadow(smap, ls[y, x])
    return out


def check_input_conditions(factors, tile_cls, mat):
    """among the covered pixels of the tiles of classes a to d: at least 500 factors strictly inside (0, 1), 200 exactly 0, 200 exactly 1"""
    f = factors[(mat != NO_MAT) & np.isin(tile_cls, list("abcd"))]
    counts = dict(partial=int(((f > 0) & (f < 1)).sum()), zero=int((f == 0).sum()), one=int((f == 1).sum()))
    assert not np.isnan(f).any()
    assert counts["partial"] >= 500 and counts["zero"] >= 200 and counts["one"] >= 200, counts
    return counts
