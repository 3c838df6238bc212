"""Analytic G-buffers for the temporal accumulation: a floor, a wall and a box as ray/plane hits through frame_constants' matrix, made in numpy, so
that the CPU tests (the numpy arbiter against the host arbiter) and the device tests (against k_ao_accumulate, injected with arctic_write_gbuffer)
judge the same inputs.  Four camera paths -- still, translated, rotated, and one that passes through the wall and back, so that the previous
camera has the current frame's surfaces BEHIND it (c3 <= 0) -- and the current byte planes of every call."""
import numpy as np

import ao_history_reference as HR

F = np.float32
SIZES = [(96, 64), (61, 37)]
CALLS = [1, 2, 5]
MOVES = ["still", "translated", "rotated", "through the wall"]
MIN_CLASS = 20
# the surfaces: (point, normal as stored -- NOT unit length --, bounds (lo, hi))
FLOOR = ((0.0, 0.0, 0.0), (0.0, 2.0, 0.0), ((-8.0, -1.0, -9.0), (8.0, 1.0, 8.0)))
WALL = ((0.0, 0.0, -3.0), (0.0, 0.0, 0.5), ((-3.0, 0.0, -4.0), (3.0, 2.6, -2.0)))
BOX = ((-0.6, 0.0, -0.9), (0.6, 1.0, 0.3))
_cache = {}


def camera(eye, pitch, yaw, aspect):
    return dict(eye=tuple(eye), rotation=(pitch, yaw), aspect=aspect, fov_y=50.0, z_near_far=(0.1, 100.0))


def cameras(move, n, aspect):
    """the camera of every call of a path"""
    k = np.arange(n)
    if move == "still":
        return [camera((0.4, 1.5, 3.6), -14.0, -92.0, aspect) for _ in k]
    if move == "translated":
        return [camera((0.4 + 0.23 * i, 1.5 + 0.05 * i, 3.6 - 0.11 * i), -14.0, -92.0, aspect) for i in k]
    if move == "rotated":
        return [camera((0.4, 1.5, 3.6), -14.0 - 1.3 * i, -92.0 + 3.7 * i, aspect) for i in k]
    # in front of the wall, beyond it (looking on, at the floor behind it), and back
    return [camera((0.4, 1.5, 3.6), -14.0, -92.0, aspect) if i % 2 == 0 else camera((0.3, 1.4, -4.5 - 0.1 * i), -20.0, -90.0, aspect) for i in k]


def desc_of(pkg, cam):
    sc = pkg.scenes
    return sc.SceneDesc(camera=cam, ambient=0.1, sun=sc.DEFAULT_SUN, objects=pkg.scene.make_objects([]))


def gbuffer(pkg, cam, W, H):
    """-> (attrs (H, W, 18) float32, material (H, W) uint32, P (4, 4) float32): the nearest hit of every pixel centre's ray, then a patch of
    degenerate normals (test_gpu_compose's four kinds) on covered pixels"""
    P = pkg.renderer.frame_constants(desc_of(pkg, cam))[0]
    inv = np.linalg.inv(P.astype(np.float64).T)
    x, y = np.meshgrid((np.arange(W) + 0.5) / W * 2 - 1, 1 - (np.arange(H) + 0.5) / H * 2)
    def unproject(z):
        p = np.stack([x, y, np.full_like(x, z), np.ones_like(x)], -1) @ inv.T
        return p[..., :3] / p[..., 3:]
    o = unproject(0.0)
    d = unproject(1.0) - o
    best = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))
    def take(t, n, ok):
        nonlocal best
        hit = ok & (t > 0) & (t < best)
        best = np.where(hit, t, best)
        normal[hit] = n
    with np.errstate(all="ignore"):
        for point, n, (lo, hi) in (FLOOR, WALL):
            n64 = np.array(n)
            t = ((np.array(point) - o) @ n64) / (d @ n64)
            p = o + t[..., None] * d
            take(t, n64, np.isfinite(t) & (p >= np.array(lo) - 1e-9).all(-1) & (p <= np.array(hi) + 1e-9).all(-1))
        lo, hi = np.array(BOX[0]), np.array(BOX[1])
        for axis in range(3):
            for bound, sign in ((lo, -1.0), (hi, 1.0)):
                t = (bound[axis] - o[..., axis]) / d[..., axis]
                p = o + t[..., None] * d
                others = [a for a in range(3) if a != axis]
                ok = np.isfinite(t) & (p[..., others] >= lo[others]).all(-1) & (p[..., others] <= hi[others]).all(-1)
                n64 = np.zeros(3)
                n64[axis] = sign * 3.0
                take(t, n64, ok)
    hit = np.isfinite(best)
    attrs = np.zeros((H, W, 18), F)
    attrs[..., 11:14] = np.where(hit[..., None], o + np.where(hit, best, 0.0)[..., None] * d, 0.0).astype(F)
    attrs[..., 8:11] = normal.astype(F)
    material = np.where(hit, 0, HR.NO_MATERIAL).astype(np.uint32)
    for k, n in enumerate([(0, 0, 0), (np.nan, 0, 1), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0)]):   # rows H-9 .. H-6, columns 4 .. 17: floor pixels in every camera
        attrs[H - 9 + k, 4:18, 8:11] = np.array(n, F)
    return attrs, material, P


def current_planes(W, H, n, seed):
    """the current byte plane of every call: mostly 0 / 255 as one ray gives them, some other bytes"""
    rng = np.random.default_rng([seed, W, H])
    out = []
    for _ in range(n):
        p = np.where(rng.uniform(size=(H, W)) < 0.6, 255, 0).astype(np.uint8)
        other = rng.uniform(size=(H, W)) < 0.2
        p[other] = rng.integers(0, 256, int(other.sum()))
        out.append(p)
    return out


def case(pkg, move, W, H, n=5):
    """-> dict(frames [(attrs, material, P)], descs, planes): the inputs of n calls along a path"""
    key = (move, W, H, n)
    if key not in _cache:
        cams = cameras(move, n, W / H)
        _cache[key] = dict(frames=[gbuffer(pkg, c, W, H) for c in cams], descs=[desc_of(pkg, c) for c in cams], planes=current_planes(W, H, n, MOVES.index(move)))
    return _cache[key]


def class_counts(pkg, W, H, hist=HR.HIST):
    """how many pixels of every class the reference sees over the second and later calls of the moving-camera paths"""
    counts = np.zeros(len(HR.CLASS_NAMES), np.int64)
    for move in MOVES[1:]:
        c = case(pkg, move, W, H)
        for _, _, cls in HR.run_sequence(c["frames"], c["planes"], hist)[1:]:
            counts += np.bincount(cls.reshape(-1), minlength=len(counts))
    return counts


def check_classes(pkg, W, H):
    counts = class_counts(pkg, W, H)
    for k, name in enumerate(HR.CLASS_NAMES):
        if k != HR.EMPTY:
            assert counts[k] >= MIN_CLASS, (name, int(counts[k]), (W, H))
    return counts
