"""The motion blur of include/arctic_hip.h (arctic_motion_blur_device and the text in front of it) restated in numpy: fp32 throughout, one rounding
per operation in the written order -- every array below is float32 and every scalar is wrapped in F(), so no operation is carried out in a wider
format.  prepare() is steps 1 to 3 (tile_max2, neighbour_max2, P), gather() is step 4 (out), blur() is both.  `defect`: for the tests that must
not be vacuous, the definition with one deliberate defect."""
import numpy as np

F = np.float32
DITHER, SOURCE_COMPOSED, SOURCE_TAA = 1, 2, 4
TILE = 8
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], F)
DEFECTS = ("tie to the last lane", "window one tile short", "window tie to the last", "f and b swapped", "dist without |t|", "rejected tap multiplied", "l_p without its floor",
           "clamp left out", "taps not centred", "cylinder left out")


def _max(a, b):
    """max(a, b) = (a < b) ? b : a"""
    return np.where(a < b, b, a).astype(F)


def clamp01(x):
    """!(x > 0) ? 0 : (x > 1 ? 1 : x): a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.where(~(x > F(0.0)), F(0.0), np.where(x > F(1.0), F(1.0), x)).astype(F)


def half_velocity(velocity, shutter=1.0, max_radius=16.0, defect=None):
    """step 1 for every pixel: (h (H, W, 2), l2 (H, W), l (H, W))"""
    v = np.asarray(velocity, F)
    with np.errstate(all="ignore"):
        h = (v * (F(0.5) * F(shutter))).astype(F)
        h = np.where(np.isfinite(h).all(-1)[..., None], h, F(0.0)).astype(F)
        hx, hy = h[..., 0], h[..., 1]
        length = np.sqrt(hx * hx + hy * hy)
        over = length > F(max_radius)
        if defect == "clamp left out":
            over = np.zeros_like(over)
        s = F(max_radius) / np.where(over, length, F(1.0))
        hx, hy = np.where(over, hx * s, hx).astype(F), np.where(over, hy * s, hy).astype(F)
        l2 = (hx * hx + hy * hy).astype(F)
        l = np.sqrt(l2) if defect == "l_p without its floor" else _max(np.sqrt(l2), F(0.5))
    return np.stack([hx, hy], -1), l2, l.astype(F)


def window(max_radius):
    return int(np.ceil(F(max_radius) / F(8.0)))


def prepare(velocity, depth=None, shutter=1.0, max_radius=16.0, defect=None, **_):
    """steps 1 to 3: (tile_max2, neighbour_max2) of shape (tiles_y, tiles_x, 2) and P (H, W, 2) = {l, z}"""
    h, l2, l = half_velocity(velocity, shutter, max_radius, defect)
    H, W = l.shape
    z = np.zeros((H, W), F) if depth is None else np.asarray(depth, F)
    P = np.stack([l, z], -1)
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    tile = np.zeros((ty, tx, 2), F)
    for y in range(ty):
        for x in range(tx):
            block = (slice(y * TILE, min(y * TILE + TILE, H)), slice(x * TILE, min(x * TILE + TILE, W)))
            key = l2[block].reshape(-1)                                          # row-major inside the tile: the order of the lane index
            k = len(key) - 1 - int(np.argmax(key[::-1])) if defect == "tie to the last lane" else int(np.argmax(key))   # argmax: the first among equals
            tile[y, x] = h[block].reshape(-1, 2)[k]
    R = window(max_radius) - (1 if defect == "window one tile short" else 0)
    with np.errstate(over="ignore"):
        t2 = (tile[..., 0] * tile[..., 0] + tile[..., 1] * tile[..., 1]).astype(F)
    near = np.zeros_like(tile)
    for y in range(ty):
        for x in range(tx):
            block = (slice(max(y - R, 0), min(y + R + 1, ty)), slice(max(x - R, 0), min(x + R + 1, tx)))
            key = t2[block].reshape(-1)
            k = len(key) - 1 - int(np.argmax(key[::-1])) if defect == "window tie to the last" else int(np.argmax(key))
            near[y, x] = tile[block].reshape(-1, 2)[k]
    return tile, near, P


def gather(color, P, neighbour_max, samples=15, depth_extent=0.05, flags=0, defect=None, **_):
    """step 4 for every pixel: out (H, W, 3)"""
    C = np.asarray(color, F)
    H, W = C.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.asarray(neighbour_max, F)[ys // TILE, xs // TILE]
    dx, dy = d[..., 0], d[..., 1]
    n, de = F(samples), F(depth_extent)
    with np.errstate(all="ignore"):
        dl = np.sqrt(dx * dx + dy * dy)
        fast = dl > F(0.5)
        lp, zp = P[..., 0], P[..., 1]
        w = (F(1.0) / lp).astype(F)
        acc = (C * w[..., None]).astype(F)
        o = ((BAYER[ys & 3, xs & 3] + F(0.5)) / F(16.0)) - F(0.5) if flags & DITHER else np.zeros((H, W), F)
        cx, cy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)

        def cone(dist, l):
            return clamp01(F(1.0) - dist / l)

        def cylinder(dist, l):
            if defect == "cylinder left out":
                return np.zeros_like(l)
            s = clamp01((dist - F(0.95) * l) / (F(0.1) * l))
            return (F(1.0) - (s * s) * (F(3.0) - F(2.0) * s)).astype(F)

        for i in range(int(samples)):
            centre = F(0.0) if defect == "taps not centred" else F(0.5)
            t = ((((F(i) + centre) + o) / n) * F(2.0) - F(1.0)).astype(F)
            qx, qy = np.floor(cx + t * dx), np.floor(cy + t * dy)
            inside = (qx >= F(0.0)) & (qx <= F(W - 1)) & (qy >= F(0.0)) & (qy <= F(H - 1))
            ix, iy = np.where(inside, qx, F(0.0)).astype(np.int64), np.where(inside, qy, F(0.0)).astype(np.int64)
            dist = (t if defect == "dist without |t|" else np.abs(t)) * dl
            lq, zq = P[iy, ix, 0], P[iy, ix, 1]
            f = clamp01(F(1.0) - (zq - zp) / de)
            b = clamp01(F(1.0) - (zp - zq) / de)
            if defect == "f and b swapped":
                f, b = b, f
            a = ((f * cone(dist, lq) + b * cone(dist, lp)) + (cylinder(dist, lq) * cylinder(dist, lp)) * F(2.0)).astype(F)
            if defect == "rejected tap multiplied":                               # weight 0 times the colour, not a select
                a = np.where(inside & (a > F(0.0)), a, F(0.0)).astype(F)
                take = fast
            else:
                take = fast & inside & (a > F(0.0))
            w = np.where(take, w + a, w).astype(F)
            acc = np.where(take[..., None], acc + C[iy, ix] * a[..., None], acc).astype(F)
        out = np.where(fast[..., None], acc / w[..., None], C).astype(F)
    return out


def blur(color, velocity, depth=None, **kw):
    """steps 1 to 4: (out, tile_max2, neighbour_max2, P)"""
    tile, near, P = prepare(velocity, depth, **kw)
    return gather(color, P, near, **kw), tile, near, P


def reinhard(c):
    c = np.asarray(c, np.float64)
    return c / (1.0 + c)
