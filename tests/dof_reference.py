"""Depth of field of include/arctic_hip.h (arctic_dof_device and the text in front of it) restated in numpy: fp32 throughout, one rounding per
operation in the written order -- every array below is float32 and every scalar is wrapped in F(), so no operation is carried out in a wider
format.  prepare() is steps 1 to 3 (tile_max, neighbour_max, P), gather() is step 4 (out), dof() is both; taps() is Vogel's spiral.  scatter()
is NOT the definition: a float64 brute-force scatter of the same discs under the same occlusion rule, which the gather is measured against.
`defect`: for the tests that must not be vacuous, the definition with one deliberate defect."""
import numpy as np

F = np.float32
SOURCE_COMPOSED, SOURCE_TAA, SOURCE_MOTION_BLUR = 1, 2, 4
TILE = 8
A0 = F(0.5641896)
INV_PI = F(0.31830987)
DEFECTS = ("unsigned radius", "no clamp to max_radius", "window one tile short", "no occlusion rule", "occlusion reversed", "rejected tap multiplied", "a_p without its floor",
           "uncovered pixel divided", "den test left out", "dist from the pixel centres")


def _max(a, b):
    """max(a, b) = (a < b) ? b : a"""
    return np.where(a < b, b, a).astype(F)


def _min(a, b):
    """min(a, b) = (b < a) ? b : a"""
    return np.where(b < a, b, a).astype(F)


def clamp01(x):
    """!(x > 0) ? 0 : (x > 1 ? 1 : x): a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.where(~(x > F(0.0)), F(0.0), np.where(x > F(1.0), F(1.0), x)).astype(F)


def taps(samples):
    """Vogel's spiral in float64, cast: (samples, 2) float32"""
    i = np.arange(int(samples), dtype=np.float64)
    r, phi = np.sqrt((i + 0.5) / int(samples)), i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi)], -1).astype(F)


def view_distance(depth, z_near=0.1, z_far=1000.0, defect=None):
    """step 1's zv"""
    d, n, f = np.asarray(depth, F), F(z_near), F(z_far)
    with np.errstate(all="ignore"):
        den = (f - d * (f - n)).astype(F)
        ok = np.ones_like(den, bool) if defect == "den test left out" else den > F(0.0)
        return np.where(ok, (n * f) / np.where(ok, den, F(1.0)), f).astype(F)


def signed_radius(depth, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, z_near=0.1, z_far=1000.0, defect=None):
    """step 1 for every pixel: (s, zv)"""
    zv = view_distance(depth, z_near, z_far, defect)
    with np.errstate(all="ignore"):
        s = (F(coc_scale) * (F(1.0) - F(focus_distance) / zv)).astype(F)
        s = np.where(np.isfinite(s), s, F(0.0)).astype(F)
        if defect == "unsigned radius":
            s = np.abs(s)
        if defect != "no clamp to max_radius":
            s = _min(_max(s, -F(max_radius)), F(max_radius))
    return s, zv


def disc(s, defect=None):
    """a of a signed radius"""
    return np.abs(s).astype(F) if defect == "a_p without its floor" else _max(np.abs(s), A0)


def window(max_radius):
    return int(np.ceil(F(max_radius) / F(8.0)))


def prepare(depth, focus_distance=5.0, coc_scale=8.0, max_radius=16.0, z_near=0.1, z_far=1000.0, defect=None, **_):
    """steps 1 to 3: (tile_max, neighbour_max) of shape (tiles_y, tiles_x) and P (H, W, 2) = {s, zv}"""
    s, zv = signed_radius(depth, focus_distance, coc_scale, max_radius, z_near, z_far, defect)
    H, W = s.shape
    P = np.stack([s, zv], -1)
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    tile = np.zeros((ty, tx), F)
    for y in range(ty):
        for x in range(tx):
            tile[y, x] = np.abs(s[y * TILE:min(y * TILE + TILE, H), x * TILE:min(x * TILE + TILE, W)]).max()
    R = window(max_radius) - (1 if defect == "window one tile short" else 0)
    near = np.zeros_like(tile)
    for y in range(ty):
        for x in range(tx):
            near[y, x] = tile[max(y - R, 0):min(y + R + 1, ty), max(x - R, 0):min(x + R + 1, tx)].max()
    return tile, near, P


def gather(color, P, neighbour_max, taps2=None, samples=16, depth_extent=0.5, defect=None, **_):
    """step 4 for every pixel: out (H, W, 3)"""
    C = np.asarray(color, F)
    H, W = C.shape[:2]
    u = taps(samples) if taps2 is None else np.asarray(taps2, F)
    ys, xs = np.mgrid[0:H, 0:W]
    R = np.asarray(neighbour_max, F)[ys // TILE, xs // TILE]
    n, de = F(samples), F(depth_extent)
    with np.errstate(all="ignore"):
        far = R > F(0.5)
        sp, zp = P[..., 0], P[..., 1]
        ap = disc(sp, defect)
        k = ((R * R) / n).astype(F)
        w = (INV_PI / (ap * ap)).astype(F)
        acc = (C * w[..., None]).astype(F)
        entered = np.zeros((H, W), bool)
        cx, cy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
        for i in range(int(samples)):
            ox, oy = (u[i, 0] * R).astype(F), (u[i, 1] * R).astype(F)
            qx, qy = np.floor(cx + ox), np.floor(cy + oy)
            inside = (qx >= F(0.0)) & (qx <= F(W - 1)) & (qy >= F(0.0)) & (qy <= F(H - 1))
            ix, iy = np.where(inside, qx, F(0.0)).astype(np.int64), np.where(inside, qy, F(0.0)).astype(np.int64)
            if defect == "dist from the pixel centres":
                dx, dy = (ix - xs).astype(F), (iy - ys).astype(F)
                dist = np.sqrt(dx * dx + dy * dy)
            else:
                dist = np.sqrt(ox * ox + oy * oy)
            sq, zq = P[iy, ix, 0], P[iy, ix, 1]
            aq = disc(sq, defect)
            behind = clamp01((zq - zp) / de)
            if defect == "occlusion reversed":
                behind = clamp01((zp - zq) / de)
            if defect == "no occlusion rule":
                behind = np.zeros_like(behind)
            e = (aq - behind * (aq - _min(aq, ap))).astype(F)
            cover = clamp01(e - dist)
            a = ((cover * k) / (aq * aq)).astype(F)
            if defect == "rejected tap multiplied":                               # weight 0 times the colour, not a select
                a = np.where(inside & (a > F(0.0)), a, F(0.0)).astype(F)
                take = far & inside
            else:
                take = far & inside & (a > F(0.0))
            w = np.where(take, w + a, w).astype(F)
            acc = np.where(take[..., None], acc + C[iy, ix] * a[..., None], acc).astype(F)
            entered |= take
        if defect == "uncovered pixel divided":
            entered = far
        out = np.where(entered[..., None], acc / w[..., None], C).astype(F)
    return out


def dof(color, depth, taps2=None, **kw):
    """steps 1 to 4: (out, tile_max, neighbour_max, P)"""
    tile, near, P = prepare(depth, **kw)
    return gather(color, P, near, taps2, **kw), tile, near, P


def scatter(color, P, depth_extent=0.5, **_):
    """float64, brute force, every pair of pixels: pixel q spreads its colour over its disc of radius a_q at the density 1 / (pi a_q^2); what
    reaches p is cut by the definition's occlusion rule (a source behind p reaches no further than p's own disc) and its one-pixel soft edge;
    p's own colour enters whole; the sum is normalised."""
    C = np.asarray(color, np.float64)
    H, W = C.shape[:2]
    s, z = np.asarray(P[..., 0], np.float64).reshape(-1), np.asarray(P[..., 1], np.float64).reshape(-1)
    a = np.maximum(np.abs(s), float(A0))
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y, flat = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64), C.reshape(-1, 3)
    out = np.zeros((H * W, 3))
    for p in range(H * W):
        dist = np.hypot(X - X[p], Y - Y[p])
        with np.errstate(invalid="ignore"):
            behind = np.clip(np.nan_to_num((z - z[p]) / float(depth_extent), nan=0.0), 0.0, 1.0)
        e = a - behind * (a - np.minimum(a, a[p]))
        cover = np.clip(e - dist, 0.0, 1.0)
        cover[p] = 1.0
        wq = cover / (np.pi * a * a)
        out[p] = (flat * wq[:, None]).sum(0) / wq.sum()
    return out.reshape(H, W, 3)


def reinhard(c):
    c = np.asarray(c, np.float64)
    return c / (1.0 + c)
