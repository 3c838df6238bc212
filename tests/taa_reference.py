"""The temporal anti-aliasing resolve (include/arctic_hip.h: arctic_taa_resolve_device and the definition in front of it) and
arctic_jitter_proj_view restated in numpy, float32 throughout, one rounding per operation in the written order: they reproduce the library's
{out, N} by bytes.  Independent of the library: nothing here calls it.  Also the analytic scene of the anti-aliasing check, and, for the tests that
must not be vacuous, the definition with one deliberate defect."""
import numpy as np

F = np.float32
LUMA_WEIGHT, SOURCE_COMPOSED = 1, 2
DEFECTS = ("jitter not added", "velocity sign", "2x2 box", "clamp left out", "N not capped", "tap order", "wrap at the edge", "rejected weight kept")


def _max(a, b):
    """the definition's max: (a < b) ? b : a"""
    return np.where(a < b, b, a)


def _min(a, b):
    """the definition's min: (b < a) ? b : a"""
    return np.where(b < a, b, a)


def halton(i, base):
    f, x = 1.0, 0.0
    while i > 0:
        f /= base
        x += f * (i % base)
        i //= base
    return x


def taa_jitter(frame, period=8):
    i = int(frame) % int(period) + 1
    return halton(i, 2) - 0.5, halton(i, 3) - 0.5


def jitter_proj_view(m, w, h, jx, jy):
    """the [col][row] matrix with the offset applied: two operations per element of rows 0 and 1, fp32"""
    m = np.array(m, F).reshape(16).copy()
    kx, ky = (F(2.0) * F(jx)) / F(w), (F(2.0) * F(jy)) / F(h)
    for c in range(4):
        m[4 * c + 0] = m[4 * c + 0] + kx * m[4 * c + 3]
        m[4 * c + 1] = m[4 * c + 1] - ky * m[4 * c + 3]
    return m.reshape(4, 4)


def box(cur, defect=None):
    """step 1: lo, hi (H, W, 3) of the 3x3 neighbourhood clamped at the frame's edge"""
    H, W = cur.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    offs = (0, 1) if defect == "2x2 box" else (-1, 0, 1)
    lo = hi = None
    for dy in offs:
        for dx in offs:
            if defect == "wrap at the edge":
                n = cur[(ys + dy) % H, (xs + dx) % W]
            else:
                n = cur[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
            if lo is None:
                lo, hi = n.copy(), n.copy()
            lo = np.where(n < lo, n, lo)
            hi = np.where(n > hi, n, hi)
    return lo, hi


def resolve(cur, velocity=None, prev=None, jitter=(0.0, 0.0), max_history=8.0, min_weight=0.0, flags=0, defect=None):
    """steps 1 to 6 for a whole frame: cur (H, W, 3), velocity (H, W, 2) or None, prev (H, W, 4) = the previous {r, g, b, N} or None = T is empty
    -> (H, W, 4) float32 {out, N}"""
    assert defect is None or defect in DEFECTS, defect
    cur = np.asarray(cur, F)
    H, W = cur.shape[:2]
    out = np.concatenate([cur, np.ones((H, W, 1), F)], -1)
    if prev is None:
        return out
    prev = np.asarray(prev, F)
    v = np.zeros((H, W, 2), F) if velocity is None else np.asarray(velocity, F)
    jx, jy = (F(0.0), F(0.0)) if defect == "jitter not added" else (F(jitter[0]), F(jitter[1]))
    mh, mw = F(max_history), F(min_weight)
    with np.errstate(all="ignore"):
        lo, hi = box(cur, defect)
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = xs.astype(F), ys.astype(F)
        vx, vy = (-v[..., 0], -v[..., 1]) if defect == "velocity sign" else (v[..., 0], v[..., 1])
        hx, hy = ((px + F(0.5)) + vx) + jx, ((py + F(0.5)) + vy) + jy
        gx, gy = hx - F(0.5), hy - F(0.5)
        ix, iy = np.floor(gx), np.floor(gy)
        ax, ay = gx - ix, gy - iy
        ok = np.isfinite(hx) & np.isfinite(hy) & (ix >= F(-1.0)) & (ix <= F(W) - F(1.0)) & (iy >= F(-1.0)) & (iy <= F(H) - F(1.0))
        x0, y0 = np.where(ok, ix, 0).astype(np.int64), np.where(ok, iy, 0).astype(np.int64)
        bx, by = F(1.0) - ax, F(1.0) - ay
        weight = [bx * by, ax * by, bx * ay, ax * ay]
        k, ke = [], [[], [], [], []]
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            e = prev[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            accepted = ok & inside & (e[..., 3] > 0)
            k.append(weight[t] if defect == "rejected weight kept" else np.where(accepted, weight[t], F(0.0)))
            for i in range(4):
                ke[i].append(np.where(accepted, weight[t] * e[..., i], F(0.0)))
        if defect == "tap order":
            total = lambda s: ((s[3] + s[2]) + s[1]) + s[0]
        else:
            total = lambda s: ((s[0] + s[1]) + s[2]) + s[3]
        S = total(k)
        passed = ok & (S > mw)
        h = np.stack([total(ke[i]) / S for i in range(3)], -1)
        hn = total(ke[3]) / S
        if defect != "clamp left out":
            h = np.where(h < lo, lo, h)
            h = np.where(h > hi, hi, h)
        N = hn + F(1.0) if defect == "N not capped" else _min(hn + F(1.0), mh)
        a = (F(1.0) / N)[..., None]
        if flags & LUMA_WEIGHT:
            wc = F(1.0) / (F(1.0) + _max(_max(_max(cur[..., 0], cur[..., 1]), cur[..., 2]), F(0.0)))
            wh = F(1.0) / (F(1.0) + _max(_max(_max(h[..., 0], h[..., 1]), h[..., 2]), F(0.0)))
            kc, kh = a * wc[..., None], (F(1.0) - a) * wh[..., None]
            blended = (cur * kc + h * kh) / (kc + kh)
        else:
            blended = h + (cur - h) * a
        out[..., :3] = np.where(passed[..., None], blended, cur)
        out[..., 3] = np.where(passed, N, F(1.0))
    assert out.dtype == F
    return out


def sequence(frames, velocities=None, jitters=None, prev=None, **kw):
    """the resolve over a list of frames -> the list of T after every call"""
    out = []
    for i, c in enumerate(frames):
        prev = resolve(c, None if velocities is None else velocities[i], prev, jitter=(0.0, 0.0) if jitters is None else jitters[i], **kw)
        out.append(prev)
    return out


# ---- the analytic scene of the anti-aliasing check: a slanted edge and a disc with HDR colours, sampled at any position ----------------------------
def analytic(x, y, W, H):
    """the colour at screen positions x, y (any shape, pixels) -> (..., 3) float64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c = np.empty(x.shape + (3,))
    c[...] = (0.05, 0.08, 0.12)
    edge = (y - 0.15 * H) - 0.37 * (x - 0.1 * W) > 0                    # a slanted edge: bright below it
    c[edge] = (1.8, 1.2, 0.6)
    disc = (x - 0.62 * W) ** 2 + (y - 0.45 * H) ** 2 < (0.22 * H) ** 2   # an HDR disc over both
    c[disc] = (9.0, 0.4, 4.0)
    return c


def analytic_frame(W, H, jitter=(0.0, 0.0)):
    """pixel p is sampled at p + 0.5 - j: the frame a camera jittered by j draws"""
    ys, xs = np.mgrid[0:H, 0:W]
    return analytic(xs + 0.5 - jitter[0], ys + 0.5 - jitter[1], W, H).astype(F)


def analytic_supersample(W, H, n=16):
    """the n x n box-filtered frame, float64"""
    ys, xs = np.mgrid[0:H, 0:W]
    acc = np.zeros((H, W, 3))
    for sy in range(n):
        for sx in range(n):
            acc += analytic(xs + (sx + 0.5) / n, ys + (sy + 0.5) / n, W, H)
    return acc / (n * n)


def reinhard(c):
    c = np.asarray(c, np.float64)
    return c / (1.0 + c)
