"""The temporal upscaler (include/arctic_hip.h: arctic_taa_upscale_device and the definition in front of it) and arctic_taa_upscale_jitter
restated in numpy from the header's text, float32 throughout, one rounding per operation in the written order: they reproduce the library's
{out, N} by bytes.  Independent of the library: nothing here calls it.  Also the analytic scene of the quality claim, a bilinear stretch to
compare against, and, for the tests that must not be vacuous, the definition with one deliberate defect."""
import numpy as np

F = np.float32
LUMA_WEIGHT, SOURCE_COMPOSED, NO_CLAMP = 1, 2, 4
JITTER_EXACT = 0x80000000
DEFECTS = ("dropped / rx", "floor without + j", "beta select removed", "clamp under NO_CLAMP", "floor select removed", "box around p", "velocity of p")
# the size pairs of the issue: (w, h) -> (W, H)
PAIRS = (((1, 1), (1, 1)), ((1, 1), (4, 4)), ((8, 8), (16, 16)), ((17, 9), (29, 14)), ((40, 24), (64, 40)), ((37, 23), (148, 92)))


def _max(a, b):
    """the definition's max: (a < b) ? b : a"""
    return np.where(a < b, b, a)


def _min(a, b):
    """the definition's min: (b < a) ? b : a"""
    return np.where(b < a, b, a)


def halton32(i, base):
    """halton(i, b) of the header in fp32: f = f / b; x = x + f * (float)(i % b)"""
    f, x, b = F(1.0), F(0.0), F(base)
    while i > 0:
        f = F(f / b)
        x = F(x + F(f * F(i % base)))
        i //= base
    return x


def jitter(index, in_size, out_size, exact=False):
    """arctic_taa_upscale_jitter -> (2,) float32"""
    (w, h), (W, H) = in_size, out_size
    if exact:
        s = W // w
        assert W == s * w and H == s * h and s in (1, 2, 4)
        i = (index & 0x7FFFFFFF) % (s * s)
        return np.array([F(0.5) - F(F(i % s) + F(0.5)) / F(s), F(0.5) - F(F(i // s) + F(0.5)) / F(s)], F)
    L = 8 * -(-W // w) * -(-H // h)
    i = (index & 0x7FFFFFFF) % L + 1
    return np.array([halton32(i, 2) - F(0.5), halton32(i, 3) - F(0.5)], F)


def nearest(n_out, n_in, j, defect=None):
    """step 1 along one axis for every output pixel: (q int64, D float32, u float32)"""
    r = F(n_in) / F(n_out)
    p = np.arange(n_out).astype(F)
    u = (p + F(0.5)) * r
    f = np.floor(u if defect == "floor without + j" else u + j)
    top = F(n_in) - F(1.0)
    qf = np.where(f < F(0.0), F(0.0), np.where(f > top, top, f)).astype(F)
    D = (((qf + F(0.5)) - j) - u) if defect == "dropped / rx" else (((qf + F(0.5)) - j) - u) / r
    return qf.astype(np.int64), D.astype(F), r


def box_at(cur, qx, qy):
    """step 2: lo, hi (H, W, 3) over the 3 x 3 input pixels around (qx, qy), clamped at the input frame's edge; a NaN neighbour is ignored"""
    h, w = cur.shape[:2]
    lo = hi = None
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            n = cur[np.clip(qy + dy, 0, h - 1), np.clip(qx + dx, 0, w - 1)]
            if lo is None:
                lo, hi = n.copy(), n.copy()
            lo = np.where(n < lo, n, lo)
            hi = np.where(n > hi, n, hi)
    return lo, hi


def upscale(cur, out_size, velocity=None, prev=None, jitter=(0.0, 0.0), max_history=32.0, min_weight=0.0, sharpness=1.0, confidence_floor=2.0 ** -6, flags=0, defect=None):
    """steps 1 to 6 for a whole output frame: cur (h, w, 3), velocity (h, w, 2) or None, prev (H, W, 4) = the previous {r, g, b, N} or None = U is
    empty -> (H, W, 4) float32 {out, N}"""
    assert defect is None or defect in DEFECTS, defect
    cur = np.asarray(cur, F)
    h, w = cur.shape[:2]
    W, H = int(out_size[0]), int(out_size[1])
    assert w <= W <= 4 * w and h <= H <= 4 * h
    jx, jy = F(jitter[0]), F(jitter[1])
    mh, mw, sh, cf = F(max_history), F(min_weight), F(sharpness), F(confidence_floor)
    with np.errstate(all="ignore"):
        qx1, Dx1, rx = nearest(W, w, jx, defect)
        qy1, Dy1, ry = nearest(H, h, jy, defect)
        qx, qy = np.broadcast_to(qx1[None, :], (H, W)), np.broadcast_to(qy1[:, None], (H, W))
        Dx, Dy = np.broadcast_to(Dx1[None, :], (H, W)), np.broadcast_to(Dy1[:, None], (H, W))
        c = cur[qy, qx]
        if defect == "box around p":
            ys, xs = np.mgrid[0:H, 0:W]
            lo, hi = box_at(cur, np.minimum(xs, w - 1), np.minimum(ys, h - 1))
        else:
            lo, hi = box_at(cur, qx, qy)
        beta = _max(F(0.0), F(1.0) - sh * (Dx * Dx + Dy * Dy)).astype(F)
        out = np.concatenate([c, _max(beta, cf)[..., None]], -1).astype(F)
        if prev is None:
            return out
        prev = np.asarray(prev, F)
        assert prev.shape == (H, W, 4)
        if velocity is None:
            v = np.zeros((H, W, 2), F)
        elif defect == "velocity of p":
            ys, xs = np.mgrid[0:H, 0:W]
            v = np.asarray(velocity, F)[np.minimum(ys, h - 1), np.minimum(xs, w - 1)]
        else:
            v = np.asarray(velocity, F)[qy, qx]
        ys, xs = np.mgrid[0:H, 0:W]
        px, py = xs.astype(F), ys.astype(F)
        if defect == "dropped / rx":
            hx, hy = ((px + F(0.5)) + v[..., 0]) + jx, ((py + F(0.5)) + v[..., 1]) + jy
        else:
            hx, hy = ((px + F(0.5)) + v[..., 0] / rx) + jx / rx, ((py + F(0.5)) + v[..., 1] / ry) + jy / ry
        gx, gy = hx - F(0.5), hy - F(0.5)
        ix, iy = np.floor(gx), np.floor(gy)
        ax, ay = gx - ix, gy - iy
        ok = np.isfinite(hx) & np.isfinite(hy) & (ix >= F(-1.0)) & (ix <= F(W) - F(1.0)) & (iy >= F(-1.0)) & (iy <= F(H) - F(1.0))
        x0, y0 = np.where(ok, ix, 0).astype(np.int64), np.where(ok, iy, 0).astype(np.int64)
        bx, by = F(1.0) - ax, F(1.0) - ay
        weight = [bx * by, ax * by, bx * ay, ax * ay]
        k, ke = [], [[], [], [], []]
        for t in range(4):
            tx, ty = x0 + (t & 1), y0 + (t >> 1)
            inside = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H)
            e = prev[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
            accepted = ok & inside & (e[..., 3] > 0)
            k.append(np.where(accepted, weight[t], F(0.0)))
            for i in range(4):
                ke[i].append(np.where(accepted, weight[t] * e[..., i], F(0.0)))
        total = lambda s: ((s[0] + s[1]) + s[2]) + s[3]
        S = total(k)
        passed = ok & (S > mw)
        hc = np.stack([total(ke[i]) / S for i in range(3)], -1)
        hn = total(ke[3]) / S
        if not (flags & NO_CLAMP) or defect == "clamp under NO_CLAMP":
            hc = np.where(hc < lo, lo, hc)
            hc = np.where(hc > hi, hi, hc)
        sum_n = hn + beta
        N = _min(sum_n, mh)
        a = (beta / N)[..., None]
        if flags & LUMA_WEIGHT:
            wc = F(1.0) / (F(1.0) + _max(_max(_max(c[..., 0], c[..., 1]), c[..., 2]), F(0.0)))
            wh = F(1.0) / (F(1.0) + _max(_max(_max(hc[..., 0], hc[..., 1]), hc[..., 2]), F(0.0)))
            kc, kh = a * wc[..., None], (F(1.0) - a) * wh[..., None]
            blended = (c * kc + hc * kh) / (kc + kh)
        else:
            blended = hc + (c - hc) * a
        if defect != "floor select removed":
            blended = np.where((sum_n == beta)[..., None], c, blended)
        if defect != "beta select removed":
            blended = np.where((beta == F(0.0))[..., None], hc, blended)
        out[..., :3] = np.where(passed[..., None], blended, c)
        out[..., 3] = np.where(passed, N, out[..., 3])
    assert out.dtype == F
    return out


def sequence(frames, out_size, velocities=None, jitters=None, prev=None, **kw):
    """the upscaler over a list of frames -> the list of U after every call"""
    out = []
    for i, c in enumerate(frames):
        prev = upscale(c, out_size, None if velocities is None else velocities[i], prev, jitter=(0.0, 0.0) if jitters is None else jitters[i], **kw)
        out.append(prev)
    return out


def still_velocity(j, in_size):
    """velocity2 of a still scene drawn with jitter j: -j in every input pixel"""
    return np.broadcast_to(np.array([-F(j[0]), -F(j[1])], F), (in_size[1], in_size[0], 2)).copy()


# ---- the analytic scene of the quality claim: edges, a thin line and a zone plate, in coordinates of the unit square ----------------------------
def analytic(u, v):
    """the HDR colour at positions u, v in [0, 1] (any shape) -> (..., 3) float64"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    c = np.empty(u.shape + (3,))
    c[...] = (0.05, 0.08, 0.12)
    edge = (v - 0.15) - 0.37 * (u - 0.1) > 0                               # a slanted edge: bright below it
    c[edge] = (1.8, 1.2, 0.6)
    disc = (u - 0.3) ** 2 + (v - 0.62) ** 2 < 0.2 ** 2                     # a disc's curved edge over it
    c[disc] = (3.0, 0.4, 2.0)
    line = np.abs((v - 0.2) + 0.61 * (u - 0.5)) < 0.006                    # a thin line, narrower than a low-resolution pixel
    c[line] = (4.0, 4.0, 3.0)
    zone = (u > 0.55) & (v > 0.45)                                         # a zone plate in the lower right quarter
    rr = (u - 0.55) ** 2 + (v - 0.45) ** 2
    z = 0.5 + 0.5 * np.cos(170.0 * rr)
    c[zone] = np.stack([z, z, z], -1)[zone] * (2.0, 1.5, 1.0)
    return c


def analytic_frame(size, j=(0.0, 0.0)):
    """the w x h frame a camera jittered by j draws: pixel p is sampled at p + 0.5 - j"""
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    return analytic((xs + 0.5 - float(j[0])) / w, (ys + 0.5 - float(j[1])) / h).astype(F)


def analytic_supersample(size, n=8):
    """the n x n box-filtered frame, float64"""
    w, h = size
    ys, xs = np.mgrid[0:h, 0:w]
    acc = np.zeros((h, w, 3))
    for sy in range(n):
        for sx in range(n):
            acc += analytic((xs + (sx + 0.5) / n) / w, (ys + (sy + 0.5) / n) / h)
    return acc / (n * n)


def stretch_bilinear(img, out_size):
    """a w x h frame stretched to W x H with pixel centres aligned and the edge clamped, float64"""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    W, H = out_size
    gx, gy = (np.arange(W) + 0.5) * w / W - 0.5, (np.arange(H) + 0.5) * h / H - 0.5
    x0, y0 = np.floor(gx).astype(int), np.floor(gy).astype(int)
    ax, ay = (gx - x0)[None, :, None], (gy - y0)[:, None, None]
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    top = img[ya][:, xa] * (1 - ax) + img[ya][:, xb] * ax
    bottom = img[yb][:, xa] * (1 - ax) + img[yb][:, xb] * ax
    return top * (1 - ay) + bottom * ay


def reinhard(c):
    c = np.asarray(c, np.float64)
    return c / (1.0 + c)
