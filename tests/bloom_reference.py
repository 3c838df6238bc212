"""Bloom as include/arctic_hip.h defines it (the text in front of arctic_bloom_device), restated in numpy from that text -- not from csrc/bloom.h.
Every operation is one numpy operation on arrays of `dt`, in the written order: with dt = float32 (the default) each rounds once, as the
definition says, and the result is what the library must give BY BYTES; with dt = float64 it is the same definition at a precision where the
roundings do not matter, the yardstick of the fp32 definition's own error.  Planes are (height, width, 3)."""
import numpy as np

F = np.float32
SOURCE_COMPOSED, SOURCE_TAA, SOURCE_MOTION_BLUR, SOURCE_DOF = 1, 2, 4, 8
DEFAULTS = dict(threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=1.0, levels=5)
EVEN = (0.0625, 0.3125, 0.4375, 0.1875)
ODD = (0.1875, 0.4375, 0.3125, 0.0625)


def _min(a, b):
    """(b < a) ? b : a"""
    return np.where(b < a, b, a)


def _max(a, b):
    """(a < b) ? b : a"""
    return np.where(a < b, b, a)


def _field(kw, name, dt):
    """a field of the record: a float32, whatever the arithmetic's precision"""
    return dt(F(kw.get(name, DEFAULTS[name])))


def level_sizes(width, height, levels):
    """[(W_k, H_k)] for k = 1 .. levels"""
    sizes = []
    for _ in range(levels):
        width, height = (width + 1) // 2, (height + 1) // 2
        sizes.append((width, height))
    return sizes


def prefilter(C, dt=F, **kw):
    """step 1: b"""
    threshold, soft_knee, clamp_max = _field(kw, "threshold", dt), _field(kw, "soft_knee", dt), _field(kw, "clamp_max", dt)
    C = np.asarray(C, F).astype(dt)
    with np.errstate(invalid="ignore"):
        x = np.where(C > 0, _min(C, clamp_max), dt(0))
    br = _max(x[..., 0], _max(x[..., 1], x[..., 2]))
    knee = threshold * soft_knee
    t = br - (threshold - knee)
    t = _min(_max(t, dt(0)), dt(2) * knee)
    soft = (t * t) / (dt(4) * knee + dt(F(1e-5)))
    m = _max(soft, br - threshold)
    contrib = _min(m / _max(br, dt(F(1e-5))), dt(1))
    return x * contrib[..., None]


def down(S, karis, dt=F):
    """step 2: DOWN(S) at every pixel of the next level"""
    Hs, Ws = S.shape[:2]
    xs, ys = np.arange((Ws + 1) // 2), np.arange((Hs + 1) // 2)

    def tex(i, j):
        cx = np.clip(2 * xs - 2 + i, 0, Ws - 1)
        cy = np.clip(2 * ys - 2 + j, 0, Hs - 1)
        return S[cy[:, None], cx[None, :]]

    def box(a, b):
        return ((tex(a, b) + tex(a + 1, b)) + (tex(a, b + 1) + tex(a + 1, b + 1))) * dt(0.25)

    def group(a, b):
        return ((box(a, b) + box(a + 2, b)) + (box(a, b + 2) + box(a + 2, b + 2))) * dt(0.25)

    G0, G1, G2, G3, G4 = group(1, 1), group(0, 0), group(2, 0), group(0, 2), group(2, 2)
    if not karis:
        return G0 * dt(0.5) + ((G1 + G2) + (G3 + G4)) * dt(0.125)

    def luma(G):
        return (dt(F(0.2126)) * G[..., 0] + dt(F(0.7152)) * G[..., 1]) + dt(F(0.0722)) * G[..., 2]

    w0 = (dt(0.5) / (dt(1) + luma(G0)))[..., None]
    w1, w2, w3, w4 = ((dt(0.125) / (dt(1) + luma(G)))[..., None] for G in (G1, G2, G3, G4))
    num = w0 * G0 + ((w1 * G1 + w2 * G2) + (w3 * G3 + w4 * G4))
    den = w0 + ((w1 + w2) + (w3 + w4))
    return num / den


def _axis(n, dt):
    """step 3's base and the four weights of every destination coordinate 0 .. n-1"""
    x = np.arange(n)
    h = x >> 1
    odd = (x & 1) == 1
    base = np.where(odd, h - 1, h - 2)
    w = np.where(odd[:, None], np.array(ODD, dt)[None, :], np.array(EVEN, dt)[None, :])
    return base, w


def up(T, width, height, dt=F):
    """step 3: UP(T) at every pixel of a width x height level"""
    Ht, Wt = T.shape[:2]
    bx, wx = _axis(width, dt)
    by, wy = _axis(height, dt)
    wx = wx[None, :, :, None]                                                    # [y, x, tap, channel]
    wy = wy[:, None, :, None]

    def tex(i, j):
        cx = np.clip(bx + i, 0, Wt - 1)
        cy = np.clip(by + j, 0, Ht - 1)
        return T[cy[:, None], cx[None, :]]

    def row(j):
        return (wx[:, :, 0] * tex(0, j) + wx[:, :, 1] * tex(1, j)) + (wx[:, :, 2] * tex(2, j) + wx[:, :, 3] * tex(3, j))

    return (wy[:, :, 0] * row(0) + wy[:, :, 1] * row(1)) + (wy[:, :, 2] * row(2) + wy[:, :, 3] * row(3))


def pyramid(C, dt=F, karis=True, **kw):
    """steps 1 to 3: ([D_1 .. D_L], [U_1 .. U_{L-1}])"""
    L = int(kw.get("levels", DEFAULTS["levels"]))
    spread = _field(kw, "spread", dt)
    D = [down(prefilter(C, dt, **kw), karis, dt)]
    for _ in range(2, L + 1):
        D.append(down(D[-1], False, dt))
    U = [None] * L
    U[L - 1] = D[L - 1]
    for k in range(L - 1, 0, -1):                                                # level k is index k - 1
        U[k - 1] = D[k - 1] + spread * up(U[k], D[k - 1].shape[1], D[k - 1].shape[0], dt)
    return D, U[:L - 1]


def composite(C, U1, dt=F, **kw):
    """step 4: out"""
    C = np.asarray(C, F).astype(dt)
    H, W = C.shape[:2]
    a = _field(kw, "intensity", dt) * up(U1, W, H, dt)
    with np.errstate(invalid="ignore"):
        return np.where(a > 0, C + a, C)


def bloom(C, dt=F, **kw):
    """(out, [D_1 .. D_L], [U_1 .. U_{L-1}])"""
    D, U = pyramid(C, dt, **kw)
    return composite(C, U[0] if U else D[0], dt, **kw), D, U
