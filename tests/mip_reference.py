"""float64 / exact-integer numpy reference for ARCTIC_OPT_TEXTURE_MIPS (the semantics: include/arctic_hip.h next to the option).

* the chain: `chain(level0)` reproduces the device's reduction bit for bit -- integer means for the five UNORM8 channels, the three sRGB8
  channels through the library's 256-entry fp32 table in binary64 and back to the nearest code, the lower one on a tie;
* sampling: `bilinear` / `trilinear` in binary64 over a chain (the device's own, read back, or this module's);
* the level of detail: `lod_from_uv` on binary64 texture coordinates, `pixel_lod` for a triangle under a camera.

Packed texel order everywhere: {diffuse r, g, b, normal r, g, b, metal-rough g, b}, arrays of shape (h, w, 8) uint8.
"""
import ctypes
import ctypes.util

import numpy as np

_table = None


def srgb_table():
    """the 256-entry sRGB8 -> linear table of the kernels (host_math.cpp srgb8_to_linear), in fp32: x = c / 255.0f,
    x <= 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f).  powf is the C library's, the very function the library calls."""
    global _table
    if _table is None:
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.powf.restype = ctypes.c_float
        libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
        f = np.float32
        t = np.zeros(256, np.float32)
        for c in range(256):
            x = f(c) / f(255.0)
            t[c] = x / f(12.92) if x <= f(0.04045) else f(libm.powf(float((x + f(0.055)) / f(1.055)), 2.4))
        _table = t
    return _table


def level_sizes(w, h):
    """[(w_k, h_k)] for k = 0 .. levels - 1: levels = 1 + floor(log2(max(w, h)))"""
    n = 1 + int(max(w, h)).bit_length() - 1
    return [(max(1, w >> k), max(1, h >> k)) for k in range(n)]


def encode(m, table=None):
    """the code whose table value is nearest to m (binary64), the lower code on a tie"""
    t = (srgb_table() if table is None else table).astype(np.float64)
    mid = (t[:-1] + t[1:]) * 0.5                     # exact: two fp32 values
    return np.searchsorted(mid, np.asarray(m, np.float64), side="left").astype(np.uint8)   # number of midpoints strictly below m


def reduce_level(lv, table=None):
    """level k + 1 from level k ((h, w, 8) uint8)"""
    t = (srgb_table() if table is None else table).astype(np.float64)
    h, w = lv.shape[:2]
    w1, h1 = max(1, w >> 1), max(1, h >> 1)
    x = np.arange(w1)
    y = np.arange(h1)
    x0, x1 = np.minimum(2 * x, w - 1), np.minimum(2 * x + 1, w - 1)
    y0, y1 = np.minimum(2 * y, h - 1), np.minimum(2 * y + 1, h - 1)
    a, b = lv[y0][:, x0], lv[y0][:, x1]
    c, d = lv[y1][:, x0], lv[y1][:, x1]
    out = np.empty((h1, w1, 8), np.uint8)
    s = (t[a[..., :3]] + t[b[..., :3]]) + (t[c[..., :3]] + t[d[..., :3]])    # exact in binary64
    out[..., :3] = encode(s * 0.25, table)
    q = a[..., 3:].astype(np.uint32) + b[..., 3:] + c[..., 3:] + d[..., 3:] + 2
    out[..., 3:] = (q >> 2).astype(np.uint8)
    return out


def chain(level0, table=None):
    out = [np.ascontiguousarray(level0, dtype=np.uint8)]
    while max(out[-1].shape[:2]) > 1:
        out.append(reduce_level(out[-1], table))
    return out


def pack(diffuse, normal, mr):
    """three (h, w, 4) RGBA8 images of one size -> (h, w, 8)"""
    return np.concatenate([diffuse[..., :3], normal[..., :3], mr[..., 1:3]], -1).astype(np.uint8)


def decode_texels(lv, table=None):
    """(h, w, 8) uint8 -> float64 channels as the kernels filter them: base rgb decoded, normal rgb on the 0..255 scale, roughness and
    metalness in [0, 1]"""
    t = (srgb_table() if table is None else table).astype(np.float64)
    out = np.empty(lv.shape, np.float64)
    out[..., :3] = t[lv[..., :3]]
    out[..., 3:6] = lv[..., 3:6]
    out[..., 6:] = lv[..., 6:] / 255.0
    return out


def bilinear(lv, u, v, q8=False, table=None):
    """today's bilinear rule on one level: texel centres at +0.5, WRAP, decoded per texel before filtering; q8: ARCTIC_OPT_SAMPLER bit 0.
    The coordinates are taken as the fp32 values the device holds, everything after in binary64."""
    h, w = lv.shape[:2]
    tex = decode_texels(lv, table)
    u = np.asarray(u, np.float64); v = np.asarray(v, np.float64)

    def axis(c, n):
        x = (c - np.floor(c)) * n - 0.5
        if q8:
            x = np.floor(x * 256.0 + 0.5) / 256.0
        x0 = np.floor(x)
        return x0.astype(np.int64) % n, (x0.astype(np.int64) + 1) % n, x - x0
    i0, i1, fx = axis(u, w)
    j0, j1, fy = axis(v, h)
    fx = fx[..., None]; fy = fy[..., None]
    return ((1 - fx) * (1 - fy)) * tex[j0, i0] + (fx * (1 - fy)) * tex[j0, i1] + ((1 - fx) * fy) * tex[j1, i0] + (fx * fy) * tex[j1, i1]


def trilinear(levels, u, v, lam, q8=False, table=None):
    """the eight channels at (u, v) with level of detail lam (clamped to [0, levels - 1], NaN -> 0)"""
    lam = np.asarray(lam, np.float64)
    lam = np.where(lam > 0, np.minimum(lam, len(levels) - 1), 0.0)
    l0 = np.floor(lam).astype(np.int64)
    f = (lam - l0)[..., None]
    l1 = np.minimum(l0 + 1, len(levels) - 1)
    u = np.broadcast_to(np.asarray(u, np.float64), lam.shape); v = np.broadcast_to(np.asarray(v, np.float64), lam.shape)
    a = np.zeros(lam.shape + (8,)); b = np.zeros(lam.shape + (8,))
    for k, lv in enumerate(levels):
        for dst, sel in ((a, l0 == k), (b, l1 == k)):
            if sel.any():
                dst[sel] = bilinear(lv, u[sel], v[sel], q8, table)
    return a + (b - a) * f


def lod_from_uv(uv00, uv10, uv01, w, h, levels):
    """lambda = 0.5 log2(max((w du_x)^2 + (h dv_x)^2, (w du_y)^2 + (h dv_y)^2)) clamped to [0, levels - 1], NaN -> 0; also returns rho^2"""
    uv00, uv10, uv01 = (np.asarray(x, np.float64) for x in (uv00, uv10, uv01))
    dx, dy = uv10 - uv00, uv01 - uv00
    rho2 = np.maximum((w * dx[..., 0]) ** 2 + (h * dx[..., 1]) ** 2, (w * dy[..., 0]) ** 2 + (h * dy[..., 1]) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = 0.5 * np.log2(rho2)
    lam = np.where(lam > 0, np.minimum(lam, levels - 1), 0.0)
    return lam, rho2


def perspective_uv(clip, uv, px, py, width, height):
    """texture coordinates of one triangle (clip (3, 4) float64 clip-space positions, uv (3, 2)) extrapolated to the pixel centres
    (px + 0.5, py + 0.5) (arrays): the plane equations of u / w, v / w and 1 / w over the screen, exact for an unclipped triangle and
    the analytic continuation of it for a clipped one (interpolation is projective-linear)."""
    clip = np.asarray(clip, np.float64); uv = np.asarray(uv, np.float64)
    iw = 1.0 / clip[:, 3]
    sx = (clip[:, 0] * iw * 0.5 + 0.5) * width
    sy = (0.5 - clip[:, 1] * iw * 0.5) * height
    M = np.stack([sx, sy, np.ones(3)], 1)                 # rows: vertices
    planes = np.linalg.solve(M, np.stack([uv[:, 0] * iw, uv[:, 1] * iw, iw], 1))   # (3 coefficients, 3 quantities)
    P = np.stack([np.asarray(px, np.float64) + 0.5, np.asarray(py, np.float64) + 0.5, np.ones(np.shape(px))], -1)
    q = P @ planes
    return q[..., :2] / q[..., 2:3]
