"""An independent float64 numpy implementation of the image-based ambient of ARCTIC_OPT_ENV_LIGHTING (semantics: include/arctic_hip.h
next to the option).  It never calls the library: the GPU tests compare the library's tables and pixels against it."""
import numpy as np

C_U, C_V = float(np.float32(0.1591)), float(np.float32(0.3183))   # the skybox's fp32 constants
LEVELS, LUT_N, SAMPLES, LUT_SAMPLES = 6, 64, 512, 1024
A_HAT = np.array([np.pi] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5)


def texel_dirs(w, h):
    """(h, w, 3) directions of the texel centres and (h, w) cos(theta)"""
    u = (np.arange(w) + 0.5) / w
    v = (np.arange(h) + 0.5) / h
    phi = (u[None, :] - 0.5) / C_U
    theta = (0.5 - v[:, None]) / C_V
    ct = np.cos(theta) * np.ones_like(phi)
    d = np.stack([ct * np.cos(phi), np.sin(theta) * np.ones_like(phi), ct * np.sin(phi)], -1)
    return d, ct


def sh_basis(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c0, c1, c2, c3, c4 = 0.5 / np.sqrt(np.pi), np.sqrt(3 / (4 * np.pi)), np.sqrt(15 / (4 * np.pi)), np.sqrt(5 / (16 * np.pi)), np.sqrt(15 / (16 * np.pi))
    return np.stack([c0 * np.ones_like(x), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3 * z * z - 1), c2 * x * z, c4 * (x * x - y * y)], -1)


def sh_project(env):
    """(9, 3): the map's irradiance coefficients, A_l folded in (the library's sh27 reshaped)"""
    h, w = env.shape[:2]
    d, ct = texel_dirs(w, h)
    wgt = np.maximum(ct, 0) / (C_U * w) / (C_V * h)
    Y = sh_basis(d)
    L = env[..., :3].astype(np.float64)
    return np.einsum("hwk,hwc,hw->kc", Y, L, wgt) * A_HAT[:, None]


def sh_irradiance(sh, n):
    return np.einsum("...k,kc->...c", sh_basis(n), np.asarray(sh, np.float64))


def mip_chain(env):
    """the 2x2 box-filtered chain, in fp32 with the library's operation order"""
    out = [np.ascontiguousarray(env, np.float32)]
    while out[-1].shape[0] > 1 or out[-1].shape[1] > 1:
        s = out[-1]
        sh, sw = s.shape[:2]
        dh, dw = max(1, sh >> 1), max(1, sw >> 1)
        ys0, ys1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
        xs0, xs1 = np.minimum(2 * np.arange(dw), sw - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
        a, b = s[ys0][:, xs0], s[ys0][:, xs1]
        c, d = s[ys1][:, xs0], s[ys1][:, xs1]
        out.append(((a + b) + (c + d)) * np.float32(0.25))
    return out


def _wrap(u, n):
    x = (u - np.floor(u)) * n - 0.5
    xf = np.floor(x)
    i0 = xf.astype(np.int64)
    i1 = i0 + 1
    i0 = np.where(i0 < 0, i0 + n, i0)
    i1 = np.where(i1 >= n, i1 - n, i1)
    return i0, i1, x - xf


def dir_uv(d):
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    u = np.arctan2(d[..., 2], d[..., 0]) * C_U + 0.5
    v = -(np.arcsin(np.clip(d[..., 1], -1, 1)) * C_V + 0.5)
    return u, v


def sample_uv(img, u, v):
    """bilinear, WRAP: (..., 3) float64"""
    h, w = img.shape[:2]
    x0, x1, fx = _wrap(u, w)
    y0, y1, fy = _wrap(v, h)
    im = img[..., :3].astype(np.float64)
    fx, fy = fx[..., None], fy[..., None]
    return (im[y0, x0] * (1 - fx) * (1 - fy) + im[y0, x1] * fx * (1 - fy) + im[y1, x0] * (1 - fx) * fy + im[y1, x1] * fx * fy)


def hammersley(n):
    i = np.arange(n, dtype=np.uint64)
    r = np.zeros(n, np.uint64)
    for b in range(32):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return i / n, r.astype(np.float64) / 4294967296.0


def ggx_half(x1, x2, alpha, n):
    """half vectors (..., S, 3) around unit normals n (..., 3) for Hammersley points x1, x2 (S,)"""
    a2 = alpha * alpha
    phi = 2 * np.pi * x1
    ch = np.sqrt((1 - x2) / (1 + (a2 - 1) * x2))
    sh = np.sqrt(np.maximum(0, 1 - ch * ch))
    up = np.where((np.abs(n[..., 2]) < 0.999)[..., None], np.array([0.0, 0, 1]), np.array([1.0, 0, 0]))
    tx = np.cross(up, n)
    tx /= np.linalg.norm(tx, axis=-1, keepdims=True)
    ty = np.cross(n, tx)
    hx, hy = sh * np.cos(phi), sh * np.sin(phi)
    H = tx[..., None, :] * hx[:, None] + ty[..., None, :] * hy[:, None] + n[..., None, :] * ch[:, None]
    return H, ch


def level_size(W, H, k):
    return max(8, min(W, 512) >> (k - 1)), max(4, min(H, 256) >> (k - 1))


def prefilter_level(env, k, texels=None):
    """(h, w, 3) float64: specular level k >= 1 of the map; texels = a list of (row, column) pairs of the level: only those texels,
    (len(texels), 3), the same numbers the whole level holds there"""
    H_, W_ = env.shape[:2]
    w, h = level_size(W_, H_, k)
    mips = mip_chain(env)
    r = k / (LEVELS - 1)
    alpha = r * r
    a2 = alpha * alpha
    n, _ = texel_dirs(w, h)
    if texels is not None:
        rc = np.asarray(texels, np.int64).reshape(-1, 2)
        n = n[rc[:, 0], rc[:, 1]]
    n = n.reshape(-1, 3)
    x1, x2 = hammersley(SAMPLES)
    out = np.zeros((n.shape[0], 3))
    omega_p = 4 * np.pi / (W_ * H_)
    for s0 in range(0, n.shape[0], 256):
        nn = n[s0:s0 + 256]
        Hv, nh = ggx_half(x1, x2, alpha, nn)
        vh = np.einsum("pc,psc->ps", nn, Hv)
        L = 2 * vh[..., None] * Hv - nn[:, None, :]
        nl = np.einsum("pc,psc->ps", nn, L)
        q = nh * nh * (a2 - 1) + 1
        D = a2 / (np.pi * q * q)
        lod = np.maximum(0, 0.5 * np.log2(4 / (SAMPLES * D) / omega_p) + 1)
        lod = np.broadcast_to(lod, nl.shape)
        u, v = dir_uv(L)
        top = len(mips) - 1
        c = np.zeros(L.shape)
        for m in range(len(mips)):
            wgt = np.where(lod >= top, 1.0 * (m == top), np.where(np.floor(lod) == m, 1 - (lod - np.floor(lod)), np.where(np.floor(lod) + 1 == m, lod - np.floor(lod), 0.0)))
            if not np.any(wgt > 0):
                continue
            c += sample_uv(mips[m], u, v) * wgt[..., None]
        keep = (nl > 0).astype(np.float64) * nl
        out[s0:s0 + 256] = np.einsum("psc,ps->pc", c, keep) / keep.sum(1)[:, None]
    return out if texels is not None else out.reshape(h, w, 3)


def brdf_lut():
    """(64, 64, 2): row = roughness cell, column = n.v cell"""
    nv = (np.arange(LUT_N) + 0.5) / LUT_N
    x1, x2 = hammersley(LUT_SAMPLES)
    out = np.zeros((LUT_N, LUT_N, 2))
    n = np.array([[0.0, 0, 1]])
    V = np.stack([np.sqrt(1 - nv * nv), np.zeros_like(nv), nv], -1)   # (64, 3)
    for j in range(LUT_N):
        r = (j + 0.5) / LUT_N
        alpha, k = r * r, r * r / 2
        Hv, _ = ggx_half(x1, x2, alpha, n)
        Hv = Hv[0]                                                    # (S, 3)
        vh_raw = V @ Hv.T                                             # (64, S)
        L = 2 * vh_raw[..., None] * Hv[None] - V[:, None, :]
        nl = np.clip(L[..., 2], 0, 1)
        nh = np.clip(Hv[:, 2], 0, 1)[None]
        vh = np.clip(vh_raw, 0, 1)
        g = (nv[:, None] / (nv[:, None] * (1 - k) + k)) * (nl / (nl * (1 - k) + k))
        gv = np.where(nl > 0, g * vh / (nh * nv[:, None]), 0.0)
        fc = (1 - vh) ** 5
        out[j, :, 0] = ((1 - fc) * gv).sum(1) / LUT_SAMPLES
        out[j, :, 1] = (fc * gv).sum(1) / LUT_SAMPLES
    return out


def lut_lookup(lut, nv, rough):
    n = lut.shape[0]
    lx = np.clip(nv * n - 0.5, 0, n - 1)
    ly = np.clip(rough * n - 0.5, 0, n - 1)
    i0, j0 = np.floor(lx).astype(int), np.floor(ly).astype(int)
    i1, j1 = np.minimum(i0 + 1, n - 1), np.minimum(j0 + 1, n - 1)
    ax, ay = (lx - i0)[..., None], (ly - j0)[..., None]
    t = lut.astype(np.float64)
    return t[j0, i0] * (1 - ax) * (1 - ay) + t[j0, i1] * ax * (1 - ay) + t[j1, i0] * (1 - ax) * ay + t[j1, i1] * ax * ay


def ibl(n, wo, base, metal, rough, sh, lut, levels):
    """the bracket of mode 1: (1 - F)(1 - metal) base E(n) / pi + P(R, rough)(F0 A + B), from the given tables (..., 3)"""
    n, wo, base = (np.asarray(a, np.float64) for a in (n, wo, base))
    metal, rough = np.asarray(metal, np.float64)[..., None], np.asarray(rough, np.float64)
    ndwo_raw = np.sum(n * wo, -1)
    ndwo = np.maximum(ndwo_raw, 0)
    F0 = 0.04 + (base - 0.04) * metal
    p5 = ((1 - ndwo) ** 5)[..., None]
    F = F0 + (np.maximum(1 - rough[..., None], F0) - F0) * p5
    E = sh_irradiance(sh, n)
    AB = lut_lookup(lut, ndwo, rough)
    R = 2 * ndwo_raw[..., None] * n - wo
    u, v = dir_uv(R)
    t = rough * (LEVELS - 1)
    k0 = np.minimum(np.floor(t).astype(int), LEVELS - 1)
    k1 = np.minimum(k0 + 1, LEVELS - 1)
    f = (t - k0)[..., None]
    P0, P1 = np.zeros(R.shape), np.zeros(R.shape)
    for k in range(LEVELS):
        s = sample_uv(levels[k], u, v)
        P0 = np.where((k0 == k)[..., None], s, P0)
        P1 = np.where((k1 == k)[..., None], s, P1)
    P = P0 + (P1 - P0) * f
    return (1 - F) * (1 - metal) * base * E / np.pi + P * (F0 * AB[..., :1] + AB[..., 1:])


def tonemap(method, c, gamma=2.2, exposure=1.0):
    """post_process.hlsl in float64 over (..., 3): the LDR value before quantisation"""
    c = np.asarray(c, np.float64)
    if method == 1:
        t = 1 - np.exp(-c * exposure)
    elif method == 2:
        mi = np.array([[0.59719, 0.35458, 0.04823], [0.07600, 0.90834, 0.01566], [0.02840, 0.13383, 0.837]])
        mo = np.array([[1.60475, -0.53108, -0.07367], [-0.10208, 1.10813, -0.00605], [-0.00327, -0.07276, 1.07]])
        v = c @ mi.T
        v = (v * (v + 0.0245786) - 0.000090537) / (v * (0.983729 * v + 0.4329510) + 0.238081)
        t = np.clip(v @ mo.T, 0, 1)
    else:
        t = c / (c + 1)
    return np.abs(t) ** (1 / gamma)


def srgb_to_linear(b):
    c = np.asarray(b, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
