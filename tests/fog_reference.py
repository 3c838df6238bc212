"""Volumetric fog (include/arctic_hip.h: arctic_fog_device and the definition in front of it) in numpy: every operation of the definition in
fp32 in the written order, so that the kernel and the host arbiter can be held to it BY BYTES; and the float64 models the physics tests judge
against.  No GPU, no library."""
import numpy as np

F = np.float32
SOURCE_COMPOSED = 1
COEFFS = tuple(F(float.fromhex(h)) for h in ("0x1p+0", "0x1.62e428p-1", "0x1.ebfdf2p-3", "0x1.c67f5p-5", "0x1.3d54d8p-7", "0x1.44d4d2p-10", "0x1.ca8f0ap-13"))
LOG2E, INV_4PI = F(1.442695), F(0.07957747)
VIEW_DTYPE = np.dtype([("eye", "<f4", 3), ("z_near", "<f4"), ("ray00", "<f4", 3), ("z_far", "<f4"), ("ray_dx", "<f4", 3), ("pad0", "<f4"), ("ray_dy", "<f4", 3), ("pad1", "<f4"),
                       ("sun_dir", "<f4", 3), ("pad2", "<f4"), ("light", "<f4", (3, 4))])
DEFAULTS = dict(flags=0, density=0.05, anisotropy=0.5, max_distance=100.0, steps=32, bias=0.002, scatter_color=(1.0, 1.0, 1.0), ambient_color=(0.0, 0.0, 0.0))


def exp2_poly(f):
    """step 2's polynomial: Horner from the top, a multiply and an add per coefficient, each rounded to fp32"""
    f = np.asarray(f, F)
    p = np.full(f.shape, COEFFS[6], F)
    for c in COEFFS[5::-1]:
        p = p * f
        p = p + c
    return p


def exp2(x):
    """step 2's fog_exp2 for x <= 0"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        x = np.where(x > F(-126.0), x, F(-126.0)).astype(F)                       # (a NaN fails the test)
        n = np.floor(x)
        p = exp2_poly(x - n)
        bits = (p.view(np.uint32).astype(np.int64) + n.astype(np.int64) * (1 << 23)) & 0xFFFFFFFF
        r = bits.astype(np.uint32).view(F)
        return np.where(F(1.0) < r, F(1.0), r).astype(F)


def view_distance(depth, z_near, z_far):
    """the depth of field's view distance of a prepass depth"""
    zn, zf = F(z_near), F(z_far)
    with np.errstate(all="ignore"):
        den = zf - depth * (zf - zn)
        return np.where(den > 0, (zn * zf) / den, zf).astype(F)


def view_record(eye=(0.0, 1.0, 0.0), z_near=0.5, z_far=50.0, ray00=(-0.5, 0.4, 1.0), ray_dx=(0.02, 0.0, 0.0), ray_dy=(0.0, -0.02, 0.0), sun_dir=(0.0, -1.0, 0.0),
                light=((0.05, 0.0, 0.0, 0.5), (0.0, 0.0, 0.05, 0.25), (0.0, -0.05, 0.0, 0.5))):
    v = np.zeros(1, VIEW_DTYPE)
    v["eye"][0], v["z_near"], v["ray00"][0], v["z_far"], v["ray_dx"][0], v["ray_dy"][0], v["sun_dir"][0], v["light"][0] = eye, z_near, ray00, z_far, ray_dx, ray_dy, sun_dir, light
    return v


# Views whose samples leave the map by ONE clause of the inside test while the others hold: a coordinate that grows with the world z of the
# sample (0 at the eye, up to max_distance) and crosses its bound near z = 14, the other two constant or well inside
EDGE_VIEWS = {
    "left": dict(light=((0.0, 0.0, -0.05, 0.7), (0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 0.5))),
    "right": dict(light=((0.0, 0.0, 0.05, 0.3), (0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 0.5))),
    "top": dict(light=((0.0, 0.0, 0.0, 0.5), (0.0, 0.0, -0.05, 0.7), (0.0, 0.0, 0.0, 0.5))),
    "bottom": dict(light=((0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.05, 0.3), (0.0, 0.0, 0.0, 0.5))),
    "deep": dict(light=((0.01, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.05, 0.3))),
}


def row(r, P):
    return ((r[0] * P[0] + r[1] * P[1]) + r[2] * P[2]) + r[3]


def fog(C, depth, shadow, view, offsets=None, flags=0, density=0.05, anisotropy=0.5, max_distance=100.0, steps=32, bias=0.002, scatter_color=(1.0, 1.0, 1.0),
        ambient_color=(0.0, 0.0, 0.0)):
    """the whole frame: C (H, W, 3) float32, depth (H, W) or None, shadow (S, S) or None, view one VIEW_DTYPE record, offsets 16 floats or None.
    Returns (out (H, W, 3), T (H, W), I (H, W)) float32, the number of lookups that read the map, and how many samples left the map by each
    clause of the inside test ALONE, the others holding: {"left", "right", "top", "bottom", "deep"}"""
    C = np.asarray(C, F)
    H, W = C.shape[:2]
    v = view[0]
    S = 0 if shadow is None else int(shadow.shape[0])
    table = np.full(16, 0.5, F) if offsets is None else np.asarray(offsets, F).ravel()
    py, px = np.mgrid[0:H, 0:W]
    offset = table[(py & 3) * 4 + (px & 3)]
    fx, fy = px.astype(F) + F(0.5), py.astype(F) + F(0.5)
    with np.errstate(all="ignore"):
        D = [(v["ray00"][a] + fx * v["ray_dx"][a]) + fy * v["ray_dy"][a] for a in range(3)]
        ln = np.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
        z = np.full((H, W), 1.0, F) if depth is None else np.asarray(depth, F)
        zv = view_distance(z, v["z_near"], v["z_far"])
        md = F(max_distance)
        z_end = np.where(md < zv, md, zv).astype(F)
        dz = z_end / F(steps)
        x = -((F(density) * LOG2E) * ln) * dz
        a = exp2(x)
        T, I = np.ones((H, W), F), np.zeros((H, W), F)
        reads = 0
        left = {"left": 0, "right": 0, "top": 0, "bottom": 0, "deep": 0}
        for k in range(int(steps)):
            zk = (F(k) + offset) * dz
            lit = np.ones((H, W), bool)
            if S:
                P = [v["eye"][c] + D[c] * zk for c in range(3)]
                u, t, w = row(v["light"][0], P), row(v["light"][1], P), row(v["light"][2], P)
                tu, tv = np.floor(u * F(S)), np.floor(t * F(S))
                last = F(S - 1)
                inside = (tu >= 0) & (tu <= last) & (tv >= 0) & (tv <= last) & ~(w > F(1.0))
                iu, iv = np.where(inside, tu, 0).astype(np.int64), np.where(inside, tv, 0).astype(np.int64)
                lit = ~(inside & ((w - F(bias)) > shadow[iv, iu]))
                reads += int(inside.sum())
                u_in, v_in, shallow = (tu >= 0) & (tu <= last), (tv >= 0) & (tv <= last), ~(w > F(1.0))
                for name, cond in (("left", (tu < 0) & v_in & shallow), ("right", (tu > last) & v_in & shallow), ("top", (tv < 0) & u_in & shallow),
                                   ("bottom", (tv > last) & u_in & shallow), ("deep", u_in & v_in & (w > F(1.0)))):
                    left[name] += int(cond.sum())
            Tn = T * a
            term = T - Tn
            I = np.where(lit, I + term, I).astype(F)
            T = Tn
        g = F(anisotropy)
        cos_t = -((D[0] * v["sun_dir"][0] + D[1] * v["sun_dir"][1]) + D[2] * v["sun_dir"][2]) / ln
        q = (F(1.0) + g * g) - (F(2.0) * g) * cos_t
        ph = ((F(1.0) - g * g) * INV_4PI) / (q * np.sqrt(q))
        rest = F(1.0) - T
        sc, am = np.asarray(scatter_color, F), np.asarray(ambient_color, F)
        fogged = np.stack([(C[..., c] * T + (sc[c] * ph) * I) + am[c] * rest for c in range(3)], -1).astype(F)
        out = np.where((T < F(1.0))[..., None], fogged, C).astype(F)
    return out, T, I, reads, left


def same(got, want, what):
    """equal by bytes, NaN included"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
