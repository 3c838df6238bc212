"""The temporal accumulation of the occlusion plane (include/arctic_hip.h: arctic_accumulate_ambient_occlusion_device and the definition in front of
it) restated in numpy, float32 throughout, one rounding per operation in the written order: it reproduces the library's output bytes AND its
history planes by bytes.  Also the class of every pixel (which rule of the definition decided it) and, for the tests that must not be vacuous, the
definition with one deliberate defect."""
import numpy as np

F = np.float32
NO_MATERIAL = 0xFFFFFFFF
# the parameters of the sequences: a cap that five calls reach, and a weight floor that drops the history of some pixels with accepted taps
HIST = dict(max_history=4.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.1)
# the class of a pixel: which rule of the definition gave its value
NO_GEOMETRY, NOT_COVERED, EMPTY, BEHIND, OUTSIDE, NONE_ACCEPTED, SOME_REJECTED, ALL_ACCEPTED = range(8)
CLASS_NAMES = ["no geometry", "not covered", "empty history", "c3 <= 0", "reprojected outside the frame", "none accepted", "some taps rejected", "all four taps accepted"]
DEFECTS = ("nearest tap", "no renormalisation", "current matrix", "count not capped", "y not flipped", "current normals", "no plane test", "rejected tap multiplied")


def unit_normal(n):
    """step 1 of the ambient occlusion: m = n / len and whether the pixel is covered by it"""
    n = np.asarray(n, F)
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        m = n / ln[..., None]
    return m, (ln != 0) & np.isfinite(ln) & np.isfinite(m).all(-1)


def accepts(mp, wp, mq, wq, normal_cos, plane_dist):
    """the occlusion filter's test (ray_ao.h: ao_accepts)"""
    with np.errstate(all="ignore"):
        d = wq - wp
        dot = (mp[..., 0] * mq[..., 0] + mp[..., 1] * mq[..., 1]) + mp[..., 2] * mq[..., 2]
        dist = np.abs((mp[..., 0] * d[..., 0] + mp[..., 1] * d[..., 1]) + mp[..., 2] * d[..., 2])
        return (dot >= F(normal_cos)) & (dist <= F(plane_dist))


def reproject(P, w, W, H, flip=True):
    """step 3: -> (inside, behind, ix, iy, ax, ay); P: (4, 4) [col][row]; w: (n, 3)"""
    P = np.asarray(P, F).reshape(16)
    with np.errstate(all="ignore"):
        c = [((P[i] * w[:, 0] + P[4 + i] * w[:, 1]) + P[8 + i] * w[:, 2]) + P[12 + i] for i in range(4)]
        front = (c[3] > 0) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[3])
        iw = F(1.0) / c[3]
        nx, ny = c[0] * iw, c[1] * iw
        sx = (nx + F(1.0)) * (F(0.5) * F(W))
        sy = ((F(1.0) - ny) if flip else (ny + F(1.0))) * (F(0.5) * F(H))
        gx, gy = sx - F(0.5), sy - F(0.5)
        ix, iy = np.floor(gx), np.floor(gy)
        ax, ay = gx - ix, gy - iy
        inside = front & (ix >= F(-1.0)) & (ix <= F(W) - F(1.0)) & (iy >= F(-1.0)) & (iy <= F(H) - F(1.0))
    return inside, ~front, ix, iy, ax, ay


def to_byte(value):
    with np.errstate(invalid="ignore"):                                          # (a NaN comes only out of a deliberate defect)
        return np.minimum(np.maximum(np.floor(value + F(0.5)), F(0.0)), F(255.0)).astype(np.uint8)


def accumulate(world, normal, geometry, cur, prev, W, H, hist=HIST, defect=None, current=None):
    """the definition for n pixels.  world, normal (n, 3); geometry (n,) bool; cur (n,) uint8; prev: None (H is empty) or a dict with P (4, 4) and
    the row-major planes value, count (H, W) and world, normal (H, W, 3) of the previous call.  current: (world (H, W, 3), m (H, W, 3)) of THIS
    frame, for the defect that tests acceptance against it.  -> dict(byte, value, count, world, normal, cls)"""
    w, n = np.asarray(world, F).reshape(-1, 3), np.asarray(normal, F).reshape(-1, 3)
    cur = np.asarray(cur, np.uint8).reshape(-1).astype(F)
    m, ok = unit_normal(n)
    geometry = np.asarray(geometry).reshape(-1) != 0
    covered = ok & geometry
    N, value = np.ones(len(w), F), cur.copy()
    cls = np.where(~geometry, NO_GEOMETRY, np.where(~covered, NOT_COVERED, EMPTY)).astype(np.int32)
    if prev is not None:
        inside, behind, ix, iy, ax, ay = reproject(prev["P"], w, W, H, flip=defect != "y not flipped")
        cls[covered & behind] = BEHIND
        cls[covered & ~behind & ~inside] = OUTSIDE
        use = np.nonzero(covered & inside)[0]
        x0, y0 = ix[use].astype(np.int32), iy[use].astype(np.int32)
        fx, fy = ax[use], ay[use]
        bx, by = F(1.0) - fx, F(1.0) - fy
        weight = [bx * by, fx * by, bx * fy, fx * fy]
        if defect == "nearest tap":
            near = (fx >= F(0.5)).astype(np.int32) + 2 * (fy >= F(0.5)).astype(np.int32)
            weight = [np.where(near == t, F(1.0), F(0.0)).astype(F) for t in range(4)]
        pv, pc = np.asarray(prev["value"], F).reshape(H, W), np.asarray(prev["count"], F).reshape(H, W)
        pw, pm = np.asarray(prev["world"], F).reshape(H, W, 3), np.asarray(prev["normal"], F).reshape(H, W, 3)
        tw, tm = (pw, pm) if defect != "current normals" else (np.asarray(current[0], F).reshape(H, W, 3), np.asarray(current[1], F).reshape(H, W, 3))
        k, kv, kc, n_acc = [], [], [], np.zeros(len(use), np.int32)
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inb = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            with np.errstate(all="ignore"):
                acc = inb & (pc[cy, cx] > 0) & accepts(m[use], w[use], tm[cy, cx], tw[cy, cx], hist["normal_cos"], np.inf if defect == "no plane test" else hist["plane_dist"])
                if defect == "rejected tap multiplied":          # a product by zero instead of a select: a NaN in a rejected tap comes through
                    z = np.where(acc, weight[t], F(0.0))
                    k.append(z); kv.append(z * pv[cy, cx]); kc.append(z * pc[cy, cx])
                else:
                    k.append(np.where(acc, weight[t], F(0.0)))
                    kv.append(np.where(acc, weight[t] * pv[cy, cx], F(0.0)))
                    kc.append(np.where(acc, weight[t] * pc[cy, cx], F(0.0)))
            n_acc += acc
        S, V, C = ((k[0] + k[1]) + k[2]) + k[3], ((kv[0] + kv[1]) + kv[2]) + kv[3], ((kc[0] + kc[1]) + kc[2]) + kc[3]
        with np.errstate(all="ignore"):
            if defect == "no renormalisation":
                hv, hn = V, C
            else:
                hv, hn = V / S, C / S
            Nn = hn + F(1.0) if defect == "count not capped" else np.minimum(hn + F(1.0), F(hist["max_history"]))
            a = F(1.0) / Nn
            blended = hv + (cur[use] - hv) * a
        take = S > F(hist["min_weight"])
        N[use] = np.where(take, Nn, F(1.0))
        value[use] = np.where(take, blended, cur[use])
        cls[use] = np.where(n_acc == 4, ALL_ACCEPTED, np.where(n_acc > 0, SOME_REJECTED, NONE_ACCEPTED))
    out = dict(byte=np.where(covered, to_byte(np.where(covered, value, F(0))), 255).astype(np.uint8), cls=cls)
    out["value"] = np.where(covered, value, F(0.0)).astype(F)
    out["count"] = np.where(covered, N, F(0.0)).astype(F)
    out["world"] = np.where(covered[:, None], w, F(0.0)).astype(F)
    out["normal"] = np.where(covered[:, None], m, F(0.0)).astype(F)
    return out


def accumulate_frame(attrs, material, cur, prev, P, hist=HIST, defect=None):
    """one call on a whole frame: attrs (H, W, 18) and material (H, W) as arctic_read_gbuffer gives them, cur (H, W) uint8, prev: the state the
    previous call returned or None, P: THIS call's proj_view.  -> (byte (H, W), state for the next call, cls (H, W))"""
    H, W = material.shape
    a = np.asarray(attrs, F).reshape(-1, 18)
    if defect == "current matrix" and prev is not None:
        prev = dict(prev, P=P)
    current = None
    if defect == "current normals":
        m, _ = unit_normal(a[:, 8:11])
        current = (a[:, 11:14].reshape(H, W, 3), m.reshape(H, W, 3))
    r = accumulate(a[:, 11:14], a[:, 8:11], np.asarray(material).reshape(-1) != NO_MATERIAL, cur, prev, W, H, hist, defect, current)
    state = dict(P=np.asarray(P, F).reshape(4, 4).copy(), value=r["value"].reshape(H, W), count=r["count"].reshape(H, W), world=r["world"].reshape(H, W, 3),
                 normal=r["normal"].reshape(H, W, 3))
    return r["byte"].reshape(H, W), state, r["cls"].reshape(H, W)


def run_sequence(frames, planes, hist=HIST, defect=None):
    """frames: [(attrs, material, P)], planes: [cur] -> [(byte, state, cls)] of every call, from an empty history"""
    out, prev = [], None
    for (attrs, material, P), cur in zip(frames, planes):
        byte, prev, cls = accumulate_frame(attrs, material, cur, prev, P, hist, defect)
        out.append((byte, prev, cls))
    return out
