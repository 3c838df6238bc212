"""The motion vectors and the accumulation's motion form (include/arctic_hip.h: arctic_motion_vectors_device,
arctic_accumulate_ambient_occlusion_motion_device and the definitions in front of them) restated in numpy, float32 throughout, one rounding per
operation in the written order: they reproduce the library's planes by bytes.  Also the per-vertex attributes (hit_reference's, which are the
vertex kernel's) for the check of bary3 / source4 against arctic_read_gbuffer, and, for the tests that must not be vacuous, each definition with
one deliberate defect."""
import numpy as np

import ao_history_reference as HR

F = np.float32
NO_OBJECT = 0xFFFFFFFF
NONE, POINT, VELOCITY = F(0.0), F(1.0), F(2.0)
MOTION_DEFECTS = ("current trs", "current positions", "B permuted", "velocity sign", "y not flipped")
ACCUMULATE_DEFECTS = ("plane test on w", "flag 0 accepted")


def mat_rows(T, p):
    """the vertex kernel's product, rows 0..2: T (n, 16) [col][row], p (n, 3) -> (n, 3)"""
    T, p = np.asarray(T, F).reshape(-1, 16), np.asarray(p, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((T[:, j] * p[:, 0] + T[:, 4 + j] * p[:, 1]) + T[:, 8 + j] * p[:, 2]) + T[:, 12 + j] * F(1.0) for j in range(3)], -1)


def prev_world(T, q, B):
    """step 4: T (n, 16), q (n, 3, 3) the three previous positions, B (n, 3) -> pw (n, 3)"""
    q, B = np.asarray(q, F).reshape(-1, 3, 3), np.asarray(B, F).reshape(-1, 3)
    X = [mat_rows(T, q[:, k]) for k in range(3)]
    with np.errstate(all="ignore"):
        return (B[:, 0:1] * X[0] + B[:, 1:2] * X[1]) + B[:, 2:3] * X[2]


def velocity(P, pw, W, H, xy, defect=None):
    """step 5: -> (velocity2 (n, 2), projectable (n,) bool)"""
    P = np.asarray(P, F).reshape(16)
    xy = np.asarray(xy).reshape(-1, 2)
    with np.errstate(all="ignore"):
        c = [((P[i] * pw[:, 0] + P[4 + i] * pw[:, 1]) + P[8 + i] * pw[:, 2]) + P[12 + i] for i in range(4)]
        ok = (c[3] > 0) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[3])
        iw = F(1.0) / c[3]
        nx, ny = c[0] * iw, c[1] * iw
        sx = (nx + F(1.0)) * (F(0.5) * F(W))
        sy = ((ny + F(1.0)) if defect == "y not flipped" else (F(1.0) - ny)) * (F(0.5) * F(H))
        cx, cy = xy[:, 0].astype(F) + F(0.5), xy[:, 1].astype(F) + F(0.5)
        v = np.stack([cx - sx, cy - sy] if defect == "velocity sign" else [sx - cx, sy - cy], -1)
    return np.where(ok[:, None], v, F(0.0)).astype(F), ok


def motion(B, has_prev, T, q, xy, P, W, H, defect=None):
    """steps 3 to 5 for n pixels WITH geometry.  has_prev (n,) bool; T (n, 16) the previous trs of every pixel's object; q (n, 3, 3) its three
    previous positions; xy (n, 2) the pixel; P the previous call's matrix or None (M is empty).  -> (prev_world4 (n, 4), velocity2 (n, 2))"""
    B = np.asarray(B, F).reshape(-1, 3)
    n = len(B)
    pw4, vel = np.zeros((n, 4), F), np.zeros((n, 2), F)
    has = np.asarray(has_prev, bool).reshape(-1) & (P is not None)
    if not has.any():
        return pw4, vel
    if defect == "B permuted":
        B = B[:, [1, 2, 0]]
    pw = prev_world(np.asarray(T, F).reshape(-1, 16)[has], np.asarray(q, F).reshape(-1, 3, 3)[has], B[has])
    v, ok = velocity(P, pw, W, H, np.asarray(xy).reshape(-1, 2)[has], defect)
    pw4[has, :3], pw4[has, 3] = pw, np.where(ok, VELOCITY, POINT)
    vel[has] = v
    return pw4, vel


def vertex_attributes(trs, lpv, v):
    """the 18 attributes the vertex kernel writes per vertex (hit_attributes.h: ha_vertex): trs, lpv (16,), v a VERTEX_DTYPE array -> (n, 18)"""
    trs, lpv = np.asarray(trs, F).reshape(16), np.asarray(lpv, F).reshape(16)
    pos = np.asarray(v["position"], F)
    with np.errstate(all="ignore"):
        world = np.stack([((trs[j] * pos[:, 0] + trs[4 + j] * pos[:, 1]) + trs[8 + j] * pos[:, 2]) + trs[12 + j] * F(1.0) for j in range(4)], -1)
        ls = np.stack([((lpv[j] * world[:, 0] + lpv[4 + j] * world[:, 1]) + lpv[8 + j] * world[:, 2]) + lpv[12 + j] * world[:, 3] for j in range(4)], -1)

        def unit(a):
            a = np.asarray(a, F)
            inv = F(1.0) / np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
            return a * inv[:, None]
        return np.concatenate([np.asarray(v["tex_coords"], F), unit(v["tangent"]), unit(v["bitangent"]), unit(v["normal"]), world[:, :3], ls], 1).astype(F)


def interpolate(B, a0, a1, a2):
    """interpolate_attr's order: B (n, 3), a_k (n, K) -> (n, K)"""
    B = np.asarray(B, F)
    with np.errstate(all="ignore"):
        return (B[:, 0:1] * a0 + B[:, 1:2] * a1) + B[:, 2:3] * a2


def accumulate(world, prev_world4, normal, geometry, cur, prev, W, H, hist=HR.HIST, defect=None):
    """the accumulation's motion form for n pixels: ao_history_reference.accumulate with step 3 reprojecting pw (rejecting everything unless the
    flag is at least 1) and step 4's plane test taken from pw.  -> dict(byte, value, count, world, normal)"""
    w, n = np.asarray(world, F).reshape(-1, 3), np.asarray(normal, F).reshape(-1, 3)
    pw4 = np.asarray(prev_world4, F).reshape(-1, 4)
    pw, flag = pw4[:, :3], pw4[:, 3]
    cur = np.asarray(cur, np.uint8).reshape(-1).astype(F)
    m, ok = HR.unit_normal(n)
    covered = ok & (np.asarray(geometry).reshape(-1) != 0)
    N, value = np.ones(len(w), F), cur.copy()
    if prev is not None:
        inside, _, ix, iy, ax, ay = HR.reproject(prev["P"], pw, W, H)
        with np.errstate(invalid="ignore"):
            known = (flag >= F(0.0)) if defect == "flag 0 accepted" else (flag >= POINT)
        use = np.nonzero(covered & inside & known)[0]
        x0, y0 = ix[use].astype(np.int32), iy[use].astype(np.int32)
        fx, fy = ax[use], ay[use]
        bx, by = F(1.0) - fx, F(1.0) - fy
        weight = [bx * by, fx * by, bx * fy, fx * fy]
        pv, pc = np.asarray(prev["value"], F).reshape(H, W), np.asarray(prev["count"], F).reshape(H, W)
        qw, qm = np.asarray(prev["world"], F).reshape(H, W, 3), np.asarray(prev["normal"], F).reshape(H, W, 3)
        at = w[use] if defect == "plane test on w" else pw[use]
        k, kv, kc = [], [], []
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inb = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            with np.errstate(all="ignore"):
                acc = inb & (pc[cy, cx] > 0) & HR.accepts(m[use], at, qm[cy, cx], qw[cy, cx], hist["normal_cos"], hist["plane_dist"])
                k.append(np.where(acc, weight[t], F(0.0)))
                kv.append(np.where(acc, weight[t] * pv[cy, cx], F(0.0)))
                kc.append(np.where(acc, weight[t] * pc[cy, cx], F(0.0)))
        S, V, C = ((k[0] + k[1]) + k[2]) + k[3], ((kv[0] + kv[1]) + kv[2]) + kv[3], ((kc[0] + kc[1]) + kc[2]) + kc[3]
        with np.errstate(all="ignore"):
            hv, hn = V / S, C / S
            Nn = np.minimum(hn + F(1.0), F(hist["max_history"]))
            blended = hv + (cur[use] - hv) * (F(1.0) / Nn)
        take = S > F(hist["min_weight"])
        N[use] = np.where(take, Nn, F(1.0))
        value[use] = np.where(take, blended, cur[use])
    out = dict(byte=np.where(covered, HR.to_byte(np.where(covered, value, F(0))), 255).astype(np.uint8))
    out["value"] = np.where(covered, value, F(0.0)).astype(F)
    out["count"] = np.where(covered, N, F(0.0)).astype(F)
    out["world"] = np.where(covered[:, None], w, F(0.0)).astype(F)
    out["normal"] = np.where(covered[:, None], m, F(0.0)).astype(F)
    return out


def accumulate_frame(attrs, material, prev_world4, cur, prev, P, hist=HR.HIST, defect=None):
    """one call on a whole frame, shaped like ao_history_reference.accumulate_frame; prev_world4 (H, W, 4); None: the plain definition"""
    if prev_world4 is None:
        return HR.accumulate_frame(attrs, material, cur, prev, P, hist)
    H, W = material.shape
    a = np.asarray(attrs, F).reshape(-1, 18)
    r = accumulate(a[:, 11:14], prev_world4, a[:, 8:11], np.asarray(material).reshape(-1) != HR.NO_MATERIAL, cur, prev, W, H, hist, defect)
    state = dict(P=np.asarray(P, F).reshape(4, 4).copy(), value=r["value"].reshape(H, W), count=r["count"].reshape(H, W), world=r["world"].reshape(H, W, 3),
                 normal=r["normal"].reshape(H, W, 3))
    return r["byte"].reshape(H, W), state


def run_sequence(frames, motions, planes, hist=HR.HIST, defect=None, mixed=()):
    """frames: [(attrs, material, P)], motions: [prev_world4 (H, W, 4)], planes: [cur] -> [(byte, state)] of every call, from an empty history;
    the calls whose index is in `mixed` take the plain definition"""
    out, prev = [], None
    for k, ((attrs, material, P), pw4, cur) in enumerate(zip(frames, motions, planes)):
        step = accumulate_frame(attrs, material, None if k in mixed else pw4, cur, prev, P, hist, defect)
        byte, prev = step[0], step[1]
        out.append((byte, prev))
    return out
