"""The arbiter of the indirect diffuse light: include/arctic_hip.h's definition (in front of arctic_trace_gi) restated in numpy float32, operation
for operation, from the header's text -- not from the library's C++.  Steps 1 to 3 of a ray, the set of a pixel, the window and the acceptance
test are the ambient occlusion's, so they are ao_reference's; every array below is float32 and every operation one numpy ufunc on float32
operands, so each rounds once, in the written order.

  point_rays()    stage 1 for points {world3, normal3} with a set each: what arctic_gi_points returns
  image_rays()    the same for a G-buffer (arctic_read_gbuffer's attributes and materials) whose rows are rows `frame_rows` of the frame
  sanitise()      stage 3's selects
  add()           stage 3: S from the rounds' records and colours
  estimate()      stage 4, unfiltered and filtered
  accumulate()    stage 5 for n pixels against a previous history (the reprojection and the acceptance are ao_history_reference's); accumulate_frame()
  compose()       stage 6's two terms, in float32 (the definition's roundings) or float64 (the device test's reference)

`defect` names a deliberate deviation, so that the tests can show they tell the definition from it:
  "p_first"       the filter adds p's own sum first, not at its place in the window       "product"   a rejected pixel's S is multiplied by 0
  "minmax"        the channels are sanitised by min / max, which let a NaN through        "count_all" a pixel without a ray counts a ray as well
"""
import numpy as np

import ao_reference as A
import ray_reference as R

F = np.float32
NO_MATERIAL = 0xFFFFFFFF


def point_rays(points, sets, dirs, n_rays, round, max_distance, bias, geometry=None):
    """-> (rays (N,) RAY_DTYPE, had (N,)): round `round`'s record of every point, the all-zero record where it has no ray"""
    points = np.asarray(points, F).reshape(-1, 6)
    dirs = np.asarray(dirs, F).reshape(-1, n_rays, 3)
    m, ok = A.normal(points[:, 3:6])
    if geometry is not None:
        ok = ok & np.asarray(geometry, bool)
    local = dirs[np.asarray(sets, np.int64), round][:, None, :]
    ry = A.rays(points[:, 0:3], m, local, max_distance, bias)[:, 0]
    out = np.zeros(len(points), R.RAY_DTYPE)
    out[ok] = ry[ok]
    return out, ok


def image_rays(attrs, material, dirs, n_rays, P, round, max_distance, bias, frame_rows=None):
    """-> (rays (rows, width) RAY_DTYPE, had (rows, width))"""
    points, sets, geometry = A.image_points(attrs, material, P, frame_rows)
    ry, had = point_rays(points, sets, dirs, n_rays, round, max_distance, bias, geometry)
    return ry.reshape(material.shape), had.reshape(material.shape)


def sanitise(l, clamp_max, defect=None):
    l, c = np.asarray(l, F), F(clamp_max)
    with np.errstate(all="ignore"):
        if defect == "minmax":
            return np.minimum(np.maximum(l, F(0)), c)
        return np.where(l > c, c, np.where(l > F(0), l, F(0))).astype(F)


def add(rays, colors, clamp_max, defect=None):
    """rays (n_rays, ...) RAY_DTYPE, colors (n_rays, ..., 4) float32 -> S (..., 4) float32"""
    colors = np.asarray(colors, F)
    S = np.zeros(colors.shape[1:], F)
    for k in range(len(rays)):
        had = rays[k]["t_max"] > F(0)
        L = sanitise(colors[k][..., 0:3], clamp_max, defect)
        with np.errstate(all="ignore"):
            plus = np.concatenate([S[..., 0:3] + L, (S[..., 3] + F(1))[..., None]], -1)
        S = np.where(had[..., None], plus, np.where((defect == "count_all"), S + np.array([0, 0, 0, 1], F), S)).astype(F)
    assert S.dtype == F
    return S


def mean(S):
    with np.errstate(all="ignore"):
        E = np.concatenate([S[..., 0:3] / S[..., 3:4], S[..., 3:4]], -1)
    return np.where(S[..., 3:4] > F(0), E, F(0)).astype(F)


def estimate(S, attrs=None, material=None, P=1, filter=False, normal_cos=0.9, plane_dist=0.05, defect=None):
    """stage 4 for a WHOLE frame: S (rows, width, 4) -> E (rows, width, 4); the filter reads the G-buffer's normals, positions and materials"""
    S = np.asarray(S, F)
    if not filter:
        return mean(S)
    rows, width = S.shape[:2]
    m, ok = A.normal(attrs[..., 8:11].reshape(-1, 3))
    m, w = m.reshape(rows, width, 3), attrs[..., 11:14].astype(F)
    covered = ok.reshape(rows, width) & (material != NO_MATERIAL)
    acc = np.zeros((rows, width, 4), F)
    if defect == "p_first":
        acc = S.copy()
    y, x = np.meshgrid(np.arange(rows), np.arange(width), indexing="ij")
    for j in A.window(P):
        for i in A.window(P):
            qy, qx = y + j, x + i
            inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
            qy, qx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, width - 1)
            mq, wq = m[qy, qx], w[qy, qx]
            with np.errstate(all="ignore"):
                diff = [wq[..., a] - w[..., a] for a in range(3)]
                near = R._dot([m[..., a] for a in range(3)], [mq[..., a] for a in range(3)]) >= F(normal_cos)
                flat = np.abs(R._dot([m[..., a] for a in range(3)], diff)) <= F(plane_dist)
            ok = inside & covered[qy, qx] & near & flat
            if i == 0 and j == 0:
                ok = np.ones((rows, width), bool)
                if defect == "p_first":
                    continue
            with np.errstate(all="ignore"):
                if defect == "product":
                    acc = (acc + S[qy, qx] * ok[..., None].astype(F)).astype(F)
                else:
                    acc = np.where(ok[..., None], acc + S[qy, qx], acc).astype(F)
    return np.where(covered[..., None], mean(acc), F(0)).astype(F)


# ---- stage 5: the temporal accumulation (the occlusion history's steps with a colour for a value) --------------------------------------------------
def accumulate(world, normal, geometry, cur, prev, W, H, hist, defect=None):
    """the definition for n pixels.  world, normal (n, 3); geometry (n,); cur (n, 4) = E; prev: None (the history is empty) or a dict with P (4, 4)
    and the row-major planes acc (H, W, 3), count (H, W), world, normal (H, W, 3) of the previous call.  -> dict(out (n, 4), acc, count, world,
    normal, accepted (n,): taps accepted, -1 where the pixel did not reproject).  defect "rejected tap multiplied": a product by zero for a select"""
    import ao_history_reference as HR
    w, n = np.asarray(world, F).reshape(-1, 3), np.asarray(normal, F).reshape(-1, 3)
    cur = np.asarray(cur, F).reshape(-1, 4)
    m, ok = HR.unit_normal(n)
    covered = ok & (np.asarray(geometry).reshape(-1) != 0) & (cur[:, 3] > F(0))
    N, acc = np.ones(len(w), F), cur[:, 0:3].copy()
    accepted = np.full(len(w), -1, np.int32)
    if prev is not None:
        inside, _, ix, iy, ax, ay = HR.reproject(prev["P"], w, W, H)
        use = np.nonzero(covered & inside)[0]
        x0, y0 = ix[use].astype(np.int32), iy[use].astype(np.int32)
        fx, fy = ax[use], ay[use]
        bx, by = F(1.0) - fx, F(1.0) - fy
        weight = [bx * by, fx * by, bx * fy, fx * fy]
        pa, pc = np.asarray(prev["acc"], F).reshape(H, W, 3), np.asarray(prev["count"], F).reshape(H, W)
        pw, pm = np.asarray(prev["world"], F).reshape(H, W, 3), np.asarray(prev["normal"], F).reshape(H, W, 3)
        k, kc, kv, n_acc = [], [], [[], [], []], np.zeros(len(use), np.int32)
        for t in range(4):
            qx, qy = x0 + (t & 1), y0 + (t >> 1)
            inb = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            with np.errstate(all="ignore"):
                a = inb & (pc[cy, cx] > 0) & HR.accepts(m[use], w[use], pm[cy, cx], pw[cy, cx], hist["normal_cos"], hist["plane_dist"])
                z = np.where(a, weight[t], F(0.0))
                k.append(z)
                kc.append(z * pc[cy, cx] if defect == "rejected tap multiplied" else np.where(a, weight[t] * pc[cy, cx], F(0.0)))
                for c in range(3):
                    kv[c].append(z * pa[cy, cx, c] if defect == "rejected tap multiplied" else np.where(a, weight[t] * pa[cy, cx, c], F(0.0)))
            n_acc += a
        with np.errstate(all="ignore"):
            S, C = ((k[0] + k[1]) + k[2]) + k[3], ((kc[0] + kc[1]) + kc[2]) + kc[3]
            Nn = np.minimum(C / S + F(1.0), F(hist["max_history"]))
            a = F(1.0) / Nn
            take = S > F(hist["min_weight"])
            N[use] = np.where(take, Nn, F(1.0))
            for c in range(3):
                V = ((kv[c][0] + kv[c][1]) + kv[c][2]) + kv[c][3]
                hv = V / S
                acc[use, c] = np.where(take, hv + (cur[use, c] - hv) * a, cur[use, c])
        accepted[use] = n_acc
    z3 = lambda a: np.where(covered[:, None], a, F(0.0)).astype(F)
    count = np.where(covered, N, F(0.0)).astype(F)
    return dict(out=np.concatenate([z3(acc), count[:, None]], 1), acc=z3(acc), count=count, world=z3(w), normal=z3(m), accepted=np.where(covered, accepted, -1))


def accumulate_frame(attrs, material, cur, prev, P, hist, defect=None):
    """one call on a whole frame: -> (out (H, W, 4), the state for the next call, accepted (H, W))"""
    H, W = material.shape
    a = np.asarray(attrs, F).reshape(-1, 18)
    r = accumulate(a[:, 11:14], a[:, 8:11], np.asarray(material).reshape(-1) != NO_MATERIAL, np.asarray(cur, F).reshape(-1, 4), prev, W, H, hist, defect)
    state = dict(P=np.asarray(P, F).reshape(4, 4).copy(), acc=r["acc"].reshape(H, W, 3), count=r["count"].reshape(H, W), world=r["world"].reshape(H, W, 3),
                 normal=r["normal"].reshape(H, W, 3))
    return r["out"].reshape(H, W, 4), state, r["accepted"].reshape(H, W)


# ---- stage 6: the composition's two terms ------------------------------------------------------------------------------------------------------------
def compose(hdr, base, metal, E, geometry, ambient, gi_strength, ambient_scale, dtype=F):
    """C + (ambient * base) * (ambient_scale - 1), then + (gi_strength * (1 - metal)) * (base * E.rgb) where E.a > 0, for the pixels with geometry;
    dtype float32: the definition's roundings (what arctic_gi_compose_pixels returns by bytes); float64: the reference of the device test"""
    T = dtype
    C, base, metal, E = np.asarray(hdr, T).reshape(-1, 3).copy(), np.asarray(base, T).reshape(-1, 3), np.asarray(metal, T).reshape(-1), np.asarray(E, T).reshape(-1, 4)
    g = np.asarray(geometry).reshape(-1) != 0
    with np.errstate(all="ignore"):
        k = T(ambient_scale) - T(1.0)
        amb = C + (T(ambient) * base) * k
        s = (T(gi_strength) * (T(1.0) - metal))[:, None]
        lit = amb + s * (base * E[:, 0:3])
    out = np.where(g[:, None], np.where((E[:, 3] > 0)[:, None], lit, amb), C)
    return out.astype(T)
