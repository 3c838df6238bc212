"""The arbiter of the ray queries: include/arctic_hip.h's definition ("ray queries", in front of arctic_trace_rays) restated in numpy float32,
operation for operation, from the header's text -- not from the library's C++.  Every array below is float32 and every operation is one numpy
ufunc on float32 operands, so each rounds once, in the written order, and nothing contracts.

  brute()        the definition itself: every ray against every triangle, the smallest t, then the smallest prim.
  build_bvh()    a median-split tree of its own (depth-first order, skip links, exact boxes) ...
  walk()         ... and the pruned walk over it.  It exists to show that pruning by max(tn, t_min) > min(tf, t_max, t_best) changes nothing
                 (tests/test_ray_reference.py), and -- once that is shown -- as the fast way to evaluate the definition for many rays.

`defect` names a deliberate deviation, so that the tests can show they tell the definition from it:
  "open_interval"  t_min < t < t_max instead of <=          "no_clamp"       t = tm, not clamped into the triangle's box interval
  "tie_larger"     among equal t the LARGER prim            "uv_open"        u + v < 1 instead of <=
  "prune_nonstrict" (walk only) a node is skipped when max(tn, t_min) >= min(tf, t_max, t_best)
"""
import numpy as np

F = np.float32
INF = F(np.inf)
NO_PRIM = 0xFFFFFFFF
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("direction", "<f4", 3), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])


def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(a < b, b, a)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def make_rays(origins, directions, t_min=0.0, t_max=np.inf):
    o = np.asarray(origins, F).reshape(-1, 3)
    r = np.zeros(len(o), RAY_DTYPE)
    r["origin"], r["direction"], r["t_min"], r["t_max"] = o, np.asarray(directions, F).reshape(-1, 3), t_min, t_max
    return r


def ray_valid(rays):
    """a ray whose origin or direction has a component that is not finite, or whose direction is zero, is a miss"""
    o, d = rays["origin"], rays["direction"]
    return np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & ~(d == 0).all(-1)


def ray_box(o, d, bmin, bmax):
    """o, d, bmin, bmax: sequences of 3 broadcastable float32 arrays -> (met, tn, tf)"""
    los, his, ok = [], [], True
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F(1.0) / d[a]
            l = (bmin[a] - o[a]) * inv
            h = (bmax[a] - o[a]) * inv
            free = (d[a] == 0) | np.isnan(l) | np.isnan(h)          # d == 0 inside the slab, or 0 * inf: (-inf, +inf)
            ok = ok & ~((d[a] == 0) & ~((bmin[a] <= o[a]) & (o[a] <= bmax[a])))
            los.append(np.where(free, -INF, _min(l, h)))
            his.append(np.where(free, INF, _max(l, h)))
        tn = _max(_max(los[0], los[1]), los[2])
        tf = _min(_min(his[0], his[1]), his[2])
        return ok & (tn <= tf), tn, tf


def ray_triangle(o, d, t_min, t_max, p0, p1, p2, defect=None):
    """o, d, p0, p1, p2: sequences of 3 broadcastable float32 arrays -> (hit, t, u, v)"""
    with np.errstate(all="ignore"):
        bmin = [_min(_min(p0[a], p1[a]), p2[a]) for a in range(3)]
        bmax = [_max(_max(p0[a], p1[a]), p2[a]) for a in range(3)]
        met, tn, tf = ray_box(o, d, bmin, bmax)
        e1 = [p1[a] - p0[a] for a in range(3)]
        e2 = [p2[a] - p0[a] for a in range(3)]
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        inv = F(1.0) / det
        tv = [o[a] - p0[a] for a in range(3)]
        u = _dot(tv, pv) * inv
        qv = _cross(tv, e1)
        v = _dot(d, qv) * inv
        tm = _dot(e2, qv) * inv
        edge = (u + v < 1) if defect == "uv_open" else (u + v <= 1)
        inside = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & edge & ~np.isnan(tm)
        t = tm if defect == "no_clamp" else _min(_max(tm, tn), tf)
        within = ((t_min < t) & (t < t_max)) if defect == "open_interval" else ((t_min <= t) & (t <= t_max))
        finite = True
        for p in (p0, p1, p2):
            for a in range(3):
                finite = finite & np.isfinite(p[a])
        return met & inside & within & finite, t, u, v


def _columns(tris):
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    return [[t[:, k, a] for a in range(3)] for k in range(3)]


def _result(n):
    h = np.zeros(n, HIT_DTYPE)
    h["prim"] = NO_PRIM
    return h


def brute(tris, rays, any_hit=False, defect=None, prims=None, chunk=2048):
    """the definition: every ray against every triangle.  tris: (n, 9) world-space triangles; prims: their numbers (default: the index)"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    prims = np.arange(len(tris), dtype=np.int64) if prims is None else np.asarray(prims, np.int64)
    out = _result(len(rays))
    if len(tris) == 0 or len(rays) == 0:
        return out
    p0, p1, p2 = [[c[None, :] for c in p] for p in _columns(tris)]
    valid = ray_valid(rays)
    for s in range(0, len(rays), chunk):
        r = rays[s:s + chunk]
        o = [r["origin"][:, a, None] for a in range(3)]
        d = [r["direction"][:, a, None] for a in range(3)]
        hit, t, u, v = ray_triangle(o, d, r["t_min"][:, None], r["t_max"][:, None], p0, p1, p2, defect)
        hit = hit & valid[s:s + chunk, None]
        anyh = hit.any(1)
        if any_hit:
            out["prim"][s:s + chunk] = np.where(anyh, 0, NO_PRIM)
            continue
        tt = np.where(hit, t, INF)
        tbest = tt.min(1)
        tie = hit & (tt == tbest[:, None])              # (-0 == +0: a tie)
        pp = np.where(tie, prims[None, :], -1 if defect == "tie_larger" else 1 << 40)
        k = pp.argmax(1) if defect == "tie_larger" else pp.argmin(1)
        rows = np.arange(len(r))
        res = out[s:s + chunk]
        res["t"] = np.where(anyh, t[rows, k], 0)
        res["u"] = np.where(anyh, u[rows, k], 0)
        res["v"] = np.where(anyh, v[rows, k], 0)
        res["prim"] = np.where(anyh, prims[k], NO_PRIM)
    return out


def tied(tris, rays):
    """per ray: is it hit, and do two or more triangles share its closest t?"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    p0, p1, p2 = [[c[None, :] for c in p] for p in _columns(tris)]
    o = [rays["origin"][:, a, None] for a in range(3)]
    d = [rays["direction"][:, a, None] for a in range(3)]
    hit, t, _, _ = ray_triangle(o, d, rays["t_min"][:, None], rays["t_max"][:, None], p0, p1, p2)
    hit = hit & ray_valid(rays)[:, None]
    tt = np.where(hit, t, INF)
    return hit.any(1), (hit & (tt == tt.min(1)[:, None])).sum(1) >= 2


class Bvh:
    """depth-first nodes with skip links: bmin, bmax (n, 3), skip (n,), first, count (n,); tris (m, 9) and prims (m,) reordered by leaf"""


def build_bvh(tris, prims=None, leaf=4):
    tris = np.ascontiguousarray(tris, F).reshape(-1, 9)
    prims = np.arange(len(tris), dtype=np.int64) if prims is None else np.asarray(prims, np.int64)
    keep = np.isfinite(tris).all(1)                     # a triangle with a vertex that is not finite is never hit
    tris, prims = tris[keep], prims[keep]
    t3 = tris.reshape(-1, 3, 3)
    lo, hi = t3.min(1), t3.max(1)
    cen = F(0.5) * lo + F(0.5) * hi
    bmin, bmax, skip, first, count, order = [], [], [], [], [], []

    def rec(ids):
        i = len(skip)
        bmin.append(lo[ids].min(0)); bmax.append(hi[ids].max(0)); skip.append(0); first.append(len(order)); count.append(0)
        if len(ids) <= leaf:
            count[i] = len(ids)
            order.extend(ids[np.argsort(prims[ids], kind="stable")].tolist())
        else:
            with np.errstate(all="ignore"):
                axis = int(np.argmax(cen[ids].max(0) - cen[ids].min(0)))   # the widest centroid axis, the lowest on a tie
            ids = ids[np.lexsort((prims[ids], cen[ids, axis]))]              # by centroid, ties by prim
            rec(ids[:len(ids) // 2]); rec(ids[len(ids) // 2:])
        skip[i] = len(skip)

    if len(tris):
        rec(np.arange(len(tris)))
    b = Bvh()
    b.bmin, b.bmax = np.array(bmin, F).reshape(-1, 3), np.array(bmax, F).reshape(-1, 3)
    b.skip, b.first, b.count = np.array(skip, np.int64), np.array(first, np.int64), np.array(count, np.int64)
    order = np.array(order, np.int64)
    b.tris, b.prims = tris[order].reshape(-1, 9), prims[order]
    return b


def walk(bvh, rays, any_hit=False, defect=None, count_triangles=False):
    """the pruned walk, all rays at once: every ray stands at its own node; -> (hits, nodes visited per ray[, triangles tested per ray])"""
    n, n_nodes = len(rays), len(bvh.skip)
    out = _result(n)
    visits = np.zeros(n, np.int64)
    tested = np.zeros(n, np.int64)
    best_t = np.full(n, INF, F)
    best_prim = np.full(n, 1 << 40, np.int64)
    at = np.where(ray_valid(rays), 0, n_nodes).astype(np.int64)
    O, D, TMIN, TMAX = rays["origin"], rays["direction"], rays["t_min"], rays["t_max"]
    while True:
        act = np.nonzero(at < n_nodes)[0]
        if len(act) == 0:
            break
        i = at[act]
        visits[act] += 1
        o = [O[act, a] for a in range(3)]
        d = [D[act, a] for a in range(3)]
        met, tn, tf = ray_box(o, d, [bvh.bmin[i, a] for a in range(3)], [bvh.bmax[i, a] for a in range(3)])
        with np.errstate(all="ignore"):
            near = _max(tn, TMIN[act])
            far = _min(_min(tf, TMAX[act]), TMAX[act] if any_hit else best_t[act])
            pruned = ~met | ((near >= far) if defect == "prune_nonstrict" else (near > far))
        # a NaN limit admits no hit; comparisons with it are false, so such a ray is never pruned -- it only walks further
        at[act] = np.where(pruned, bvh.skip[i], i + 1)
        leafs = ~pruned & (bvh.count[i] > 0)
        for k in range(int(bvh.count.max()) if n_nodes else 0):
            sel = leafs & (bvh.count[i] > k)
            if not sel.any():
                break
            ra, tri = act[sel], bvh.first[i[sel]] + k
            tested[ra] += 1
            T = bvh.tris[tri]
            hit, t, u, v = ray_triangle([O[ra, a] for a in range(3)], [D[ra, a] for a in range(3)], TMIN[ra], TMAX[ra],
                                        [T[:, a] for a in range(3)], [T[:, 3 + a] for a in range(3)], [T[:, 6 + a] for a in range(3)], defect)
            prim = bvh.prims[tri]
            if defect == "tie_larger":
                better = hit & ((t < best_t[ra]) | ((t == best_t[ra]) & ((prim > best_prim[ra]) | (best_prim[ra] == 1 << 40))))
            else:
                better = hit & ((t < best_t[ra]) | ((t == best_t[ra]) & (prim < best_prim[ra])))
            w = ra[better]
            best_t[w], best_prim[w] = t[better], prim[better]
            out["t"][w], out["u"][w], out["v"][w], out["prim"][w] = t[better], u[better], v[better], prim[better]
            if any_hit:
                at[ra[hit]] = n_nodes
    if any_hit:
        found = out["prim"] != NO_PRIM
        out["t"], out["u"], out["v"] = 0, 0, 0
        out["prim"] = np.where(found, 0, NO_PRIM)
    return (out, visits, tested) if count_triangles else (out, visits)


def world_triangles(objects, meshes):
    """the scene's triangles: objects = records with "trs" (16 floats, glm order) and "mesh_idx"; meshes = list of (vertices with "position",
    indices) as the passes read them.  -> (tris (m, 9), prims (m,)): triangles with an index out of range are skipped but numbered"""
    tris, prims, prim = [], [], 0
    for ob in objects:
        if int(ob["mesh_idx"]) >= len(meshes):
            continue
        verts, ind = meshes[int(ob["mesh_idx"])]
        M = np.asarray(ob["trs"], F)
        x, y, z = (np.ascontiguousarray(verts["position"][:, a], F) for a in range(3))
        with np.errstate(all="ignore"):
            w = np.stack([((M[i] * x + M[4 + i] * y) + M[8 + i] * z) + M[12 + i] * F(1.0) for i in range(3)], -1)
        idx = np.asarray(ind, np.int64).reshape(-1, 3)
        ok = (idx < len(verts)).all(1)
        tris.append(w[idx[ok]].reshape(-1, 9))
        prims.append(prim + np.nonzero(ok)[0])
        prim += len(idx)
    if not tris:
        return np.zeros((0, 9), F), np.zeros(0, np.int64)
    return np.concatenate(tris).astype(F), np.concatenate(prims).astype(np.int64)


def sun_rays(attrs, sun_dir, bias):
    """arctic_trace_sun_visibility's rays from arctic_read_gbuffer's attributes (rows, width, 18): o = world + bias * n, d = -sun_dir"""
    world, nrm = attrs[..., 11:14].reshape(-1, 3).astype(F), attrs[..., 8:11].reshape(-1, 3).astype(F)
    with np.errstate(all="ignore"):
        o = world + F(bias) * nrm
    return make_rays(o, np.broadcast_to(-np.asarray(sun_dir, F), o.shape), 0.0, np.inf)


def soup_triangles(rng, n_tris):
    """the kind of triangles the definition was tried on: a third snapped to a grid with shared edges, a quarter axis-aligned on four shared
    planes, a few degenerate.  -> (n_tris, 9)"""
    t = rng.uniform(-4, 4, (n_tris, 1, 3)).astype(F) + rng.uniform(-1, 1, (n_tris, 3, 3)).astype(F)
    kind = rng.integers(0, 12, n_tris)
    grid = kind < 4
    # grid cells of a height field on half-integer coordinates: neighbouring cells share edges and vertices exactly
    g = max(1, int(round((n_tris / 16) ** 0.5)))        # about one grid triangle per cell half, whatever the count: neighbours do share edges
    gx, gz = rng.integers(-g, g, n_tris), rng.integers(-g, g, n_tris)
    hgt = lambda x, z: ((x * 7 + z * 13) % 5).astype(F) * F(0.25)
    upper = rng.integers(0, 2, n_tris).astype(bool)
    c = [(gx, gz), (gx + 1, gz), (gx + 1, gz + 1), (gx, gz + 1)]
    pick = np.where(upper[:, None], [0, 1, 2], [0, 2, 3])
    for k in range(3):                                  # (g above is the grid's half-width in cells)
        cx = np.choose(pick[:, k], [c[j][0] for j in range(4)]); cz = np.choose(pick[:, k], [c[j][1] for j in range(4)])
        corner = np.stack([cx * F(0.5), hgt(cx, cz), cz * F(0.5)], -1).astype(F)
        t[grid, k] = corner[grid]
    planes = (kind >= 4) & (kind < 7)
    axis, level = rng.integers(0, 3, n_tris), rng.choice(np.array([-2.0, 0.0, 1.5, 3.0], F), n_tris)
    for a in range(3):
        m = planes & (axis == a)
        t[m, :, a] = level[m, None]
    snap = planes & (rng.random(n_tris) < 0.5)
    t[snap] = np.round(t[snap] * 2) / 2                 # (the plane levels are multiples of 0.5 too)
    deg = np.nonzero(kind == 11)[0][:max(1, n_tris // 20)]
    t[deg, 2] = t[deg, 1]                                # degenerate: two equal vertices
    return t.astype(F).reshape(-1, 9)


def soup_rays(rng, tris, n_rays):
    """rays for such triangles: aimed at random points of them, exactly at their vertices and edge midpoints, parallel to an axis, with a zero
    direction component, from origins inside the shared planes or on the grid, with finite intervals and with hits behind the origin"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    n_tris = len(t)
    centre, half = F(0.5) * (t.min((0, 1)) + t.max((0, 1))), F(0.5) * (t.max((0, 1)) - t.min((0, 1))) + F(1.0)
    o = (centre + half * rng.uniform(-1.2, 1.2, (n_rays, 3))).astype(F)
    aim = t[rng.integers(0, n_tris, n_rays)]
    w = rng.dirichlet(np.ones(3), n_rays).astype(F)
    target = (aim * w[:, :, None]).sum(1).astype(F)
    how = rng.integers(0, 10, n_rays)
    target = np.where((how == 0)[:, None], aim[:, 0], target)                               # exactly at a vertex
    target = np.where((how == 1)[:, None], F(0.5) * aim[:, 0] + F(0.5) * aim[:, 1], target)   # an edge midpoint
    d = (target - o).astype(F)
    par = how == 2                                       # parallel to an axis, through the target
    ax = rng.integers(0, 3, n_rays)
    for a in range(3):
        m = par & (ax == a)
        o[m] = target[m]; o[m, a] = centre[a] - F(2.0) * half[a]
        d[m] = 0; d[m, a] = F(1.0)
    two = how == 3                                       # one zero component
    d[two, ax[two]] = 0
    inplane = how == 4                                   # origin in a plane of some triangle's box (for axis-aligned triangles: in the shared plane)
    o[inplane, ax[inplane]] = t[rng.integers(0, n_tris, n_rays), rng.integers(0, 3, n_rays), ax][inplane]
    d = np.where((how == 4)[:, None], (target - o).astype(F), d)
    snapo = how == 5                                     # origin on the grid, aimed at a grid vertex: rays along shared edges and planes
    o[snapo] = np.round(o[snapo] * 2) / 2
    d = np.where(snapo[:, None], (np.round(target * 2) / 2 - o).astype(F), d)
    rays = make_rays(o, d, 0.0, np.inf)
    lim = how == 6                                       # a finite interval
    rays["t_min"][lim] = rng.uniform(0, 0.5, int(lim.sum())).astype(F)
    rays["t_max"][lim] = rng.uniform(0.5, 1.5, int(lim.sum())).astype(F)
    neg = how == 7                                       # hits behind the origin count when t_min allows them
    rays["t_min"][neg] = -INF
    return rays


def soup(rng, n_tris, n_rays):
    """-> (tris (n_tris, 9), rays): soup_triangles and soup_rays for them"""
    tris = soup_triangles(rng, n_tris)
    return tris, soup_rays(rng, tris, n_rays)
