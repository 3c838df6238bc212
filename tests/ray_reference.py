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
  "nan_prunes"     (walk only) a NaN slab product of the NODE test -- 0 * inf: a zero direction component, or one whose reciprocal overflows, and
                   an origin in the box's plane -- reads as "box missed" instead of "no constraint": what an odd ray meets in a walk that does
                   not look for the NaN

The generators at the end lay rays out by the WAVE of 64 they fall into on the device, where trace.hip chooses the walk per wave (ray_odd):
wave_rays, edge_records, subnormal_rays, and soup_gbuffer for the sun's rays.
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


def ray_odd(rays):
    """RayPrep::odd of ray_query.h restated: some d == 0, or some float32(1) / d that is not finite -- the rays whose node test can meet 0 * inf.
    A wave of 64 on the device takes the walk that looks for the NaN when one of its VALID lanes is odd (wave_walks)"""
    d = rays["direction"]
    with np.errstate(all="ignore"):
        return ((d == 0) | ~np.isfinite(F(1.0) / d)).any(-1)


def ray_box(o, d, bmin, bmax, nan_prunes=False):
    """o, d, bmin, bmax: sequences of 3 broadcastable float32 arrays -> (met, tn, tf)"""
    los, his, ok = [], [], True
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F(1.0) / d[a]
            l = (bmin[a] - o[a]) * inv
            h = (bmax[a] - o[a]) * inv
            if nan_prunes:                                          # the defect: d == 0 counts as a reciprocal of +inf, and a NaN product misses
                n = np.where(d[a] == 0, INF, inv)
                ok = ok & ~(np.isnan((bmin[a] - o[a]) * n) | np.isnan((bmax[a] - o[a]) * n))
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
        met, tn, tf = ray_box(o, d, [bvh.bmin[i, a] for a in range(3)], [bvh.bmax[i, a] for a in range(3)], defect == "nan_prunes")
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


# ---- rays laid out by wave ------------------------------------------------------------------------------------------------------------------
WAVE = 64
SUBNORMAL_ODD = (0x00000000, 0x00000001, 0x00200000)                # |d|: zero; the smallest subnormal; 2^-128, the largest whose reciprocal overflows
SUBNORMAL_PLAIN = (0x00200001, 0x00400000, 0x007FFFFF, 0x00800000)  # one step above it; 2^-127; the largest subnormal; the smallest normal number


def wave_walks(rays):
    """per wave of 64 consecutive rays, the walk trace.hip takes for it -- "odd" when a valid lane is odd, "plain" when it has valid lanes and
    none is odd, "none" when no lane walks --, computed from ray_odd and ray_valid alone"""
    valid = ray_valid(rays)
    odd = valid & ray_odd(rays)
    return ["odd" if odd[s:s + WAVE].any() else "plain" if valid[s:s + WAVE].any() else "none" for s in range(0, len(rays), WAVE)]


def tile_walks(rays, active, rows, width, row0_in_tile=0):
    """the same for arctic_trace_sun_visibility, whose waves are the 8 x 8 tiles of the handle's rows x width pixels (one ray each, row-major;
    the first row is row row0_in_tile of its tile row): -> the walks of the tiles, row by row"""
    valid = ray_valid(rays) & active
    odd = valid & ray_odd(rays)
    th, tw = -(-(rows + row0_in_tile) // 8), -(-width // 8)
    out = []
    for plane in (valid, odd):
        full = np.zeros((th * 8, tw * 8), bool)
        full[row0_in_tile:row0_in_tile + rows, :width] = plane.reshape(rows, width)
        out.append(full.reshape(th, 8, tw, 8).any((1, 3)).reshape(-1))
    return ["odd" if o else "plain" if v else "none" for v, o in zip(*out)]


EDGE_NAMES = ["d = (0, 0, 0)", "d = (-0, 0, -0)", "o.x = NaN", "o.y = +inf", "o.z = -inf", "d.z = NaN", "d.x = +inf", "d.y = -inf",
              "t_min = NaN", "t_max = NaN", "t_min = +inf", "t_max = -inf", "t_min > t_max", "t_min = -inf, t_max = +inf"]
EDGE_INVALID = 8                                                   # records 0..7 are not valid rays; 8..12 are valid and admit no t; 13 admits every t


def edge_records(base=None):
    """the fixed list of bad rays (EDGE_NAMES), each written into a copy of `base` (one ray; default: (1, 1, 0) + t (0.25, 0.5, 1), which is not
    odd).  Every record but the last is a miss whatever the triangles.  t_min > t_max is 1.5 > 0.5: limits that, swapped, would admit the hit of
    a ray aimed at a target at t = 1"""
    base = make_rays([[1, 1, 0]], [[0.25, 0.5, 1]]) if base is None else np.asarray(base, RAY_DTYPE).reshape(1)
    r = np.repeat(base, len(EDGE_NAMES))
    r["direction"][0] = (0.0, 0.0, 0.0)
    r["direction"][1] = (-0.0, 0.0, -0.0)
    r["origin"][2, 0], r["origin"][3, 1], r["origin"][4, 2] = np.nan, np.inf, -np.inf
    r["direction"][5, 2], r["direction"][6, 0], r["direction"][7, 1] = np.nan, np.inf, -np.inf
    r["t_min"][8], r["t_max"][9], r["t_min"][10], r["t_max"][11] = np.nan, np.nan, np.inf, -np.inf
    r["t_min"][12], r["t_max"][12] = 1.5, 0.5
    r["t_min"][13], r["t_max"][13] = -np.inf, np.inf
    return r


def _lanes(*parts):
    out = []
    for kind, count in parts:
        out += [kind] * count
    return out


def _with_edges(lanes, edges):
    lanes = list(lanes)
    for lane, k in edges.items():
        lanes[lane] = ("edge", k)
    return lanes


_ALL_EDGES = dict(zip([0, 1, 2, 3, 4, 5, 6, 31, 32, 59, 60, 61, 62, 63], range(14)))
# a lane is "plain" / "odd" (a ray of that kind from the pool), ("edge", k) (edge record k written over such a ray), or "bad_plain" / "bad_odd"
# (such a ray made invalid: the former stays not odd, the latter stays odd)
WAVE_LAYOUTS = {
    # 9 waves, 529 rays: crosses one 256-thread workgroup boundary
    1: [_lanes(("plain", 64)),
        _lanes(("odd", 64)),
        _lanes(("plain", 63), ("odd", 1)),
        _lanes(("odd", 1), ("plain", 63)),
        _with_edges(_lanes(("plain", 64)), {0: 0, 1: 5, 2: 3, 31: 8, 32: 11, 63: 12}),   # invalid odd lanes (d = 0, d.z = NaN) in a plain wave
        _lanes(("bad_odd", 1), ("bad_plain", 1)) * 32,
        _lanes(("plain", 64)),
        _lanes(("plain", 64)),
        _lanes(("plain", 17))],
    # every edge record in a plain wave and in an odd wave, and a partial wave that one lane makes odd
    2: [_with_edges(_lanes(("plain", 64)), _ALL_EDGES),
        _with_edges(_lanes(("odd", 64)), _ALL_EDGES),
        _lanes(("plain", 16), ("odd", 1))],
}


def _spoil(ray, k, odd):
    """one ray made invalid, the k-th way; odd: keep it odd (ray_odd), else keep it not odd"""
    bad = (np.nan, np.inf, -np.inf)
    if odd and k % 6 == 4:
        ray["direction"] = (0.0, 0.0, 0.0)
    elif odd and k % 6 == 5:
        ray["direction"][k % 3] = np.nan                            # (1 / NaN is not finite: odd whatever the ray was)
    elif not odd and k % 6 >= 4:
        ray["direction"][k % 3] = bad[1 + k % 2]                    # (1 / inf = 0 is finite: not odd)
    else:
        ray["origin"][k % 3] = bad[(k // 3) % 3]
    return ray


def vertex_rays(rng, tris, n_rays):
    """rays that are not odd, aimed from general origins exactly at vertices that two or more triangles share (at any vertex where none is
    shared) and at points of axis-aligned triangles: the closest hit of such a ray is often shared by several triangles (tied), and the smaller
    prim has to win"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    v, owner = t.reshape(-1, 3), np.repeat(np.arange(len(t)), 3)
    uniq, inv = np.unique(v, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    owners = np.zeros(len(uniq), np.int64)
    np.add.at(owners, np.unique(np.stack([inv, owner], 1), axis=0)[:, 0], 1)
    shared = uniq[owners >= 2] if (owners >= 2).any() else uniq
    target = shared[rng.integers(0, len(shared), n_rays)]
    flat = np.nonzero((t.max(1) == t.min(1)).any(1))[0]             # axis-aligned triangles: those of one shared plane overlap, and tie at the slab's t
    if len(flat):
        inside = (t[flat[rng.integers(0, len(flat), n_rays)]] * rng.dirichlet(np.ones(3), n_rays).astype(F)[:, :, None]).sum(1).astype(F)
        target = np.where((rng.random(n_rays) < 0.5)[:, None], inside, target)
    off = (rng.uniform(0.5, 3.0, (n_rays, 3)) * rng.choice([-1.0, 1.0], (n_rays, 3))).astype(F)
    o = (target + off).astype(F)
    return make_rays(o, (target - o).astype(F), 0.0, np.inf)


def planar_rays(rng, tris, n_rays):
    """odd rays whose origin lies in a plane of a triangle's box on an axis where the direction is zero, or so small that its reciprocal
    overflows (1e-45): the node test's 0 * inf.  They are aimed at the triangle's vertex in that plane; a third of them run parallel to an axis"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    k, a = rng.integers(0, len(t), n_rays), rng.integers(0, 3, n_rays)
    upper = rng.integers(0, 2, n_rays).astype(bool)
    coord = t[k, :, a]
    vertex = t[k, np.where(upper, coord.argmax(1), coord.argmin(1))]
    off = (rng.uniform(0.5, 3.0, (n_rays, 3)) * rng.choice([-1.0, 1.0], (n_rays, 3))).astype(F)
    how = rng.integers(0, 3, n_rays)
    rows = np.arange(n_rays)
    off[rows, a] = 0
    off[how == 2, (a[how == 2] + 1) % 3] = 0                         # parallel to the third axis
    o = (vertex + off).astype(F)
    d = (vertex - o).astype(F)
    assert (d[rows, a] == 0).all()
    tiny = how == 1
    d[tiny, a[tiny]] = (F(1e-45) * rng.choice(np.array([-1, 1], F), n_rays))[tiny]
    return make_rays(o, d, 0.0, np.inf)


def wave_pool(rng, tris, prims=None, n_soup=2048, n_vertex=1024, n_planar=192):
    """the rays wave_rays deals from: soup_rays, vertex_rays and planar_rays, classified once.  SPECIAL among the rays that are not odd: those
    whose result a walk that prunes at equality changes (defect "prune_nonstrict" in this module's own tree, which is split as the library's
    is) -- they come first -- and those whose closest hit two triangles share (tied); among the odd rays: those whose result a walk changes
    that takes a NaN slab product for a miss (defect "nan_prunes") -- they come first -- and the planar_rays"""
    p = soup_rays(rng, tris, n_soup)
    p = np.concatenate([p[ray_valid(p)], vertex_rays(rng, tris, n_vertex), planar_rays(rng, tris, n_planar)])
    odd = ray_odd(p)
    hit, tie = tied(tris, p)
    bvh = build_bvh(tris, prims)
    sensitive = np.zeros(len(p), bool)
    sensitive[~odd] = walk(bvh, p[~odd])[0] != walk(bvh, p[~odd], defect="prune_nonstrict")[0]
    sensitive[odd] = walk(bvh, p[odd])[0] != walk(bvh, p[odd], defect="nan_prunes")[0]
    special = np.where(odd, np.arange(len(p)) >= len(p) - n_planar, tie) | sensitive
    return dict(rays=p, odd=odd, hit=hit, special=special, first=sensitive)


class _Deck:
    """the rays of one kind (odd, or not) that wave_rays deals from, as three fixed orders of pool indices:
      any      every ray of the kind that is not special, in the pool's order
      hitting  those of `any` that hit something, in the pool's order
      special  the special ones: those whose result the walk's defect changes first, then the others
    next() goes round  any, special, hitting  and takes the first ray of that order not dealt yet (of `any` where the order is used up), so a
    third of the lanes are special rays while they last and at least a third hit.  bases: rays that hit, kept back for the edge records"""
    def __init__(self, pool, ids, n_bases):
        hit, special, first = pool["hit"], pool["special"], pool["first"]
        hitting = ids[hit[ids]]
        self.bases = list(np.concatenate([hitting[~special[hitting]], hitting[special[hitting]]])[:n_bases])   # (not special ones, where there are enough)
        assert len(self.bases) == n_bases, "the pool is too small"
        rest = np.setdiff1d(ids, self.bases)
        plain, chosen = rest[~special[rest]], rest[special[rest]]
        self.orders = [plain, np.concatenate([chosen[first[chosen]], chosen[~first[chosen]]]), plain[hit[plain]]]
        self.at, self.dealt, self.turn = [0, 0, 0], set(), 0

    def next(self):
        for order in (self.turn % 3, 0):
            ids = self.orders[order]
            while self.at[order] < len(ids) and ids[self.at[order]] in self.dealt:
                self.at[order] += 1
            if self.at[order] < len(ids):
                self.turn += 1
                self.dealt.add(ids[self.at[order]])
                return ids[self.at[order]]
        raise AssertionError("the pool is too small")


def wave_rays(rng, tris, layout, prims=None, pool=None):
    """rays for the device's waves: a pool (wave_pool; made from rng where none is given) split by ray_odd and dealt into the lanes of
    WAVE_LAYOUTS[layout] (or of a list of that form) as _Deck describes.  Edge records are written over rays that hit something, so that a walk
    which ignored the record's defect would report a hit.
    -> (rays, waves): per wave dict(start, stop, lanes = the layout's lane kinds, edges = {lane: record number}, walk = "plain" / "odd" / "none"
    as the LAYOUT implies it -- tests check that claim with wave_walks)"""
    spec = WAVE_LAYOUTS[layout] if isinstance(layout, int) else layout
    pool = wave_pool(rng, tris, prims) if pool is None else pool
    p = pool["rays"]
    n_edge = {False: 0, True: 0}
    for w in spec:
        n_edge["odd" in w] += sum(isinstance(l, tuple) for l in w)
    deck = {o: _Deck(pool, np.nonzero(pool["odd"] == o)[0], n_edge[o]) for o in (False, True)}
    stronger = lambda a, b: max(a, b, key=["none", "plain", "odd"].index)
    rays, waves = [], []
    for w in spec:
        base_odd = "odd" in w                                        # edge records of an odd wave go over odd rays
        start, walk = len(rays), "none"
        for lane, kind in enumerate(w):
            if isinstance(kind, tuple):
                r = edge_records(p[deck[base_odd].bases.pop(0)])[kind[1]]
                if kind[1] >= EDGE_INVALID:
                    walk = stronger(walk, "odd" if base_odd else "plain")
            elif kind in ("plain", "odd"):
                r = p[deck[kind == "odd"].next()].copy()
                walk = stronger(walk, kind)
            else:
                r = _spoil(p[deck[kind == "bad_odd"].next()].copy(), lane // 2, kind == "bad_odd")
            rays.append(r)
        waves.append(dict(start=start, stop=len(rays), lanes=list(w), edges={l: k[1] for l, k in enumerate(w) if isinstance(k, tuple)}, walk=walk))
    assert all(wv["stop"] - wv["start"] == WAVE for wv in waves[:-1])
    return np.array(rays, RAY_DTYPE), waves


def subnormal_rays(tris, seed=5):
    """rays with ONE direction component at each bit pattern of SUBNORMAL_ODD and SUBNORMAL_PLAIN, of both signs, on each axis; the other two
    components are general, so such a ray runs (nearly) inside the plane of its origin's coordinate on that axis.  Per axis two triangles -- the
    one that reaches furthest up that axis, and another whose box has an extent on it where there is one -- and per triangle three origins: in
    the box's upper plane on that axis, aimed at the vertex there; one ulp above that plane (the triangle is missed; above the furthest one,
    everything is); strictly inside the box, aimed at a point of the triangle (a hit).
    -> (plain, odd): two sets, each (rays, pattern): `plain` holds the rays whose reciprocals are all finite, `odd` the others; each is padded to
    whole waves of 64 with soup rays that are not odd; pattern = |d| 's bits on the axis in question, -1 for a padding ray"""
    rng = np.random.default_rng(seed)
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    t = t[np.isfinite(t).all((1, 2))]
    lo, hi = t.min(1), t.max(1)
    sets = {False: ([], []), True: ([], [])}
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        top = int(np.argmax(hi[:, a]))
        wide = np.nonzero((hi[:, a] > lo[:, a]) & (np.arange(len(t)) != top))[0]
        for k in dict.fromkeys([top] + ([int(wide[rng.integers(len(wide))])] if len(wide) else [])):
            vertex = t[k][int(np.argmax(t[k][:, a]))]
            w = np.array([0.5, 0.25, 0.25], F)
            inner = (t[k] * w[:, None]).sum(0).astype(F)             # a point well inside the triangle
            for where, target in (("plane", vertex), ("above", vertex), ("inside", inner)):
                for bits in SUBNORMAL_ODD + SUBNORMAL_PLAIN:
                    for sign in (0, 0x80000000):
                        off = rng.uniform(0.75, 2.5, 2).astype(F) * rng.choice(np.array([-1, 1], F), 2)
                        o, d = target.copy(), np.zeros(3, F)
                        o[b], o[c] = target[b] + off[0], target[c] + off[1]
                        d[b], d[c] = target[b] - o[b], target[c] - o[c]
                        d[a] = np.array([bits | sign], np.uint32).view(F)[0]
                        if where == "plane":
                            o[a] = hi[k, a]
                        elif where == "above":
                            o[a] = np.nextafter(hi[k, a], INF)
                        rays, pats = sets[bits in SUBNORMAL_ODD]
                        rays.append(make_rays([o], [d])[0]); pats.append(bits)
    pad = soup_rays(rng, t.reshape(-1, 9), 256)
    pad = pad[ray_valid(pad) & ~ray_odd(pad)]
    out = []
    for is_odd in (False, True):
        rays, pats = sets[is_odd]
        n_pad = -len(rays) % WAVE
        out.append((np.concatenate([np.array(rays, RAY_DTYPE), pad[:n_pad]]), np.array(pats + [-1] * n_pad, np.int64)))
    return out[0], out[1]


def soup_gbuffer(rng, tris, height, width, axes=(1, 2)):
    """a G-buffer to inject for arctic_trace_sun_visibility: (attrs (height, width, 18) float32 with unit normals in 8..10 and world positions in
    11..13, material (height, width) uint32).  Half of the world positions are random points of the triangles.  The others lie on an edge of a
    triangle that runs at the triangle's largest or smallest coordinate on one of `axes` -- so the pixel's coordinate on that axis is a plane of
    that triangle's box and of every box it bounds --, or are such points snapped to multiples of 0.25 on those axes; their normals are +-x, so
    that a bias keeps them in that plane.  About an eighth of the pixels have no geometry (NO_PRIM as the material), the 8 x 8 tile at (16, 8)
    and row 20 among them; six covered pixels have a world coordinate that is not finite"""
    t = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    n = height * width
    world = (t[rng.integers(0, len(t), n)] * rng.dirichlet(np.ones(3), n).astype(F)[:, :, None]).sum(1).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    kind = rng.integers(0, 8, n)
    edges = []                                                       # (triangle, corner i, corner j, axis): an edge at the box's plane on that axis
    for a in axes:
        for i, j in ((0, 1), (1, 2), (2, 0)):
            same = (t[:, i, a] == t[:, j, a]) & ((t[:, i, a] == t[:, :, a].max(1)) | (t[:, i, a] == t[:, :, a].min(1))) & (t[:, :, a].max(1) > t[:, :, a].min(1))
            edges += [(k, i, j, a) for k in np.nonzero(same)[0]]
    for px in np.nonzero(kind >= 4)[0]:
        if kind[px] < 7 and edges:
            k, i, j, a = edges[rng.integers(len(edges))]
            lam = F(rng.uniform(0.1, 0.9))
            world[px] = t[k, i] + lam * (t[k, j] - t[k, i])
            world[px, a] = t[k, i, a]                                # exactly in the plane
        else:
            for a in axes:
                world[px, a] = np.round(world[px, a] * 4) / 4
        nrm[px] = (rng.choice([-1.0, 1.0]), 0.0, 0.0)
    material = np.zeros((height, width), np.uint32)
    material.reshape(-1)[kind == 0] = NO_PRIM
    material[8:16, 16:24] = NO_PRIM
    material[20 % height] = NO_PRIM
    covered = np.nonzero(material.reshape(-1) != NO_PRIM)[0]
    for m, px in enumerate(rng.choice(covered, 6, replace=False)):
        world[px, m % 3] = (np.nan, np.inf, -np.inf)[m // 2]
    attrs = np.zeros((height, width, 18), F)
    attrs[..., 8:11], attrs[..., 11:14] = nrm.reshape(height, width, 3), world.reshape(height, width, 3)
    return attrs, material
