"""The arbiter of the ambient occlusion: include/arctic_hip.h's definition (in front of arctic_trace_ambient_occlusion) restated in numpy float32,
operation for operation, from the header's text -- not from the library's C++.  The triangle test and the walk are ray_reference's; every
array below is float32 and every operation one numpy ufunc on float32 operands, so each rounds once, in the written order.

  normal(), frame(), rays()   steps 1 to 3 for any number of points
  ray_hits()                  step 3's answers, one bool per ray (by the pruned walk, or brute: the loop over every triangle)
  point_hits()                step 4 for points {world3, normal3} with a set each: what arctic_ambient_occlusion_points returns
  image_hits()                the same for a G-buffer (arctic_read_gbuffer's attributes and materials) whose rows are rows `frame_rows` of the frame
  result(), filtered()        the two results

`defect` names a deliberate deviation, so that the tests can show they tell the definition from it:
  "local_row"     the pattern takes the shard's row, not the frame's        "swap_xy"       set (x % P) * P + y % P
  "no_bias"       o = world                                                 "no_normalise"  m = n
  "no_radius"     t_max = +inf                                              "window_shift"  the window is -1..2 (P = 4), 0..1 (P = 2)
  "floor"         the result is 255 * V / T rounded down                    "p_tested"      p has to pass the tests of every other pixel
"""
import numpy as np

import ray_reference as R

F = np.float32
NO_MATERIAL = 0xFFFFFFFF


def normal(n, defect=None):
    """step 1: n (N, 3) -> (m (N, 3), ok (N,)): ok is false where len is zero or not finite or an m[i] is not finite"""
    n = np.asarray(n, F).reshape(-1, 3)
    n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        length = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
        m = np.stack([n0 / length, n1 / length, n2 / length], -1)
    ok = (length != 0) & np.isfinite(length) & np.isfinite(m).all(-1)
    if defect == "no_normalise":
        m = n.copy()
    assert m.dtype == F
    return m, ok


def frame(m):
    """step 2: -> (t, bt), each (N, 3)"""
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        s = np.copysign(F(1.0), m2)
        a = F(-1.0) / (s + m2)
        b = (m0 * m1) * a
        t = np.stack([F(1.0) + ((s * m0) * m0) * a, s * b, (-s) * m0], -1)
        bt = np.stack([b, s + (m1 * m1) * a, -m1], -1)
    assert t.dtype == F and bt.dtype == F
    return t, bt


def rays(world, m, local, radius, bias, defect=None):
    """step 3 for N points and their K local directions each (local: (N, K, 3)) -> (N, K) RAY_DTYPE records"""
    world, local = np.asarray(world, F).reshape(-1, 3), np.asarray(local, F)
    t, bt = frame(m)
    with np.errstate(all="ignore"):
        o = world if defect == "no_bias" else world + F(bias) * m
        d = np.stack([(t[:, None, i] * local[:, :, 0] + bt[:, None, i] * local[:, :, 1]) + m[:, None, i] * local[:, :, 2] for i in range(3)], -1)
    out = np.zeros(local.shape[:2], R.RAY_DTYPE)
    out["origin"], out["direction"] = o[:, None, :], d
    out["t_min"], out["t_max"] = 0.0, np.inf if defect == "no_radius" else F(radius)
    return out


def ray_hits(tris, ry, active, brute=False, bvh=None):
    """one bool per ray of ry (N, K): any hit; rays of points that are not `active` (N,) are not cast"""
    hit = np.zeros(ry.shape, bool)
    flat = ry[active].reshape(-1)
    if len(flat) and len(tris):
        if brute:
            found = R.brute(tris, flat, any_hit=True)
        else:
            found, _ = R.walk(R.build_bvh(tris) if bvh is None else bvh, flat, any_hit=True)
        hit[active] = (found["prim"] != R.NO_PRIM).reshape(-1, ry.shape[1])
    return hit


def point_rays(points, sets, dirs, n_rays, radius, bias, defect=None):
    """-> (rays (N, n_rays), ok (N,)) for points (N, 6) = {world3, normal3} with direction set sets[k] of dirs (P * P, n_rays, 3)"""
    points = np.asarray(points, F).reshape(-1, 6)
    dirs = np.asarray(dirs, F).reshape(-1, n_rays, 3)
    m, ok = normal(points[:, 3:6], defect)
    return rays(points[:, 0:3], m, dirs[np.asarray(sets, np.int64)], radius, bias, defect), ok


def point_hits(tris, points, sets, dirs, n_rays, radius, bias, defect=None, brute=False, bvh=None):
    """arctic_ambient_occlusion_points: (N,) uint8, 0 for a point that is not covered"""
    ry, ok = point_rays(points, sets, dirs, n_rays, radius, bias, defect)
    return ray_hits(tris, ry, ok, brute, bvh).sum(1).astype(np.uint8)


def set_index(x, y, P, defect=None):
    return (x % P) * P + y % P if defect == "swap_xy" else (y % P) * P + x % P


def image_points(attrs, material, P, frame_rows=None, defect=None):
    """a G-buffer's pixels as points: -> (points (rows * width, 6), sets, geometry (rows * width,): the pixel has geometry)"""
    rows, width = material.shape
    frame_rows = np.arange(rows) if frame_rows is None or defect == "local_row" else np.asarray(frame_rows)
    y, x = np.meshgrid(frame_rows, np.arange(width), indexing="ij")
    points = np.concatenate([attrs[..., 11:14], attrs[..., 8:11]], -1).reshape(-1, 6).astype(F)
    return points, set_index(x, y, P, defect).reshape(-1), material.reshape(-1) != NO_MATERIAL


def image_ray_hits(tris, attrs, material, dirs, n_rays, P, radius, bias, frame_rows=None, defect=None, brute=False, bvh=None):
    """-> (hit (rows * width, n_rays) bool, covered (rows * width,), rays (rows * width, n_rays))"""
    points, sets, geometry = image_points(attrs, material, P, frame_rows, defect)
    ry, ok = point_rays(points, sets, dirs, n_rays, radius, bias, defect)
    covered = ok & geometry
    return ray_hits(tris, ry, covered, brute, bvh), covered, ry


def image_hits(tris, attrs, material, dirs, n_rays, P, radius, bias, frame_rows=None, defect=None, brute=False, bvh=None):
    """-> (hits (rows, width) uint8, covered (rows, width))"""
    hit, covered, _ = image_ray_hits(tris, attrs, material, dirs, n_rays, P, radius, bias, frame_rows, defect, brute, bvh)
    return hit.sum(1).astype(np.uint8).reshape(material.shape), covered.reshape(material.shape)


def result(hits, n_rays, covered=None, defect=None):
    """the unfiltered result: (510 * (n_rays - hits) + n_rays) / (2 * n_rays)"""
    v = n_rays - hits.astype(np.int64)
    out = (255 * v) // n_rays if defect == "floor" else (510 * v + n_rays) // (2 * n_rays)
    if covered is not None:
        out = np.where(covered, out, 255)
    return out.astype(np.uint8)


def window(P, defect=None):
    lo = -(P // 2) + (1 if defect == "window_shift" and P > 1 else 0)
    return range(lo, lo + P)


def filtered(hits, covered, attrs, n_rays, P, normal_cos, plane_dist, defect=None):
    """the filtered result of a WHOLE frame: -> (result (rows, width) uint8, accepted (rows, width): pixels accepted, p included; 0 where p is not
    covered), cut (rows, width, 4): the window reaches over the frame's left, right, top, bottom border)"""
    rows, width = hits.shape
    m, _ = normal(attrs[..., 8:11].reshape(-1, 3))
    m, w = m.reshape(rows, width, 3), attrs[..., 11:14].astype(F)
    V, accepted = np.zeros((rows, width), np.int64), np.zeros((rows, width), np.int64)
    cut = np.zeros((rows, width, 4), bool)
    y, x = np.meshgrid(np.arange(rows), np.arange(width), indexing="ij")
    for j in window(P, defect):
        for i in window(P, defect):
            qy, qx = y + j, x + i
            cut[..., 0] |= qx < 0; cut[..., 1] |= qx >= width; cut[..., 2] |= qy < 0; cut[..., 3] |= qy >= rows
            inside = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
            qy, qx = np.clip(qy, 0, rows - 1), np.clip(qx, 0, width - 1)
            mq, wq = m[qy, qx], w[qy, qx]
            with np.errstate(all="ignore"):
                diff = [wq[..., a] - w[..., a] for a in range(3)]
                near = R._dot([m[..., a] for a in range(3)], [mq[..., a] for a in range(3)]) >= F(normal_cos)
                flat = np.abs(R._dot([m[..., a] for a in range(3)], diff)) <= F(plane_dist)
            ok = inside & covered[qy, qx] & near & flat
            if i == 0 and j == 0 and defect != "p_tested":
                ok = np.ones((rows, width), bool)
            V += np.where(ok, n_rays - hits[qy, qx].astype(np.int64), 0)
            accepted += ok
    T = n_rays * accepted
    with np.errstate(all="ignore"):
        out = np.where(T > 0, ((255 * V) // np.maximum(T, 1)) if defect == "floor" else (510 * V + T) // np.maximum(2 * T, 1), 0)
    return np.where(covered, out, 255).astype(np.uint8), np.where(covered, accepted, 0), cut


def tile_walks(ry, covered, rows, width, row0_in_tile=0):
    """per ray index k, the walks of the 8 x 8 tiles (ray_reference.tile_walks): -> list over k of lists over tiles of "plain" / "odd" / "none" """
    return [R.tile_walks(np.ascontiguousarray(ry[:, k]), covered, rows, width, row0_in_tile) for k in range(ry.shape[1])]


def cone_directions(n_rays, P, half_angle_deg, down=False, seed=0):
    """a table for the tests: unit directions inside a cone about local +z (-z: down), uniformly over its cap, each set drawn on its own"""
    rng = np.random.default_rng([seed, n_rays, P])
    cos_t = 1.0 - rng.random((P * P, n_rays)) * (1.0 - np.cos(np.radians(half_angle_deg)))
    phi = rng.random((P * P, n_rays)) * 2.0 * np.pi
    s = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    return np.stack([s * np.cos(phi), s * np.sin(phi), -cos_t if down else cos_t], -1).astype(F)
