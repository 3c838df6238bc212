"""What tests/test_cluster_bounds.py (CPU) and the reused-handle tests of tests/test_gpu_cluster_cull.py (GPU) share: the scenes and the camera
and sun sequences, a seeded permutation of a mesh's triangles, the two rules for a vertex block's box restated in numpy, and geometry.hip's
box_outside replayed in float64.  No device, no test in here.

The rules.  tbounds[c] bounds the positions of the valid triangles [256 c, 256 c + 256) (a workgroup of k_setup); infinite when one of them is
not finite or the cluster has no valid triangle.
  "clusters" (renderer.cpp: cluster_bounds, arctic_cluster_bounds): vbounds[b] = the union of tbounds[t // 256] over the valid triangles t that
      use a vertex of block b; infinite when no valid triangle does.
  "triangles" (what cluster_bounds did before): vbounds[b] = the union of the boxes of those triangles themselves; infinite when one of them
      holds a position that is not finite, or none uses the block.
k_vertex skips a block whose box is outside (strict = 2) and leaves its XVert slots as they were; k_setup keeps a cluster whose box is not
outside (strict = 1) and reads the slots of every valid triangle in it.  A HOLE is a valid triangle of a kept cluster with a vertex in a skipped
block.  Under "clusters" there is none (box_outside's comment in geometry.hip); under "triangles" the scenarios below have hundreds.
"""
import copy

import numpy as np

CLUSTER = 256          # SETUP_THREADS (common.h) and the 256 vertices of a workgroup of k_vertex
INF_BOX = np.float32([-np.inf] * 3 + [np.inf] * 3)

# ---- scenes and sequences ------------------------------------------------------------------------------------------------------------
QUAD_W, QUAD_H = 256, 144
CAMERA_A = dict(eye=(0.0, 0.0, 6.0), rotation=(0.0, -90.0), aspect=QUAD_W / QUAD_H, fov_y=45.0, z_near_far=(0.1, 50.0))      # looks down -z at the quad


def _cam(**kw):
    return dict(CAMERA_A, **kw)


# A shows the whole quad (every slot written with on-screen coordinates); the others turn or move away, so that blocks are skipped while clusters stay
QUAD_CAMERAS = [CAMERA_A, _cam(rotation=(35.0, -90.0)), CAMERA_A, _cam(eye=(0.0, 4.0, 6.0)), CAMERA_A, _cam(eye=(0.0, 5.0, 9.0))]
FRAME_ROTATIONS = [(-15.0, 0.0), (-15.0, 90.0), (40.0, 60.0), (-15.0, 0.0), (-15.0, 180.0)]      # config 3's camera, turned on the spot; the first is its own
SUN_ROTATIONS = [(-70.0, 12.0), (-30.0, 100.0), (-20.0, -60.0), (-70.0, 12.0)]                    # the first is DEFAULT_SUN's: its frustum holds the hall


# A box through the eye's plane.  The side planes of box_outside pass through the eye; two of them, one and two pixels outside the scissor, bound
# half-spaces of which neither holds the other: behind the eye the one-pixel plane's is the smaller.  While k_vertex tested its blocks against
# the two-pixel planes and k_setup its clusters against the one-pixel planes, a box with a corner behind the eye in the wedge between them was
# skipped as a block and kept as a cluster -- even when the two boxes are the SAME box, as for this wall of one cluster and one block beside
# the eye, 60 units long.  The sweep turns the camera through that wedge in steps of 0.02 degrees; WALL_VISIBLE looks straight at the wall.
WALL_VISIBLE = (0.0, -90.0)
WALL_SWEEP = [(0.0, round(-51.80 + 0.02 * k, 2)) for k in range(31)]      # -51.8 .. -51.2: the wedge is about 0.2 degrees wide around -51.4


def wall(S):
    """(vertices, indices): 200 triangles, 121 vertices at x = -1, z in [-30, 30], facing the eye at the origin"""
    return S.quad((-1.0, -0.5, -30.0), (0, 1.0, 0), (0, 0, 60.0), 10, 10)


def wall_camera(rotation):
    return dict(eye=(0.0, 0.0, 0.0), rotation=tuple(rotation), aspect=QUAD_W / QUAD_H, fov_y=45.0, z_near_far=(0.1, 100.0))


def small_quad(S):
    """(vertices, indices) of the 24 x 24 quad of test_objects_on_the_scissors_sides: 1152 triangles, 625 vertices"""
    return S.quad((-0.05, -0.05, 0.0), (0.1, 0, 0), (0, 0.1, 0), 24, 24)


def big_quad(S):
    """(vertices, indices) of the 48 x 48 quad that fills camera A's frame: 4608 triangles (18 clusters, rows of the quad), 2401 vertices (10 blocks)"""
    return S.quad((-4.0, -2.25, 0.0), (8.0, 0, 0), (0, 4.5, 0), 48, 48)


def permuted(indices, seed):
    """the same triangles in another order: nothing promises that a mesh's triangle order follows its vertex order"""
    t = np.asarray(indices, np.uint32).reshape(-1, 3)
    return np.ascontiguousarray(t[np.random.default_rng(seed).permutation(len(t))]).ravel()


def permuted_meshes(meshes, seed=1234):
    return [(v, permuted(i, seed + k)) + tuple(rest) for k, (v, i, *rest) in enumerate(meshes)]


def permuted_scene(sc, seed=1234):
    out = copy.copy(sc)
    out.meshes = permuted_meshes(sc.meshes, seed)
    return out


def quad_desc(S, camera):
    return S.SceneDesc(camera=camera, ambient=0.1, sun=S.DEFAULT_SUN, objects=S.make_objects([(np.eye(4), 0)]))


def with_camera_rotation(desc, rotation):
    d = copy.deepcopy(desc)
    d.camera["rotation"] = tuple(rotation)
    return d


def with_sun_rotation(desc, rotation):
    d = copy.deepcopy(desc)
    d.sun = dict(d.sun, rotation=tuple(rotation))
    return d


# ---- the two rules in numpy ----------------------------------------------------------------------------------------------------------
def _tables(vertices, indices):
    pos = np.asarray(vertices["position"], np.float32).reshape(-1, 3)
    tri = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    valid = (tri < len(pos)).all(1) if len(tri) else np.zeros(0, bool)
    return pos, tri, valid, (len(tri) + CLUSTER - 1) // CLUSTER, (len(pos) + CLUSTER - 1) // CLUSTER


def _empty(n):
    return np.full((n, 3), np.inf, np.float32), np.full((n, 3), -np.inf, np.float32)


def _close(lo, hi, bad):
    """boxes that are empty (never grown: min = inf > max = -inf) or marked bad become infinite"""
    box = np.concatenate([lo, hi], 1)
    box[bad | ~(lo[:, 0] <= hi[:, 0])] = INF_BOX
    return box


def cluster_boxes(vertices, indices):
    pos, tri, valid, n_tb, _ = _tables(vertices, indices)
    lo, hi = _empty(n_tb)
    bad = np.zeros(n_tb, bool)
    t = np.nonzero(valid)[0]
    p = pos[tri[t]]                                      # (m, 3 corners, xyz)
    np.minimum.at(lo, t // CLUSTER, np.fmin.reduce(p, 1))
    np.maximum.at(hi, t // CLUSTER, np.fmax.reduce(p, 1))
    np.logical_or.at(bad, t // CLUSTER, ~np.isfinite(p).all((1, 2)))
    return _close(lo, hi, bad)


def block_boxes(vertices, indices, rule):
    """vbounds under rule "clusters" (the library's) or "triangles" (the one it replaces)"""
    pos, tri, valid, _, n_vb = _tables(vertices, indices)
    lo, hi = _empty(n_vb)
    bad = np.zeros(n_vb, bool)
    t = np.nonzero(valid)[0]
    if rule == "clusters":
        tb = cluster_boxes(vertices, indices)
        src_lo, src_hi, src_bad = tb[t // CLUSTER, :3], tb[t // CLUSTER, 3:], np.zeros(len(t), bool)      # (an infinite cluster box carries through min / max)
    else:
        p = pos[tri[t]]
        src_lo, src_hi, src_bad = np.fmin.reduce(p, 1), np.fmax.reduce(p, 1), ~np.isfinite(p).all((1, 2))
    for j in range(3):
        b = tri[t, j] // CLUSTER
        np.minimum.at(lo, b, src_lo)
        np.maximum.at(hi, b, src_hi)
        np.logical_or.at(bad, b, src_bad)
    return _close(lo, hi, bad)


def uses(vertices, indices):
    """(cluster, block) pairs: the cluster holds a valid triangle with a vertex of the block"""
    _, tri, valid, _, _ = _tables(vertices, indices)
    t = np.nonzero(valid)[0]
    pairs = np.stack([np.repeat(t // CLUSTER, 3), (tri[t] // CLUSTER).ravel()], 1)
    return np.unique(pairs, axis=0) if len(pairs) else pairs


def contains(outer, inner):
    """component by component; an infinite box contains everything"""
    return bool((outer[:3] <= inner[:3]).all() and (outer[3:] >= inner[3:]).all())


def violations(tb, vb, vertices, indices):
    """the (cluster, block) pairs of `uses` whose block box does not contain the cluster's box"""
    return [(int(c), int(b)) for c, b in uses(vertices, indices) if not contains(vb[b], tb[c])]


# ---- box_outside (geometry.hip) in float64 -------------------------------------------------------------------------------------------
def box_outside(boxes, trs, clip_from_world, vp_w, vp_h, scissor, strict, side_pixels=1.0):
    """geometry.hip's box_outside for every box of `boxes` (n, 6): the same corners, planes, margins and E, in float64.  trs and clip_from_world
    are 16 floats in the library's order (m[4 col + row]); scissor = (x0, y0, x1, y1).  Infinite boxes are never outside.  side_pixels: how far
    the scissor's sides are moved out -- one pixel, for clusters and blocks alike; the kernel used to take `strict` pixels (WEDGE below)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    T, Cm = np.asarray(trs, np.float64).reshape(4, 4), np.asarray(clip_from_world, np.float64).reshape(4, 4)      # [col][row]
    lo, hi = boxes[:, :3], boxes[:, 3:]
    k = np.arange(8)
    pick = np.stack([k & 1, (k >> 1) & 1, (k >> 2) & 1], 1).astype(bool)                                         # corner k takes hi where bit set
    with np.errstate(invalid="ignore", over="ignore"):
        corner = np.where(pick[None], hi[:, None, :], lo[:, None, :])                                           # (n, 8, 3)
        c4 = np.concatenate([corner, np.ones(corner.shape[:2] + (1,))], -1)
        clip = (c4 @ T) @ Cm                                                                                    # row vector x [col][row] = mul(M, v)
        a4 = np.concatenate([np.maximum(np.abs(lo), np.abs(hi)), np.ones((len(boxes), 1))], -1)
        ac = (a4 @ np.abs(T)) @ np.abs(Cm)                                                                      # (n, 4): the sum of the magnitudes of the terms
        E = 4.0e-6 * strict
        ex, ey, ez, ew = (E * ac[:, i, None] for i in range(4))
        hx, hy = 0.5 * vp_w, 0.5 * vp_h
        x0, y0, x1, y1 = scissor
        xl, xr = (x0 - side_pixels) / hx - 1.0, (x1 + side_pixels) / hx - 1.0
        yt, yb = 1.0 - (y0 - side_pixels) / hy, 1.0 - (y1 + side_pixels) / hy
        x, y, z, w = (clip[..., i] for i in range(4))
        inside = [~(z < -ez), ~(z - w > ez + ew),
                  ~(x - xl * w < -(ex + abs(xl) * ew)), ~(x - xr * w > ex + abs(xr) * ew),
                  ~(y - yt * w > ey + abs(yt) * ew), ~(y - yb * w < -(ey + abs(yb) * ew))]
    return np.any([~p.any(1) for p in inside], 0)


def holes(meshes, objects, clip_from_world, vp_w, vp_h, scissor, tables):
    """(vertex blocks, blocks skipped, holes) of one pass: tables[mesh] = (tbounds, vbounds)"""
    n_blocks = n_skipped = n_holes = 0
    for o in objects:
        v, idx = meshes[int(o["mesh_idx"])][:2]
        tb, vb = tables[int(o["mesh_idx"])]
        trs = np.asarray(o["trs"], np.float32)
        kept = ~box_outside(tb, trs, clip_from_world, vp_w, vp_h, scissor, 1.0)
        skipped = box_outside(vb, trs, clip_from_world, vp_w, vp_h, scissor, 2.0)
        _, tri, valid, _, _ = _tables(v, idx)
        t = np.nonzero(valid)[0]
        n_holes += int((kept[t // CLUSTER] & skipped[tri[t] // CLUSTER].any(1)).sum())
        n_blocks += len(vb); n_skipped += int(skipped.sum())
    return n_blocks, n_skipped, n_holes
