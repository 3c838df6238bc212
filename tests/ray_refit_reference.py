"""The arbiter of the refit: include/arctic_hip.h's "a refitted structure" restated in numpy float32 on top of ray_reference.py -- from the
header's text, not from the library's C++.

  refit(bvh, tris_now)     a tree built on A (ray_reference.build_bvh) refitted to triangles B: the topology, the slot order and the prims stay;
                           slot k takes B[prim] -- nine quiet NaNs when a float of it is not finite --; a leaf's box is the union of its live
                           slots (the empty box +inf / -inf without one), an interior box the union of its two children's.
  subtree_boxes(...)       for every node the union over the live slots of its whole subtree, straight from the slots: what every box must equal
                           BY VALUE whatever order the unions were formed in (min / max of finite floats are exact; the sign of a zero is not defined).
  ray_reference.walk runs on the result as it stands: a dead slot fails ray_triangle's finite test, an empty box is missed or visited in vain.
"""
import copy

import numpy as np

import ray_reference as R

F = np.float32
DEAD_BITS = 0x7FC00000
NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("skip", "<u4"), ("bmax", "<f4", 3), ("leaf", "<u4")])
TRI_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("p2", "<f4", 3), ("prim", "<u4"), ("pad", "<u4", 2)])


def dead_triangle():
    return np.full(9, DEAD_BITS, np.uint32).view(F)


def slots_now(prims, tris_now):
    """the slots' contents: B[prim], dead where a float is not finite"""
    t = np.ascontiguousarray(tris_now, F).reshape(-1, 9)[np.asarray(prims, np.int64)].copy()
    t[~np.isfinite(t).all(1)] = dead_triangle()
    return t


def slot_ranges(skip, first, count):
    """per node the slots of its subtree [s0, s1): the nodes are depth-first and the slots are stored by leaf in the same order"""
    n = len(skip)
    s0, s1 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        if count[i]:
            s0[i], s1[i] = first[i], first[i] + count[i]
        else:
            s0[i], s1[i] = s0[i + 1], s1[skip[i + 1]]
    return s0, s1


def subtree_boxes(skip, first, count, slots):
    """(bmin, bmax) per node: the union over the live slots of the subtree; +inf / -inf where it has none"""
    n = len(skip)
    t = np.ascontiguousarray(slots, F).reshape(-1, 3, 3)
    live = np.isfinite(t).all((1, 2))
    lo = np.where(live[:, None], t.min(1), np.inf).astype(F)
    hi = np.where(live[:, None], t.max(1), -np.inf).astype(F)
    s0, s1 = slot_ranges(skip, first, count)
    bmin, bmax = np.full((n, 3), np.inf, F), np.full((n, 3), -np.inf, F)
    for i in range(n):
        bmin[i], bmax[i] = lo[s0[i]:s1[i]].min(0), hi[s0[i]:s1[i]].max(0)
    return bmin, bmax


def refit(bvh, tris_now):
    """the definition: a copy of `bvh` (built on other triangles) refitted to tris_now.  The unions are formed as the header words them: leaves
    from their live slots, interior nodes from their two children, children before parents"""
    b = copy.copy(bvh)
    b.tris = slots_now(bvh.prims, tris_now)
    n = len(b.skip)
    t = b.tris.reshape(-1, 3, 3)
    live = np.isfinite(t).all((1, 2))
    b.bmin, b.bmax = np.full((n, 3), np.inf, F), np.full((n, 3), -np.inf, F)
    for i in range(n - 1, -1, -1):
        if b.count[i]:
            for k in range(b.first[i], b.first[i] + b.count[i]):
                if live[k]:
                    b.bmin[i], b.bmax[i] = np.minimum(b.bmin[i], t[k].min(0)), np.maximum(b.bmax[i], t[k].max(0))
        else:
            for c in (i + 1, b.skip[i + 1]):
                b.bmin[i], b.bmax[i] = np.minimum(b.bmin[i], b.bmin[c]), np.maximum(b.bmax[i], b.bmax[c])
    return b


def check_structure(nodes, tris, build_nodes, build_tris, tris_now):
    """a structure the library returned (NODE_DTYPE, TRI_DTYPE) against the definition: topology and prims those of the build, slots B's triangles
    by bytes (dead ones nine 0x7FC00000), every box the union over its subtree's live slots by value.  -> number of empty boxes"""
    assert len(nodes) == len(build_nodes) and len(tris) == len(build_tris)
    assert (nodes["skip"] == build_nodes["skip"]).all() and (nodes["leaf"] == build_nodes["leaf"]).all()
    assert (tris["prim"] == build_tris["prim"]).all() and not tris["pad"].any()
    got = np.concatenate([tris["p0"], tris["p1"], tris["p2"]], 1).astype(F) if len(tris) else np.zeros((0, 9), F)
    want = slots_now(tris["prim"], tris_now) if len(tris) else got
    assert got.tobytes() == want.tobytes()
    count, first = (nodes["leaf"] & 7).astype(np.int64), (nodes["leaf"] >> 3).astype(np.int64)
    bmin, bmax = subtree_boxes(nodes["skip"].astype(np.int64), first, count, got)
    assert (nodes["bmin"] == bmin).all() and (nodes["bmax"] == bmax).all()          # by value: -0 == +0
    return int((bmin[:, 0] == np.inf).sum())
