"""The arbiter of the re-split: include/arctic_hip.h's "a re-split structure" restated in numpy float32 on top of ray_reference.py and
ray_refit_reference.py -- from the header's text, not from the library's C++.

  slot_order(prims, tris_now)   the stored prims in the order of the slots: the builder's recursion applied to the triangles as they are now.
                                Per segment the axis of the widest centroid extent over its live members (fp32 cmax - cmin, strict >, the
                                lowest axis on a tie, axis 0 without a live member); the members by (centroid[axis], prim), -0 == +0, dead ones
                                last by prim; the lower half left; a segment of at most four slots is a leaf, ordered by prim.
  resplit(bvh, tris_now)        a tree built on A (ray_reference.build_bvh) re-split to B: A's topology, slot_order's prims, then the refit of
                                ray_refit_reference (slot contents, dead slots, boxes).

`defect` names a deliberate deviation, so that the tests can show that they tell the definition from it:
  "tie_larger"      equal centroids fall to the LARGER prim         "axis_ge"        >= in the choice of the axis: the highest axis on a tie
  "neg_zero_less"   -0 orders before +0                             "dead_first"     dead triangles order before the live ones
  "leaf_unsorted"   a leaf keeps the order its parent's split left it in
"""
import copy

import numpy as np

import ray_reference as R
import ray_refit_reference as RR

F = np.float32
DEFECTS = ("tie_larger", "axis_ge", "neg_zero_less", "dead_first", "leaf_unsorted")


def centroids(tris_now, prims):
    """(centroid (m, 3), live (m,)) of the stored triangles: the box's, 0.5f * lo + 0.5f * hi per axis, each operation rounding once"""
    t = np.ascontiguousarray(tris_now, F).reshape(-1, 9)[np.asarray(prims, np.int64)].reshape(-1, 3, 3)
    live = np.isfinite(t).all((1, 2))
    with np.errstate(all="ignore"):
        lo, hi = R._min(R._min(t[:, 0], t[:, 1]), t[:, 2]), R._max(R._max(t[:, 0], t[:, 1]), t[:, 2])
        c = F(0.5) * lo + F(0.5) * hi
    return np.where(live[:, None], c, F(0)).astype(F), live


def split_axis(c, defect=None):
    """c: the live members' centroids (k, 3), k >= 1"""
    with np.errstate(all="ignore"):
        ext = c.max(0) - c.min(0)                       # fp32; may overflow to +inf, which still orders
    axis, widest = 0, ext[0]
    for a in (1, 2):
        if (ext[a] >= widest) if defect == "axis_ge" else (ext[a] > widest):
            axis, widest = a, ext[a]
    return axis


def slot_order(prims, tris_now, leaf=4, defect=None):
    prims = np.asarray(prims, np.int64)
    cen, live = centroids(tris_now, prims)
    out = []

    def rec(ids):
        if len(ids) <= leaf:
            out.extend((ids if defect == "leaf_unsorted" else ids[np.argsort(prims[ids], kind="stable")]).tolist())
            return
        lv = ids[live[ids]]
        axis = split_axis(cen[lv], defect) if len(lv) else 0
        key = cen[ids, axis].astype(np.float64)
        if defect == "neg_zero_less":
            key = np.where((key == 0) & np.signbit(key), -1e-300, key)
        else:
            key = np.where(key == 0, 0.0, key)          # -0 == +0
        key = np.where(live[ids], key, 0.0)             # among dead triangles the prim alone
        dead = ~live[ids]
        first = live[ids] if defect == "dead_first" else dead
        tie = -prims[ids] if defect == "tie_larger" else prims[ids]
        ids = ids[np.lexsort((tie, key, first))]
        rec(ids[:len(ids) // 2]); rec(ids[len(ids) // 2:])

    if len(prims):
        rec(np.arange(len(prims)))
    return prims[np.array(out, np.int64)] if len(out) else prims


def resplit(bvh, tris_now, defect=None):
    """the definition: a copy of `bvh` (built on other triangles) re-split to tris_now"""
    b = copy.copy(bvh)
    b.prims = slot_order(bvh.prims, tris_now, defect=defect)
    return RR.refit(b, tris_now)
