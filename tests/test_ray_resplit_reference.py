"""The re-split on a machine without a GPU: the numpy definition (tests/ray_resplit_reference.py) and the library's host arbiter
arctic_resplit_triangles -- bvh.cpp's bvh_resplit -- against each other, against a full build of the moved triangles (arctic_refit_triangles(B, B):
with every triangle finite a re-split structure IS that build's) and against the loop over every triangle, bit for bit.

Sizes: 1, 4 (one leaf), 5 (a root and two leaves), 8, 9, 255, 256, 257 (64 / 65 leaves: one and two treelets of the refit), 4097, 16385 (4097
leaves: a third refit stage)."""
import numpy as np
import pytest

import ray_reference as R
import ray_refit_reference as RR
import ray_resplit_reference as RS
from test_ray_refit_reference import changed

F = np.float32
NONE = R.NO_PRIM
TRI_COUNTS = [1, 4, 5, 8, 9, 255, 256, 257, 4097, 16385]
CHANGES = ["rigid", "reversed", "same", "displaced"]
NO_RAYS = np.zeros(0, R.RAY_DTYPE)

_CASES = {}


def case(n_tris, how):
    key = (n_tris, how)
    if key not in _CASES:
        rng = np.random.default_rng(47000 + 10 * n_tris + CHANGES.index(how))
        a = R.soup_triangles(rng, n_tris)
        b = changed(rng, a, how)
        _CASES[key] = (a, b, R.soup_rays(rng, b, 257))
    return _CASES[key]


def raw(tris):
    return np.concatenate([tris["p0"], tris["p1"], tris["p2"]], 1) if len(tris) else np.zeros((0, 9), F)


def same_structure(got, want):
    """triangles, skip and leaf by bytes, boxes by value (the sign of a zero bound is not defined)"""
    (nodes, tris), (wn, wt) = got, want
    assert len(nodes) == len(wn) and len(tris) == len(wt)
    assert nodes["skip"].tobytes() == wn["skip"].tobytes() and nodes["leaf"].tobytes() == wn["leaf"].tobytes()
    assert tris.tobytes() == wt.tobytes()
    assert (nodes["bmin"] == wn["bmin"]).all() and (nodes["bmax"] == wn["bmax"]).all()


def against_numpy(pkg, a, b, defect=None):
    """the library's re-split of A's tree to B against the numpy definition's -> (nodes, tris, numpy tree)"""
    _, nodes, tris = pkg.renderer.resplit_triangles(a, b, NO_RAYS, structure=True)
    tree = RS.resplit(R.build_bvh(a), b, defect=defect)
    ok = (len(tris) == len(tree.prims) and (tris["prim"] == tree.prims).all() and raw(tris).tobytes() == tree.tris.tobytes()
          and (nodes["skip"] == tree.skip).all() and ((nodes["leaf"] & 7) == tree.count).all()
          and ((nodes["leaf"] >> 3)[tree.count > 0] == tree.first[tree.count > 0]).all()
          and (nodes["bmin"] == tree.bmin).all() and (nodes["bmax"] == tree.bmax).all())
    return ok, nodes, tris, tree


@pytest.mark.parametrize("how", CHANGES)
@pytest.mark.parametrize("n_tris", TRI_COUNTS)
def test_resplit_equals_a_build_of_the_moved_triangles(pkg, n_tris, how):
    a, b, rays = case(n_tris, how)
    _, nodes, tris = pkg.renderer.resplit_triangles(a, b, NO_RAYS, structure=True)
    _, fresh_nodes, fresh_tris = pkg.renderer.refit_triangles(b, b, NO_RAYS, structure=True)     # a build on B
    same_structure((nodes, tris), (fresh_nodes, fresh_tris))
    ok, _, _, tree = against_numpy(pkg, a, b)
    assert ok
    fresh = R.build_bvh(b)                                                                  # numpy's own build of B: the same order, too
    assert (tree.prims == fresh.prims).all() and tree.tris.tobytes() == fresh.tris.tobytes()
    assert (tree.bmin == fresh.bmin).all() and (tree.bmax == fresh.bmax).all()
    for any_hit in (False, True):                                                           # the walk over it: the loop over every triangle of B
        want = pkg.renderer.trace_triangles(b, rays, any_hit=any_hit, brute=True) if n_tris > 1000 else R.brute(b, rays, any_hit=any_hit)
        assert pkg.renderer.resplit_triangles(a, b, rays, any_hit=any_hit).tobytes() == want.tobytes()
        assert pkg.renderer.resplit_triangles(a, b, rays, any_hit=any_hit, brute=True).tobytes() == want.tobytes()
        if not any_hit:                                                                     # not vacuous (a handful of triangles is hit by few rays)
            assert (want["prim"] != NONE).sum() * (4 if n_tris >= 255 else 64) >= len(rays)
    if how != "same" and n_tris > 8:                                                        # ... and the order did change: a refit is another structure
        _, _, refitted = pkg.renderer.refit_triangles(a, b, NO_RAYS, structure=True)
        assert refitted["prim"].tobytes() != tris["prim"].tobytes()


def lattice(rng, nx, ny, nz, step=(1.0, 1.0, 1.0)):
    """one small triangle per lattice point, in a shuffled order: whole planes of equal centroid coordinates"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(F) * np.array(step, F)
    shape = np.array([[0, 0, 0], [0.25, 0, 0.125], [0, 0.25, 0.125]], F)
    t = (g[:, None, :] + shape[None]).astype(F)
    return t[rng.permutation(len(t))].reshape(-1, 9)


def tie_cases():
    rng = np.random.default_rng(99)
    cases = {}
    cases["lattice"] = lattice(rng, 5, 4, 3)                                                # 60 triangles, 5 planes along the split axis
    soup = R.soup_triangles(rng, 40)
    cases["duplicates"] = np.concatenate([soup, soup[::2], soup[:7], soup[:7]])[rng.permutation(74)]
    z = np.zeros((9, 3, 3), F)                                                              # centroids -0 and +0 on the split axis, between others
    z[:, :, 1] = np.array([0, 0.25, 0.5], F)[None, :] + np.arange(9, dtype=F)[:, None] * F(0.001)
    x = np.array([-0.0, 0.0, -0.0, 0.0, 1.0, 2.0, -1.0, -2.0, 0.0], F)
    z[:, :, 0] = x[:, None]
    cases["signed_zeros"] = z.reshape(-1, 9)
    flat = np.zeros((12, 3, 3), F)                                                          # every centroid (+-0, 0, 0): no extent on any axis, prims decide
    flat[:, :, 0] = np.where(np.arange(12) % 3 == 0, F(0.0), F(-0.0))[:, None]
    cases["all_zero"] = flat.reshape(-1, 9)
    cases["extents_equal_xyz"] = lattice(rng, 3, 3, 3)
    cases["extents_equal_yz"] = lattice(rng, 2, 4, 4)
    cases["extents_equal_xz"] = lattice(rng, 4, 2, 4)
    return cases


@pytest.mark.parametrize("name", ["lattice", "duplicates", "signed_zeros", "all_zero", "extents_equal_xyz", "extents_equal_yz", "extents_equal_xz"])
def test_ties_fall_to_the_prim_and_to_the_lowest_axis(pkg, name):
    b = tie_cases()[name]
    a = R.soup_triangles(np.random.default_rng(len(b)), len(b))                             # the tree was split for something else entirely
    ok, nodes, tris, tree = against_numpy(pkg, a, b)
    assert ok
    _, fresh_nodes, fresh_tris = pkg.renderer.refit_triangles(b, b, NO_RAYS, structure=True)
    same_structure((nodes, tris), (fresh_nodes, fresh_tris))
    assert sorted(tris["prim"].tolist()) == list(range(len(b)))


def test_the_numpy_definition_tells_the_defects_apart(pkg):
    """each deviation changes the order on at least one of the tie cases (or the dead case), where the library agrees with the definition"""
    cases = tie_cases()
    dead = cases["lattice"].copy()
    dead[[3, 17, 18, 40], 4] = np.nan
    cases["dead"] = dead
    where = {"tie_larger": ["lattice", "duplicates", "all_zero"], "axis_ge": ["extents_equal_xyz", "extents_equal_yz", "extents_equal_xz"],
             "neg_zero_less": ["signed_zeros", "all_zero"], "dead_first": ["dead"], "leaf_unsorted": ["lattice", "duplicates"]}
    assert set(where) == set(RS.DEFECTS)
    for defect, names in where.items():
        for name in names:
            b = cases[name]
            prims = np.arange(len(b))
            right, wrong = RS.slot_order(prims, b), RS.slot_order(prims, b, defect=defect)
            assert right.tolist() != wrong.tolist(), (defect, name)
            a = R.soup_triangles(np.random.default_rng(7), len(b))
            assert against_numpy(pkg, a, b)[0] and not against_numpy(pkg, a, b, defect=defect)[0], (defect, name)


def dead_cases():
    rng = np.random.default_rng(123)
    a = R.soup_triangles(rng, 257)
    b = changed(rng, a, "rigid")
    one = b.copy(); one[100, 2] = np.inf
    leaf = b.copy(); leaf[[5, 50, 99, 200, 256], 0] = np.nan; leaf[50, 7] = -np.inf       # five dead: they fill the last two leaves (2 and 3 slots)
    every = np.full_like(b, np.nan); every[::2] = np.inf
    return a, b, {"one": one, "leaf": leaf, "every": every}


@pytest.mark.parametrize("name", ["one", "leaf", "every"])
def test_dead_triangles_order_last_and_come_back(pkg, name):
    a, b_finite, cases = dead_cases()
    b = cases[name]
    ok, nodes, tris, tree = against_numpy(pkg, a, b)
    assert ok
    gone = np.nonzero(~np.isfinite(b).all(1))[0]
    n_dead = len(gone)
    # behind every live one in every segment: the dead fill the last slots, but for the leaf that also holds live ones (a leaf is ordered by prim)
    firsts = (nodes["leaf"] >> 3)[(nodes["leaf"] & 7) != 0].astype(np.int64)
    start = int(firsts[firsts <= len(tris) - n_dead].max())
    at = np.nonzero(np.isin(tris["prim"], gone))[0]
    assert len(at) == n_dead and at.min() >= start
    assert (raw(tris).view(np.uint32)[at] == RR.DEAD_BITS).all() and np.isfinite(np.delete(raw(tris), at, 0)).all()
    empty = int((nodes["bmin"][:, 0] == np.inf).sum())
    assert empty == {"one": 0, "leaf": 3, "every": len(nodes)}[name]
    if name == "leaf":                                                                      # 257 slots end in leaves of 2 and 3 under one node: all three empty
        last = np.nonzero(nodes["leaf"] & 7)[0][-2:]
        assert (nodes["leaf"][last] & 7).tolist() == [2, 3] and (nodes["bmin"][last] == np.inf).all() and (nodes["bmax"][last] == -np.inf).all()
        assert (nodes["bmin"][last[0] - 1] == np.inf).all() and tris["prim"][-5:].tolist() == [5, 50, 99, 200, 256]
    if name == "every":
        assert tris["prim"].tolist() == list(range(len(b)))
    rays = R.soup_rays(np.random.default_rng(5), b_finite, 257)
    for any_hit in (False, True):
        want = R.brute(b, rays, any_hit=any_hit)
        assert pkg.renderer.resplit_triangles(a, b, rays, any_hit=any_hit).tobytes() == want.tobytes()
        assert R.walk(tree, rays, any_hit=any_hit)[0].tobytes() == want.tobytes()
    # a following refit to finite vertices revives the dead slots: the order stays, every slot is B's triangle again, no box is empty
    back = RR.refit(tree, b_finite)
    assert (back.prims == tree.prims).all() and back.tris.tobytes() == b_finite[tree.prims].tobytes() and np.isfinite(back.bmin).all()
    for any_hit in (False, True):
        assert R.walk(back, rays, any_hit=any_hit)[0].tobytes() == R.brute(b_finite, rays, any_hit=any_hit).tobytes()
