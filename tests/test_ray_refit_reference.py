"""The refit on a machine without a GPU: the numpy definition (tests/ray_refit_reference.py) and the library's host arbiter
arctic_refit_triangles -- bvh.cpp's bvh_refit, the same ray_query.h functions the kernels of ray_refit.hip run -- against the loop over every
triangle, bit for bit.  A tree built on A and refitted to B must answer exactly as brute force on B, however poor it has become.

Sizes: 1 (one leaf), 4, 5 (a root and two leaves), 256 (exactly 64 leaves: one treelet), 257 (65 leaves: two stages), 1000, 16385 (4097 leaves:
three stages).  Rays: 1, 63, 64, 65, 1000 -- prefixes of one list of 1000 per case, since a ray's answer does not depend on its neighbours."""
import numpy as np
import pytest

import ray_reference as R
import ray_refit_reference as RR

F = np.float32
NONE = R.NO_PRIM
TRI_COUNTS = [1, 4, 5, 256, 257, 1000, 16385]
RAY_COUNTS = [1, 63, 64, 65, 1000]
CHANGES = ["rigid", "displaced", "same", "reversed"]


def changed(rng, a, how):
    """B = A under one of four changes (fp32 throughout)"""
    t = a.reshape(-1, 3, 3)
    if how == "rigid":
        c, s = F(np.cos(0.9)), F(np.sin(0.9))
        rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], F)
        return ((t @ rot.T).astype(F) + np.array([0.75, -0.5, 1.25], F)).astype(F).reshape(-1, 9)
    if how == "displaced":                               # a large random move per VERTEX: the tree is then poor, and must stay exact
        return (t + rng.uniform(-3, 3, t.shape).astype(F)).astype(F).reshape(-1, 9)
    if how == "same":
        return a.copy()
    return a[::-1].copy()                                # triangle k goes where triangle n - 1 - k was: the order in space reversed


_CASES = {}


def case(n_tris, how):
    key = (n_tris, how)
    if key not in _CASES:
        rng = np.random.default_rng(31000 + 10 * n_tris + CHANGES.index(how))
        a = R.soup_triangles(rng, n_tris)
        b = changed(rng, a, how)
        _CASES[key] = (a, b, R.soup_rays(rng, b, 1000))
    return _CASES[key]


def library_brute(pkg, tris, rays, any_hit):
    return pkg.renderer.trace_triangles(tris, rays, any_hit=any_hit, brute=True)       # pinned to numpy by tests/test_ray_query_abi.py


@pytest.mark.parametrize("how", CHANGES)
@pytest.mark.parametrize("n_tris", TRI_COUNTS)
def test_refit_triangles_equals_brute_force_on_the_moved_triangles(pkg, n_tris, how):
    a, b, rays = case(n_tris, how)
    want = {}
    for any_hit in (False, True):
        want[any_hit] = library_brute(pkg, b, rays, any_hit) if n_tris > 1000 else R.brute(b, rays, any_hit=any_hit)
    if n_tris == 1000:
        assert library_brute(pkg, b, rays, False).tobytes() == want[False].tobytes()
    for n_rays in RAY_COUNTS:
        for any_hit in (False, True):
            got = pkg.renderer.refit_triangles(a, b, rays[:n_rays], any_hit=any_hit)
            assert got.tobytes() == want[any_hit][:n_rays].tobytes(), (n_rays, any_hit)
            flat = pkg.renderer.refit_triangles(a, b, rays[:n_rays], any_hit=any_hit, brute=True)
            assert flat.tobytes() == want[any_hit][:n_rays].tobytes()
    hit = want[False]["prim"] != NONE
    assert hit.sum() * 4 >= len(rays) and (want[False]["prim"][hit] < n_tris).all()        # not vacuous
    assert ((want[True]["prim"] == 0) == hit).all()
    # the structure: B's triangles by bytes, boxes by value, the build's topology
    _, nodes0, tris0 = pkg.renderer.refit_triangles(a, a, rays[:1], structure=True)        # refitted to itself: the build
    _, nodes, tris = pkg.renderer.refit_triangles(a, b, rays[:1], structure=True)
    assert RR.check_structure(nodes0, tris0, nodes0, tris0, a) == 0
    assert RR.check_structure(nodes, tris, nodes0, tris0, b) == 0
    leaves = int(((nodes["leaf"] & 7) != 0).sum())
    assert leaves == {1: 1, 4: 1, 5: 2, 256: 64, 257: 65, 1000: 256, 16385: 4097}[n_tris]
    assert len(tris) == n_tris and sorted(tris["prim"].tolist()) == list(range(n_tris))
    if how == "same":
        assert nodes.tobytes() == nodes0.tobytes() or ((nodes["bmin"] == nodes0["bmin"]).all() and (nodes["bmax"] == nodes0["bmax"]).all())
        assert tris.tobytes() == tris0.tobytes()


@pytest.mark.parametrize("how", CHANGES)
@pytest.mark.parametrize("n_tris", [1, 5, 257, 1000])
def test_the_definition_in_numpy(pkg, n_tris, how):
    """the numpy refit of a numpy tree: walks to brute force on B, and is the structure the library returns"""
    a, b, rays = case(n_tris, how)
    rays = rays[:257]
    tree = RR.refit(R.build_bvh(a), b)
    for any_hit in (False, True):
        want = R.brute(b, rays, any_hit=any_hit)
        got, visits = R.walk(tree, rays, any_hit=any_hit)
        assert got.tobytes() == want.tobytes()
    _, nodes, tris = pkg.renderer.refit_triangles(a, b, rays[:1], structure=True)
    assert (nodes["skip"] == tree.skip).all() and ((nodes["leaf"] & 7) == tree.count).all()
    assert ((nodes["leaf"] >> 3)[tree.count > 0] == tree.first[tree.count > 0]).all() and (tris["prim"] == tree.prims).all()
    assert np.concatenate([tris["p0"], tris["p1"], tris["p2"]], 1).tobytes() == tree.tris.tobytes()
    assert (nodes["bmin"] == tree.bmin).all() and (nodes["bmax"] == tree.bmax).all()


def dead_case(n_tris=257):
    rng = np.random.default_rng(77)
    a = R.soup_triangles(rng, n_tris)
    b = changed(rng, a, "rigid")
    build = R.build_bvh(a)
    leaf = int(np.nonzero(build.count == 4)[0][3])                                       # a full leaf: all four of its triangles die
    dead = build.prims[build.first[leaf]:build.first[leaf] + 4]
    former = (build.bmin[leaf].copy(), build.bmax[leaf].copy())
    b[dead, 0] = np.nan
    b[dead[1], 4] = np.inf
    other = np.setdiff1d(np.arange(n_tris), dead)[::17]                                  # and single slots of other leaves, by NaN and by infinities
    b[other[0::2], 8] = -np.inf
    b[other[1::2], 3] = np.nan
    rays = R.soup_rays(rng, b[np.isfinite(b).all(1)], 400)
    # rays with zero direction components, and origins inside the dead leaf's former box (in A's space: where the build put it)
    inside = (former[0] + (former[1] - former[0]) * rng.uniform(0.1, 0.9, (60, 3))).astype(F)
    d = rng.uniform(-1, 1, (60, 3)).astype(F)
    d[0:20, 0] = 0
    d[20:40, 1:] = 0
    extra = R.make_rays(inside, d)
    zero = rays[:60].copy()
    zero["direction"][:30, 2] = 0
    zero["direction"][30:, :2] = 0
    return a, b, np.concatenate([rays, extra, zero]), leaf, dead


def test_dead_slots_are_never_hit_and_boxes_go_empty(pkg):
    a, b, rays, leaf, dead = dead_case()
    for any_hit in (False, True):
        want = R.brute(b, rays, any_hit=any_hit)
        assert pkg.renderer.refit_triangles(a, b, rays, any_hit=any_hit).tobytes() == want.tobytes()
        got, _ = R.walk(RR.refit(R.build_bvh(a), b), rays, any_hit=any_hit)
        assert got.tobytes() == want.tobytes()
    want = R.brute(b, rays)
    assert (want["prim"] != NONE).sum() * 4 >= len(rays) and not np.isin(want["prim"], np.nonzero(~np.isfinite(b).all(1))[0]).any()
    _, nodes0, tris0 = pkg.renderer.refit_triangles(a, a, rays[:1], structure=True)
    _, nodes, tris = pkg.renderer.refit_triangles(a, b, rays[:1], structure=True)
    assert RR.check_structure(nodes, tris, nodes0, tris0, b) == 1                        # exactly the leaf whose four triangles died
    assert (nodes["bmin"][leaf] == np.inf).all() and (nodes["bmax"][leaf] == -np.inf).all()
    gone = np.isin(tris["prim"], np.nonzero(~np.isfinite(b).all(1))[0])
    assert gone.sum() == (~np.isfinite(b).all(1)).sum() > 4
    raw = np.concatenate([tris["p0"], tris["p1"], tris["p2"]], 1).view(np.uint32)
    assert (raw[gone] == RR.DEAD_BITS).all() and np.isfinite(raw[~gone].view(F)).all()
    # a dead triangle against rq_triangle's two cases, in numpy: some d == 0, and every d != 0
    nan9 = RR.dead_triangle().reshape(1, 9)
    probes = R.make_rays([[0, 0, 0], [0, 0, 0]], [[0, 1, 0], [1, 2, 3]], -np.inf, np.inf)
    assert (R.brute(nan9, probes)["prim"] == NONE).all() and (pkg.renderer.refit_triangles(a[:1], nan9, probes)["prim"] == NONE).all()


def test_every_triangle_dead_and_back(pkg):
    a, b, rays, _, _ = dead_case()
    nothing = np.full_like(b, np.nan)
    nothing[::3] = np.inf
    for any_hit in (False, True):
        got = pkg.renderer.refit_triangles(a, nothing, rays, any_hit=any_hit)
        assert (got["prim"] == NONE).all() and not got["t"].any()
    _, nodes0, tris0 = pkg.renderer.refit_triangles(a, a, rays[:1], structure=True)
    _, nodes, tris = pkg.renderer.refit_triangles(a, nothing, rays[:1], structure=True)
    assert RR.check_structure(nodes, tris, nodes0, tris0, nothing) == len(nodes)          # every box empty, the root's included
    # "back to life" is the same statement read the other way: a refit depends on the build's topology and on B alone
    _, nodes1, tris1 = pkg.renderer.refit_triangles(a, a, rays[:1], structure=True)
    assert nodes1.tobytes() == nodes0.tobytes() and tris1.tobytes() == tris0.tobytes()


def test_a_build_with_non_finite_triangles_refits_what_it_stored(pkg):
    """the arbiter builds on A as arctic_trace_triangles does: A's non-finite triangles get no slot, so they cannot come back -- which is why the
    handle does not refit such a build (tests/test_gpu_ray_refit.py); the stored ones still follow B exactly"""
    a, b, rays, _, dead = dead_case()
    a2 = a.copy()
    a2[dead] = np.nan
    b2 = changed(np.random.default_rng(3), a, "rigid")                                   # finite everywhere, the dropped ones included
    _, nodes, tris = pkg.renderer.refit_triangles(a2, b2, rays[:1], structure=True)
    assert len(tris) == len(a) - len(dead) and not np.isin(tris["prim"], dead).any()
    keep = np.ones(len(a), bool); keep[dead] = False
    masked = b2.copy(); masked[~keep] = np.nan
    assert pkg.renderer.refit_triangles(a2, b2, rays).tobytes() == R.brute(masked, rays).tobytes()
