"""Pins tests/ray_reference.py, the numpy float32 arbiter of the ray queries (include/arctic_hip.h, "ray queries"): rays against one triangle with
results worked out by hand, the edge cases of the definition, and -- for each deliberate defect the arbiter can be asked to carry -- a case whose
result the defect changes, so that a library with that defect cannot pass the bit-for-bit comparisons of the other ray tests."""
import numpy as np
import pytest

import ray_reference as R

F = np.float32
MISS = (0.0, 0.0, 0.0, R.NO_PRIM)
# a triangle in the plane z = 2 (axis-aligned: its box has no thickness in z), legs of length 4 along x and y.  For a ray (x, y, 0) + t (0, 0, 1):
# pv = (-4, 0, 0), det = -16, u = x / 4, v = y / 4, tm = 2 -- all exact in fp32 for the coordinates used here -- and the slab gives t = 2 as well
TRI = np.array([[0, 0, 2, 4, 0, 2, 0, 4, 2]], F)
EPS = 2.0 ** -20


def up(x, y, z=0.0, **kw):
    return R.make_rays([[x, y, z]], [[0, 0, 1]], **kw)


def one(hits):
    assert len(hits) == 1
    return tuple(hits[0].tolist())


def both(tris, rays, **kw):
    """brute force and the walk over the arbiter's own tree agree; -> the hits"""
    b = R.brute(tris, rays, **kw)
    w, _ = R.walk(R.build_bvh(tris), rays, **kw)
    assert w.tobytes() == b.tobytes()
    return b


@pytest.mark.parametrize("x,y,u,v", [(1, 1, 0.25, 0.25),                               # inside
                                     (0, 0, 0, 0), (4, 0, 1, 0), (0, 4, 0, 1),          # each vertex
                                     (2, 0, 0.5, 0), (0, 2, 0, 0.5), (2, 2, 0.5, 0.5)])  # each edge midpoint
def test_hits_worked_out_by_hand(x, y, u, v):
    assert one(both(TRI, up(x, y))) == (2.0, u, v, 0)
    assert one(both(TRI, up(x, y), any_hit=True)) == (0.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("x,y", [(2, -EPS), (-EPS, 2), (2 + EPS, 2 + EPS), (4 + EPS, 0), (0, 4 + EPS)])
def test_just_outside_each_edge_is_a_miss(x, y):
    assert one(both(TRI, up(x, y))) == MISS
    assert one(both(TRI, up(x, y), any_hit=True)) == MISS


def test_interval_ends_are_inclusive_and_hits_behind_the_origin_need_t_min():
    assert one(both(TRI, up(1, 1, 5.0))) == MISS                                       # t = -3 < t_min = 0
    assert one(both(TRI, up(1, 1, 5.0, t_min=-np.inf))) == (-3.0, 0.25, 0.25, 0)
    assert one(both(TRI, up(1, 1, t_min=2.0))) == (2.0, 0.25, 0.25, 0)                  # exactly at t_min
    assert one(both(TRI, up(1, 1, t_max=2.0))) == (2.0, 0.25, 0.25, 0)                  # exactly at t_max
    assert one(both(TRI, up(1, 1, t_min=2.0, t_max=2.0))) == (2.0, 0.25, 0.25, 0)
    assert one(both(TRI, up(1, 1, t_min=np.nextafter(F(2), F(3))))) == MISS
    assert one(both(TRI, up(1, 1, t_max=np.nextafter(F(2), F(1))))) == MISS
    # the defect: open ends lose exactly these
    assert one(R.brute(TRI, up(1, 1, t_min=2.0), defect="open_interval")) == MISS
    assert one(R.brute(TRI, up(1, 1, t_max=2.0), defect="open_interval")) == MISS


def test_floor_at_a_grazing_angle_takes_the_slab_value():
    floor = np.array([[0, 0, 0, 4000, 0, 0, 0, 0, 4000]], F)                            # in the plane y = 0
    for o, d in (((1.1, 0.1, 1.3), (0.3, -0.001, 0.7)), ((1.0, 0.3, 1.0), (1.0, -0.0007, 0.5)), ((3, 0.7, 5), (0.9, -0.0003, 0.4))):
        rays = R.make_rays([o], [d])
        slab = (F(0) - F(o[1])) * (F(1) / F(d[1]))                                       # l = h of the y axis: the box is flat there
        h = both(floor, rays)
        assert h["prim"][0] == 0 and h["t"][0] == slab
        raw = R.brute(floor, rays, defect="no_clamp")
        assert raw["prim"][0] == 0 and raw["t"][0] != slab                               # Moeller-Trumbore's own parameter is a few ulp off: the clamp is seen
        assert abs(float(raw["t"][0]) - float(slab)) <= 4 * float(np.spacing(slab))


def test_zero_direction_components():
    # two zero components: d = (0, 0, 1).  Origin in the box's plane x = 0 / y = 0: inclusive; outside by one step: the box is missed
    assert one(both(TRI, up(0, 1))) == (2.0, 0.0, 0.25, 0)
    assert one(both(TRI, up(1, 0))) == (2.0, 0.25, 0.0, 0)
    assert one(both(TRI, up(-EPS, 1))) == MISS
    assert one(both(TRI, up(4, 0))) == (2.0, 1.0, 0.0, 0) and one(both(TRI, up(np.nextafter(F(4), F(5)), 0))) == MISS
    # one zero component: d = (0, 1, 1) from (x, 0, 1) reaches the plane at t = 1, y = 1
    for x, want in ((0, (1.0, 0.0, 0.25, 0)), (1, (1.0, 0.25, 0.25, 0)), (3, (1.0, 0.75, 0.25, 0)), (-EPS, MISS), (3.5, MISS)):
        assert one(both(TRI, R.make_rays([[x, 0, 1]], [[0, 1, 1]]))) == want
    # a ray INSIDE the triangle's plane (d.z = 0, o.z = 2): det = 0, a miss although the box is met
    assert one(both(TRI, R.make_rays([[-1, 1, 2]], [[1, 0, 0]]))) == MISS
    # a direction component so small that its reciprocal overflows, origin in the box's plane: no constraint from that axis, as for d == 0
    tiny = F(1e-45)
    with np.errstate(over="ignore"):
        assert not np.isfinite(F(1) / tiny)
    assert one(both(TRI, R.make_rays([[0, 1, 0]], [[tiny, 0, 1]]))) == (2.0, 0.0, 0.25, 0)
    assert one(both(TRI, R.make_rays([[0, 1, 0]], [[-tiny, 0, 1]]))) == (2.0, 0.0, 0.25, 0)
    assert one(both(TRI, R.make_rays([[-EPS, 1, 0]], [[-tiny, 0, 1]]))) == MISS


def test_rays_that_are_not_finite_and_zero_directions_miss():
    assert one(both(TRI, R.make_rays([[1, 1, 0]], [[0, 0, 0]]))) == MISS
    assert one(both(TRI, R.make_rays([[1, 1, 0]], [[-0.0, 0.0, -0.0]]))) == MISS
    for bad in (np.nan, np.inf, -np.inf):
        for field in ("origin", "direction"):
            for a in range(3):
                r = up(1, 1)
                r[field][0, a] = bad
                assert one(both(TRI, r)) == MISS and one(both(TRI, r, any_hit=True)) == MISS
    # the limits are used as given: an infinite one is no limit on that side, a NaN admits nothing
    assert one(both(TRI, up(1, 1, t_min=-np.inf, t_max=np.inf))) == (2.0, 0.25, 0.25, 0)
    for kw in (dict(t_min=np.nan), dict(t_max=np.nan), dict(t_min=np.inf), dict(t_max=-np.inf)):
        assert one(both(TRI, up(1, 1, **kw))) == MISS
    # a triangle with a vertex that is not finite is never hit, and does not disturb its neighbours
    for bad in (np.nan, np.inf):
        two = np.concatenate([TRI, TRI + F(1)]).copy()
        two[0, 4] = bad
        assert one(both(two, up(1.5, 1.5))) == (3.0, 0.125, 0.125, 1)


def test_ties_go_to_the_smaller_prim():
    # the same triangle three times, and a larger coplanar one in front of them in the array
    tris = np.concatenate([np.array([[-8, -8, 2, 24, -8, 2, -8, 24, 2]], F), TRI, TRI, TRI])
    assert one(both(tris, up(1, 1))) == (2.0, 0.28125, 0.28125, 0)
    assert one(both(tris[1:], up(1, 1))) == (2.0, 0.25, 0.25, 0)
    assert one(both(tris[::-1], up(1, 1))) == (2.0, 0.25, 0.25, 0)
    assert one(R.brute(tris[1:], up(1, 1), defect="tie_larger")) == (2.0, 0.25, 0.25, 2)
    # numbering is the caller's: with prims given the smaller NUMBER wins, wherever it stands
    assert one(R.brute(tris[1:], up(1, 1), prims=[7, 3, 5])) == (2.0, 0.25, 0.25, 3)
    assert one(R.walk(R.build_bvh(tris[1:], prims=[7, 3, 5]), up(1, 1))[0]) == (2.0, 0.25, 0.25, 3)
    # -0.0 and +0.0 are the same t
    flat = np.array([[0, 0, 0, 4, 0, 0, 0, 4, 0], [0, 0, -0.0, 4, 0, -0.0, 0, 4, -0.0]], F)
    assert one(both(flat, up(1, 1, 0.0, t_min=-1.0)))[3] == 0 and one(both(flat[::-1], up(1, 1, 0.0, t_min=-1.0)))[3] == 0


def test_pruning_is_strict():
    # one axis-aligned triangle: the root's interval is the single value tn = tf = 2; a walk that skips a node at equality never sees it
    bvh = R.build_bvh(TRI)
    assert R.walk(bvh, up(1, 1))[0].tobytes() == R.brute(TRI, up(1, 1)).tobytes()
    assert one(R.walk(bvh, up(1, 1), defect="prune_nonstrict")[0]) == MISS
    # ... and a tie in ANOTHER leaf: ten coplanar copies, the walk must still reach the one with the smallest prim after it has found t = 2
    tris = np.concatenate([TRI + np.array([k, 0, 0] * 3, F) for k in (3, 2, 1, 0.5, 0.25, 0, 0, 0, 0, 0)])
    rays = up(3.5, 0.25)
    want = R.brute(tris, rays)
    bvh = R.build_bvh(tris)
    assert len(bvh.skip) > 1 and R.walk(bvh, rays)[0].tobytes() == want.tobytes()
    assert R.walk(bvh, rays, defect="prune_nonstrict")[0].tobytes() != want.tobytes()


def test_uv_edge_is_inclusive():
    for x, y in ((2, 2), (4, 0), (0, 4), (1, 3)):
        assert one(R.brute(TRI, up(x, y)))[3] == 0
        assert one(R.brute(TRI, up(x, y), defect="uv_open")) == MISS


def test_world_triangles_numbering_and_transform():
    verts = np.zeros(4, [("position", "<f4", 3)])
    verts["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    ind = np.array([0, 1, 2, 0, 1, 9, 1, 2, 3], np.uint32)                              # the second triangle has an index out of range
    M = np.eye(4, dtype=F); M[:3, 3] = (10, 20, 30); M[0, 0] = 2
    obj = np.zeros(3, [("trs", "<f4", 16), ("mesh_idx", "<u8")])
    obj["trs"] = M.T.reshape(16)
    obj["mesh_idx"] = [0, 5, 0]                                                         # the second object's mesh does not exist
    tris, prims = R.world_triangles(obj, [(verts, ind)])
    assert prims.tolist() == [0, 2, 3, 5]                                               # skipped triangles are numbered, missing objects are not
    assert tris[0].tolist() == [10, 20, 30, 12, 20, 30, 10, 21, 30]


@pytest.fixture(scope="module")
def run():
    tris, rays = R.soup(np.random.default_rng(2024), 400, 3000)
    return tris, rays, R.brute(tris, rays), R.build_bvh(tris)


def test_the_pruned_walk_is_brute_force_bit_for_bit(run):
    """the run the definition was tried on before it was written down: 400 triangles -- a third on a grid with shared edges, a quarter axis-aligned on
    four shared planes, some degenerate --, 3000 rays that include axis-parallel ones, origins inside the shared planes and rays aimed exactly at
    grid vertices and edge midpoints"""
    tris, rays, want, bvh = run
    got, visits = R.walk(bvh, rays)
    assert got.tobytes() == want.tobytes()
    hit, tie = R.tied(tris, rays)
    assert (want["prim"] != R.NO_PRIM).tolist() == hit.tolist()
    assert hit.sum() >= len(rays) // 4 and tie.sum() >= 5                               # not vacuous: rays hit, and closest hits are shared
    assert len(bvh.skip) == 255 and visits.mean() < len(bvh.skip) / 3                   # ... and the walk does prune
    a, _ = R.walk(bvh, rays, any_hit=True)
    assert a.tobytes() == R.brute(tris, rays, any_hit=True).tobytes()
    assert ((a["prim"] == 0) == hit).all()


@pytest.mark.parametrize("defect", ["open_interval", "no_clamp", "tie_larger", "uv_open"])
def test_the_run_tells_the_definition_from_each_defect(run, defect):
    tris, rays, want, bvh = run
    assert R.brute(tris, rays, defect=defect).tobytes() != want.tobytes()
    assert R.walk(bvh, rays, defect=defect)[0].tobytes() != want.tobytes()


def test_the_run_tells_strict_pruning_from_non_strict(run):
    tris, rays, want, bvh = run
    assert R.walk(bvh, rays, defect="prune_nonstrict")[0].tobytes() != want.tobytes()


def bits(*patterns):
    return np.array(patterns, np.uint32).view(F)


def test_ray_odd_worked_out_by_hand():
    """1 / d overflows exactly up to |d| = 2^-128 (bits 0x00200000): 2^128 is one step past the largest float, and 1 / (2^-128 (1 + 2^-21)) rounds
    to a finite one"""
    tiny = bits(0x00000001)[0]
    assert tiny > 0 and tiny / F(2) == 0 and bits(0x007FFFFF)[0] + tiny == bits(0x00800000)[0]      # numpy does not flush subnormals
    with np.errstate(over="ignore"):
        assert np.isinf(F(1) / bits(0x00200000)[0]) and F(1) / bits(0x00200001)[0] == bits(0x7F7FFFF8)[0]
    odd = [0x00000000, 0x00000001, 0x00200000]
    plain = [0x00200001, 0x00400000, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF]
    for pattern, want in [(b, True) for b in odd] + [(b, False) for b in plain]:
        for sign in (0, 0x80000000):
            for axis in range(3):
                d = np.array([1.0, -2.0, 0.5], F)
                d[axis] = bits(pattern | sign)[0]
                assert R.ray_odd(R.make_rays([[0, 0, 0]], [d])).tolist() == [want], (hex(pattern | sign), axis)
    assert bits(0x80000000)[0] == 0 and np.signbit(bits(0x80000000)[0])                             # (-0.0 is among them)
    # what the limits and the origin hold does not matter; a NaN component is odd (its reciprocal is not finite), an infinite one is not (1 / inf = 0)
    r = R.make_rays([[np.nan, 0, np.inf]] * 3, [[1, 2, 3], [1, np.nan, 3], [np.inf, 2, -np.inf]], t_min=np.nan, t_max=-np.inf)
    assert R.ray_odd(r).tolist() == [False, True, False]
    assert R.ray_odd(R.make_rays([[0, 0, 0]] * 2, [[0, 0, 0], [-0.0, 0.0, -0.0]])).tolist() == [True, True]


def test_a_nan_slab_product_is_no_constraint():
    # d = (0, 0, 1) from the box's plane x = 0: (0 - 0) * inf is NaN.  The definition: no constraint -- a hit; the defect: the root is skipped
    bvh = R.build_bvh(TRI)
    assert one(R.walk(bvh, up(0, 1))[0]) == (2.0, 0.0, 0.25, 0) and one(R.walk(bvh, up(0, 1), defect="nan_prunes")[0]) == MISS
    # the same with a component whose reciprocal overflows
    tiny = R.make_rays([[0, 1, 0]], [[F(1e-45), 0, 1]])
    assert one(R.walk(bvh, tiny)[0]) == (2.0, 0.0, 0.25, 0) and one(R.walk(bvh, tiny, defect="nan_prunes")[0]) == MISS
    # strictly inside the slab, and outside it, there is no NaN: the defect changes nothing
    for x in (1, -EPS):
        assert R.walk(bvh, up(x, 1), defect="nan_prunes")[0].tobytes() == R.walk(bvh, up(x, 1))[0].tobytes()
    # only odd rays can meet it
    plain = R.make_rays([[0, 1, 0]], [[2.0 ** -126, 2.0 ** -100, 1]])
    assert not R.ray_odd(plain)[0] and R.walk(bvh, plain, defect="nan_prunes")[0].tobytes() == R.walk(bvh, plain)[0].tobytes()


def test_the_run_tells_no_constraint_from_a_nan_that_prunes(run):
    tris, rays, want, bvh = run
    got = R.walk(bvh, rays, defect="nan_prunes")[0]
    differ = (got != want)
    assert differ.any() and R.ray_odd(rays)[differ].all()                                          # ... and rays that are not odd are not touched


def test_edge_records_against_one_triangle():
    base = R.make_rays([[1, 1, 0]], [[0.25, 0.5, 1]])                                               # reaches z = 2 at (1.5, 2, 2): u = 0.375, v = 0.5
    assert one(both(TRI, base)) == (2.0, 0.375, 0.5, 0) and not R.ray_odd(base)[0]
    e = R.edge_records()
    assert len(e) == len(R.EDGE_NAMES) == 14 and e.tobytes() == R.edge_records(base).tobytes()
    assert R.ray_valid(e).tolist() == [False] * R.EDGE_INVALID + [True] * 6
    assert R.ray_odd(e).tolist() == [True, True, False, False, False, True, False, False] + [False] * 6
    assert np.signbit(e["direction"][1]).tolist() == [True, False, True] and (e["direction"][1] == 0).all()
    assert e["t_min"][12] > e["t_max"][12]
    for any_hit in (False, True):
        got = both(TRI, e, any_hit=any_hit)
        assert [tuple(h) for h in got[:13].tolist()] == [MISS] * 13
        assert tuple(got[13].tolist()) == ((0.0, 0.0, 0.0, 0) if any_hit else (2.0, 0.375, 0.5, 0))
    # swapped limits WOULD admit the hit of a ray aimed at a target at t = 1: the record is not a miss for want of a triangle
    at_one = R.make_rays([[1, 1, 1.5]], [[0.25, 0.5, 0.5]])
    assert one(both(TRI, at_one))[0] == 1.0 and one(both(TRI, R.edge_records(at_one)[12:13])) == MISS
