"""tests/shadow_w_inputs.py on its own terms, without a device: the classes are what their names say, lane by lane, by the very predicates of
shadow_coords.h restated on bit patterns; the quotients still cover the map; and -- with the CPU oracle's calculate_shadow alone -- the covered
pixels of the general-w tiles hold hundreds of penumbra, fully lit and fully shadowed pixels each, so that a wrong operand, lane or branch in the
device's division shows."""
import numpy as np

import shadow_w_inputs as SW


def _near_one_divisible(ls):
    """shadow_coords.h: near_one_divisible, on numpy arrays"""
    a = np.abs(ls[..., :3])
    return (((ls[..., 3].view(np.uint32).astype(np.int64) - 0x3F7FFFFA) & 0xFFFFFFFF) <= 12) & (a.min(-1) > 2.0 ** -100) & (a.max(-1) < 2.0 ** 100)


def _tiles(a):
    """(tiles_y, tiles_x, 64): the lanes of each 8 x 8 tile"""
    h, w = a.shape
    return a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(h // 8, w // 8, 64)


def test_classes_take_the_branches_they_are_named_for(pkg):
    mat = pkg.scenes.random_gbuffer(np.random.default_rng(1), SW.H, SW.W, 4, coverage=0.9)[1]
    ls, tile_cls, lane_cls, q, zero_lanes = SW.light_space(mat=mat, smap=SW.shadow_map())
    tiles = SW.tile_classes()
    assert all((tiles == c).sum() == 16 for c in SW.CLASSES)
    w = ls[..., 3]
    all_one = (_tiles(w) == 1.0).all(-1)
    all_near = _tiles(_near_one_divisible(ls)).all(-1)
    general = ~all_one & ~all_near                                   # the wave's branch, as shadow_coords selects it
    assert (all_one == (tiles == "e")).all()                         # the control, and nothing else, takes the first branch
    assert general[tiles != "e"].all()                               # every other tile takes the division -- the c tiles because of ONE lane:
    near_lanes = _tiles(_near_one_divisible(ls))
    assert (near_lanes[tiles == "c"].sum(-1) == 63).all() and len(zero_lanes) == 16
    for y, x, comp in zero_lanes:
        assert ls[y, x, comp] == 0.0 and tile_cls[y, x] == "c" and mat[y, x] != SW.NO_MAT and w[y, x] != 1.0
    assert {bool(np.signbit(ls[y, x, c])) for y, x, c in zero_lanes} == {False, True} and {c for _, _, c in zero_lanes} == {0, 1, 2}
    steps = w.view(np.uint32).astype(np.int64) - 0x3F800000
    c, d = lane_cls == "c", lane_cls == "d"
    assert set(np.unique(np.abs(steps[c]))) == {1, 2, 3, 4, 5, 6} and set(np.unique(steps[d])) == {-7, 7}
    assert ((w[lane_cls == "a"] >= 0.5) & (w[lane_cls == "a"] <= 2)).all()
    b = w[lane_cls == "b"]
    assert (b < 0).mean() > 0.8 and (np.abs(b) == np.float32(2.0 ** -20)).sum() >= 20 and (np.abs(b) == np.float32(2.0 ** 20)).sum() >= 20
    m = _tiles(lane_cls)[tiles == "m"]
    assert all(len(np.unique(t)) == 5 for t in m)                    # the mixed tiles hold every class, lane by lane
    # the quotients are the usual ranges: the map (|x|, |y| <= 1, z <= 1), its borders and the outside
    got = ls[..., :3].astype(np.float64) / w[..., None].astype(np.float64)
    ok = np.ones(w.shape, bool)
    for y, x, comp in zero_lanes:
        ok[y, x] = False
    assert np.abs(got - q)[ok].max() < 1e-6
    assert (np.abs(q[..., :2]) > 1).any(-1).mean() > 0.1 and (q[..., 2] > 1).mean() > 0.05 and (q[..., 0] < 0).mean() > 0.4


def test_input_conditions(pkg, oracle):
    mat = pkg.scenes.random_gbuffer(np.random.default_rng(SW.SEED + 2), SW.H, SW.W, 4, coverage=0.9)[1]
    smap = SW.shadow_map()
    ls, tile_cls, _, _, _ = SW.light_space(mat=mat, smap=smap)
    assert smap.shape == (SW.S, SW.S) and smap.min() >= 0.2 and smap.max() <= 0.9
    counts = SW.check_input_conditions(SW.shadow_factors(oracle, smap, ls, mat), tile_cls, mat)
    print("covered pixels of the general-w tiles:", counts)
    one = SW.with_w_one(ls, tile_cls)
    assert (one[..., 3] == 1).all() and np.array_equal(one[..., :3], ls[..., :3])


def test_every_case_of_the_gpu_tests_meets_the_conditions(pkg, oracle):
    """the frames tests/test_gpu_shadow_w.py injects, from its own builders: each meets the input conditions, and the positions are in place"""
    import test_gpu_shadow_w as T
    _, attrs, mat, smap, tile_cls = T.base_inputs(pkg)
    print("base:", T.conditions(oracle, smap, attrs, mat, tile_cls)[1])
    assert (attrs[..., 17] != 1).mean() > 0.6
    for feature in list(T.EXTENDED) + ["pbr"]:
        case, I = T.extended_inputs(pkg, feature)
        assert I.shadow.shape == (SW.S, SW.S) and (I.attrs[..., 17] != 1).mean() > 0.6
        print(case.name, T.conditions(oracle, I.shadow, I.attrs, I.mat, I.tile_cls)[1])
