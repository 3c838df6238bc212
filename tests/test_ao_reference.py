"""The numpy arbiter of the ambient occlusion (tests/ao_reference.py) on its own, no GPU: pixels worked by hand pin it, every deliberate defect
shows on the inputs the device test uses, the inputs meet the conditions that test relies on (tests/ao_scenes.py), and the definition means what
it is meant to: an open floor is fully visible, a point in front of a wall sees half the sky.  Plus ao_directions."""
import numpy as np
import pytest

import ao_reference as A
import ao_scenes as AS
import ray_reference as R
import ray_scenes as S

F = np.float32


def f32(*x):
    return np.array(x, F)


def test_normal_and_frame_by_hand():
    m, ok = A.normal([[0, 0, 2], [0, 0, -0.5], [0, 0, -0.0], [3, 0, 4], [0, 0, 0], [3e19, 3e19, 3e19], [1e-30, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]])
    assert ok.tolist() == [True, True, False, True, False, False, False, False, False]
    assert m[0].tolist() == [0, 0, 1] and m[1].tolist() == [0, 0, -1]
    assert m[3].tobytes() == (f32(3, 0, 4) / F(5)).tobytes()                                # a normal that is not a unit vector: 3-4-5
    # m = (0, 0, 1): s = 1, a = -1/2, b = 0: t = (1, 0, -0), bt = (0, 1, -0)
    t, bt = A.frame(f32(0, 0, 1).reshape(1, 3))
    assert t[0].tolist() == [1, 0, 0] and bt[0].tolist() == [0, 1, 0] and np.signbit(t[0, 2]) and np.signbit(bt[0, 2])
    # m = (0, 0, -1): s = -1, a = 1/2, b = 0: t = (1, -0, 0), bt = (0, -1, -0)
    t, bt = A.frame(f32(0, 0, -1).reshape(1, 3))
    assert t[0].tolist() == [1, 0, 0] and bt[0].tolist() == [0, -1, 0] and np.signbit(t[0, 1])
    # m2 = -0.0 takes s = -1: a = -1 / (-1 + -0) = 1; m = (0, 0, -0.0) gives t = (1, -0, 0), bt = (0, -1, -0): finite, like any other
    t, bt = A.frame(f32(0, 0, -0.0).reshape(1, 3))
    assert t[0].tolist() == [1, 0, 0] and bt[0].tolist() == [0, -1, 0]
    # ... and the unit vector (0.6, 0.8, -0): a = 1, b = 0.48: t = (1 - 0.36, -0.48, 0.6), bt = (0.48, -1 + 0.64, -0.8), all in float32
    m = f32(0.6, 0.8, -0.0).reshape(1, 3)
    t, bt = A.frame(m)
    b = F(0.6) * F(0.8)
    assert t[0].tobytes() == f32(F(1) + (F(-0.6) * F(0.6)), -b, F(0.6)).tobytes() and bt[0].tobytes() == f32(b, F(-1) + F(0.8) * F(0.8), F(-0.8)).tobytes()
    # a general unit vector: the frame is orthonormal to rounding
    rng = np.random.default_rng(1)
    m, ok = A.normal(rng.normal(size=(200, 3)))
    t, bt = A.frame(m)
    for a, b in ((t, t), (bt, bt)):
        assert np.abs((a * b).sum(1) - 1).max() < 1e-5
    for a, b in ((t, bt), (t, m), (bt, m)):
        assert np.abs((a * b).sum(1)).max() < 1e-5
    assert np.abs(np.cross(t, bt) - m).max() < 1e-5                                          # right-handed: t x bt = m


def test_rays_and_results_by_hand():
    # world (1, 2, 3), n = (0, 0, 2), bias 0.25, l = (0.5, -0.25, 2): o = (1, 2, 3.25), d = (0.5, -0.25, 2) (t = x, bt = y, m = z)
    pts = f32(1, 2, 3, 0, 0, 2).reshape(1, 6)
    ry, ok = A.point_rays(pts, [0], f32(0.5, -0.25, 2).reshape(1, 1, 3), 1, 7.0, 0.25)
    assert ok[0] and ry[0, 0]["origin"].tolist() == [1, 2, 3.25] and ry[0, 0]["direction"].tolist() == [0.5, -0.25, 2] and ry[0, 0]["t_min"] == 0 and ry[0, 0]["t_max"] == 7
    # one triangle above the point at z = 5 (t = 1.75 / 2): hit inside the radius, missed with a radius below it, and by the ray of set 1
    tri = f32(-9, -9, 5, 9, -9, 5, 0, 9, 5).reshape(1, 9)
    dirs = f32(0.5, -0.25, 2, 0, 0, -1).reshape(2, 1, 3)
    assert A.point_hits(tri, pts, [0], dirs, 1, 7.0, 0.25).tolist() == [1]
    assert A.point_hits(tri, pts, [0], dirs, 1, 0.5, 0.25).tolist() == [0]
    assert A.point_hits(tri, pts, [0], dirs, 1, 0.5, 0.25, defect="no_radius").tolist() == [1]
    assert A.point_hits(tri, pts, [1], dirs, 1, 7.0, 0.25).tolist() == [0]
    for brute in (False, True):
        assert A.point_hits(tri, np.concatenate([pts, f32(1, 2, 3, 0, 0, 0).reshape(1, 6)]), [0, 0], dirs, 1, 7.0, 0.25, brute=brute).tolist() == [1, 0]
    # the unfiltered result: (510 * (n - hits) + n) / (2 n): 255 * v / n rounded to nearest, halves up
    assert A.result(np.array([0, 1, 2, 3]), 3).tolist() == [255, 170, 85, 0]
    assert A.result(np.array([0, 1, 63, 64]), 64).tolist() == [255, 251, 4, 0]                # 255 * 63 / 64 = 251.02, 255 / 64 = 3.98
    assert A.result(np.array([1]), 2).tolist() == [128] and A.result(np.array([1]), 2, defect="floor").tolist() == [127]
    assert A.result(np.array([2]), 4, covered=np.array([False])).tolist() == [255]
    assert [A.set_index(x, y, 4) for x, y in ((0, 0), (1, 0), (5, 2), (3, 7))] == [0, 1, 9, 15] and A.set_index(1, 0, 4, "swap_xy") == 4
    assert list(A.window(4)) == [-2, -1, 0, 1] and list(A.window(2)) == [-1, 0] and list(A.window(1)) == [0]


def test_filter_by_hand():
    # a 1 x 4 frame, P = 2 (window -1..0 in x, and the row above, which is outside): flat floor at y = 0 but the last pixel, which stands 1 higher
    attrs = np.zeros((1, 4, 18), F)
    attrs[..., 9] = 1.0
    attrs[0, :, 11] = [0, 1, 2, 3]
    attrs[0, 3, 12] = 1.0
    hits, covered = np.array([[0, 2, 1, 2]], np.uint8), np.array([[True, True, True, True]])
    res, acc, cut = A.filtered(hits, covered, attrs, 2, 2, 0.9, 0.05)
    # pixel 0: alone (its left neighbour is outside): V = 2, T = 2 -> 255.  1: with 0: V = 2 + 0 -> (510 * 2 + 4) / 8 = 128.  2: with 1: V = 1 + 0 -> 64.
    # 3: pixel 2 lies 1 below its plane: rejected; alone: V = 0 -> 0
    assert acc.tolist() == [[1, 2, 2, 1]] and res.tolist() == [[255, 128, 64, 0]]
    assert cut[0, :, 0].tolist() == [True, False, False, False] and cut[..., 2].all() and not cut[..., 1].any() and not cut[..., 3].any()
    covered[0, 1] = False                                                                     # a pixel that is not covered: 255, and accepted by nobody
    res, acc, _ = A.filtered(hits, covered, attrs, 2, 2, 0.9, 0.05)
    assert acc.tolist() == [[1, 0, 1, 1]] and res.tolist() == [[255, 255, 128, 0]]
    attrs[0, 2, 8:11] = (0.6, 0.8, 0)                                                         # dot = 0.8 < 0.9: pixel 3 would reject it by the normal too
    res, acc, _ = A.filtered(hits, np.ones((1, 4), bool), attrs, 2, 2, 0.9, 10.0)
    assert acc.tolist() == [[1, 2, 1, 1]]


@pytest.mark.parametrize("n_tris", [5, 1000])
def test_the_injected_inputs_meet_their_conditions(pkg, n_tris):
    c = AS.injected_case(pkg, n_tris)
    seen = AS.check_injected_conditions(c)
    for key, v in seen.items():
        print(n_tris, "triangles, pattern %d, %d rays, radius %s: no hit / every ray hits / between =" % key, v)
    if n_tris == 1000:
        print("odd table:", AS.check_odd_conditions(AS.odd_case(pkg)))
    # the shortcut of ao_scenes (one walk with 64 rays serves every n_rays) against the reference used directly, and the walk against the loop
    for n, P in ((5, 2), (4, 4)):
        direct, _ = A.image_hits(c.data.tris, c.attrs, c.material, AS.table(c.master, n, P), n, P, c.radius, AS.BIAS, brute=(n == 5))
        assert direct.tobytes() == AS.injected_want(c, n, P, c.radius)[0].tobytes()


def test_every_unfiltered_defect_shows_on_the_injected_inputs(pkg):
    c = AS.injected_case(pkg, 1000)
    width, height = S.SUN_SIZE
    n, P = 4, 4                                                                               # (255 * v / 4 is no integer: rounding down shows)
    dirs = AS.table(c.master, n, P)
    rows = S.owned(pkg, height, AS.SHARDS["rows 3..30"])
    want = AS.injected_want(c, n, P, c.radius, rows)
    for defect in (None, "local_row", "swap_xy", "no_bias", "no_normalise", "no_radius", "floor"):
        hits, covered = A.image_hits(c.data.tris, c.attrs[rows], c.material[rows], dirs, n, P, c.radius, AS.BIAS, frame_rows=rows, defect=defect, bvh=c.bvh)
        got = A.result(hits, n, covered, defect)
        differ = int((got != want[2]).sum())
        print(defect, differ, "pixels differ")
        assert (differ == 0) == (defect is None), defect
        if defect == "no_normalise":                                                          # ... at the pixels whose normal is not a unit vector
            assert (got != want[2]).reshape(-1)[np.isin(rows[:, None] * width + np.arange(width), c.kinds["not unit"]).reshape(-1)].any()
    # interleaved bands of 8 rows start at multiples of 8 in the frame and in the shard: there the shard's row IS the frame's row modulo the pattern
    rows = S.owned(pkg, height, AS.SHARDS["bands of 8, shard 1 of 2"])
    assert (rows % 4 == np.arange(len(rows)) % 4).all()


def raster_case(pkg, oracle):
    def make():
        width, height = S.SUN_SIZE
        o = AS.raster_upload(pkg, oracle.Oracle(width, height, 64, 16))
        sc = AS.raster_scene(pkg)
        o.pass_gbuffer(sc.desc)
        attrs, material = o.read_gbuffer()[:2]
        o.close()
        return S.Case(attrs=attrs, material=material, want=AS.raster_want(pkg, sc.desc, attrs, material))
    return S.once(("ao raster on the oracle",), make)


def test_the_rasterised_scene_meets_its_conditions(pkg, oracle):
    c = raster_case(pkg, oracle)
    for P, v in AS.check_raster_conditions(c.want).items():
        print("pattern %d: windows that accept all / some / only themselves =" % P, v)


def test_every_filter_defect_shows(pkg, oracle):
    f = AS.FILTER
    for P, w in raster_case(pkg, oracle).want.items():
        attrs = raster_case(pkg, oracle).attrs
        for defect in ("window_shift", "floor"):
            got, _, _ = A.filtered(w.hits, w.covered, attrs, f["n_rays"], P, f["normal_cos"], f["plane_dist"], defect)
            assert (got != w.filtered).sum() >= 10, (P, defect)
    # "p is always accepted" decides only where p fails its own test: a world position that is not finite (the injected G-buffer has six)
    c = AS.injected_case(pkg, 1000)
    hits, covered, _ = AS.injected_want(c, 4, 2, np.inf)
    want, acc, _ = A.filtered(hits, covered, c.attrs, 4, 2, -1.0, 1e30)
    got, _, _ = A.filtered(hits, covered, c.attrs, 4, 2, -1.0, 1e30, "p_tested")
    bad = covered & ~np.isfinite(c.attrs[..., 11:14]).all(-1)
    assert bad.sum() >= 3 and (acc[bad] == 1).all() and (want[bad] == 255).all() and (got[bad] != 255).all() and (got[~bad] == want[~bad]).all()


def test_an_open_floor_is_fully_visible(pkg):
    floor = f32(-50, 0, -50, 50, 0, -50, 50, 0, 50, -50, 0, -50, 50, 0, 50, -50, 0, 50).reshape(2, 9)
    rng = np.random.default_rng(5)
    pts = np.zeros((64, 6), F)
    pts[:, 0], pts[:, 2], pts[:, 4] = rng.uniform(-40, 40, 64), rng.uniform(-40, 40, 64), 1.0
    dirs = pkg.renderer.ao_directions(16, 4)
    hits = A.point_hits(floor, pts, np.arange(64) % 16, dirs, 16, np.inf, 1e-3)
    assert (A.result(hits, 16) == 255).all()
    assert (A.point_hits(floor, pts, np.arange(64) % 16, dirs, 16, np.inf, -1e-3) > 0).all()  # (from below the floor the rays do hit it: the bias matters)


def test_a_point_in_front_of_a_wall_sees_half_the_sky(pkg):
    """a wall 200 wide and 100 high standing on the floor, a floor point 0.01 in front of its middle, every ray of all 16 sets of ao_directions(64, 4)
    with infinite radius: 1024 cosine-weighted directions, half of whose measure lies on the wall's side.  Mean visibility within 4 binomial
    standard deviations of one half: |V / T - 0.5| <= 4 sqrt(0.25 / 1024) = 0.0625 (stratification only tightens it)"""
    floor = f32(-500, 0, -500, 500, 0, -500, 500, 0, 500, -500, 0, -500, 500, 0, 500, -500, 0, 500).reshape(2, 9)
    wall = f32(-100, 0, 0, 100, 0, 0, 100, 100, 0, -100, 0, 0, 100, 100, 0, -100, 100, 0).reshape(2, 9)
    tris = np.concatenate([floor, wall])
    pts = np.tile(f32(0, 0, 0.01, 0, 1, 0), (16, 1))
    for seed in (0, 1, 2):
        dirs = pkg.renderer.ao_directions(64, 4, seed=seed)
        hits = A.point_hits(tris, pts, np.arange(16), dirs, 64, np.inf, 1e-3)
        visible = (64 - hits.astype(np.int64)).sum() / 1024.0
        print("seed", seed, "mean visibility", visible)
        assert abs(visible - 0.5) <= 0.0625


@pytest.mark.parametrize("n_rays,pattern", [(64, 4), (16, 4), (64, 2), (4, 4), (1, 1), (5, 2)])
def test_ao_directions(pkg, n_rays, pattern):
    d = pkg.renderer.ao_directions(n_rays, pattern, seed=7)
    assert d.shape == (pattern * pattern, n_rays, 3) and d.dtype == np.float32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() <= 1e-6 and (d[..., 2] > 0).all()
    if n_rays * pattern * pattern >= 256:
        assert abs(d[..., 2].astype(np.float64).mean() - 2.0 / 3.0) < 0.05                   # cosine-weighted: E[z] = 2/3; sd of 256 independent samples 0.015
    assert pkg.renderer.ao_directions(n_rays, pattern, seed=7).tobytes() == d.tobytes()
    if n_rays >= 4:
        assert pkg.renderer.ao_directions(n_rays, pattern, seed=8).tobytes() != d.tobytes()
    if pattern > 1 and n_rays >= 4:                                                           # the sets are decorrelated: no two share a direction
        flat = d.reshape(-1, 3)
        assert len(np.unique(flat, axis=0)) == len(flat)
