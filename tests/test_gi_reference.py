"""The indirect diffuse light on a machine without a GPU: the host arbiters arctic_gi_points and arctic_gi_estimate_pixels -- the functions of
csrc/gi.h that the kernels run -- against the numpy restatement of the header's text (tests/gi_reference.py), by bytes; that the inputs are what
they are taken for; and that the comparisons tell the definition from its near misses (gi_reference's defects)."""
import numpy as np
import pytest

import ao_reference as A
import gi_reference as GI
import gi_scenes as GS
import ray_reference as R

F = np.float32
MAX_DISTANCE, BIAS = 7.5, 2e-3


@pytest.fixture(scope="module")
def renderer(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    import os
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return pkg.renderer


@pytest.mark.parametrize("P", [1, 2, 4])
def test_rays_equal_numpy_by_bytes(renderer, P):
    points, kinds = GS.hostile_points()
    n_rays = 3
    dirs = GS.cosine_table(n_rays, P, 5)
    sets = np.random.default_rng(P).integers(0, P * P, len(points))
    m, ok = A.normal(points[:, 3:6])
    # the inputs are what they are taken for: m2 = -0.0 is covered, the zero, NaN, infinite, overflowing and underflowing normals are not
    assert ok[kinds == 1].all() and ok[kinds == 2].all() and np.signbit(m[kinds == 1][:, 2]).all()
    for k in (3, 4, 5, 6, 7, 10):
        assert not ok[kinds == k].any(), k
    assert ok[kinds == 8].all() and ok[kinds == 9].all() and ok[kinds >= 100].all() and ok[kinds == 0].all()
    for round in range(n_rays):
        want, had = GI.point_rays(points, sets, dirs, n_rays, round, MAX_DISTANCE, BIAS)
        got = renderer.gi_points(points, sets, dirs, round, max_distance=MAX_DISTANCE, bias=BIAS)
        assert got.dtype == R.RAY_DTYPE and got.tobytes() == want.tobytes(), (P, round, np.nonzero(got != want)[0][:8])
        assert (had == ok).all() and not want[~ok].tobytes().strip(b"\0")             # the all-zero record
        assert (got["t_max"][ok] == F(MAX_DISTANCE)).all() and (got["t_min"] == 0).all()
        assert not np.isfinite(got["origin"][kinds >= 100]).all(1).any()               # a world that is not finite gives a ray that is a miss by definition
        # a covered point's direction is the frame applied to ITS set's direction of THIS round
        t, bt = A.frame(m)
        l = dirs[sets, round]
        with np.errstate(all="ignore"):
            d = np.stack([(t[:, i] * l[:, 0] + bt[:, i] * l[:, 1]) + m[:, i] * l[:, 2] for i in range(3)], -1)
        assert got["direction"][ok].tobytes() == d[ok].astype(F).tobytes()
    if P > 1:                                                                          # the set matters, and so does the round
        other = renderer.gi_points(points, (sets + 1) % (P * P), dirs, 0, max_distance=MAX_DISTANCE, bias=BIAS)
        assert (other["direction"][ok] != renderer.gi_points(points, sets, dirs, 0, max_distance=MAX_DISTANCE, bias=BIAS)["direction"][ok]).any(1).mean() > 0.9
    a, b = (renderer.gi_points(points, sets, dirs, k, max_distance=MAX_DISTANCE, bias=BIAS) for k in (0, 1))
    assert (a["direction"][ok] != b["direction"][ok]).any(1).all() and a["origin"].tobytes() == b["origin"].tobytes()


@pytest.mark.parametrize("P", [1, 2, 4])
def test_sum_and_estimate_equal_numpy_by_bytes(renderer, P):
    c = GS.synthetic_frame(P=P)
    geometry = c.material != GS.NO_MATERIAL
    had = c.rays["t_max"] > 0
    assert (had == had[0]).all() and 0.6 < had[0].mean() < 1.0 and (~had[0][c.material == GS.NO_MATERIAL]).all()
    S_want = GI.add(c.rays, c.colors, c.clamp_max)
    kw = dict(n_rays=c.n_rays, pattern=P, clamp_max=c.clamp_max, max_distance=50.0)
    S, E = renderer.gi_estimate_pixels(c.rays, c.colors, **kw)
    assert S.tobytes() == S_want.tobytes() and E.tobytes() == GI.estimate(S_want).tobytes()
    # the sanitising: NaN -> 0, -inf and negatives -> 0, above the clamp -> the clamp, +inf -> the clamp; S itself holds no NaN and nothing negative
    assert not np.isnan(S).any() and (S >= 0).all() and (S[had[0]][:, 3] == c.n_rays).all() and not S[~had[0]].any()
    assert np.isinf(S[c.wall & had[0]][:, 0:3]).all()                                  # three clamps of 3e38 overflow the sum
    fy, fx = c.odd
    for k, v in enumerate([0.0, 0.0, 0.0, 1e30]):                                      # (1e30 is below this clamp: it stands)
        ch, round = k % 3, k % c.n_rays
        rest = sum(GI.sanitise(c.colors[r, fy[k], fx[k], ch], c.clamp_max) for r in range(c.n_rays) if r != round)
        covered = had[0][fy[k], fx[k]]
        assert covered.sum() >= 5 and np.allclose(S[fy[k], fx[k], ch][covered], (rest + F(v))[covered], rtol=1e-6)
    low = GI.add(c.rays, c.colors, 2.0)                                                # a clamp inside the colours' range: about half of them are cut
    S_low, E_low = renderer.gi_estimate_pixels(c.rays, c.colors, **dict(kw, clamp_max=2.0))
    assert S_low.tobytes() == low.tobytes() and E_low.tobytes() == GI.estimate(low).tobytes() and (low[..., 0:3] <= 2.0 * c.n_rays).all()
    assert (low[had[0]][:, 0:3] != S_want[had[0]][:, 0:3]).mean() > 0.5 and (low[c.wall & had[0]][:, 0:3] == 2.0 * c.n_rays).all()
    assert (GI.add(c.rays, c.colors, c.clamp_max, defect="minmax") != S_want).any() or np.isnan(GI.add(c.rays, c.colors, c.clamp_max, defect="minmax")).any()
    assert (GI.add(c.rays, c.colors, c.clamp_max, defect="count_all")[..., 3] != S_want[..., 3]).any()
    # filtered
    f = dict(filter=True, normal_cos=c.normal_cos, plane_dist=c.plane_dist)
    want = GI.estimate(S_want, c.attrs, c.material, P, **f)
    S2, E2 = renderer.gi_estimate_pixels(c.rays, c.colors, c.attrs[..., 8:11], c.attrs[..., 11:14], geometry, **kw, **f)
    assert S2.tobytes() == S_want.tobytes() and E2.tobytes() == want.tobytes(), np.argwhere((E2 != want).any(-1))[:8]
    assert not E2[~had[0]].any() and (E2[had[0]][:, 3] >= c.n_rays).all() and (E2[..., 3] <= c.n_rays * P * P).all()
    floor = had[0] & ~c.wall
    assert np.isfinite(E2[floor]).all()                                                # the wall's infinities stay behind the edge ...
    if P > 1:
        assert (E2[..., 3] > c.n_rays).mean() > 0.5 and (E2[floor][:, 3] < c.n_rays * P * P).any()   # windows that accept, and windows the edge cuts
        leaked = GI.estimate(S_want, c.attrs, c.material, P, defect="product", **f)
        assert np.isnan(leaked[floor]).any()                                           # ... which a product by zero would not keep there
        assert (GI.estimate(S_want, c.attrs, c.material, P, defect="p_first", **f) != want).any()    # the order of the sum is part of the definition
        loose = GI.estimate(S_want, c.attrs, c.material, P, filter=True, normal_cos=-2.0, plane_dist=1e30)
        _, E3 = renderer.gi_estimate_pixels(c.rays, c.colors, c.attrs[..., 8:11], c.attrs[..., 11:14], geometry, filter=True, normal_cos=-2.0, plane_dist=1e30, **kw)
        assert E3.tobytes() == loose.tobytes() and (loose != want).any()
    else:
        assert E2.tobytes() == GI.estimate(S_want).tobytes()                           # a window of one pixel: the unfiltered estimate of the covered pixels


@pytest.mark.parametrize("move", ["translated", "rotated", "through the wall"])
def test_the_history_over_four_frames_equals_numpy(pkg, renderer, move):
    """the scenes of tests/ao_history_scenes.py: four calls along a camera path, E random with some pixels that had no ray, and -- in the second
    call's E -- NaN colours on the box, whose taps the floor's pixels reject: they must stay there.  By bytes wherever no NaN stands; where one does
    (the box's own pixels, which blend their own NaN), both sides must hold a NaN in the same place: a NaN's sign and payload are not part of the
    definition and differ between numpy's and the compiler's instruction selection"""
    import ao_history_reference as HR
    import ao_history_scenes as HS
    W, H = 61, 37
    c = HS.case(pkg, move, W, H, 4)
    hist = dict(max_history=3.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.1)
    rng = np.random.default_rng([7, HS.MOVES.index(move)])
    prev, leaked, seen, poisoned = None, None, np.zeros(6, np.int64), 0
    for k, (attrs, mat, P) in enumerate(c["frames"]):
        cur = rng.uniform(0, 3, (H, W, 4)).astype(F)
        cur[..., 3] = np.where(rng.uniform(size=(H, W)) < 0.9, 3, 0)
        if k == 1:
            box = np.abs(attrs[..., 8:11]).max(-1) == 3.0                                # the box's stored normals have length 3
            cur[box, 0:3] = np.nan
            poisoned = int((box & (cur[..., 3] > 0)).sum())
        a = attrs.reshape(-1, 18)
        want, state, accepted = GI.accumulate_frame(attrs, mat, cur, prev, P, hist)
        got = renderer.gi_accumulate_pixels(a[:, 11:14], a[:, 8:11], mat.reshape(-1) != GS.NO_MATERIAL, cur, None if prev is None else prev["P"], W, H,
                                            None if prev is None else (prev["acc"], prev["count"], prev["world"], prev["normal"]), **hist)
        same = lambda x, y: np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1), equal_nan=True)
        assert same(got[0], want) and same(got[1], state["acc"]) and same(got[2], state["count"]) and same(got[3], state["world"]) and same(got[4], state["normal"]), k
        finite = np.isfinite(want).all(-1)
        assert got[0].reshape(H, W, 4)[finite].tobytes() == want[finite].tobytes()      # by bytes wherever no NaN stands
        assert (want[cur[..., 3] == 0] == 0).all() and (state["count"][cur[..., 3] == 0] == 0).all()   # E.a == 0: not covered, an all-zero entry
        if k == 2:                                                                       # the call that taps the poisoned entries
            floor = (np.abs(attrs[..., 8:11]).max(-1) == 2.0) & (cur[..., 3] > 0)
            assert np.isfinite(want[floor]).all()
            leaked = GI.accumulate_frame(attrs, mat, cur, prev, P, hist, defect="rejected tap multiplied")[0]
        seen += np.bincount(accepted.reshape(-1) + 1, minlength=6)
        prev = state
    assert seen[1] >= 20                                                                 # pixels all of whose taps were rejected: the history restarts there
    if move == "through the wall":                                                       # (beyond the wall the camera sees nothing it saw before: every tap is rejected)
        assert seen[1] >= 1000 and seen[2:].sum() == 0
    else:
        assert seen[5] >= 300 and seen[2:5].sum() >= 50 and poisoned >= 50 and np.isnan(leaked[floor]).any()                                             # a product by zero would have let them through


def test_the_composition_terms_equal_numpy_by_bytes(renderer):
    rng = np.random.default_rng(11)
    n = 4000
    hdr, base, metal = rng.uniform(0, 6, (n, 3)).astype(F), rng.uniform(0, 1, (n, 3)).astype(F), rng.uniform(0, 1, n).astype(F)
    E = rng.uniform(0, 4, (n, 4)).astype(F)
    E[::3, 3] = 0
    E[::3, 0:3] = np.nan                                                                 # behind E.a == 0: never looked at
    E[1::7, 3] = np.nan                                                                  # a NaN count is no light either
    geometry = rng.uniform(size=n) < 0.8
    for strength, scale in ((1.0, 1.0), (0.0, 1.0), (0.7, 0.0), (2.5, 0.3)):
        got = renderer.gi_compose_pixels(hdr, base, metal, E, geometry, 0.3, gi_strength=strength, ambient_scale=scale)
        want = GI.compose(hdr, base, metal, E, geometry, 0.3, strength, scale)
        assert got.tobytes() == want.tobytes() and np.isfinite(got).all(), (strength, scale)
        assert got[~geometry].tobytes() == hdr[~geometry].tobytes()
        if strength == 0.0 and scale == 1.0:
            assert got.tobytes() == hdr.tobytes()                                        # both terms add an exact zero
        lit = geometry & (E[:, 3] > 0)
        if strength > 0:
            assert (got[lit] != hdr[lit]).any(1).mean() > 0.95
    # float64 agrees with the fp32 terms: five roundings (two products and a sum per term) of values below 6 + 2.5 * 4 = 16
    want64 = GI.compose(hdr, base, metal, E, geometry, 0.3, 2.5, 0.3, dtype=np.float64)
    assert np.abs(got - want64).max() <= 5 * 2.0 ** -24 * 16
    for bad in (dict(gi_strength=-0.1), dict(gi_strength=np.nan), dict(gi_strength=np.inf), dict(ambient_scale=-0.1), dict(ambient_scale=1.1), dict(ambient_scale=np.nan), dict(flags=2)):
        with pytest.raises(renderer.ArcticError):
            renderer.gi_compose_pixels(hdr, base, metal, E, geometry, 0.3, **bad)
