"""Depth of field on a machine without a GPU: the numpy restatement (tests/dof_reference.py) pinned on pixels worked by hand, the host arbiters
arctic_dof_prepare and arctic_dof_pixels against it BY BYTES, every deliberate defect shown to change output bytes, and what the feature is for:
a sharp foreground in front of a blurred background keeps its bits, a constant field stays constant, and the gather comes closer to a float64
brute-force scatter of the same discs than the unfiltered frame is."""
import numpy as np
import pytest

import dof_reference as D

F = np.float32
SIZES = ((8, 8), (17, 9), (40, 24), (72, 40))     # (width, height); the last: 9 x 5 tiles, max_radius 16 gives a window of two tiles cut at every edge
NAN = F(np.nan)
CAMERA = dict(z_near=0.5, z_far=50.0)              # zv = 25 / (50 - 49.5 d)


@pytest.fixture(scope="module")
def lib(pkg):
    """the library, built when a clean tree has none yet"""
    import os
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def same(got, want, what):
    """the same bytes, no element left out -- where a value is a NaN, a NaN (its payload is no part of the definition)"""
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaNs elsewhere", int((np.isnan(got) != nan).sum()))
    a, b = np.where(nan, F(0.0), got), np.where(nan, F(0.0), want)
    assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), "elements differ")


def arbiters(pkg, color, depth, taps2=None, **kw):
    """steps 1 to 4 by the host arbiters, every pixel listed: (out, tile_max, neighbour_max, P)"""
    H, W = np.asarray(depth).shape
    tile, near, P = pkg.renderer.dof_prepare(depth, **kw)
    ys, xs = np.mgrid[0:H, 0:W]
    out = pkg.renderer.dof_pixels(np.stack([xs, ys], -1).reshape(-1, 2), color, P, near, taps2, **kw)
    return out.reshape(H, W, 3), tile, near, P


def both(pkg, color, depth, taps2=None, **kw):
    """numpy's result, which the arbiters must reproduce by bytes"""
    want = D.dof(color, depth, taps2, **kw)
    for g, w, name in zip(arbiters(pkg, color, depth, taps2, **kw), want, ("out", "tile_max", "neighbour_max", "P")):
        same(g, w, name)
    return want


def colours(W, H, seed=1):
    return np.random.default_rng(seed).uniform(0.25, 4.0, (H, W, 3)).astype(F)


def test_the_spiral_is_vogels_and_lies_in_the_disc(pkg, lib):
    for n in (1, 2, 16, 48, 64):
        t = pkg.renderer.dof_taps(n)
        assert t.dtype == F and t.shape == (n, 2) and t.tobytes() == D.taps(n).tobytes()
        assert (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1] <= F(1.0)).all()
        i = np.arange(n)
        assert np.allclose(np.hypot(*t.T.astype(np.float64)), np.sqrt((i + 0.5) / n), atol=1e-6)
    t = pkg.renderer.dof_taps(3)
    golden = np.pi * (3.0 - np.sqrt(5.0))
    assert abs(golden - 2.399963229728653) < 1e-15 and np.allclose(np.arctan2(t[1, 1], t[1, 0]), golden, atol=1e-6)


def test_pixels_worked_by_hand(pkg, lib):
    C = colours(8, 8)
    cam = dict(z_near=1.0, z_far=2.0, focus_distance=1.0, coc_scale=4.0, max_radius=16.0)
    one = np.ones((8, 8), F)
    centre, right = np.zeros((1, 2), F), np.array([[0.5, 0.0]], F)
    # depth 1.0: den = 2 - 1 * (2 - 1) = 1, zv = 2, s = 4 * (1 - 1/2) = 2 everywhere; the maxima are 2
    out, tile, near, P = both(pkg, C, one, centre, samples=1, **cam)
    assert (tile == 2).all() and (near == 2).all() and (P[..., 0] == 2).all() and (P[..., 1] == 2).all()
    # one tap on the pixel itself: dist 0, behind 0, e = 2, cover 1, k = 4 / 1, a = 4 / 4 = 1.  out = (c * w + c) / (w + 1), w = (1/pi) / 4
    w = D.INV_PI / F(4.0)
    assert out.tobytes() == ((C * w + C * F(1.0)) / (w + F(1.0))).astype(F).tobytes()
    # the tap (0.5, 0): ox = 1, the right neighbour at dist 1: cover = clamp01(2 - 1) = 1, a = 1.  In column 7 it is outside: nothing enters,
    # and the pixel keeps its bits
    out, _, _, _ = both(pkg, C, one, right, samples=1, **cam)
    assert out[:, :7].tobytes() == ((C[:, :7] * w + C[:, 1:] * F(1.0)) / (w + F(1.0))).astype(F).tobytes() and out[:, 7].tobytes() == C[:, 7].tobytes()
    # two taps: k = 4 / 2 = 2, a = 2 / 4 = 0.5 each, in order
    two = np.array([[0.0, 0.0], [0.5, 0.0]], F)
    out, _, _, _ = both(pkg, C, one, two, samples=2, **cam)
    h = F(0.5)
    assert out[:, :7].tobytes() == (((C[:, :7] * w + C[:, :7] * h) + C[:, 1:] * h) / ((w + h) + h)).astype(F).tobytes()
    # depth 0 is the near plane (zv = 1 * 2 / 2 = 1 = the focus: s = 0); a depth above 1 with den <= 0, and a NaN, are the far plane
    z = one.copy()
    z[0, 0], z[0, 1], z[0, 2], z[0, 3] = 0.0, 3.0, NAN, 2.0                       # den = 2, -1, NaN, 0
    _, _, _, P = both(pkg, C, z, centre, samples=1, **cam)
    assert P[0, :4, 1].tolist() == [1.0, 2.0, 2.0, 2.0] and P[0, :4, 0].tolist() == [0.0, 2.0, 2.0, 2.0]
    # in front of the focus plane s is negative, and it is clamped on both sides: focus 1.5 -> at zv = 1: 64 * (1 - 1.5) = -32 -> -16; zv = 2: 16
    _, tile, _, P = both(pkg, C, z, centre, samples=1, **dict(cam, focus_distance=1.5, coc_scale=64.0))
    assert P[0, 0, 0] == -16.0 and P[0, 1, 0] == 16.0 and tile[0, 0] == 16.0
    # coc_scale = 0: nothing is out of focus, the frame is copied
    out, tile, near, P = both(pkg, C, z, None, samples=16, **dict(cam, coc_scale=0.0))
    assert out.tobytes() == C.tobytes() and (tile == 0).all() and (near == 0).all() and (P[..., 0] == 0).all()
    # the occlusion rule: the pixel (3, 3) is at the focus (depth 0: s = 0, a = A0), everything else behind it at s = 2.  Its tap to the right
    # lands on a background pixel at dist 1: behind = 1, e = min(2, A0) = A0, cover = clamp01(A0 - 1) = 0: rejected, and (3, 3) keeps its bits.
    # The background pixel (2, 3) looks at (3, 3), which is in FRONT: behind = 0, e = a_q = A0: cover 0 as well -- a sharp disc is small
    z = one.copy()
    z[3, 3] = 0.0
    out, _, near, _ = both(pkg, C, z, right, samples=1, depth_extent=0.25, **cam)
    assert (near == 2).all() and out[3, 3].tobytes() == C[3, 3].tobytes() and out[3, 2].tobytes() == C[3, 2].tobytes()
    assert out[3, 4].tobytes() == ((C[3, 4] * w + C[3, 5] * F(1.0)) / (w + F(1.0))).astype(F).tobytes()
    assert (D.dof(C, z, right, samples=1, depth_extent=0.25, defect="no occlusion rule", **cam)[0][3, 3] != C[3, 3]).any()
    # a NaN colour behind a zero weight does not spread: (4, 3) is NaN, (3, 3) rejects it
    Cn = C.copy()
    Cn[3, 4] = NAN
    out, _, _, _ = both(pkg, Cn, z, right, samples=1, depth_extent=0.25, **cam)
    assert out[3, 3].tobytes() == Cn[3, 3].tobytes() and np.isnan(out[3, 4]).all() and np.isfinite(np.delete(out.reshape(-1, 3), [3 * 8 + 4], 0)).all()
    assert np.isnan(D.dof(Cn, z, right, samples=1, depth_extent=0.25, defect="rejected tap multiplied", **cam)[0][3, 3]).all()
    # a 1 x 1 frame
    c1 = colours(1, 1)
    out, tile, near, P = both(pkg, c1, np.ones((1, 1), F), two, samples=2, **cam)
    assert tile.shape == (1, 1) and near[0, 0] == 2 and out.tobytes() == ((c1 * w + c1 * h) / (w + h)).astype(F).tobytes()


def test_the_window_at_the_grids_edge(pkg, lib):
    W, H = SIZES[3]
    C = colours(W, H)
    cam = dict(z_near=1.0, z_far=2.0, focus_distance=1.0, coc_scale=4.0)
    z = np.zeros((H, W), F)                                                      # everything at the focus ...
    z[3, 2], z[39, 71] = 1.0, 0.5                                                # ... but one pixel in tile (0, 0): s = 2, one in the last tile: zv = 4/3, s = 1
    _, tile, near, _ = both(pkg, C, z, None, samples=4, max_radius=16.0, **cam)  # Rt = 2
    assert (tile != 0).sum() == 2 and tile[0, 0] == 2.0 and tile[4, 8] == 1.0
    reach = np.zeros((5, 9), bool)
    reach[:3, :3], reach[2:, 6:] = True, True
    assert ((near != 0) == reach).all() and (near[:3, :3] == 2.0).all() and (near[2:, 6:] == 1.0).all()
    _, _, near, _ = both(pkg, C, z, None, samples=4, max_radius=8.0, **cam)      # Rt = 1
    assert (near != 0).sum() == 2 * 2 + 2 * 2
    _, _, near, _ = both(pkg, C, z, None, samples=4, max_radius=17.0, **cam)     # Rt = ceil(17 / 8) = 3
    assert (near != 0).sum() == 4 * 4 + 4 * 4
    z[20, 36] = 1.0                                                              # where two windows meet the larger wins
    _, _, near, _ = both(pkg, C, z, None, samples=4, max_radius=16.0, **cam)
    assert near[2, 6] == 2.0 and near[4, 8] == 1.0 and near[2, 2] == 2.0


def random_planes(rng, W, H):
    """(colour, depth) with everything the definition distinguishes: regions of one depth each (the near plane 0, in front of the focus, about
    at it, behind it, the far plane 1.0 exactly, beyond it) so that the maxima have ties, single pixels with noise, NaN depths and NaN colours"""
    C = rng.uniform(0.0, 4.0, (H, W, 3)).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    region = (ys // 6) * 97 + xs // 11
    kinds = np.array([0.0, 0.5, 0.9, 0.91162, 0.95, 0.98, 1.0, 1.2, 0.9], F)
    pick = rng.integers(0, len(kinds), region.max() + 1)
    z = kinds[pick[region]]
    noisy = rng.random((H, W)) < 0.1
    z = np.where(noisy, z + rng.uniform(-0.03, 0.03, (H, W)).astype(F), z).astype(F)
    where = rng.permutation(W * H)                                               # every kind at least once, also in a frame of two regions
    z.reshape(-1)[where[:len(kinds)]] = kinds
    for k in range(max(W * H // 200, 1)):                                        # a few of each, at least one
        z.reshape(-1)[where[len(kinds) + k]] = NAN
        C[rng.integers(0, H), rng.integers(0, W), k % 3] = NAN
    if W * H <= 64:                                                              # one tile: a NaN under a disc of max_radius would be gathered by every pixel,
        C = np.nan_to_num(C, nan=1.0)                                            # so the frame's one NaN colour lies on its pixel at the focus distance 5
        C.reshape(-1, 3)[where[3], 0] = NAN                                      # (kinds[3]: |s| < A0 under every block below), which no tap covers
    return C, z


CASES = [dict(samples=1), dict(samples=16), dict(samples=48, max_radius=16.0), dict(samples=16, max_radius=6.5, coc_scale=20.0, depth_extent=0.05),
         dict(samples=16, coc_scale=0.0)]


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
def test_the_arbiters_equal_numpy_by_bytes(pkg, lib, width, height):
    rng = np.random.default_rng(9500 + width)
    C, z = random_planes(rng, width, height)
    assert (z == 0).any() and (z == 1).any() and (z > 1).any() and np.isnan(z).any() and np.isnan(C).any()
    for kw in CASES:
        out, tile, _, P = both(pkg, C, z, None, **dict(CAMERA, **kw))
        assert np.isfinite(out).all(-1).mean() >= 0.75, (kw, float(np.isfinite(out).all(-1).mean()))
        if kw.get("coc_scale", 8.0) > 0:
            assert (P[..., 0] < 0).any() and (P[..., 0] > 0).any()               # a focus plane inside the scene
    # a table of the caller's, pixels in any order, some twice
    taps2 = rng.uniform(-0.7, 0.7, (7, 2)).astype(F)
    tile, near, P = D.prepare(z, **CAMERA)
    xy = np.stack([rng.integers(0, width, 50), rng.integers(0, height, 50)], -1)
    got = pkg.renderer.dof_pixels(xy, C, P, near, taps2, samples=7, **CAMERA)
    same(got, D.gather(C, P, near, taps2, samples=7)[xy[:, 1], xy[:, 0]], "any order")


@pytest.mark.parametrize("defect", D.DEFECTS)
def test_every_deliberate_defect_changes_output_bytes(defect):
    W, H = SIZES[3]
    C, z = random_planes(np.random.default_rng(9600), W, H)
    kw = dict(samples=16, max_radius=16.0, **CAMERA)
    good = np.concatenate([a.reshape(-1) for a in D.dof(C, z, **kw)])
    broken = np.concatenate([a.reshape(-1) for a in D.dof(C, z, defect=defect, **kw)])
    assert np.nan_to_num(good, nan=-1.0).tobytes() != np.nan_to_num(broken, nan=-1.0).tobytes(), defect


# ---- what it is for: three scenes at 64 x 40, numpy alone -------------------------------------------------------------------------------------------
W0, H0 = 64, 40
LENS = dict(z_near=0.5, z_far=50.0, focus_distance=2.0, coc_scale=12.0, max_radius=16.0, depth_extent=0.5)


def depth_of(zv, z_near=0.5, z_far=50.0):
    """the prepass depth of a view distance: the forward projection"""
    return (z_far / (z_far - z_near) * (1.0 - z_near / np.asarray(zv, np.float64))).astype(F)


def texture(seed):
    """a background with detail at every scale: blocks of 4 x 4 pixels of random colour"""
    rng = np.random.default_rng(seed)
    return np.kron(rng.uniform(0.1, 3.0, (H0 // 4, W0 // 4, 3)), np.ones((4, 4, 1))).astype(F)


def test_a_sharp_foreground_in_front_of_a_blurred_background_keeps_its_bits():
    """(a) a square at the focus distance in front of a background at 40 (s = 12 * (1 - 2/40) = 11.4).  Every foreground pixel none of whose taps
    is closer than a sharp disc's radius A0 has all its taps uncovered -- one on the foreground meets a disc of radius A0, one on the background
    is behind and may not reach past the pixel's own A0 -- and equals C by bits.  The background IS blurred, and without the rule it bleeds in"""
    C = texture(3)
    square = np.zeros((H0, W0), bool)
    square[12:28, 24:40] = True
    C[square] = np.random.default_rng(4).uniform(0.5, 2.0, (int(square.sum()), 3)).astype(F)
    z = np.where(square, depth_of(2.0), depth_of(40.0)).astype(F)
    for samples in (16, 48):
        out, _, near, P = D.dof(C, z, samples=samples, **LENS)
        assert (np.abs(P[square][:, 0]) < 1e-3).all() and (P[~square][:, 0] > 11.0).all()
        nearest = np.sqrt((D.taps(samples).astype(np.float64) ** 2).sum(-1)).min() * near[np.mgrid[0:H0, 0:W0][0] // 8, np.mgrid[0:H0, 0:W0][1] // 8]
        uncovered = square & (nearest > float(D.A0) + 1e-3)
        changed = (out != C).any(-1)
        print(f"sharp foreground, {samples} samples: {int(uncovered.sum())} of {int(square.sum())} foreground pixels have every tap uncovered; {int(changed[~square].sum())} of "
              f"{int((~square).sum())} background pixels changed")
        assert uncovered.sum() == square.sum() and out[uncovered].tobytes() == C[uncovered].tobytes()
        assert changed[~square].mean() >= 0.9
        bled = D.dof(C, z, samples=samples, defect="no occlusion rule", **LENS)[0]
        assert (bled[square] != C[square]).any(-1).mean() >= 0.5


def test_a_constant_field_stays_constant():
    """(b) one colour at random depths -- in front of the focus, behind it, the far plane, beyond it: the constant within 1e-6 relative"""
    rng = np.random.default_rng(5)
    colour = np.array((0.7, 1.3, 2.9), F)
    C = np.broadcast_to(colour, (H0, W0, 3)).copy()
    z = np.where(rng.random((H0, W0)) < 0.5, depth_of(rng.uniform(0.6, 45.0, (H0, W0))), rng.choice(np.array([0.0, 1.0, 1.5, 0.97], F), (H0, W0))).astype(F)
    for samples in (1, 16, 48):
        out = D.dof(C, z, samples=samples, **LENS)[0]
        rel = np.abs(out.astype(np.float64) - colour) / colour
        print(f"constant field, {samples} samples: the largest relative difference is {rel.max():.3e}, {int((out != C).any(-1).sum())} pixels differ in bits")
        assert rel.max() <= 1e-6, float(rel.max())


def scatter_scene():
    """a sharp object at the focus, a near object far out of focus in front of it, a textured background behind"""
    C = texture(7)
    ys, xs = np.mgrid[0:H0, 0:W0]
    zv = np.full((H0, W0), 30.0)
    focus = (np.abs(xs - 40) <= 9) & (np.abs(ys - 22) <= 9)
    front = (xs - 16) ** 2 + (ys - 16) ** 2 <= 49
    C[focus] = np.where(((xs + ys) % 4 < 2)[focus][:, None], (3.0, 2.5, 0.3), (0.2, 0.4, 2.0)).astype(F)
    C[front] = (2.5, 0.4, 0.4)
    zv[focus], zv[front] = 2.0, 1.0
    return C, depth_of(zv)


def scatter_ratio(samples):
    C, z = scatter_scene()
    out, _, _, P = D.dof(C, z, samples=samples, **LENS)
    truth = D.scatter(C, P, **LENS)
    one = np.abs(D.reinhard(C) - D.reinhard(truth)).mean()
    gathered = np.abs(D.reinhard(out) - D.reinhard(truth)).mean()
    return one, gathered


def test_the_gather_comes_closer_to_a_brute_force_scatter_than_the_frame_is():
    """(c) against a float64 scatter of the same discs under the same occlusion rule, through Reinhard, over the whole frame: the gather's mean
    error is smaller than the unfiltered frame's.  The figures are printed (DESIGN.md 6u quotes them)"""
    for samples in (16, 48):
        one, gathered = scatter_ratio(samples)
        print(f"scatter, {samples} samples: the frame {one:.4f}, the gather {gathered:.4f}, ratio {gathered / one:.3f}")
        assert gathered < one, (samples, one, gathered)
