"""The motion blur on a machine without a GPU: the numpy restatement (tests/motion_blur_reference.py) pinned on pixels worked by hand, the host
arbiters arctic_motion_blur_prepare and arctic_motion_blur_pixels against it BY BYTES, every deliberate defect shown to change output bytes, and
what the feature is for: a moving disc is brought closer to the mean of its sub-frame positions, a static square in front of a moving background
keeps its colour when the depth plane is given, and a tile outside a fast tile's window is copied."""
import numpy as np
import pytest

import motion_blur_reference as M

F = np.float32
SIZES = ((8, 8), (17, 9), (40, 24), (72, 40))     # (width, height); the last: 9 x 5 tiles, max_radius 16 gives a window of two tiles cut at every edge
NAN, INF = F(np.nan), F(np.inf)


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


def arbiters(pkg, color, velocity, depth=None, **kw):
    """steps 1 to 4 by the host arbiters, every pixel listed: (out, tile_max2, neighbour_max2, P)"""
    H, W = np.asarray(velocity).shape[:2]
    tile, near, P = pkg.renderer.motion_blur_prepare(velocity, depth, **kw)
    ys, xs = np.mgrid[0:H, 0:W]
    out = pkg.renderer.motion_blur_pixels(np.stack([xs, ys], -1).reshape(-1, 2), color, P, near, **kw)
    return out.reshape(H, W, 3), tile, near, P


def both(pkg, color, velocity, depth=None, **kw):
    """numpy's result, which the arbiters must reproduce by bytes"""
    want = M.blur(color, velocity, depth, **kw)
    for g, w, name in zip(arbiters(pkg, color, velocity, depth, **kw), want, ("out", "tile_max2", "neighbour_max2", "P")):
        same(g, w, name)
    return want


def colours(W, H, seed=1):
    return np.random.default_rng(seed).uniform(0.25, 4.0, (H, W, 3)).astype(F)


def test_pixels_worked_by_hand(pkg, lib):
    C = colours(8, 8)
    v = np.zeros((8, 8, 2), F)
    # a still frame is copied; P = {0.5, 0}; the maxima are zero
    out, tile, near, P = both(pkg, C, v, samples=7)
    assert out.tobytes() == C.tobytes() and (tile == 0).all() and (near == 0).all() and (P[..., 0] == 0.5).all() and (P[..., 1] == 0).all()
    # the clamp to max_radius: v = (60, 80), shutter 1: h = (30, 40), len 50 > 10: s = 10 / 50, h = h * s
    v[2, 5] = (60.0, 80.0)
    s = F(10.0) / F(50.0)
    _, tile, near, P = both(pkg, C, v, max_radius=10.0, samples=1)
    hx, hy = F(30.0) * s, F(40.0) * s
    assert tile[0, 0].tolist() == [hx, hy] and near[0, 0].tolist() == [hx, hy] and P[2, 5, 0] == np.sqrt(hx * hx + hy * hy) and (np.delete(P[..., 0].reshape(-1), 2 * 8 + 5) == 0.5).all()
    # a velocity that is not finite is no velocity: h = (0, 0), l = 0.5 -- also when shutter = 0 turns an infinity into a NaN
    for bad, shutter in (((NAN, 3.0), 1.0), ((INF, 0.0), 1.0), ((2.0, -INF), 1.0), ((INF, 1.0), 0.0), ((3e38, 3e38), 4.0)):
        v[:] = 0
        v[4, 4] = bad
        out, tile, near, P = both(pkg, C, v, shutter=shutter, samples=3)
        assert (tile == 0).all() and (P[..., 0] == 0.5).all() and out.tobytes() == C.tobytes(), bad
    # 1e30 is finite: its squares overflow, len = inf, s = 0, h = 0 * h = 0
    v[4, 4] = (1e30, 0.0)
    _, tile, _, P = both(pkg, C, v, samples=3)
    assert (tile == 0).all() and (P[..., 0] == 0.5).all()
    # the tie of the tile maximum: (3, 4) in lane 10, (4, 3) in lane 5 and (5, 0) in lane 20 have the same squared length: lane 5 wins.  shutter 2: h = v
    v[:] = 0
    v[1, 2], v[0, 5], v[2, 4] = (3.0, 4.0), (4.0, 3.0), (5.0, 0.0)
    _, tile, _, _ = both(pkg, C, v, shutter=2.0, samples=1)
    assert tile[0, 0].tolist() == [4.0, 3.0]
    v[0, 5] = 0
    _, tile, _, _ = both(pkg, C, v, shutter=2.0, samples=1)
    assert tile[0, 0].tolist() == [3.0, 4.0]
    # samples = 1: t = 0, the tap is the pixel itself, dist 0: f = b = 1, both cones and cylinders 1, a = 4.  out = (c*w + c*4) / (w + 4)
    v[:] = (8.0, 0.0)                                                            # h = (4, 0) everywhere, l = 4
    out, _, near, P = both(pkg, C, v, samples=1)
    w = F(1.0) / F(4.0)
    assert (near == (4.0, 0.0)).all() and (P[..., 0] == 4.0).all()
    assert out.tobytes() == ((C * w + C * F(4.0)) / (w + F(4.0))).astype(F).tobytes()
    # a tap outside the frame: samples = 2, t = -0.5 and 0.5; pixel (0, 0): floor(0.5 - 2) = -2 is outside, floor(0.5 + 2) = 2 is pixel (2, 0)
    # at dist 2: cone = 1 - 2/4 = 0.5 twice, the cylinders 1: a = (0.5 + 0.5) + 2 = 3.  Pixel (7, 0) likewise with (5, 0)
    out, _, _, _ = both(pkg, C, v, samples=2)
    assert out[0, 0].tobytes() == ((C[0, 0] * w + C[0, 2] * F(3.0)) / (w + F(3.0))).astype(F).tobytes()
    assert out[0, 7].tobytes() == ((C[0, 7] * w + C[0, 5] * F(3.0)) / (w + F(3.0))).astype(F).tobytes()
    assert out[3, 4].tobytes() == (((C[3, 4] * w + C[3, 2] * F(3.0)) + C[3, 6] * F(3.0)) / ((w + F(3.0)) + F(3.0))).astype(F).tobytes()
    # NaN depth of a tap: f = b = 0, the cylinders stay: a = 2.  NaN depth of the pixel itself: the same for each of its taps
    z = np.full((8, 8), 0.5, F)
    z[0, 2], z[5, 4] = NAN, NAN
    out, _, _, _ = both(pkg, C, v, z, samples=2)
    assert out[0, 0].tobytes() == ((C[0, 0] * w + C[0, 2] * F(2.0)) / (w + F(2.0))).astype(F).tobytes()
    assert out[5, 4].tobytes() == (((C[5, 4] * w + C[5, 2] * F(2.0)) + C[5, 6] * F(2.0)) / ((w + F(2.0)) + F(2.0))).astype(F).tobytes()
    # the depth order: a tap 10 extents BEHIND the pixel has f = 0, b = 1: a = cone(l_p) + 2 = 2.5; one in FRONT has f = 1, b = 0: the same here
    z[:] = 0.5
    z[1, 2], z[1, 6] = 1.0, 0.0
    out, _, _, _ = both(pkg, C, v, z, samples=2)
    assert out[1, 4].tobytes() == (((C[1, 4] * w + C[1, 2] * F(2.5)) + C[1, 6] * F(2.5)) / ((w + F(2.5)) + F(2.5))).astype(F).tobytes()
    # the dither: samples = 1, t = 2o.  Pixel (1, 0): B = 8, o = 8.5/16 - 0.5 = 0.03125, t = 0.0625: the tap is the pixel itself at dist 0.25:
    # cone = 0.9375 twice, a = 3.875.  Pixel (0, 0): B = 0, o = -0.46875, t = -0.9375: floor(0.5 - 3.75) is outside: out = (c*w) / w
    out, _, _, _ = both(pkg, C, v, samples=1, flags=M.DITHER)
    assert out[0, 1].tobytes() == ((C[0, 1] * w + C[0, 1] * F(3.875)) / (w + F(3.875))).astype(F).tobytes()
    assert out[0, 0].tobytes() == ((C[0, 0] * w) / w).astype(F).tobytes()
    assert M.BAYER.tolist() == [[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]
    # a NaN colour behind a zero weight: only (7, 7) moves, so d = (4, 0) for the tile and every other pixel is still (l = 0.5).  Pixel (0, 3),
    # samples = 4: the taps are x = -3, -1 (outside), 1 and 3 at dist 1 and 3 -- both cones 0, the cylinder of 0.5 is 0: a = 0, and the NaN at
    # (3, 3) does not enter: out = (c * 2) / 2 = c
    v[:] = 0
    v[7, 7] = (8.0, 0.0)
    Cn = C.copy()
    Cn[3, 3] = NAN
    out, _, near, _ = both(pkg, Cn, v, samples=4)
    assert near[0, 0].tolist() == [4.0, 0.0] and out[3, 0].tobytes() == Cn[3, 0].tobytes() and np.isnan(out[3, 3]).all() and np.isfinite(np.delete(out.reshape(-1, 3), 27, 0)).all()
    assert np.isnan(M.blur(Cn, v, samples=4, defect="rejected tap multiplied")[0][3, 0]).all()
    # a 1 x 1 frame: v = (3, 0): d = h = (1.5, 0); samples = 3: t = -2/3, 0, 2/3: the outer taps fall outside, the middle one is the pixel: a = 4
    c1, v1 = colours(1, 1), np.array([[[3.0, 0.0]]], F)
    out, tile, near, P = both(pkg, c1, v1, samples=3)
    w1 = F(1.0) / F(1.5)
    assert tile.shape == (1, 1, 2) and near[0, 0].tolist() == [1.5, 0.0] and P[0, 0].tolist() == [1.5, 0.0]
    assert out.tobytes() == ((c1 * w1 + c1 * F(4.0)) / (w1 + F(4.0))).astype(F).tobytes()


def test_the_window_and_its_tie_at_the_grids_edge(pkg, lib):
    W, H = SIZES[3]
    C = colours(W, H)
    v = np.zeros((H, W, 2), F)
    v[3, 2], v[39, 71] = (6.0, 0.0), (0.0, 6.0)                                  # one fast pixel in tile (0, 0), one in the last tile (8, 4)
    _, tile, near, _ = both(pkg, C, v, max_radius=16.0, samples=3)               # Rt = 2
    assert (tile != 0).any(-1).sum() == 2 and tile[0, 0].tolist() == [3.0, 0.0] and tile[4, 8].tolist() == [0.0, 3.0]
    reach = np.zeros((5, 9), bool)
    reach[:3, :3], reach[2:, 6:] = True, True
    assert ((near != 0).any(-1) == reach).all() and (near[:3, :3] == (3.0, 0.0)).all() and (near[2:, 6:] == (0.0, 3.0)).all()
    _, _, near, _ = both(pkg, C, v, max_radius=8.0, samples=3)                   # Rt = 1
    reach[:] = False
    reach[:2, :2], reach[3:, 7:] = True, True
    assert ((near != 0).any(-1) == reach).all()
    _, _, near, _ = both(pkg, C, v, max_radius=17.0, samples=3)                  # Rt = ceil(17 / 8) = 3
    assert (near != 0).any(-1).sum() == 4 * 4 + 4 * 4
    # equal lengths in one window: row-major, the first wins.  Tiles (1, 0) and (0, 1) both reach tile (1, 1); (1, 0) comes first
    v[:] = 0
    v[2, 12], v[12, 2] = (0.0, 10.0), (10.0, 0.0)
    _, tile, near, _ = both(pkg, C, v, max_radius=8.0, samples=3)
    assert tile[0, 1].tolist() == [0.0, 5.0] and tile[1, 0].tolist() == [5.0, 0.0] and near[1, 1].tolist() == [0.0, 5.0] and near[0, 0].tolist() == [0.0, 5.0]
    assert near[2, 0].tolist() == [5.0, 0.0] and near[0, 2].tolist() == [0.0, 5.0] and near[2, 2].tolist() == [0.0, 0.0]


def random_planes(rng, W, H):
    """(colour, velocity2, depth) with everything the definition distinguishes: regions of one velocity each (zero, below a pixel, ordinary, far
    beyond max_radius) so that the maxima have ties, single pixels with noise, velocities that are NaN or infinite, NaN colours and NaN depths"""
    C = rng.uniform(0.0, 4.0, (H, W, 3)).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    region = (ys // 6) * 97 + xs // 11
    kinds = np.array([(0.0, 0.0), (0.3, -0.2), (5.0, 2.0), (-9.0, 7.0), (0.0, -14.0), (90.0, -40.0), (2.0, 2.0), (-0.75, 0.0)], F)
    pick = rng.integers(0, len(kinds), region.max() + 1)
    v = kinds[pick[region]]
    noisy = rng.random((H, W)) < 0.1
    v = np.where(noisy[..., None], v + rng.uniform(-3, 3, (H, W, 2)).astype(F), v).astype(F)
    z = (0.3 + 0.05 * pick[region] + rng.uniform(0, 0.04, (H, W))).astype(F)
    n = W * H
    for k in range(max(n // 200, 1)):                                            # a few of each, at least one
        y, x = rng.integers(0, H), rng.integers(0, W)
        v[y, x] = ((NAN, 1.0), (INF, 0.0), (2.0, -INF), (1e30, 1e30))[k % 4]
        z[rng.integers(0, H), rng.integers(0, W)] = NAN
        C[rng.integers(0, H), rng.integers(0, W), k % 3] = NAN
    return C, v, z


CASES = [dict(samples=1), dict(samples=7, flags=M.DITHER), dict(samples=15, max_radius=16.0), dict(samples=15, max_radius=6.5, shutter=0.5, depth_extent=0.01, flags=M.DITHER)]


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
def test_the_arbiters_equal_numpy_by_bytes(pkg, lib, width, height):
    rng = np.random.default_rng(9000 + width)
    C, v, z = random_planes(rng, width, height)
    for kw in CASES:
        for depth in (z, None):
            out = both(pkg, C, v, depth, **kw)[0]
            assert np.isfinite(out).all(-1).mean() >= 0.75 or width * height <= 64, (kw, float(np.isfinite(out).all(-1).mean()))
    # pixels in any order, some twice
    tile, near, P = M.prepare(v, z)
    xy = np.stack([rng.integers(0, width, 50), rng.integers(0, height, 50)], -1)
    got = pkg.renderer.motion_blur_pixels(xy, C, P, near, samples=7)
    same(got, M.gather(C, P, near, samples=7)[xy[:, 1], xy[:, 0]], "any order")


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_deliberate_defect_changes_output_bytes(defect):
    W, H = SIZES[3]
    C, v, z = random_planes(np.random.default_rng(9100), W, H)
    kw = dict(samples=7, max_radius=16.0, flags=M.DITHER)
    good = np.concatenate([a.reshape(-1) for a in M.blur(C, v, z, **kw)])
    broken = np.concatenate([a.reshape(-1) for a in M.blur(C, v, z, defect=defect, **kw)])
    assert np.nan_to_num(good, nan=-1.0).tobytes() != np.nan_to_num(broken, nan=-1.0).tobytes(), defect


# ---- what it is for: three scenes at 64 x 40, numpy alone -----------------------------------------------------------------------------------------
W0, H0 = 64, 40


def stripes(offset=0.0):
    """a striped background: the colour depends on the column alone, four columns per stripe"""
    xs = np.arange(W0) + 0.5 - offset
    k = np.floor(xs / 4.0).astype(int) % 3
    return np.broadcast_to(np.array([(0.2, 0.6, 1.5), (1.2, 0.3, 0.1), (0.5, 0.5, 0.5)])[k][None], (H0, W0, 3)).copy()


def disc_frame(cx, cy, radius=7.0):
    ys, xs = np.mgrid[0:H0, 0:W0]
    inside = (xs + 0.5 - cx) ** 2 + (ys + 0.5 - cy) ** 2 <= radius * radius
    frame = stripes()
    frame[inside] = (4.0, 2.0, 0.5)
    return frame, inside


def disc_ratio(samples, flags=0):
    vel = np.array([12.0, 4.0])
    sharp, inside = disc_frame(32.0, 20.0)
    truth = np.mean([disc_frame(32.0 + vel[0] * ((k + 0.5) / 64 - 0.5), 20.0 + vel[1] * ((k + 0.5) / 64 - 0.5))[0] for k in range(64)], 0)
    v = np.where(inside[..., None], -vel, 0.0).astype(F)                         # velocity2 points to where the surface point WAS
    z = np.where(inside, 0.3, 0.8).astype(F)
    out = M.blur(sharp.astype(F), v, z, shutter=1.0, max_radius=8.0, samples=samples, depth_extent=0.05, flags=flags)[0]
    differ = (np.abs(truth - sharp) > 1e-9).any(-1)                               # (the mean of 64 equal numbers may round)
    one = np.abs(M.reinhard(sharp) - M.reinhard(truth))[differ].mean()
    blurred = np.abs(M.reinhard(out) - M.reinhard(truth))[differ].mean()
    return int(differ.sum()), one, blurred


def test_a_moving_disc_comes_closer_to_the_mean_of_its_positions():
    """Against the mean of 64 sub-frame positions, through Reinhard, on the pixels where that mean differs from the sharp frame.  The condition is
    the issue's: the blurred frame's error is at most 0.6 of the sharp frame's at 15 samples.  The figures are printed (DESIGN.md 6t quotes them)"""
    for samples, flags in ((15, 0), (15, M.DITHER), (31, 0), (7, 0)):
        n, one, blurred = disc_ratio(samples, flags)
        print(f"moving disc, {samples} samples, flags {flags}: {n} pixels, one frame {one:.4f}, blurred {blurred:.4f}, ratio {blurred / one:.3f}")
        if samples == 15 and flags == 0:
            assert n >= 200 and blurred <= 0.6 * one, (n, one, blurred)


def test_a_static_square_in_front_keeps_its_colour_only_with_the_depth_plane():
    """A static square (depth 0.3) in front of a striped background (depth 0.8) that moves at (10, 0).  With the depth plane every pixel of the
    square's interior -- the square less its outermost ring, whose taps closer than half a pixel can floor into the background -- stays within 4
    fp32 ulps per channel (the division by w); without it the background bleeds in: the mean change exceeds 0.05"""
    C = stripes().astype(F)
    square = np.zeros((H0, W0), bool)
    square[12:28, 24:40] = True
    interior = np.zeros_like(square)
    interior[13:27, 25:39] = True
    colour = np.array((2.0, 1.0, 3.0), F)
    C[square] = colour
    v = np.where(square[..., None], 0.0, (10.0, 0.0)).astype(F)
    z = np.where(square, 0.3, 0.8).astype(F)
    kw = dict(shutter=1.0, max_radius=8.0, samples=15, depth_extent=0.05)
    with_depth, without = M.blur(C, v, z, **kw)[0], M.blur(C, v, None, **kw)[0]
    ulps = np.abs(with_depth[interior].view(np.int32).astype(np.int64) - C[interior].view(np.int32).astype(np.int64)).max()
    change = np.abs(without[interior].astype(np.float64) - C[interior])
    print(f"static square: with depth at most {ulps} ulps from its colour; without depth the change is max {change.max():.3f}, mean {change.mean():.3f}")
    assert ulps <= 4 and change.mean() > 0.05
    assert (with_depth[~square] != C[~square]).any()                             # and the background IS blurred


def test_a_tile_outside_the_window_is_copied():
    """only tile (0, 0) moves, at (6, 0): with max_radius 8 the window is one tile, so every pixel of a tile outside columns 0..15, rows 0..15
    is C bit for bit"""
    C = colours(W0, H0, 5)
    v = np.zeros((H0, W0, 2), F)
    v[:8, :8] = (6.0, 0.0)
    out, _, near, _ = M.blur(C, v, shutter=1.0, max_radius=8.0, samples=15)
    outside = np.ones((H0, W0), bool)
    outside[:16, :16] = False
    changed = (out != C).any(-1)
    print(f"locality: {int(changed.sum())} pixels changed, the last in column {np.nonzero(changed.any(0))[0].max()}, row {np.nonzero(changed.any(1))[0].max()}")
    assert out[outside].tobytes() == C[outside].tobytes() and changed[:8, :8].all()
    # inside the window but beyond the reach of a tap (3 pixels) a still pixel's taps with a weight all fall into the pixel itself: its own colour
    # averaged with itself, which the division by w may round
    rel = np.abs(out[:, 12:].astype(np.float64) - C[:, 12:]) / C[:, 12:]
    assert rel.max() <= 4 * 2.0 ** -24, float(rel.max())
