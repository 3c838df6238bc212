"""The temporal anti-aliasing resolve on a machine without a GPU: the numpy restatement (tests/taa_reference.py) pinned on pixels worked by hand,
the host arbiter arctic_taa_pixels and arctic_jitter_proj_view against it BY BYTES, every deliberate defect shown to change output bytes, and what
the feature is for: eight jittered frames of an analytic scene resolve to at most half the error of one frame, and a translating pattern is
tracked through velocity2."""
import numpy as np
import pytest

import taa_reference as T

F = np.float32
SIZES = ((1, 1), (8, 8), (17, 9), (40, 24))     # (width, height)


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


def frame3(centre, others, special=None):
    """a 3x3 grey frame: `centre` at (1, 1), `others` elsewhere, special = {(x, y): value}"""
    c = np.full((3, 3, 3), others, F)
    c[1, 1] = centre
    for (x, y), v in (special or {}).items():
        c[y, x] = v
    return c


def history3(value, n, special=None):
    p = np.empty((3, 3, 4), F)
    p[..., :3], p[..., 3] = value, n
    for (x, y), v in (special or {}).items():
        p[y, x] = v
    return p


def test_pixels_worked_by_hand():
    cur = frame3(2.0, 0.0, {(2, 2): 4.0})                     # the box of (1, 1): lo 0, hi 4
    # T is empty: N = 1, out = c
    assert T.resolve(cur)[1, 1].tolist() == [2.0, 2.0, 2.0, 1.0]
    # zero velocity, j = 0: the running mean.  h = 1, N_q = 3: N = 4, a = 0.25, out = 1 + (2 - 1) * 0.25
    assert T.resolve(cur, None, history3(1.0, 3.0))[1, 1].tolist() == [1.25, 1.25, 1.25, 4.0]
    # ... and the cap: max_history = 2 gives N = 2, a = 0.5
    assert T.resolve(cur, None, history3(1.0, 3.0), max_history=2.0)[1, 1].tolist() == [1.5, 1.5, 1.5, 2.0]
    # the jitter and the velocity add up: v = (-0.25, 0), j = (0.25, 0) is the pixel's own centre
    vel = np.zeros((3, 3, 2), F)
    vel[..., 0] = -0.25
    varied = history3(1.0, 1.0, {(0, 1): (3.0, 3.0, 3.0, 1.0)})
    assert T.resolve(cur, vel, varied, jitter=(0.25, 0.0))[1, 1].tolist() == [1.5, 1.5, 1.5, 2.0]
    # ... without the jitter the fetch lies a quarter pixel to the left: h = 0.75 * 1 + 0.25 * 3 = 1.5, out = 1.5 + 0.5 * 0.5
    assert T.resolve(cur, vel, varied)[1, 1].tolist() == [1.75, 1.75, 1.75, 2.0]
    # a tap outside the frame: pixel (0, 1), v = (-0.5, 0): ix = -1, ax = 0.5; the left taps are rejected, S = 0.5, h = the right tap's
    vel[..., 0] = -0.5
    edge = frame3(0.0, 0.0, {(0, 1): 2.0, (1, 2): 4.0})
    got = T.resolve(edge, vel, history3(1.0, 3.0))[1, 0]
    assert got.tolist() == [1.25, 1.25, 1.25, 4.0]
    # min_weight rejecting: S = 0.5 is not above 0.5
    assert T.resolve(edge, vel, history3(1.0, 3.0), min_weight=0.5)[1, 0].tolist() == [2.0, 2.0, 2.0, 1.0]
    assert T.resolve(edge, vel, history3(1.0, 3.0), min_weight=0.49)[1, 0].tolist() == [1.25, 1.25, 1.25, 4.0]
    # a 1x1 frame: every neighbour is the pixel itself, the history is clamped to c
    one = T.resolve(np.full((1, 1, 3), 2.0, F), None, np.array([[[9.0, 0.0, 2.0, 5.0]]], F))
    assert one[0, 0].tolist() == [2.0, 2.0, 2.0, 6.0]
    # a NaN neighbour is ignored: (1, 0) is the second neighbour of (1, 1)
    nan = frame3(2.0, 0.0, {(1, 0): np.nan, (2, 2): 4.0})
    assert T.resolve(nan, None, history3(1.0, 3.0))[1, 1].tolist() == [1.25, 1.25, 1.25, 4.0]
    assert T.resolve(nan, None, history3(9.0, 1.0))[1, 1].tolist() == [3.0, 3.0, 3.0, 2.0]          # clamped to hi = 4: 4 + (2 - 4) * 0.5
    # ... but the FIRST neighbour starts the fold: a NaN there leaves lo and hi NaN, and no comparison clamps
    first = frame3(2.0, 0.0, {(0, 0): np.nan})
    assert T.resolve(first, None, history3(9.0, 1.0))[1, 1].tolist() == [5.5, 5.5, 5.5, 2.0]
    # a NaN, infinite or huge velocity rejects everything
    for v in (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38):
        for axis in (0, 1):
            vel = np.zeros((3, 3, 2), F)
            vel[1, 1, axis] = v
            assert T.resolve(cur, vel, history3(1.0, 3.0))[1, 1].tolist() == [2.0, 2.0, 2.0, 1.0], v
    # a NaN history colour behind a rejected tap (N_q = 0) is not looked at: v = (0.5, 0) takes (1, 1) and (2, 1) with 0.5 each
    vel = np.zeros((3, 3, 2), F)
    vel[1, 1, 0] = 0.5
    poisoned = history3(1.0, 3.0, {(2, 1): (np.nan, np.nan, np.nan, 0.0)})
    assert T.resolve(cur, vel, poisoned)[1, 1].tolist() == [1.25, 1.25, 1.25, 4.0]
    poisoned[1, 2, 3] = np.nan                                                                          # a NaN count is not > 0 either
    assert T.resolve(cur, vel, poisoned)[1, 1].tolist() == [1.25, 1.25, 1.25, 4.0]
    # the clamp engaging, below and above: h = 10 -> 4, out = 4 + (2 - 4) * 0.5; h = -3 -> 0, out = 0 + (2 - 0) * 0.5
    assert T.resolve(cur, None, history3(10.0, 1.0))[1, 1].tolist() == [3.0, 3.0, 3.0, 2.0]
    assert T.resolve(cur, None, history3(-3.0, 1.0))[1, 1].tolist() == [1.0, 1.0, 1.0, 2.0]
    # both blend forms: c = (3, 1, 0), h = (1, 1, 1), a = 0.5.  Plain: h + (c - h) * 0.5
    hdr = frame3(0.0, 0.0, {(1, 1): (3.0, 1.0, 0.0), (2, 2): 4.0})
    assert T.resolve(hdr, None, history3(1.0, 1.0))[1, 1].tolist() == [2.0, 1.0, 0.5, 2.0]
    # with the luma weight: wc = 1 / (1 + 3) = 0.25, wh = 1 / (1 + 1) = 0.5, kc = 0.125, kh = 0.25: out = (c * 0.125 + h * 0.25) / 0.375
    want = [float((F(3.0) * F(0.125) + F(0.25)) / F(0.375)), float((F(0.125) + F(0.25)) / F(0.375)), float(F(0.25) / F(0.375)), 2.0]
    assert T.resolve(hdr, None, history3(1.0, 1.0), flags=T.LUMA_WEIGHT)[1, 1].tolist() == want
    assert want[0] == pytest.approx(5.0 / 3.0, rel=1e-6) and want[1] == 1.0
    # ... a negative colour weighs 1: max(..., 0)
    dark = frame3(-1.0, -2.0, {(2, 2): 4.0})
    assert T.resolve(dark, None, history3(-1.0, 1.0), flags=T.LUMA_WEIGHT)[1, 1].tolist() == [-1.0, -1.0, -1.0, 2.0]


def test_the_halton_jitter():
    assert T.taa_jitter(0) == (0.0, 1.0 / 3.0 - 0.5) and T.taa_jitter(1) == (-0.25, 2.0 / 3.0 - 0.5) and T.taa_jitter(2) == (0.25, 1.0 / 9.0 - 0.5)
    assert T.taa_jitter(8) == T.taa_jitter(0) and T.taa_jitter(3, period=3) == T.taa_jitter(0)
    pts = np.array([T.taa_jitter(i) for i in range(8)])
    assert (np.abs(pts) < 0.5).all() and len({tuple(p) for p in pts}) == 8 and abs(pts.mean(0)).max() < 0.07


def random_frames(rng, W, H, calls, nan_calls=None):
    """colours in [0, 4) with NaNs (in the calls of nan_calls; None: in every call), velocities of a few pixels with entries that point outside
    the frame or are not finite"""
    frames, vels, jitters = [], [], []
    for k in range(calls):
        c = rng.uniform(0, 4, (H, W, 3)).astype(F)
        nans = rng.uniform(size=(H, W)) < 0.03
        if nan_calls is None or k in nan_calls:
            c[nans, 1] = np.nan
        v = rng.uniform(-3, 3, (H, W, 2)).astype(F)
        v[rng.uniform(size=(H, W)) < 0.2] = 0.0
        pick = rng.uniform(size=(H, W))
        v[pick < 0.05, 0] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -3e38, 100.0, -100.0])
        frames.append(c)
        vels.append(v)
        jitters.append(T.taa_jitter(k))
    return frames, vels, jitters


@pytest.mark.parametrize("width, height", SIZES)
@pytest.mark.parametrize("flags", [0, T.LUMA_WEIGHT])
def test_the_arbiter_equals_numpy_by_bytes(pkg, lib, width, height, flags):
    rng = np.random.default_rng(7000 + width)
    frames, vels, jitters = random_frames(rng, width, height, 5)
    ys, xs = np.mgrid[0:height, 0:width]
    xy = np.stack([xs, ys], -1).reshape(-1, 2)
    order = rng.permutation(len(xy))                                            # n pixels in any order
    kw = dict(max_history=3.0, min_weight=0.1, flags=flags)
    prev = None
    for call in range(5):                                                        # sequences of 1, 2 and 5 calls are this one's prefixes
        want = T.resolve(frames[call], vels[call], prev, jitter=jitters[call], **kw)
        got = pkg.renderer.taa_pixels(xy[order], frames[call], vels[call].reshape(-1, 2)[order], prev, jitter=jitters[call], **kw)
        assert got.tobytes() == want.reshape(-1, 4)[order].tobytes(), (call, np.nanmax(np.abs(got - want.reshape(-1, 4)[order])))
        prev = want
    assert width * height < 64 or (prev[..., 3].max() == 3.0 and (prev[..., 3] == 1.0).any())       # the cap is reached, and some pixels were rejected
    # a NULL velocity is zero
    assert pkg.renderer.taa_pixels(xy, frames[0], None, prev, **kw).tobytes() == T.resolve(frames[0], None, prev, **kw).tobytes()


def test_jitter_proj_view_equals_numpy_by_bits(pkg, lib):
    rng = np.random.default_rng(7100)
    for w, h, jx, jy in ((40, 24, 0.4, -0.3), (1, 1, 1.0, -1.0), (3840, 2160, *T.taa_jitter(5)), (17, 9, -0.0, 0.5)):
        m = rng.normal(size=(4, 4)).astype(F)
        got = pkg.renderer.jitter_proj_view(m, w, h, jx, jy)
        assert got.tobytes() == T.jitter_proj_view(m, w, h, jx, jy).tobytes()
        assert (got[:, 2:] == m[:, 2:]).all() and (got[:, :2] != m[:, :2]).any()
    # a point at screen position s under m lies at s + j under the jittered matrix
    m = np.array([[1.2, 0, 0, 0], [0, 1.7, 0, 0], [0, 0, -1.0, -1.0], [0.1, -0.2, -0.2, 0.3]], np.float64)     # [col][row]
    J = T.jitter_proj_view(m, 40, 24, 0.4, -0.3).astype(np.float64)
    screen = lambda M, p: (lambda c: np.array([(c[0] / c[3] + 1) * 20.0, (1 - c[1] / c[3]) * 12.0]))(np.append(p, 1.0) @ M)
    for p in ((0.3, 0.2, -2.0), (-1.0, 0.5, -4.0)):
        assert np.abs(screen(J, p) - screen(m.astype(F).astype(np.float64), p) - (0.4, -0.3)).max() < 1e-5
    # the python wrapper leaves its argument alone, and the renderer does not call the function at all with (0, 0) (tests/test_gpu_taa.py)
    same = m.astype(F).copy()
    pkg.renderer.jitter_proj_view(same, 40, 24, 0.4, -0.3)
    assert same.tobytes() == m.astype(F).tobytes()
    assert pkg.renderer.taa_jitter(5) == T.taa_jitter(5) and pkg.renderer.taa_jitter(9, period=4) == T.taa_jitter(9, 4)


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_every_deliberate_defect_changes_output_bytes(defect):
    rng = np.random.default_rng(7200)
    W, H = 17, 9
    frames, vels, jitters = random_frames(rng, W, H, 3)
    kw = dict(max_history=2.0, min_weight=0.1)
    for flags in (0, T.LUMA_WEIGHT):
        prev = T.sequence(frames[:2], vels[:2], jitters[:2], flags=flags, **kw)[-1]
        good = T.resolve(frames[2], vels[2], prev, jitter=jitters[2], flags=flags, **kw)
        broken = T.resolve(frames[2], vels[2], prev, jitter=jitters[2], flags=flags, defect=defect, **kw)
        assert good.tobytes() != broken.tobytes(), (defect, flags)


def aa_sequence(W, H, flags):
    jitters = [T.taa_jitter(i) for i in range(8)]
    frames = [T.analytic_frame(W, H, j) for j in jitters]
    vels = [np.broadcast_to(np.array([-j[0], -j[1]], F), (H, W, 2)) for j in jitters]          # a still scene under jitter j: velocity2 = -j
    differ = np.zeros((H, W), bool)
    for f in frames[1:]:
        differ |= (f != frames[0]).any(-1)
    return frames, differ, T.sequence(frames, vels, jitters, max_history=8.0, flags=flags)[-1]


def test_eight_jittered_frames_halve_the_error_of_one():
    """Measured with this reference at 40x24 (56 pixels differ between the frames): mean absolute error through Reinhard against the 16x16
    supersample, one frame 0.296; the resolve 0.0227 (ratio 0.077) without the luma weight, 0.105 (ratio 0.356) with it.  max |out - mean| of the
    fp32 resolve against the float64 mean of the 8 frames: 3.9e-7; the bound is 4 x that, for the summation order."""
    W, H = 40, 24
    ref = T.reinhard(T.analytic_supersample(W, H))
    for flags in (0, T.LUMA_WEIGHT):
        frames, differ, out = aa_sequence(W, H, flags)
        assert differ.sum() >= 40 and (out[..., 3] == 8.0).all()
        single = np.abs(T.reinhard(frames[-1]) - ref)[differ].mean()
        resolved = np.abs(T.reinhard(out[..., :3]) - ref)[differ].mean()
        print(f"flags {flags}: one frame {single:.4f}, resolved {resolved:.4f}, ratio {resolved / single:.3f}")
        assert resolved <= 0.5 * single, (flags, resolved, single)
        if flags == 0:
            mean = np.stack(frames).astype(np.float64).mean(0)
            worst = np.abs(out[..., :3] - mean).max()
            print(f"max |out - mean| = {worst:.3e}")
            assert worst <= 4 * 3.9e-7, worst


def test_a_translating_pattern_is_tracked_through_velocity2():
    W, H, calls = 40, 24, 4
    rng = np.random.default_rng(7300)
    plane = rng.uniform(0, 4, (H + 2 * calls, W + 3 * calls, 3)).astype(F)
    # frame k shows the plane moved by (3, -2) pixels per frame: pixel (x, y) of frame k is plane[y + 2k, x - 3k + 3 * calls]
    frames = [plane[2 * k:2 * k + H, 3 * (calls - k):3 * (calls - k) + W] for k in range(calls)]
    assert (frames[1][:-2, 3:] == frames[0][2:, :-3]).all()
    vel = np.broadcast_to(np.array([-3.0, 2.0], F), (H, W, 2))                          # from this pixel to where its point WAS
    tracked = T.sequence(frames, [vel] * calls, max_history=8.0)
    still = T.sequence(frames, None, max_history=8.0)
    for k in range(calls):
        inside = np.zeros((H, W), bool)
        inside[:H - 2 * k, 3 * k:] = True                                               # the point has been on the screen in every frame so far
        assert (tracked[k][inside][:, 3] == k + 1).all() and (tracked[k][~inside][:, 3] <= k).all()
        assert tracked[k][inside][:, :3].tobytes() == frames[k][inside].tobytes()        # the mean of k + 1 equal samples
    assert (still[-1][..., 3] == calls).all()
    assert (still[-1][..., :3] != frames[-1]).any(-1).mean() > 0.9                        # without the velocity the history is another point's
