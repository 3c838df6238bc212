"""The temporal upscaler on a machine without a GPU: the numpy restatement (tests/taa_upscale_reference.py) pinned on pixels worked by hand, the
host arbiter arctic_taa_upscale_pixels and arctic_taa_upscale_jitter against it BY BYTES at every size pair, the four properties the header
promises (P1: it is the resolve at ratio 1; P2: the first frame; P3: the exact phases rebuild the point-sampled frame by bits; P4: hostile
velocities and NaN colours stay where they are), every deliberate defect shown to change output bytes, and what the feature is for: jittered
half-size frames of an analytic scene come closer to the supersampled full-size frame than a stretched frame does."""
import json
import os

import numpy as np
import pytest

import taa_reference as T
import taa_upscale_reference as U

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITY = os.path.join(ROOT, "profiles", "taa_upscale_quality.json")
# the quality claim's configuration (tools/taa_upscale_quality.py measures it with the same function and writes QUALITY)
QUALITY_CASE = dict(in_size=(48, 32), out_size=(96, 64), frames=16, sharpness=1.0, confidence_floor=1.0 / 64, flags=0)


@pytest.fixture(scope="module")
def lib(pkg):
    """the library, built when a clean tree has none yet"""
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def grey(values):
    """a frame of grey pixels from a 2-D list"""
    return np.repeat(np.asarray(values, F)[..., None], 3, -1)


def test_pixels_worked_by_hand():
    # 2x2 -> 4x4 (rx = 0.5) under j = (0.25, 0.25), the phase that puts output pixels (even, even) on samples
    cur = grey([[1.0, 2.0], [3.0, 4.0]])
    kw = dict(jitter=(0.25, 0.25), sharpness=1.0, confidence_floor=0.125, flags=U.NO_CLAMP)
    first = U.upscale(cur, (4, 4), **kw)
    # px = 0: ux = 0.25, floor(0.5) = 0, D = ((0.5 - 0.25) - 0.25) / 0.5 = 0: beta = 1.  px = 1: ux = 0.75, floor(1.0) = 1, D = ((1.5 - 0.25) - 0.75) / 0.5 = 1
    assert first[0, 0].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert first[0, 1].tolist() == [2.0, 2.0, 2.0, 0.125]                 # beta = max(0, 1 - 1 * (1 + 0)) = 0: N = confidence_floor
    assert first[0, 2].tolist() == [2.0, 2.0, 2.0, 1.0]                   # px = 2: ux = 1.25, floor(1.5) = 1, D = 0
    assert first[0, 3].tolist() == [2.0, 2.0, 2.0, 0.125]                 # px = 3: floor(2.0) = 2 is clamped to 1, D = (1.25 - 1.75) / 0.5 = -1
    assert first[1, 1].tolist() == [4.0, 4.0, 4.0, 0.125] and first[3, 3].tolist() == [4.0, 4.0, 4.0, 0.125]
    # with sharpness 0.25 the sample one output pixel away still counts: beta = 1 - 0.25 = 0.75, and two away diagonally 1 - 0.25 * 2 = 0.5
    soft = U.upscale(cur, (4, 4), **dict(kw, sharpness=0.25))
    assert soft[0, 1, 3] == 0.75 and soft[1, 1, 3] == 0.5
    # the second frame of the same phase, a still scene (v = -j): hx = (px + 0.5) - 0.5 + 0.5, the taps' weights are (1, 0, 0, 0)
    vel = U.still_velocity((0.25, 0.25), (2, 2))
    second = U.upscale(grey([[10.0, 20.0], [30.0, 40.0]]), (4, 4), vel, first, **kw)
    assert second[0, 0].tolist() == [5.5, 5.5, 5.5, 2.0]                  # N = 1 + 1, a = 0.5: 1 + (10 - 1) * 0.5
    assert second[0, 1].tolist() == [2.0, 2.0, 2.0, 0.125]                # beta = 0: out = h, N = min(0.125 + 0, 32)
    # ... the cap: max_history = 1.5 gives N = 1.5, a = 1 / 1.5
    capped = U.upscale(grey([[10.0, 20.0], [30.0, 40.0]]), (4, 4), vel, first, max_history=1.5, **kw)
    a = F(1.0) / F(1.5)
    assert capped[0, 0].tolist() == [float(F(1.0) + F(9.0) * a)] * 3 + [1.5]
    # the phase (-0.25, 0.25) puts pixel (1, 0) on input pixel 0: ux = 0.75, floor(0.5) = 0, D = ((0.5 + 0.25) - 0.75) / 0.5 = 0
    kw2 = dict(kw, jitter=(-0.25, 0.25))
    vel2 = U.still_velocity((-0.25, 0.25), (2, 2))
    third = U.upscale(grey([[7.0, 8.0], [9.0, 6.0]]), (4, 4), vel2, first, **kw2)
    n = F(0.125) + F(1.0)
    assert third[0, 1].tolist() == [float(F(2.0) + F(5.0) * (F(1.0) / n))] * 3 + [1.125]      # h = 2 with N = 0.125: a = 1 / 1.125
    assert third[0, 0].tolist() == [1.0, 1.0, 1.0, 1.0]                   # px = 0 under this phase: floor(-0.0 ...) q = 0, D = 1: beta = 0, out = h
    # ... and when the history holds nothing but a vanishing floor, hn + beta == beta: out = c by bits, N = 1
    tiny = dict(kw2, confidence_floor=2.0 ** -25)
    first_tiny = U.upscale(cur, (4, 4), **dict(tiny, jitter=(0.25, 0.25)))
    assert first_tiny[0, 1].tolist() == [2.0, 2.0, 2.0, 2.0 ** -25]
    assert U.upscale(grey([[7.0, 8.0], [9.0, 6.0]]), (4, 4), vel2, first_tiny, **tiny)[0, 1].tolist() == [7.0, 7.0, 7.0, 1.0]
    # the clamp: without NO_CLAMP h = 2 at pixel (1, 0) is clamped into the box around q = (0, 0) of the new frame, [6, 9] -> 6; a = 1 / 1.125
    clamped = U.upscale(grey([[7.0, 8.0], [9.0, 6.0]]), (4, 4), vel2, first, **dict(kw2, flags=0))
    assert clamped[0, 1].tolist() == [float(F(6.0) + F(1.0) * (F(1.0) / n))] * 3 + [1.125]
    # a ratio that is no integer: 2 -> 3, rx = fl(2 / 3).  px = 1: ux = fl(1.5 * rx) = 1, floor(1) = 1, D = fl(0.5 / rx) = 0.75
    rx = F(2.0) / F(3.0)
    assert F(1.5) * rx == F(1.0) and F(0.5) / rx == F(0.75)
    odd = U.upscale(grey([[1.0, 2.0]]), (3, 1), sharpness=1.0, confidence_floor=0.01)
    assert odd[0, 1].tolist() == [2.0, 2.0, 2.0, float(F(1.0) - F(0.75) * F(0.75))]
    # ratio 1 is the resolve: the running mean of tests/test_taa_reference.py.  h = 1, N_q = 3: N = 4, a = 0.25
    cur3 = np.zeros((3, 3, 3), F)
    cur3[1, 1], cur3[2, 2] = 2.0, 4.0
    hist = np.empty((3, 3, 4), F)
    hist[..., :3], hist[..., 3] = 1.0, 3.0
    assert U.upscale(cur3, (3, 3), None, hist, sharpness=0.0, max_history=8.0)[1, 1].tolist() == [1.25, 1.25, 1.25, 4.0]
    # a NaN, infinite or huge velocity rejects: step 4's result
    for v in (np.nan, np.inf, -np.inf, 1e30, -3e38):
        bad = U.still_velocity((0.25, 0.25), (2, 2))
        bad[0, 0, 0] = v
        assert U.upscale(grey([[10.0, 20.0], [30.0, 40.0]]), (4, 4), bad, first, **kw)[0, 0].tolist() == [10.0, 10.0, 10.0, 1.0], v


def test_the_jitter_helper_equals_numpy_by_bytes(pkg, lib):
    R = pkg.renderer
    for (w, h), (W, H) in U.PAIRS + (((1920, 1080), (3840, 2160)), ((2560, 1440), (3840, 2160)), ((4096, 4096), (16384, 16384))):
        L = 8 * -(-W // w) * -(-H // h)
        for i in list(range(L + 2)) + [12345, 0x7FFFFFFF]:
            got = R.taa_upscale_jitter(i, (w, h), (W, H))
            assert got.dtype == F and got.tobytes() == U.jitter(i, (w, h), (W, H)).tobytes(), (w, h, W, H, i)
            assert (np.abs(got) <= 0.5).all()
        assert R.taa_upscale_jitter(L, (w, h), (W, H)).tobytes() == R.taa_upscale_jitter(0, (w, h), (W, H)).tobytes()     # it repeats
        assert len({R.taa_upscale_jitter(i, (w, h), (W, H)).tobytes() for i in range(L)}) == L
    assert U.jitter(0, (8, 8), (16, 16)).tolist() == [0.0, float(F(1.0) / F(3.0) - F(0.5))]
    # the exact phases: every (kx, ky) once, 0.5 - (k + 0.5) / s, all dyadic
    for s in (1, 2, 4):
        seen = set()
        for i in range(2 * s * s):
            got = R.taa_upscale_jitter(i, (17, 9), (17 * s, 9 * s), exact=True)
            assert got.tobytes() == U.jitter(i, (17, 9), (17 * s, 9 * s), exact=True).tobytes()
            assert got.tolist() == [0.5 - ((i % (s * s)) % s + 0.5) / s, 0.5 - ((i % (s * s)) // s + 0.5) / s]
            seen.add(got.tobytes())
        assert len(seen) == s * s
    for bad in (dict(in_size=(8, 8), out_size=(24, 24)), dict(in_size=(8, 8), out_size=(16, 32)), dict(in_size=(8, 8), out_size=(12, 12))):
        with pytest.raises(R.ArcticError):
            R.taa_upscale_jitter(0, exact=True, **bad)
    for bad in (dict(in_size=(8, 8), out_size=(7, 8)), dict(in_size=(8, 8), out_size=(33, 8)), dict(in_size=(0, 8), out_size=(0, 8)), dict(in_size=(8192, 8), out_size=(16385, 8))):
        with pytest.raises(R.ArcticError):
            R.taa_upscale_jitter(0, **bad)


def random_frames(rng, in_size, out_size, calls, nan_calls=None):
    """input frames with colours in [0, 4) and NaNs (in the calls of nan_calls; None: in every call), input-size velocities of a few pixels with
    entries that point outside the frame or are not finite, and the helper's jitters"""
    w, h = in_size
    frames, vels, jitters = [], [], []
    for k in range(calls):
        c = rng.uniform(0, 4, (h, w, 3)).astype(F)
        if nan_calls is None or k in nan_calls:
            c[rng.uniform(size=(h, w)) < 0.03, 1] = np.nan
        v = rng.uniform(-2, 2, (h, w, 2)).astype(F)
        v[rng.uniform(size=(h, w)) < 0.3] = 0.0
        v[rng.uniform(size=(h, w)) < 0.05, 0] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -3e38, 100.0, -100.0])
        frames.append(c)
        vels.append(v)
        jitters.append(U.jitter(k, in_size, out_size))
    return frames, vels, jitters


def all_pixels(out_size):
    ys, xs = np.mgrid[0:out_size[1], 0:out_size[0]]
    return np.stack([xs, ys], -1).reshape(-1, 2)


@pytest.mark.parametrize("in_size, out_size", U.PAIRS, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("flags", [0, U.LUMA_WEIGHT, U.NO_CLAMP, U.LUMA_WEIGHT | U.NO_CLAMP])
def test_the_arbiter_equals_numpy_by_bytes(pkg, lib, in_size, out_size, flags):
    rng = np.random.default_rng(9000 + in_size[0] + out_size[0])
    frames, vels, jitters = random_frames(rng, in_size, out_size, 5)
    xy = all_pixels(out_size)
    order = rng.permutation(len(xy))                                            # n pixels in any order
    prev = None
    for call in range(5):                                                        # sequences of 1, 2 and 5 calls are this one's prefixes
        kw = dict(jitter=jitters[call], max_history=3.0, min_weight=0.1, sharpness=(0.0, 0.7, 2.0)[call % 3], confidence_floor=0.05, flags=flags)
        want = U.upscale(frames[call], out_size, vels[call], prev, **kw)
        got = pkg.renderer.taa_upscale_pixels(xy[order], frames[call], out_size, vels[call], prev, **kw)
        assert got.tobytes() == want.reshape(-1, 4)[order].tobytes(), (call, np.nanmax(np.abs(got - want.reshape(-1, 4)[order])))
        prev = want
    assert out_size[0] * out_size[1] < 64 or (np.nanmax(prev[..., 3]) == 3.0 and (prev[..., 3] < 1.0).any())   # the cap is reached, and some pixels hold less than a frame
    # a NULL velocity is zero
    assert pkg.renderer.taa_upscale_pixels(xy, frames[0], out_size, None, prev, **kw).tobytes() == U.upscale(frames[0], out_size, None, prev, **kw).tobytes()


@pytest.mark.parametrize("width, height", ((1, 1), (8, 8), (17, 9), (40, 24)))
@pytest.mark.parametrize("flags", [0, T.LUMA_WEIGHT])
def test_p1_at_ratio_one_it_is_the_resolve(pkg, lib, width, height, flags):
    """W = w, H = h, sharpness = 0, |j| < 0.5, the clamp on: {out, N} is arctic_taa_pixels' and tests/taa_reference.py's by bytes, whatever
    confidence_floor says, through five calls with hostile velocities and NaN colours and with max_history = 1 among the settings.  The
    history is the resolve's own: every stored N is 1 or more, which the header's select on hn + beta == beta relies on."""
    import test_taa_reference as TR
    rng = np.random.default_rng(9100 + width)
    frames, vels, jitters = TR.random_frames(rng, width, height, 5)
    jitters[3] = (0.499, -0.499)
    xy = all_pixels((width, height))
    for max_history in (3.0, 1.0):
        prev = None
        for call in range(5):
            kw = dict(jitter=jitters[call], max_history=max_history, min_weight=0.1, flags=flags)
            want = T.resolve(frames[call], vels[call], prev, **kw)
            resolve = pkg.renderer.taa_pixels(xy, frames[call], vels[call].reshape(-1, 2), prev, **kw)
            got = pkg.renderer.taa_upscale_pixels(xy, frames[call], (width, height), vels[call], prev, sharpness=0.0, confidence_floor=(1.0, 0.3, 2.0 ** -30)[call % 3], **kw)
            numpy = U.upscale(frames[call], (width, height), vels[call], prev, sharpness=0.0, confidence_floor=0.3, **kw)
            assert got.tobytes() == resolve.tobytes() == want.tobytes() == numpy.tobytes(), (max_history, call)
            prev = want


@pytest.mark.parametrize("in_size, out_size", U.PAIRS + (((37, 23), (55, 34)), ((37, 23), (74, 46))), ids=lambda v: "x".join(map(str, v)))
def test_p2_the_first_frame_is_the_nearest_sample(pkg, lib, in_size, out_size):
    """U empty: every output pixel is C[q] of a sample whose unjittered position lies nearest to its centre (float64 here), every output value
    is written, and N = max(beta, confidence_floor)"""
    (w, h), (W, H) = in_size, out_size
    rng = np.random.default_rng(9200 + W)
    cur = rng.uniform(0, 4, (h, w, 3)).astype(F)
    for k in range(4):
        j = U.jitter(k, in_size, out_size)
        got = np.full((W * H, 4), -77.0, F)
        got[:] = pkg.renderer.taa_upscale_pixels(all_pixels(out_size), cur, out_size, jitter=j, sharpness=1.0, confidence_floor=0.25)
        got = got.reshape(H, W, 4)
        assert got.tobytes() == U.upscale(cur, out_size, jitter=j, sharpness=1.0, confidence_floor=0.25).tobytes()
        ux, uy = (np.arange(W) + 0.5) * (w / W), (np.arange(H) + 0.5) * (h / H)
        dx = np.abs((np.arange(w)[None, :] + 0.5 - float(j[0])) - ux[:, None])   # (W, w): distance of sample q from pixel p, input pixels
        dy = np.abs((np.arange(h)[None, :] + 0.5 - float(j[1])) - uy[:, None])
        qx, qy = U.nearest(W, w, j[0])[0], U.nearest(H, h, j[1])[0]                  # the definition's q: no other sample lies nearer
        assert (dx[np.arange(W), qx] <= dx.min(1) + 1e-5).all() and (dy[np.arange(H), qy] <= dy.min(1) + 1e-5).all()   # (a centre between two samples may take either)
        assert (got[..., :3] == cur[qy][:, qx]).all()
        assert (got[..., 3] >= 0.25).all() and (got[..., 3] <= 1.0).all() and np.isfinite(got).all()


@pytest.mark.parametrize("s", (2, 4))
def test_p3_the_exact_phases_rebuild_the_point_sampled_frame_by_bits(pkg, lib, s):
    """a still analytic scene, the s * s exact phases, NO_CLAMP, sharpness 1, confidence_floor 2^-25: after s * s frames `out` is the scene
    point-sampled at W x H by bits, and it stays so; N = min(k, max_history) after k rounds"""
    in_size, out_size = (17, 9), (17 * s, 9 * s)
    want = U.analytic_frame(out_size)
    kw = dict(max_history=2.0, sharpness=1.0, confidence_floor=2.0 ** -25, flags=U.NO_CLAMP)
    xy = all_pixels(out_size)
    prev = None
    for k in range(3 * s * s):
        j = pkg.renderer.taa_upscale_jitter(k, in_size, out_size, exact=True)
        frame = U.analytic_frame(in_size, j)
        prev = U.upscale(frame, out_size, U.still_velocity(j, in_size), prev, jitter=j, **kw)
        if k % (s * s) == s * s - 1 or k == 0:
            got = pkg.renderer.taa_upscale_pixels(xy, frame, out_size, U.still_velocity(j, in_size), before if k else None, jitter=j, **kw)
            assert got.tobytes() == prev.tobytes()
        before = prev
        if k % (s * s) == s * s - 1:
            rounds = (k + 1) // (s * s)
            assert prev[..., :3].tobytes() == want.tobytes(), (s, k)
            assert (prev[..., 3] == min(rounds, 2.0)).all(), (s, k)
    # and before the last phase of the first round some pixels still hold a neighbour's sample
    partial = None
    for k in range(s * s - 1):
        j = U.jitter(k, in_size, out_size, exact=True)
        partial = U.upscale(U.analytic_frame(in_size, j), out_size, U.still_velocity(j, in_size), partial, jitter=j, **kw)
    assert (partial[..., 3] == F(2.0 ** -25)).sum() == 17 * 9 and partial[..., :3].tobytes() != want.tobytes()


def test_p4_hostile_velocities_and_nan_colours_stay_where_they_are(pkg, lib):
    in_size, out_size = (17, 9), (29, 14)
    (w, h), (W, H) = in_size, out_size
    rng = np.random.default_rng(9400)
    base = rng.uniform(0, 4, (h, w, 3)).astype(F)
    prev = U.upscale(base, out_size, jitter=(0.1, -0.2), sharpness=1.0, confidence_floor=0.05)
    cur = rng.uniform(0, 4, (h, w, 3)).astype(F)
    j = (-0.3, 0.2)
    kw = dict(jitter=j, sharpness=1.0, confidence_floor=0.05, max_history=8.0)
    qx, _, _ = U.nearest(W, w, F(j[0]))
    qy, _, _ = U.nearest(H, h, F(j[1]))
    mine = lambda x, y: (qy[:, None] == y) & (qx[None, :] == x)                    # the output pixels whose nearest sample is input pixel (x, y)
    clean = U.upscale(cur, out_size, None, prev, **kw)
    first = U.upscale(cur, out_size, **kw)
    xy = all_pixels(out_size)
    for v in (np.nan, np.inf, -np.inf, 1e30, -3e38, 1000.0):
        for axis in (0, 1):
            vel = np.zeros((h, w, 2), F)
            vel[4, 7, axis] = v
            got = pkg.renderer.taa_upscale_pixels(xy, cur, out_size, vel, prev, **kw).reshape(H, W, 4)
            hit = mine(7, 4)
            assert hit.sum() >= 1 and got[~hit].tobytes() == clean[~hit].tobytes() and got[hit].tobytes() == first[hit].tobytes(), (v, axis)
    # a NaN colour: through c it enters the pixels whose q it is and that this frame samples (beta > 0), and no other; the box ignores it
    nan = cur.copy()
    nan[4, 7] = np.nan
    got = pkg.renderer.taa_upscale_pixels(xy, nan, out_size, None, prev, **kw).reshape(H, W, 4)
    assert got.tobytes() == U.upscale(nan, out_size, None, prev, **kw).tobytes()
    hit = mine(7, 4)
    assert np.isnan(got[..., :3]).any(-1)[hit].all() and not np.isnan(got[~hit]).any()
    # ... and under beta == 0 the select keeps it out: sharpness 65536 leaves beta 0 wherever D != 0
    sharp = dict(kw, sharpness=65536.0, flags=U.NO_CLAMP)
    got = pkg.renderer.taa_upscale_pixels(xy, nan, out_size, None, prev, **sharp).reshape(H, W, 4)
    assert got.tobytes() == U.upscale(nan, out_size, None, prev, **sharp).tobytes() and not np.isnan(got).any()


DEFECT_SETUP = {"clamp under NO_CLAMP": dict(flags=U.NO_CLAMP)}


@pytest.mark.parametrize("defect", U.DEFECTS)
def test_every_deliberate_defect_changes_output_bytes(defect):
    rng = np.random.default_rng(9500)
    in_size, out_size = (17, 9), (29, 14)
    frames, vels, jitters = random_frames(rng, in_size, out_size, 3)
    if defect == "floor select removed":
        # the select fires where a history of nothing but a vanishing floor meets a sample on the pixel's centre: P3's second phase
        in_size, out_size = (17, 9), (34, 18)
        jitters = [U.jitter(k, in_size, out_size, exact=True) for k in range(2)]
        frames, vels = [rng.uniform(0, 4, (9, 17, 3)).astype(F) for _ in jitters], [U.still_velocity(j, in_size) for j in jitters]
        kw = dict(sharpness=1.0, confidence_floor=2.0 ** -25, flags=U.NO_CLAMP)
        prev = U.upscale(frames[0], out_size, vels[0], None, jitter=jitters[0], **kw)
        good, broken = (U.upscale(frames[1], out_size, vels[1], prev, jitter=jitters[1], defect=d, **kw) for d in (None, defect))
        assert good.tobytes() != broken.tobytes() and (good[:, 1::2, :3][::2] == frames[1]).all()
        return
    for flags in (0, U.LUMA_WEIGHT):
        kw = dict(max_history=4.0, min_weight=0.1, sharpness=2.0, confidence_floor=0.05, flags=flags)
        extra = DEFECT_SETUP.get(defect, {})
        kw.update(extra, flags=flags | extra.get("flags", 0))
        prev = U.sequence(frames[:2], out_size, vels[:2], jitters[:2], **kw)[-1]
        good = U.upscale(frames[2], out_size, vels[2], prev, jitter=jitters[2], **kw)
        broken = U.upscale(frames[2], out_size, vels[2], prev, jitter=jitters[2], defect=defect, **kw)
        assert good.tobytes() != broken.tobytes(), (defect, flags)


def measure_quality(in_size, out_size, frames, sharpness, confidence_floor, flags):
    """mean absolute error through Reinhard against the 8 x 8 supersample at the output size, of: one unjittered frame stretched bilinearly; the
    same `frames` jittered frames through the low-resolution resolve, then stretched; and the upscaler.  Deterministic: numpy alone"""
    ref = U.reinhard(U.analytic_supersample(out_size))
    js = [U.jitter(i, in_size, out_size) for i in range(frames)]
    low = [U.analytic_frame(in_size, j) for j in js]
    vels = [U.still_velocity(j, in_size) for j in js]
    err = lambda img: float(np.abs(U.reinhard(img) - ref).mean())
    single = err(U.stretch_bilinear(U.analytic_frame(in_size), out_size))
    resolved = err(U.stretch_bilinear(T.sequence(low, vels, js, max_history=float(frames))[-1][..., :3], out_size))
    up = U.sequence(low, out_size, vels, js, max_history=float(frames), sharpness=sharpness, confidence_floor=confidence_floor, flags=flags)[-1]
    upscaled = err(up[..., :3])
    return dict(mae_single_stretched=single, mae_lowres_resolve_stretched=resolved, mae_upscaled=upscaled, ratio_vs_single=upscaled / single,
                ratio_vs_lowres_resolve=upscaled / resolved)


def test_jittered_half_size_frames_beat_a_stretched_frame():
    """The quality claim at ratio 2, 48x32 -> 96x64, 16 frames of the helper's Halton sequence, sharpness 1, the clamp on.  Measured with this
    reference and recorded in profiles/taa_upscale_quality.json: one frame stretched 0.0415, the low-resolution resolve stretched 0.0408, the
    upscaler 0.0126: ratios 0.303 and 0.308.  The bound is halfway between each recorded ratio and 1; the reference is deterministic, so the
    margin only guards against a later change of the definition."""
    recorded = json.load(open(QUALITY))["cpu"]
    for key, value in QUALITY_CASE.items():
        assert recorded[key] == (list(value) if isinstance(value, tuple) else value), key
    got = measure_quality(**QUALITY_CASE)
    print({k: round(v, 5) for k, v in got.items()})
    assert recorded["ratio_vs_single"] < 1.0 and recorded["ratio_vs_lowres_resolve"] < 1.0
    assert got["mae_upscaled"] < got["mae_single_stretched"] and got["mae_upscaled"] < got["mae_lowres_resolve_stretched"]
    assert got["ratio_vs_single"] <= 0.5 * (recorded["ratio_vs_single"] + 1.0), got
    assert got["ratio_vs_lowres_resolve"] <= 0.5 * (recorded["ratio_vs_lowres_resolve"] + 1.0), got
