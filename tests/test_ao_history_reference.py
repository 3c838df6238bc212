"""The temporal accumulation on a machine without a GPU: the numpy arbiter (tests/ao_history_reference.py) pinned on pixels worked by hand, the host
arbiter arctic_accumulate_pixels against it by bytes over sequences of calls on the device tests' inputs (tests/ao_history_scenes.py), deliberate
defects that must show on those inputs, the arbiter's refusals, and what the accumulation means: K independent 0 / 255 planes average to their
mean, a constant plane stays that constant."""
import numpy as np
import pytest

import ao_history_reference as HR
import ao_history_scenes as HS

F = np.float32
INVALID = -1
W, H = 8, 4
HAND = dict(max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.0)   # the parameters of the pixels worked by hand
IDENTITY = np.eye(4, dtype=F)                                                    # c = (w0, w1, w2, 1): sx = (w0 + 1) * W / 2, sy = (1 - w1) * H / 2


def at(gx, gy, z=0.0):
    """the world position that the identity matrix reprojects to tap position (gx, gy) of the W x H frame: exact in float32 for dyadic gx, gy"""
    return (F((gx + 0.5) * 2 / W - 1), F(1 - (gy + 0.5) * 2 / H), F(z))


def flat_history(value=100.0, count=3.0):
    """a previous call that saw the plane z = 0 facing +z in every pixel"""
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    world = np.stack([(xs + 0.5) * 2 / W - 1, 1 - (ys + 0.5) * 2 / H, np.zeros((H, W))], -1).astype(F)
    normal = np.zeros((H, W, 3), F)
    normal[..., 2] = 1
    return dict(P=IDENTITY, value=np.full((H, W), value, F), count=np.full((H, W), count, F), world=world, normal=normal)


def one(world, prev, cur=255, normal=(0, 0, 2), geometry=True, hist=HAND, defect=None):
    r = HR.accumulate(np.array([world], F), np.array([normal], F), [geometry], [cur], prev, W, H, hist, defect)
    return int(r["byte"][0]), float(r["value"][0]), float(r["count"][0]), int(r["cls"][0])


def test_still_camera_on_a_floor_by_hand():
    # the pixel falls on itself: weights (1, 0, 0, 0), hv = 100, hn = 3, N = 4, value = 100 + (255 - 100) / 4 = 138.75 -> 139
    assert one(at(3, 1), flat_history()) == (139, 138.75, 4.0, HR.ALL_ACCEPTED)
    # an empty history: N = 1 and the byte is the input
    assert one(at(3, 1), None, cur=77) == (77, 77.0, 1.0, HR.EMPTY)
    # no geometry, and a degenerate normal: 255 and the all-zero entry
    assert one(at(3, 1), flat_history(), cur=10, geometry=False) == (255, 0.0, 0.0, HR.NO_GEOMETRY)
    assert one(at(3, 1), flat_history(), cur=10, normal=(0, 0, 0)) == (255, 0.0, 0.0, HR.NOT_COVERED)
    # half a pixel to the right and down: four taps of a quarter each; values 0, 40, 80, 120 at counts 1, 3, 5, 7 -> hv = 60, hn = 4, N = 5, value = 60 + (255 - 60) / 5 = 99
    h = flat_history()
    h["value"][1:3, 3:5] = [[0, 40], [80, 120]]
    h["count"][1:3, 3:5] = [[1, 3], [5, 7]]
    assert one(at(3.5, 1.5), h) == (99, 99.0, 5.0, HR.ALL_ACCEPTED)
    # max_history = 1: N = 1, a = 1, the value is the input again
    assert one(at(3.5, 1.5), h, cur=201, hist=dict(HAND, max_history=1.0)) == (201, 201.0, 1.0, HR.ALL_ACCEPTED)
    # the cap: counts of 3 under max_history = 2 -> N = 2, value = 100 + 155 / 2
    assert one(at(3, 1), flat_history(), hist=dict(HAND, max_history=2.0)) == (178, 177.5, 2.0, HR.ALL_ACCEPTED)


def test_a_tap_pair_straddling_a_depth_edge_by_hand():
    # taps (2, 1) and (3, 1) at a half each; (3, 1) belongs to a surface one unit behind: rejected by the plane test, the history is tap (2, 1) alone
    h = flat_history()
    h["value"][1, 2], h["value"][1, 3] = 40, 200
    h["world"][1, 3, 2] = -1.0
    assert one(at(2.5, 1), h) == (94, 93.75, 4.0, HR.SOME_REJECTED)              # hv = (0.5 * 40) / 0.5 = 40; 40 + 215 / 4
    assert one(at(2.5, 1), h, defect="no renormalisation")[1] != 93.75
    assert one(at(2.5, 1), h, defect="no plane test")[1] != 93.75
    # ... and a tap whose normal has turned away is rejected by the normal test
    h = flat_history()
    h["value"][1, 2], h["value"][1, 3] = 40, 200
    h["normal"][1, 3] = (1, 0, 0)
    assert one(at(2.5, 1), h) == (94, 93.75, 4.0, HR.SOME_REJECTED)
    # min_weight: S = 0.5 is not > 0.5, the history is dropped
    assert one(at(2.5, 1), h, cur=9, hist=dict(HAND, min_weight=0.5)) == (9, 9.0, 1.0, HR.SOME_REJECTED)
    # nobody accepted: S = 0, not > 0
    h["count"][:] = 0
    assert one(at(2.5, 1), h, cur=9) == (9, 9.0, 1.0, HR.NONE_ACCEPTED)


def test_behind_the_previous_camera_and_outside_its_frame_by_hand():
    persp = IDENTITY.copy()
    persp[3, 3], persp[2, 3] = 0, -1                                             # [col][row]: c3 = -w2, the camera looks down -z
    h = dict(flat_history(), P=persp)
    assert one((0.0, 0.0, 1.0), h, cur=5) == (5, 5.0, 1.0, HR.BEHIND)            # c3 = -1
    assert one((0.0, 0.0, 0.0), h, cur=5) == (5, 5.0, 1.0, HR.BEHIND)            # c3 = 0: not > 0
    assert one((np.nan, 0.0, -1.0), h, cur=5) == (5, 5.0, 1.0, HR.BEHIND)        # c0 is not finite
    h = flat_history()
    for gx, gy in ((-2, 1), (W, 1), (3, -2), (3, H), (-1.25, 1), (3, -1.25)):    # one pixel outside each border, and just past ix = -1
        assert one(at(gx, gy), h, cur=5) == (5, 5.0, 1.0, HR.OUTSIDE), (gx, gy)
    # ix = -1: taps (-1, 1) outside, (0, 1) at a half -> its value alone; the same at ix = W - 1, iy = -1 and iy = H - 1
    for gx, gy in ((-0.5, 1), (W - 0.5, 1), (3, -0.5), (3, H - 0.5)):
        assert one(at(gx, gy), h) == (139, 138.75, 4.0, HR.SOME_REJECTED), (gx, gy)
    assert one(at(-1, 1), h, cur=5) == (5, 5.0, 1.0, HR.SOME_REJECTED)           # ix = -1 exactly, ax = 0: the only weight lies outside, S = 0
    assert one(at(W - 1, H - 1), h) == (139, 138.75, 4.0, HR.SOME_REJECTED)      # the last pixel on itself: three taps outside


def test_a_nan_in_a_rejected_taps_history_stays_out_by_hand():
    h = flat_history()
    h["value"][1, 2] = 40
    h["value"][1, 3], h["count"][1, 3], h["world"][1, 3, 2] = np.nan, np.nan, -1.0   # rejected by its count AND by the plane test
    assert one(at(2.5, 1), h) == (94, 93.75, 4.0, HR.SOME_REJECTED)
    h["count"][1, 3] = 2.0                                                        # rejected by the plane test alone
    assert one(at(2.5, 1), h) == (94, 93.75, 4.0, HR.SOME_REJECTED)
    assert np.isnan(one(at(2.5, 1), h, defect="rejected tap multiplied")[1])     # what a product by zero would give
    h["world"][1, 3] = np.nan                                                     # a NaN position is rejected by the plane test
    assert one(at(2.5, 1), h) == (94, 93.75, 4.0, HR.SOME_REJECTED)


def arbiter_sequence(pkg, frames, planes, hist):
    """the host arbiter driven like the library drives the kernel -> [(byte, (value, count, world, normal))]"""
    out, prev, P_prev = [], None, None
    for (attrs, material, P), cur in zip(frames, planes):
        Hh, Ww = material.shape
        a = attrs.reshape(-1, 18)
        byte, value, count, world, normal = pkg.renderer.accumulate_pixels(a[:, 11:14], a[:, 8:11], material.reshape(-1) != HR.NO_MATERIAL, cur, P_prev, Ww, Hh, prev, **hist)
        prev, P_prev = (value, count, world, normal), P
        out.append((byte.reshape(Hh, Ww), prev))
    return out


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b, dtype=np.asarray(a).dtype).tobytes()


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("move", HS.MOVES)
def test_host_arbiter_equals_numpy_by_bytes(pkg, move, size):
    c = HS.case(pkg, move, *size)
    want = HR.run_sequence(c["frames"], c["planes"])
    for n in HS.CALLS:
        got = arbiter_sequence(pkg, c["frames"][:n], c["planes"][:n], HR.HIST)
        for k in range(n):
            byte, state, _ = want[k]
            assert same_bytes(byte, got[k][0]), (move, size, n, k, int((byte != got[k][0]).sum()))
            for name, plane in zip(("value", "count", "world", "normal"), got[k][1]):
                assert same_bytes(state[name], plane.reshape(state[name].shape)), (move, size, n, k, name)
    assert not same_bytes(want[-1][0], c["planes"][4])                            # the accumulation did something


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_class_is_there_under_the_moving_cameras(pkg, size):
    counts = HS.check_classes(pkg, *size)
    print({n: int(c) for n, c in zip(HR.CLASS_NAMES, counts)})


@pytest.mark.parametrize("defect", [d for d in HR.DEFECTS if d != "rejected tap multiplied"])
def test_a_defect_shows_on_the_device_tests_inputs(pkg, defect):
    """nearest tap instead of four, no division by S, this call's matrix instead of the previous one's, N not capped, y not flipped, acceptance on
    this frame's normals and positions, no plane test: each changes output bytes on the frames the device is judged on"""
    changed = 0
    for move in HS.MOVES:
        c = HS.case(pkg, move, *HS.SIZES[0])
        for (b0, _, _), (b1, _, _) in zip(HR.run_sequence(c["frames"], c["planes"]), HR.run_sequence(c["frames"], c["planes"], defect=defect)):
            changed += int((b0 != b1).sum())
    assert changed >= 20, (defect, changed)


def test_every_refusal_of_the_arbiter(pkg):
    hr = pkg.renderer
    px = dict(world=[(0, 0, 0)], normal=[(0, 0, 1)], geometry=[1], cur=[7])
    assert hr.accumulate_pixels(**px)[0][0] == 7
    for bad in (dict(max_history=0.5), dict(max_history=65537.0), dict(max_history=np.nan), dict(max_history=np.inf), dict(normal_cos=np.inf), dict(normal_cos=np.nan),
                dict(plane_dist=-1e-6), dict(plane_dist=np.nan), dict(min_weight=-0.1), dict(min_weight=1.0), dict(min_weight=np.nan), dict(width=0), dict(height=0),
                dict(width=16385), dict(height=16385)):
        with pytest.raises(hr.ArcticError) as e:
            hr.accumulate_pixels(**px, **bad)
        assert e.value.code == INVALID, bad
    for k in range(4):
        h = np.zeros(1, pkg.scene.AO_HISTORY_DTYPE)
        h["max_history"], h["normal_cos"], h["plane_dist"], h["reserved"][0, k] = 4, 0.9, 0.05, 1
        with pytest.raises(hr.ArcticError) as e:
            hr.accumulate_pixels(**px, hist=h)
        assert e.value.code == INVALID
    # the edges of the ranges are inside
    for good in (dict(max_history=1.0), dict(max_history=65536.0), dict(plane_dist=0.0), dict(plane_dist=np.inf), dict(min_weight=0.0), dict(min_weight=0.999), dict(normal_cos=-5.0)):
        assert hr.accumulate_pixels(**px, **good)[0][0] == 7
    # null arrays, a null block, a matrix without a history: straight at the C-ABI
    import ctypes as C
    from importlib import import_module
    L = import_module("arctic_renderer_amd.binding").lib()
    h = hr._ao_history_arguments(4.0, 0.9, 0.05, 0.0)
    w, n, g, cur, out = np.zeros(3, F), np.array([0, 0, 1], F), np.ones(1, np.uint8), np.full(1, 7, np.uint8), np.full(1, 99, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [p(h), 1, p(w), p(n), p(g), p(cur), None, 4, 4, None, None, None, None, p(out), None, None, None, None]
    assert L.arctic_accumulate_pixels(*args) == 0 and out[0] == 7
    out[0] = 99
    for k in (0, 2, 3, 4, 5, 13):
        assert L.arctic_accumulate_pixels(*[None if i == k else a for i, a in enumerate(args)]) == INVALID and out[0] == 99, k
    m = np.eye(4, dtype=F)
    hist4 = [np.zeros(16, F), np.ones(16, F), np.zeros(48, F), np.zeros(48, F)]
    for k in range(4):
        a = list(args)
        a[6] = p(m)
        a[9:13] = [None if i == k else p(x) for i, x in enumerate(hist4)]
        assert L.arctic_accumulate_pixels(*a) == INVALID and out[0] == 99, k
    assert L.arctic_accumulate_pixels(p(h), 0, *([None] * 4), None, 4, 4, *([None] * 9)) == 0   # no pixel: nothing is needed


def test_independent_planes_average_to_their_mean_and_a_constant_stays():
    """a fixed frame under a still camera (every pixel falls on itself), K = 32 calls of independent 0 / 255 planes with mean v = 0.6 and
    max_history >= K: the accumulated value is the running mean of K Bernoulli samples, so value / 255 lies within 4 binomial standard deviations
    sqrt(v (1 - v) / K) of v -- in every one of the 32 pixels (the chance that an exact binomial leaves that band is below 1e-4 per pixel)."""
    K, v = 32, 0.6
    h0 = flat_history()
    attrs = np.zeros((H, W, 18), F)
    attrs[..., 11:14], attrs[..., 8:11] = h0["world"], (0, 0, 3)
    material = np.zeros((H, W), np.uint32)
    rng = np.random.default_rng(2024)
    planes = [np.where(rng.uniform(size=(H, W)) < v, 255, 0).astype(np.uint8) for _ in range(K)]
    hist = dict(HR.HIST, max_history=64.0, min_weight=0.0)
    seq = HR.run_sequence([(attrs, material, IDENTITY)] * K, planes, hist)
    value, count = seq[-1][1]["value"], seq[-1][1]["count"]
    assert (count == K).all()
    mean = np.mean([p.astype(np.float64) for p in planes], 0)
    assert np.abs(value - mean).max() <= 1e-3                                     # it IS the running mean
    sigma = np.sqrt(v * (1 - v) / K)
    print(f"largest deviation {np.abs(value / 255 - v).max():.4f}, 4 sigma {4 * sigma:.4f}")
    assert np.abs(value / 255.0 - v).max() <= 4 * sigma
    assert np.abs(seq[-1][0].astype(np.float64) - value).max() <= 0.5
    # under a cap of 8 the same sequence weighs the latest planes more: it is no longer the mean
    capped = HR.run_sequence([(attrs, material, IDENTITY)] * K, planes, dict(hist, max_history=8.0))[-1][1]
    assert (capped["count"] == 8).all() and np.abs(capped["value"] - mean).max() > 1.0
    # a constant plane stays that constant by bytes, also under a moving camera's fractional weights
    for c in (0, 1, 127, 254, 255):
        const = [np.full((H, W), c, np.uint8)] * 6
        for byte, _, _ in HR.run_sequence([(attrs, material, IDENTITY)] * 6, const, HR.HIST):
            assert (byte == c).all(), c


def test_a_constant_plane_stays_constant_under_the_moving_cameras(pkg):
    for move in HS.MOVES[1:]:
        c = HS.case(pkg, move, *HS.SIZES[1])
        for value in (1, 200):
            planes = [np.full(p.shape, value, np.uint8) for p in c["planes"]]
            for byte, state, cls in HR.run_sequence(c["frames"], planes):
                covered = cls > HR.NOT_COVERED
                assert (byte[covered] == value).all() and (byte[~covered] == 255).all(), (move, value)
