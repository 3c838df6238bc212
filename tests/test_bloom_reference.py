"""Bloom on a machine without a GPU.  tests/bloom_reference.py -- numpy, written from include/arctic_hip.h -- is pinned on pixels worked by hand
(scalar arithmetic, one np.float32 operation per step, with the footprints written out); the host arbiters arctic_bloom_pyramid and
arctic_bloom_pixels -- csrc/bloom.h, the functions the kernels run -- equal it BY BYTES with no pixel left out; eleven deliberate defects in a
copy of the reference each change output bytes; and the definition's behaviour is checked on numpy alone at 64 x 40.

Measured here (printed by the tests): the constant frame (b) differs from the float64 closed form by 2.6e-8, 6.0e-8 and 7.3e-9 relative at
1, 5 and 8 levels; Karis (d) leaves the peak of an isolated firefly in a black field where it is (ratio 1.0000000) and lowers it to 0.9999956
in a grey field that enters the pyramid -- see that test; fp32 against the float64 definition (e) differs by 3.1e-7 relative in `out` and by
2.6e-7 of a plane's largest value in the pyramids."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import bloom_reference as B

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((1, 1), (3, 5), (8, 8), (17, 9), (40, 24), (72, 40), (136, 72))          # (width, height); 17 x 9 at 8 levels ends in four 1 x 1 levels;
                                                                                # 136 x 72: 5 x 3 workgroups of 16 x 16 at level 1, 3 x 2 at level 2
LEVELS = (1, 2, 5, 8)
RECORDS = (dict(B.DEFAULTS), dict(threshold=0.7, soft_knee=0.25, clamp_max=50.0, intensity=1.5, spread=0.75))
TOL = 1e-4                                                                      # the project's standing bar


@pytest.fixture(scope="module")
def lib(pkg):
    """the library, built when a clean tree has none yet"""
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def same(got, want, what):
    """the same bytes, no element left out -- where a value is a NaN, a NaN (its payload is no part of the definition)"""
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape, got.dtype, want.dtype)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaNs elsewhere", int((np.isnan(got) != nan).sum()))
    a, b = np.where(nan, F(0.0), got), np.where(nan, F(0.0), want)
    assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()), "elements differ")


def same_bloom(got, want, what):
    """(out, D, U) against (out, D, U)"""
    assert len(got[1]) == len(want[1]) and len(got[2]) == len(want[2]), what
    same(got[0], want[0], (what, "out"))
    for name, g, w in (("D", got[1], want[1]), ("U", got[2], want[2])):
        for k, (a, b) in enumerate(zip(g, w)):
            same(a, b, (what, name, k + 1))
            assert not np.isnan(b).any()


def random_plane(rng, W, H):
    """an HDR frame with everything the definition distinguishes: mostly dim, some pixels far above any threshold, a dark region below every
    threshold, and single values that are NaN, +inf, -inf, negative, -0, 1e30 and exactly at the records' thresholds"""
    C = (rng.uniform(0.0, 1.0, (H, W, 3)) ** 4 * 20.0).astype(F)
    ys, xs = np.mgrid[0:H, 0:W]
    C[(ys // 5 + xs // 7) % 4 == 0] *= F(0.01)
    odd = np.array([np.nan, np.inf, -np.inf, -3.0, -0.0, 1e30, 1.0, 0.7, 0.5, 0.525, 65504.0], F)
    flat = C.reshape(-1)
    where = rng.permutation(flat.size)[:len(odd)]
    flat[where] = odd[:len(where)]
    return C


@functools.lru_cache(maxsize=None)
def case(width, height):
    """the frame of a size, the same for every test that asks (read only)"""
    C = random_plane(np.random.default_rng(5100 + 3 * width + height), width, height)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def reference(width, height, levels, record):
    """(out, D, U) of the numpy definition for case(width, height): computed once, shared, left unchanged"""
    out, D, U = B.bloom(case(width, height), levels=levels, **{k: v for k, v in RECORDS[record].items() if k != "levels"})
    for a in [out] + D + U:
        a.setflags(write=False)
    return out, D, U


def record_kw(record, levels):
    return dict(RECORDS[record], levels=levels)


def arbiters(pkg, C, **kw):
    """steps 1 to 4 by the host arbiters, every pixel listed: (out, D, U)"""
    H, W = C.shape[:2]
    D, U = pkg.renderer.bloom_pyramid(C, **kw)
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], -1).astype(np.int32)
    out = pkg.renderer.bloom_pixels(xy, C, U[0] if U else D[0], **kw).reshape(H, W, 3)
    return out, D, U


# ---- by hand: scalars, one rounding per line ---------------------------------------------------------------------------------------------------------
def hand_prefilter(c, threshold, soft_knee, clamp_max):
    threshold, soft_knee, clamp_max = F(threshold), F(soft_knee), F(clamp_max)
    x = [(min(F(v), clamp_max) if v > 0 else F(0.0)) for v in c]
    br = max(x)
    knee = F(threshold * soft_knee)
    t = F(br - F(threshold - knee))
    t = min(max(t, F(0.0)), F(F(2.0) * knee))
    soft = F(F(t * t) / F(F(F(4.0) * knee) + F(1e-5)))
    m = max(soft, F(br - threshold))
    contrib = min(F(m / max(br, F(1e-5))), F(1.0))
    return [F(v * contrib) for v in x]


def hand_down(S, x, y, karis):
    """S: a nested list [row][column] of 3-lists of np.float32"""
    Hs, Ws = len(S), len(S[0])
    cols = [min(max(2 * x - 2 + i, 0), Ws - 1) for i in range(6)]
    rows = [min(max(2 * y - 2 + j, 0), Hs - 1) for j in range(6)]
    out = []
    G = []
    for ch in range(3):
        t = [[F(S[rows[j]][cols[i]][ch]) for i in range(6)] for j in range(6)]     # t[j][i]
        box = lambda a, b: F(F(F(t[b][a] + t[b][a + 1]) + F(t[b + 1][a] + t[b + 1][a + 1])) * F(0.25))
        group = lambda a, b: F(F(F(box(a, b) + box(a + 2, b)) + F(box(a, b + 2) + box(a + 2, b + 2))) * F(0.25))
        G.append([group(1, 1), group(0, 0), group(2, 0), group(0, 2), group(2, 2)])
    if not karis:
        for ch in range(3):
            g = G[ch]
            out.append(F(F(g[0] * F(0.5)) + F(F(F(g[1] + g[2]) + F(g[3] + g[4])) * F(0.125))))
        return out
    w = []
    for k in range(5):
        l = F(F(F(F(0.2126) * G[0][k]) + F(F(0.7152) * G[1][k])) + F(F(0.0722) * G[2][k]))
        w.append(F(F(0.5 if k == 0 else 0.125) / F(F(1.0) + l)))
    den = F(w[0] + F(F(w[1] + w[2]) + F(w[3] + w[4])))
    for ch in range(3):
        g = G[ch]
        num = F(F(w[0] * g[0]) + F(F(F(w[1] * g[1]) + F(w[2] * g[2])) + F(F(w[3] * g[3]) + F(w[4] * g[4]))))
        out.append(F(num / den))
    return out


def hand_up(T, x, y):
    Ht, Wt = len(T), len(T[0])

    def axis(v):
        h = v >> 1
        return (h - 1, [F(0.1875), F(0.4375), F(0.3125), F(0.0625)]) if v & 1 else (h - 2, [F(0.0625), F(0.3125), F(0.4375), F(0.1875)])
    (bx, wx), (by, wy) = axis(x), axis(y)
    cols = [min(max(bx + i, 0), Wt - 1) for i in range(4)]
    rows = [min(max(by + j, 0), Ht - 1) for j in range(4)]
    out = []
    for ch in range(3):
        r = [F(F(F(wx[0] * T[rows[j]][cols[0]][ch]) + F(wx[1] * T[rows[j]][cols[1]][ch])) + F(F(wx[2] * T[rows[j]][cols[2]][ch]) + F(wx[3] * T[rows[j]][cols[3]][ch]))) for j in range(4)]
        out.append(F(F(F(wy[0] * r[0]) + F(wy[1] * r[1])) + F(F(wy[2] * r[2]) + F(wy[3] * r[3]))))
    return out


def hand_bloom(C, threshold, soft_knee, clamp_max, intensity, spread, levels):
    """the whole definition with scalars and python lists: (out, D, U) as arrays"""
    H, W = C.shape[:2]
    S = [[hand_prefilter(C[y, x], threshold, soft_knee, clamp_max) for x in range(W)] for y in range(H)]
    D = []
    for k in range(levels):
        w, h = (len(S[0]) + 1) // 2, (len(S) + 1) // 2
        S = [[hand_down(S, x, y, k == 0) for x in range(w)] for y in range(h)]
        D.append(S)
    U = [None] * levels
    U[levels - 1] = D[levels - 1]
    for k in range(levels - 1, 0, -1):
        up = [[hand_up(U[k], x, y) for x in range(len(D[k - 1][0]))] for y in range(len(D[k - 1]))]
        U[k - 1] = [[[F(D[k - 1][y][x][ch] + F(F(spread) * up[y][x][ch])) for ch in range(3)] for x in range(len(up[0]))] for y in range(len(up))]
    out = np.empty((H, W, 3), F)
    for y in range(H):
        for x in range(W):
            t = hand_up(U[0], x, y)
            for ch in range(3):
                a = F(F(intensity) * t[ch])
                out[y, x, ch] = F(C[y, x, ch] + a) if a > 0 else C[y, x, ch]
    return out, [np.array(d, F) for d in D], [np.array(u, F) for u in U[:levels - 1]]


def by_hand(C, **kw):
    kw = dict(B.DEFAULTS, **kw)
    with np.errstate(all="ignore"):
        return hand_bloom(np.asarray(C, F), **kw)


def test_level_sizes_and_the_layout(pkg, lib):
    assert B.level_sizes(17, 9, 8) == [(9, 5), (5, 3), (3, 2), (2, 1), (1, 1), (1, 1), (1, 1), (1, 1)]
    assert B.level_sizes(1, 1, 3) == [(1, 1)] * 3 and B.level_sizes(136, 72, 2) == [(68, 36), (34, 18)]
    for W, H in SIZES:
        for L in LEVELS:
            lay = pkg.renderer.bloom_layout(W, H, L)
            sizes = B.level_sizes(W, H, L)
            floats = [w * h * 3 for w, h in sizes]
            assert lay["sizes"] == sizes and lay["offsets"] == [sum(floats[:k]) for k in range(L)]
            assert lay["down_floats"] == sum(floats) and lay["up_floats"] == sum(floats[:-1])


def test_one_pixel_frames_by_hand():
    """a 1 x 1 frame: every texel of every footprint is the one pixel.  c = (4, 2, 1) under threshold 1, knee 0.5: br = 4, t = min(3.5, 1) = 1,
    soft = 1 / 2.00001, m = max(soft, 3) = 3, contrib = 0.75, b = (3, 1.5, 0.75) exactly; every box and group is b; Karis: every l is
    0.2126 * 3 + 0.7152 * 1.5 + 0.0722 * 0.75 and D_1 = num / den"""
    C = np.array([[[4.0, 2.0, 1.0]]], F)
    assert [float(v) for v in hand_prefilter(C[0, 0], 1.0, 0.5, 65504.0)] == [3.0, 1.5, 0.75]
    assert B.prefilter(C).tolist() == [[[3.0, 1.5, 0.75]]]
    l = F(F(F(F(0.2126) * F(3.0)) + F(F(0.7152) * F(1.5))) + F(F(0.0722) * F(0.75)))
    w0, w = F(F(0.5) / F(F(1.0) + l)), F(F(0.125) / F(F(1.0) + l))
    den = F(w0 + F(F(w + w) + F(w + w)))
    d1 = [F(F(F(w0 * b) + F(F(F(w * b) + F(w * b)) + F(F(w * b) + F(w * b)))) / den) for b in (F(3.0), F(1.5), F(0.75))]
    for L in (1, 8):
        out, D, U = B.bloom(C, levels=L)
        assert len(D) == L and len(U) == L - 1 and all(d.shape == (1, 1, 3) for d in D)
        assert D[0][0, 0].tolist() == [float(v) for v in d1]
        same_bloom((out, D, U), by_hand(C, levels=L), ("1x1", L))
    # at one level the composite is the tent of the one texel in x, then in y, times intensity 0.5
    out = B.bloom(C, levels=1)[0]
    row = lambda v: F(F(F(F(0.0625) * v) + F(F(0.3125) * v)) + F(F(F(0.4375) * v) + F(F(0.1875) * v)))
    assert out[0, 0].tolist() == [float(F(c + F(F(0.5) * row(row(v))))) for c, v in zip(C[0, 0], d1)]


def test_two_by_two_by_hand():
    """2 x 2: level 1 is one pixel whose footprint's columns and rows clamp to 0, 0, 0, 1, 1, 1"""
    C = np.array([[[4.0, 2.0, 1.0], [0.5, 0.25, 8.0]], [[1.0, 1.0, 1.0], [0.0, 6.0, 3.0]]], F)
    for L in (1, 2):
        for rec in RECORDS:
            kw = dict(rec, levels=L)
            same_bloom(B.bloom(C, **kw), by_hand(C, **kw), ("2x2", L))
    b = B.prefilter(C, threshold=0.0, soft_knee=0.0)
    assert b.tobytes() == C.tobytes()                                            # threshold 0, knee 0: contrib is br / br = 1
    # plain form on one channel, worked: boxes of the clamped footprint [[a a a b b b] x3, [c c c d d d] x3]
    S = np.zeros((2, 2, 3), F)
    S[..., 0] = [[16.0, 32.0], [48.0, 64.0]]
    a, bb, c, d = 16.0, 32.0, 48.0, 64.0
    box = {(0, 0): a, (2, 0): (a + bb) / 2, (4, 0): bb, (0, 2): (a + c) / 2, (2, 2): (a + bb + c + d) / 4, (4, 2): (bb + d) / 2, (0, 4): c, (2, 4): (c + d) / 2, (4, 4): d,
           (1, 1): a, (3, 1): bb, (1, 3): c, (3, 3): d}
    group = lambda i, j: (box[(i, j)] + box[(i + 2, j)] + box[(i, j + 2)] + box[(i + 2, j + 2)]) / 4
    want = group(1, 1) * 0.5 + (group(0, 0) + group(2, 0) + group(0, 2) + group(2, 2)) * 0.125    # (small integers over powers of two: exact in any order)
    assert float(B.down(S, False)[0, 0, 0]) == want == 40.0


def test_one_bright_pixel_and_the_corner():
    """one pixel of 16 on black, threshold 0 and knee 0 (b = C), one level.  Its place in a destination's footprint decides which of the five
    groups hold it; a group that holds it has the value 16 / 16 = 1 per covering texel.  In the frame's corner the clamped footprint repeats it"""
    C = np.zeros((8, 8, 3), F)
    C[4, 4] = 16.0
    kw = dict(threshold=0.0, soft_knee=0.0, levels=1)
    D1 = B.pyramid(C, **kw)[0][0]
    lit = {(x, y) for y in range(4) for x in range(4) if D1[y, x, 0] != 0}
    assert lit == {(x, y) for y in (1, 2, 3) for x in (1, 2, 3)}                  # 2x - 2 <= 4 <= 2x + 3
    # destination (2, 2): the pixel is texel (2, 2) of the footprint, inside all five groups, each of which is 1: D_1 = 1 up to Karis' roundings
    l = F(F(F(F(0.2126) * F(1)) + F(F(0.7152) * F(1))) + F(F(0.0722) * F(1)))
    w0, w = F(F(0.5) / F(F(1) + l)), F(F(0.125) / F(F(1) + l))
    assert D1[2, 2].tolist() == [float(F(F(w0 + F(F(w + w) + F(w + w))) / F(w0 + F(F(w + w) + F(w + w)))))] * 3 == [1.0] * 3
    # destination (1, 1): texel (4, 4), in G0 [1..4]^2 and G4 [2..5]^2 only; (3, 3): texel (0, 0), in G1 [0..3]^2 only
    g = F(1.0)
    assert D1[1, 1].tolist() == [float(F(F(F(w0 * g) + F(F(F(0) + F(0)) + F(F(0) + F(w * g)))) / F(w0 + F(F(F(0.125) + F(0.125)) + F(F(0.125) + w)))))] * 3
    assert D1[3, 3].tolist() == [float(F(F(F(0) + F(F(F(w * g) + F(0)) + F(0))) / F(F(0.5) + F(F(w + F(0.125)) + F(F(0.125) + F(0.125))))))] * 3
    same_bloom(B.bloom(C, **kw), by_hand(C, **kw), "one bright pixel")
    # the corner: pixel (0, 0) fills texels (0..2, 0..2) of destination (0, 0)'s footprint: 9 of G1's 16 texels, 4 of G0's, 1 of G2's, G3's and G4's
    K = np.zeros((8, 8, 3), F)
    K[0, 0] = 16.0
    D1 = B.pyramid(K, **kw)[0][0]
    G = [F(4), F(9), F(3), F(3), F(1)]
    wk = [F(F(0.5 if k == 0 else 0.125) / F(F(1) + F(F(F(F(0.2126) * v) + F(F(0.7152) * v)) + F(F(0.0722) * v)))) for k, v in enumerate(G)]
    num = F(F(wk[0] * G[0]) + F(F(F(wk[1] * G[1]) + F(wk[2] * G[2])) + F(F(wk[3] * G[3]) + F(wk[4] * G[4]))))
    assert D1[0, 0].tolist() == [float(F(num / F(wk[0] + F(F(wk[1] + wk[2]) + F(wk[3] + wk[4])))))] * 3
    assert (D1[2:, :] == 0).all() and (D1[:, 2:] == 0).all()                     # 2x - 2 <= 0: x <= 1
    same_bloom(B.bloom(K, **kw), by_hand(K, **kw), "the corner")


def test_even_and_odd_in_up():
    """a coarse row 0, 16, 32, 48: even x = 2 reads texels -1..2 (clamped 0, 0, 1, 2) with (1, 5, 7, 3) / 16, odd x = 3 reads 0..3 with (3, 7, 5, 1) / 16"""
    T = np.zeros((1, 4, 3), F)
    T[0, :, 0] = [0.0, 16.0, 32.0, 48.0]
    got = B.up(T, 8, 1)[0, :, 0].tolist()
    assert got[2] == (1 * 0 + 5 * 0 + 7 * 16 + 3 * 32) / 16 == 13.0 and got[3] == (3 * 0 + 7 * 16 + 5 * 32 + 1 * 48) / 16 == 20.0
    assert got[0] == (7 * 0 + 3 * 16) / 16 == 3.0 and got[7] == (3 * 32 + 13 * 48) / 16 == 45.0      # both edges clamp
    assert B.up(T.transpose(1, 0, 2).copy(), 1, 8)[:, 0, 0].tolist() == got      # the same rule in y
    assert [float(v) for v in (hand_up(T.tolist(), x, 0)[0] for x in range(8))] == got


def test_the_knee():
    """threshold 1, soft_knee 0.5: knee = 0.5.  br = 0.5: t = 0, soft = 0, m = max(0, -0.5) = 0: nothing.  br = 1: t = 0.5, soft = 0.25 / 2.00001,
    m = soft.  br = 1.5: t = min(1, 1) = 1, soft = 1 / 2.00001 < 0.5 = br - threshold: the line.  And threshold 0, soft_knee 0: b = x"""
    soft = lambda t: F(F(F(t) * F(t)) / F(F(F(4.0) * F(0.5)) + F(1e-5)))
    for br, m in ((0.5, F(0.0)), (1.0, soft(0.5)), (1.5, F(0.5)), (0.25, F(0.0)), (0.75, soft(0.25))):
        C = np.array([[[br, br / 2, 0.0]]], F)
        want = [F(F(v) * min(F(m / F(br)), F(1.0))) for v in (br, br / 2, 0.0)]
        assert B.prefilter(C).tolist() == [[[float(v) for v in want]]], br
        assert [float(v) for v in hand_prefilter(C[0, 0], 1.0, 0.5, 65504.0)] == [float(v) for v in want]
    assert B.prefilter(np.array([[[0.5, 0.25, 0.0]]], F)).tobytes() == np.zeros(3, F).tobytes()      # +0, by bits
    rng = np.random.default_rng(2)
    C = rng.uniform(0.0, 9.0, (4, 5, 3)).astype(F)
    assert B.prefilter(C, threshold=0.0, soft_knee=0.0).tobytes() == C.tobytes()
    assert B.prefilter(C, threshold=0.0, soft_knee=1.0).tobytes() == C.tobytes()   # knee = 0 either way
    assert (B.prefilter(C, threshold=2.0, soft_knee=0.0)[C.max(-1) <= 2.0] == 0).all()               # a hard threshold


def test_odd_colours():
    """NaN and negative channels become 0, +inf becomes clamp_max, and -inf 0, before anything else is worked out"""
    kw = dict(threshold=1.0, soft_knee=0.5, clamp_max=8.0)
    for c, x in (([np.nan, 4.0, 2.0], [0.0, 4.0, 2.0]), ([np.inf, 4.0, 2.0], [8.0, 4.0, 2.0]), ([-np.inf, 4.0, 2.0], [0.0, 4.0, 2.0]), ([-3.0, -0.0, 2.0], [0.0, 0.0, 2.0]),
                 ([np.nan, np.nan, np.nan], [0.0, 0.0, 0.0]), ([1e30, 16.0, 0.5], [8.0, 8.0, 0.5])):
        got = B.prefilter(np.array([[c]], F), **kw)
        want = B.prefilter(np.array([[x]], F), **kw)
        assert got.tobytes() == want.tobytes() and np.isfinite(got).all() and (got >= 0).all(), c
        assert [float(v) for v in hand_prefilter(np.array(c, F), 1.0, 0.5, 8.0)] == got[0, 0].tolist()
    assert B.prefilter(np.array([[[np.nan, -1.0, -np.inf]]], F), **kw).tobytes() == np.zeros(3, F).tobytes()


@pytest.mark.parametrize("width, height", SIZES[:4], ids=lambda v: str(v))
def test_the_reference_equals_the_scalars_on_small_frames(width, height):
    """the vectorised restatement against the scalar one, whole frames: 1 x 1 to 17 x 9 (the scalar one is slow)"""
    for L in ((1, 2, 5, 8) if width * height <= 64 else (2, 8)):
        same_bloom(reference(width, height, L, 1), by_hand(case(width, height), **record_kw(1, L)), (width, height, L))


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
def test_arbiters_equal_numpy_by_bytes(pkg, lib, width, height):
    C = case(width, height)
    assert np.isnan(C).any() or width * height < 4
    for L in LEVELS:
        for rec in range(len(RECORDS)):
            same_bloom(arbiters(pkg, C, **record_kw(rec, L)), reference(width, height, L, rec), (width, height, L, rec))


# ---- deliberate defects: each in a copy of the reference's source, each must change output bytes ------------------------------------------------------
DEFECTS = {
    "an addition order changed": ("((tex(a, b) + tex(a + 1, b)) + (tex(a, b + 1) + tex(a + 1, b + 1)))", "(((tex(a, b) + tex(a + 1, b)) + tex(a, b + 1)) + tex(a + 1, b + 1))"),
    "wrap instead of clamp": ("cx = np.clip(2 * xs - 2 + i, 0, Ws - 1)", "cx = (2 * xs - 2 + i) % Ws"),
    "floor instead of ceil level sizes": ("xs, ys = np.arange((Ws + 1) // 2), np.arange((Hs + 1) // 2)", "xs, ys = np.arange(max(Ws // 2, 1)), np.arange(max(Hs // 2, 1))"),
    "the footprint shifted by one": ("cx = np.clip(2 * xs - 2 + i, 0, Ws - 1)", "cx = np.clip(2 * xs - 1 + i, 0, Ws - 1)"),
    "odd and even weights swapped": ("np.where(odd[:, None], np.array(ODD, dt)[None, :], np.array(EVEN, dt)[None, :])", "np.where(odd[:, None], np.array(EVEN, dt)[None, :], np.array(ODD, dt)[None, :])"),
    "Karis dropped": ("D = [down(prefilter(C, dt, **kw), karis, dt)]", "D = [down(prefilter(C, dt, **kw), False, dt)]"),
    "the knee's denominator changed": ("(dt(4) * knee + dt(F(1e-5)))", "(dt(2) * knee + dt(F(1e-5)))"),
    "spread applied at the wrong level": ("U[k - 1] = D[k - 1] + spread * up(U[k], D[k - 1].shape[1], D[k - 1].shape[0], dt)",
                                          "U[k - 1] = spread * D[k - 1] + up(U[k], D[k - 1].shape[1], D[k - 1].shape[0], dt)"),
    "the select replaced by a plain add": ("return np.where(a > 0, C + a, C)", "return C + a"),
    "a contracted multiply-add": ("U[k - 1] = D[k - 1] + spread * up(U[k], D[k - 1].shape[1], D[k - 1].shape[0], dt)",
                                  "U[k - 1] = (D[k - 1].astype(np.float64) + np.float64(spread) * up(U[k], D[k - 1].shape[1], D[k - 1].shape[0], dt).astype(np.float64)).astype(dt)"),
    "a NaN let through the prefilter": ("x = np.where(C > 0, _min(C, clamp_max), dt(0))", "x = _min(_max(C, dt(0)), clamp_max)"),
}


def defective(name):
    """a copy of tests/bloom_reference.py with one line replaced"""
    old, new = DEFECTS[name]
    source = open(os.path.join(HERE, "bloom_reference.py")).read()
    assert source.count(old) == 1, (name, "the line to replace is not there exactly once")
    spec = importlib.util.spec_from_loader("bloom_defect", loader=None)
    module = importlib.util.module_from_spec(spec)
    exec(compile(source.replace(old, new), "bloom_defect:" + name, "exec"), module.__dict__)
    return module


def changed(got, want):
    planes = lambda r: [r[0]] + list(r[1]) + list(r[2])
    a, b = planes(got), planes(want)
    return len(a) != len(b) or any(x.shape != y.shape or x.tobytes() != y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(DEFECTS), ids=lambda n: n.replace(" ", "-"))
def test_a_defect_changes_bytes(name):
    kw = record_kw(1, 3)
    if name == "the select replaced by a plain add":
        # where bloom reaches a pixel both forms add; the select shows where none does: a dark frame with a -0 pixel, whose sum with +0 is +0,
        # and a NaN pixel with a payload of its own, which the select hands on by bits
        C = np.full((9, 17, 3), 0.25, F)
        C[4, 8] = F(-0.0)
        C[6, 3] = np.array([0x7FA00001], np.uint32).view(F)[0]
        assert B.bloom(C, **kw)[0].tobytes() == C.tobytes()
    else:
        C = case(17, 9)
    want = B.bloom(C, **kw)
    assert not changed(B.bloom(C, **kw), want)                                   # (the definition itself gives the same bytes twice)
    with np.errstate(all="ignore"):
        got = defective(name).bloom(C, **kw)
    assert changed(got, want), name
    if name == "the select replaced by a plain add":
        assert got[0][4, 8].tobytes() != C[4, 8].tobytes() and np.isnan(got[0][6, 3]).all()
        print("the NaN pixel's bits under the plain add:", [hex(v) for v in got[0][6, 3].view(np.uint32)], "against", [hex(v) for v in C[6, 3].view(np.uint32)])


# ---- behaviour, numpy alone, 64 x 40 ---------------------------------------------------------------------------------------------------------------------
W0, H0 = 64, 40


def test_a_frame_below_the_knee_is_untouched():
    """(a) every pixel has br <= threshold - knee: every plane is +0 by bits and out is C by bits, NaN pixels included"""
    rng = np.random.default_rng(11)
    C = rng.uniform(0.0, 0.5, (H0, W0, 3)).astype(F)                             # threshold 1, knee 0.5
    C[3, 5] = C[20, 40, 1] = F(np.nan)
    C[7, 7] = F(-2.0)
    C[9, 9] = F(-0.0)
    for L in (1, 5, 8):
        out, D, U = B.bloom(C, levels=L)
        for plane in D + U:
            assert plane.tobytes() == np.zeros(plane.shape, F).tobytes()
        assert out.tobytes() == C.tobytes()


def test_a_constant_frame_against_the_closed_form():
    """(b) a grey c above the threshold under a hard threshold: b = c - threshold, every D_k is b, U_1 = b * sum(spread^i, i < L) and
    out = c + intensity * (c - threshold) * sum(spread^i): float64, against fp32 within the project's 1e-4 relative"""
    c, thr, intensity, spread = 3.3, 0.9, 0.45, 0.7
    C = np.full((H0, W0, 3), c, F)
    for L in (1, 5, 8):
        out = B.bloom(C, threshold=thr, soft_knee=0.0, intensity=intensity, spread=spread, levels=L)[0]
        want = c + intensity * (c - thr) * sum(spread ** i for i in range(L))
        err = np.abs(out.astype(np.float64) - want).max() / want
        print(f"constant frame, {L} levels: closed form {want:.9f}, largest relative error {err:.3e}")
        assert err <= TOL, (L, err)


def test_every_plane_is_finite_and_not_negative():
    """(c) whatever C holds, every D_k and U_k is finite and >= 0; a NaN pixel stays NaN and every other pixel of out is finite"""
    rng = np.random.default_rng(12)
    C = (rng.uniform(0.0, 1.0, (H0, W0, 3)) ** 6 * 1e5).astype(F)
    kinds = np.array([np.nan, np.inf, -np.inf, -1e30, 1e38, -0.0, 65504.0, 3.4e38], F)
    pick = rng.random((H0, W0, 3)) < 0.08
    C[pick] = kinds[rng.integers(0, len(kinds), int(pick.sum()))]
    for rec in RECORDS:
        for L in (1, 5, 8):
            with np.errstate(over="ignore"):
                out, D, U = B.bloom(C, **dict(rec, levels=L, clamp_max=65504.0, intensity=16.0))
            for plane in D + U:
                assert np.isfinite(plane).all() and (plane >= 0).all() and not (plane.view(np.uint32) == 0x80000000).any()
            assert (np.isnan(out) == np.isnan(C)).all()
            rest = ~np.isnan(C) & np.isfinite(C) & (np.abs(C) < 1e38)
            assert np.isfinite(out[rest]).all()


def test_karis_lowers_a_firefly():
    """(d) one pixel at clamp_max in a dim field: level 1's peak with Karis' weights against the peak without them (the dropped-Karis defect).

    What the definition can and cannot do here, reasoned before anything was run.  The peak of level 1 is the destination whose footprint holds
    the firefly at texel 2 or 3 of either axis: there it lies inside ALL FIVE groups, and each group is firefly / 16 plus its share m_g of the
    field.  Karis' weights depend on a group's own luminance alone, so where the five groups are equal they cancel: in a field that the
    prefilter turns black (any field below threshold - knee) the peak is firefly / 16 with and without them, the ratio is 1 up to the
    roundings of num / den, and Karis suppresses NOTHING of an isolated firefly.  It acts only through the differences m_g of the field: the
    weighted mean falls below the plain one by about Var(G) / (1 + l), that is, relative to the peak g = firefly / 16, by Var(m) / (g * (1 + g)).
    That inequality (Chebyshev's, for weights that fall as the values rise) holds per channel only where a group's channel and its luminance
    are ordered alike -- in a GREY field; in a coloured one a channel of the peak can rise (measured: 4.0935798 against 4.0935764).  With a
    grey field uniform in [0, 0.2] that enters the pyramid (threshold 0), Var(m) is some 1e-4, which fp32 resolves (6e-8) only while
    g * g < 1e3: clamp_max = 64 gives g = 4 and a fall of some 5e-6, clamp_max = 65504 gives 1e-11 -- nothing.  So the condition `ratio < 1`
    is asserted for the case where the definition can meet it, and the black field's ratio of 1 is asserted as what it is."""
    rng = np.random.default_rng(13)
    field = np.repeat(rng.uniform(0.0, 0.2, (H0, W0, 1)).astype(F), 3, axis=2)
    peak = lambda C, **kw: (float(B.pyramid(C, levels=1, **kw)[0][0].max()), float(B.pyramid(C, levels=1, karis=False, **kw)[0][0].max()))
    C = field.copy()
    C[20, 32] = F(65504.0)
    with_karis, without = peak(C)                                                # the default record: the field is below threshold - knee
    print(f"firefly at 65504 in a field the prefilter turns black: level 1's peak {with_karis:.4f} with Karis, {without:.4f} without: ratio {with_karis / without:.7f}")
    assert abs(with_karis / without - 1.0) <= 1e-6
    C = field.copy()
    C[20, 32] = F(64.0)
    with_karis, without = peak(C, threshold=0.0, soft_knee=0.0, clamp_max=64.0)
    print(f"firefly at clamp_max = 64 in a field that enters the pyramid: level 1's peak {with_karis:.6f} with Karis, {without:.6f} without: ratio {with_karis / without:.7f}")
    assert with_karis / without < 1.0


def test_fp32_against_the_float64_definition():
    """(e) the same definition in float64 on a random HDR frame.  `out` is held to the 1e-4 bar relative to itself.  A plane's elements near the
    knee are differences of nearly equal numbers (t = br - (threshold - knee)), whose error is bounded by the operands' rounding, not by the
    result's size: the planes are held to 1e-4 of the plane's largest value"""
    rng = np.random.default_rng(14)
    C = (rng.uniform(0.0, 1.0, (H0, W0, 3)) ** 4 * 30.0).astype(F) + F(1e-3)
    worst_out = worst_plane = 0.0
    for rec in RECORDS:
        for L in (1, 5, 8):
            kw = dict(rec, levels=L)
            out32, D32, U32 = B.bloom(C, **kw)
            out64, D64, U64 = B.bloom(C, np.float64, **kw)
            worst_out = max(worst_out, float((np.abs(out32 - out64) / np.abs(out64)).max()))
            for a, b in zip(D32 + U32, D64 + U64):
                assert b.dtype == np.float64
                worst_plane = max(worst_plane, float(np.abs(a - b).max() / b.max()))
    print(f"fp32 against float64: out {worst_out:.3e} relative, planes {worst_plane:.3e} of the plane's largest value")
    assert worst_out <= TOL and worst_plane <= TOL
