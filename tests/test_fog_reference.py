"""Volumetric fog on a machine without a GPU: numpy in fp32 (tests/fog_reference.py) reproduces the host arbiter arctic_fog_pixels -- the very
functions k_fog_march runs -- BY BYTES, no pixel left out; fog_exp2 measured on every float of [0, 1]; the physics against float64 closed forms
and a 4096-step march; arctic_fog_view against the camera's and the sun's matrices."""
import numpy as np
import pytest

import fog_reference as G

F = np.float32
SIZES = ((8, 8), (13, 11), (64, 40))
MAPS = (0, 16, 64)
STEPS = (1, 7, 32, 128)
RECORD = dict(density=0.12, anisotropy=0.6, max_distance=45.0, bias=0.004, scatter_color=(3.0, 2.5, 2.0), ambient_color=(0.05, 0.06, 0.08))
# a view whose samples cross the map (fog_reference.view_record's rows), and a hostile one: rows that send every sample far outside, to minus
# infinity and through NaN (the fields are finite, the products overflow).  The samples that leave the map by each clause of the inside test
# alone are fog_reference.EDGE_VIEWS' business (test_every_clause_of_the_inside_test_decides_samples)
HOSTILE = dict(eye=(1e30, -1e30, 3e30), ray00=(-3e30, 2e30, 1e30), ray_dx=(1e29, 0.0, -1e29), ray_dy=(0.0, -1e29, 1e29),
               light=((3e38, -3e38, 3e38, -1.0), (-3e38, 3e38, 1.0, 0.5), (1e-30, 0.0, 0.0, 0.5)))


def planes(width, height, seed=0):
    """C with NaN, infinite and negative colours; depths 0, 1.0, beyond 1 and NaN among ordinary ones"""
    rng = np.random.default_rng(4100 + width + seed)
    C = rng.uniform(0.0, 4.0, (height, width, 3)).astype(F)
    C[0, 0] = (np.nan, 1.0, 2.0); C[1, 2] = (np.inf, -np.inf, 0.5); C[2, 1] = (-1.5, -0.0, 7.0); C[height - 1, width - 1] = (0.0, -0.0, np.nan)
    z = rng.uniform(0.90, 0.9999, (height, width)).astype(F)
    z[0, 1], z[1, 1], z[3, 0], z[3, 3], z[height - 1, 0] = 0.0, 1.0, 1.5, np.nan, 1.0
    z[4:, 5:] = 1.0                                                              # the sky
    return C, z


def shadow_map(S, seed=0):
    """depths with lit and shadowed blocks, and a NaN and an infinite texel"""
    if S == 0:
        return None
    rng = np.random.default_rng(4200 + S + seed)
    m = rng.uniform(0.3, 0.7, (S, S)).astype(F)
    m[S // 4:S // 2] = 1.0
    m[:, S // 2:S // 2 + S // 8] = 0.0
    m[1, 1], m[2, 2] = np.nan, np.inf
    return m


def table(seed=0):
    return ((np.random.default_rng(4300 + seed).permutation(16) + 0.25) / 16.0).astype(F)


def all_pixels(width, height):
    py, px = np.mgrid[0:height, 0:width]
    return np.stack([px.ravel(), py.ravel()], -1).astype(np.int32)


def arbiter(pkg, C, z, m, view, offsets=None, **kw):
    """arctic_fog_pixels of every pixel; the map it reads is a copy with sentinels around it: -1e30 shadows every sample that reads one, so a
    lookup outside the map would not equal numpy, which bounds its own"""
    height, width = C.shape[:2]
    if m is not None:
        S = m.shape[0]
        room = np.full(S * S + 2 * 4 * S, -1e30, F)
        room[4 * S:4 * S + S * S] = m.ravel()
        m = room[4 * S:4 * S + S * S].reshape(S, S)
    out, terms = pkg.renderer.fog_pixels(all_pixels(width, height), C, view, z, m, offsets, terms=True, **kw)
    return out.reshape(height, width, 3), terms[:, 0].reshape(height, width), terms[:, 1].reshape(height, width)


def same_fog(got, want, what):
    for g, w, name in zip(got, want, ("out", "T", "I")):
        G.same(g, w, (what, name))


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
def test_numpy_equals_the_arbiter_by_bytes(pkg, width, height):
    C, z = planes(width, height)
    views = (G.view_record(), G.view_record(**HOSTILE))
    read_total = 0
    for S in MAPS:
        m = shadow_map(S)
        for steps in STEPS:
            for vi, view in enumerate(views):
                kw = dict(RECORD, steps=steps)
                offsets = table(steps) if steps in (7, 128) else None
                want = G.fog(C, z, m, view, offsets, **kw)
                same_fog(arbiter(pkg, C, z, m, view, offsets, **kw), want[:3], (width, height, S, steps, vi))
                T, I = want[1].astype(np.float64), want[2].astype(np.float64)
                ok = np.isfinite(T)
                assert (T[ok] <= 1.0).all() and (I[ok] >= 0.0).all() and (I[ok] <= (1.0 - T[ok]) + steps * 2.0 ** -24).all()      # the exact properties
                if vi == 0:
                    read_total += want[3]
                    if S:
                        shadowed = (I < (1.0 - T) - 1e-6).mean()
                        assert steps == 1 or 0.02 <= shadowed <= 0.98, (S, steps, shadowed)   # the map decides: neither all lit nor all dark
                else:
                    assert want[3] == 0                                          # the hostile rows never reach a texel
    assert read_total > 0
    m = shadow_map(16)
    # density 0: the input by bits, NaN and -0 included
    out, T, I = arbiter(pkg, C, z, m, views[0], **dict(RECORD, density=0.0, steps=7))
    G.same(out, C, "density 0")
    assert (T == 1.0).all() and (I == 0.0).all()
    same_fog((out, T, I), G.fog(C, z, m, views[0], **dict(RECORD, density=0.0, steps=7))[:3], "density 0, numpy")
    # max_distance nearer than every surface, no depth plane, and the largest density
    for kw, zz in ((dict(RECORD, max_distance=0.75, steps=32), z), (dict(RECORD, steps=32), None), (dict(RECORD, density=64.0, steps=128), z)):
        same_fog(arbiter(pkg, C, zz, m, views[0], table(3), **kw), G.fog(C, zz, m, views[0], table(3), **kw)[:3], kw)
    # a NaN colour stays in its own pixel
    out = arbiter(pkg, C, z, m, views[0], **dict(RECORD, steps=7))[0]
    assert (np.isnan(out).any(-1) == np.isnan(C).any(-1)).all()


EDGE_CASES = [(name, S, steps) for name in G.EDGE_VIEWS for S in (16, 64) for steps in (7, 32)]


def edge_case(width, height, name, S, steps):
    """(C, z, map, view, offsets, kw) of an edge case, and numpy's result: samples leave the map by the clause `name` alone, and others read it"""
    C, z = planes(width, height)
    view = G.view_record(**G.EDGE_VIEWS[name])
    offsets = table(steps) if steps == 7 else None
    kw = dict(RECORD, steps=steps)
    want = G.fog(C, z, shadow_map(S), view, offsets, **kw)
    assert want[4][name] > 0 and want[3] > 0, (name, S, steps, want[3], want[4])
    assert sum(v for k, v in want[4].items() if k != name) == 0, (name, want[4])   # ... and by no other clause
    return C, z, shadow_map(S), view, offsets, kw, want


@pytest.mark.parametrize("width, height", SIZES, ids=lambda v: str(v))
def test_every_clause_of_the_inside_test_decides_samples(pkg, width, height):
    """light rows that send samples off each of the four sides of the map with the other coordinate inside, and beyond depth 1 with the texel
    inside: per case such samples exist (and samples that read the map), and the arbiter equals numpy by bytes.  An evaluation without that
    clause reads another texel, or compares where the definition says lit"""
    for name, S, steps in EDGE_CASES:
        C, z, m, view, offsets, kw, want = edge_case(width, height, name, S, steps)
        same_fog(arbiter(pkg, C, z, m, view, offsets, **kw), want[:3], (width, height, name, S, steps))
        dark = want[2].astype(np.float64) < (1.0 - want[1].astype(np.float64)) - 1e-6
        assert dark.any(), (name, S, steps)                                       # the map shadows some of the samples that stay inside


def test_fog_exp2_on_every_float_of_0_to_1(pkg):
    """p against binary64 2^f on every float of [0, 1], in chunks: the relative error stays below 1.2e-7 (8.2e-8 measured on a 37th of them,
    plus one fp32 rounding) and 1 <= p < 4, which the bit addition needs; fog_exp2(0) and fog_exp2(-0.0) are 1 by bits"""
    R = pkg.renderer
    one = int(np.array(1.0, F).view(np.uint32))
    worst, lo, hi = 0.0, np.inf, -np.inf
    chunk = 1 << 25
    for start in range(0, one + 1, chunk):
        f = np.arange(start, min(start + chunk, one + 1), dtype=np.uint32).view(F)
        p = R.fog_exp2_poly(f)
        ref = np.exp2(f.astype(np.float64))
        err = np.abs(p - ref)
        err /= ref
        worst, lo, hi = max(worst, float(err.max())), min(lo, float(p.min())), max(hi, float(p.max()))
    print(f"fog_exp2: the largest relative error of p on every float of [0, 1] is {worst:.3e}; p in [{lo!r}, {hi!r}]")
    assert worst <= 1.2e-7 and 1.0 <= lo and hi < 4.0
    some = np.concatenate([np.linspace(0.0, 1.0, 4097), [2.0 ** -24, 2.0 ** -30, 1.0 - 2.0 ** -24]]).astype(F)
    G.same(R.fog_exp2_poly(some), G.exp2_poly(some), "numpy's polynomial")
    for x in (0.0, -0.0):
        assert np.array(R.fog_exp2(x), F).view(np.uint32) == one and G.exp2(F(x)).view(np.uint32) == one
    xs = np.concatenate([-np.geomspace(1e-12, 200.0, 4000), [-126.0, -126.5, -1000.0, -np.inf, np.nan, -1.0, -2.0, -125.999]]).astype(F)
    got = np.array([R.fog_exp2(float(x)) for x in xs], F)
    G.same(got, G.exp2(xs), "fog_exp2")
    assert (got <= 1.0).all() and (got >= 2.0 ** -126).all()
    fine = xs >= -126.0
    rel = np.abs(got[fine] - np.exp2(xs[fine].astype(np.float64))) / np.exp2(xs[fine].astype(np.float64))
    assert rel.max() <= 1.2e-7 + 2.0 ** -24                                        # (the clamp to 1 moves a value by one rounding at most)


# ---- the physics, against float64 ------------------------------------------------------------------------------------------------------------------------
def rays64(view, width, height, z, max_distance):
    v = view[0]
    py, px = np.mgrid[0:height, 0:width]
    D = [(np.float64(v["ray00"][a]) + (px + 0.5) * np.float64(v["ray_dx"][a])) + (py + 0.5) * np.float64(v["ray_dy"][a]) for a in range(3)]
    ln = np.sqrt(D[0] ** 2 + D[1] ** 2 + D[2] ** 2)
    z_end = np.minimum(G.view_distance(z, v["z_near"], v["z_far"]).astype(np.float64), max_distance)
    return D, ln, z_end


def test_lit_everywhere_matches_the_closed_forms(pkg):
    """S = 0: T = e^(-sigma len z_end) within 1e-4 relative while T > 1e-3, and I = 1 - T within 1e-4 relative wherever the definition's own
    arithmetic lets that bar hold, and within 3.3e-5 absolute everywhere under the guard.  The figures are derived, per step count N: N
    multiplications by an `a` whose relative error is at most 1.2e-7 + 2^-24 move T by at most N * 1.8e-7; the sum's rounding adds at most
    N * 2^-24, an ABSOLUTE figure (every term and partial sum is below 1); the rounding of x itself (three operations) moves a^N by 3 * 2^-24
    * tau relative, 1.3e-6 at tau = 6.9.  So |I - (1 - T)| <= b(N) = N * (1.8e-7 + 2^-24) + 1.3e-6 absolute: 3.3e-5 at N = 128, 9.0e-6 at
    32, 3.0e-6 at 7, 1.5e-6 at 1 -- and 1e-4 RELATIVE is held wherever 1 - T >= b(N) / 1e-4, that is 0.33, 0.09, 0.03 and 0.015.  Nearer to
    T = 1 no evaluation of this definition can hold it: a T_k next to 1 is known to 2^-24 only, per step (measured: an I of 0.054 is 2.0e-4
    off at 128 steps, 1.1e-5 absolute)"""
    width, height = SIZES[2]
    _, z = planes(width, height)
    z = np.where(np.isfinite(z), np.clip(z, 0.0, 1.0), 1.0).astype(F)
    C = np.ones((height, width, 3), F)
    view = G.view_record()
    worst, worst_abs, judged_large = 0.0, 0.0, 0
    for density in (0.01, 0.12, 0.8):
        for steps in STEPS:
            kw = dict(RECORD, density=density, steps=steps)
            _, T, I = arbiter(pkg, C, z, None, view, **kw)
            _, ln, z_end = rays64(view, width, height, z, kw["max_distance"])
            want = np.exp(-np.float64(F(density)) * ln * z_end)
            judged = want > 1e-3
            assert judged.any()
            eT = (np.abs(T - want) / want)[judged].max()
            aI = np.abs(I - (1.0 - want))[judged].max()
            bound = steps * (1.8e-7 + 2.0 ** -24) + 1.3e-6                          # b(N)
            large = judged & (1.0 - want >= bound / 1e-4)
            eI = (np.abs(I - (1.0 - want)) / (1.0 - want))[large].max() if large.any() else 0.0
            worst, worst_abs, judged_large = max(worst, eT, eI), max(worst_abs, aI), judged_large + int(large.sum())
            assert eT <= 1e-4 and eI <= 1e-4 and aI <= bound, (density, steps, eT, eI, aI, bound)
    print(f"lit everywhere: the largest relative error of T, and of I where 1 - T >= b(N) / 1e-4, is {worst:.3e}; the largest absolute error of I {worst_abs:.3e}")
    assert judged_large >= 1000


def test_one_depth_step_and_a_striped_map(pkg):
    """a map that is one depth step, so that the visibility flips once along each ray at a known z: I differs from the float64 integral by at
    most the largest single term, 1 - a (a bound, not a measurement), plus the 3.3e-5 the fp32 evaluation of I is bounded by; and on a striped map the error
    against a 4096-step float64 march is smaller at 64 steps than at 8"""
    width, height = 32, 24
    view = G.view_record(eye=(0.0, 8.0, 0.0), ray00=(-0.32, 0.12, 1.0), ray_dx=(0.02, 0.0, 0.0), ray_dy=(0.0, -0.02, 0.0),
                         light=((0.02, 0.0, 0.0, 0.5), (0.0, 0.0, 0.02, 0.1), (0.0, -0.05, 0.0, 0.5)))
    v = view[0]
    C = np.zeros((height, width, 3), F)
    z = np.full((height, width), 0.97, F)
    D, ln, z_end = rays64(view, width, height, z, 40.0)
    sigma = np.float64(F(0.06))
    # the sun shines straight down; the map holds the depth w0 everywhere: a point is lit while w - bias <= w0, w = 0.5 - 0.05 y: lit above y0
    w0 = 0.2
    m = np.full((64, 64), w0, F)
    y0 = (0.5 - np.float64(F(w0))) / 0.05                                        # bias 0
    for steps in (8, 32, 128):
        kw = dict(density=0.06, anisotropy=0.0, max_distance=40.0, steps=steps, bias=0.0, scatter_color=(1.0, 1.0, 1.0), ambient_color=(0.0, 0.0, 0.0))
        _, T, I = arbiter(pkg, C, z, m, view, **kw)
        # along the ray y = eye.y + D.y z: lit where y >= y0.  D.y < 0 below the horizon: lit for z <= z_flip; D.y >= 0: lit everywhere
        with np.errstate(all="ignore"):
            z_flip = np.where(D[1] < 0, (y0 - np.float64(v["eye"][1])) / D[1], np.inf)
        z_lit = np.clip(z_flip, 0.0, z_end)
        want = 1.0 - np.exp(-sigma * ln * z_lit)                                 # the float64 integral of sigma len T over the lit part
        largest_term = 1.0 - np.exp(-sigma * ln * z_end / steps)
        diff = np.abs(I - want)
        assert (z_lit < z_end).mean() >= 0.25 and (z_lit == z_end).mean() >= 0.1  # rays that flip, and rays that never do
        assert (diff <= largest_term + 3.3e-5).all(), (steps, float((diff - largest_term).max()))   # (the fp32 error of I: the bound derived above)
    # stripes across v (world z): lit and shadowed slabs alternate along every ray
    stripes = np.where((np.arange(64) // 5) % 2 == 0, 1.0, 0.0).astype(F)[:, None].repeat(64, 1)

    def march(steps):
        kw = dict(density=0.06, anisotropy=0.0, max_distance=40.0, steps=steps, bias=0.0, scatter_color=(1.0, 1.0, 1.0), ambient_color=(0.0, 0.0, 0.0))
        return arbiter(pkg, C, z, stripes, view, **kw)[2].astype(np.float64)
    n = 4096
    k = (np.arange(n) + 0.5) / n
    zs = z_end[..., None] * k
    Pz = np.float64(v["eye"][2]) + D[2][..., None] * zs
    Px = np.float64(v["eye"][0]) + D[0][..., None] * zs
    Py = np.float64(v["eye"][1]) + D[1][..., None] * zs
    tu, tv, w = np.floor((0.02 * Px + 0.5) * 64), np.floor((np.float64(F(0.02)) * Pz + np.float64(F(0.1))) * 64), 0.5 - 0.05 * Py
    inside = (tu >= 0) & (tu <= 63) & (tv >= 0) & (tv <= 63) & ~(w > 1.0)
    lit = ~(inside & (w > stripes[np.clip(tv, 0, 63).astype(int), np.clip(tu, 0, 63).astype(int)]))
    tau = sigma * ln[..., None] * z_end[..., None]
    want = (lit * (np.exp(-tau * (np.arange(n) / n)) - np.exp(-tau * ((np.arange(n) + 1) / n)))).sum(-1)
    e8, e64, e128 = (np.abs(march(n) - want).mean() for n in (8, 64, 128))
    print(f"striped map: mean |I - I_4096| is {e8:.3e} at 8 steps, {e64:.3e} at 64 and {e128:.3e} at 128")
    assert (lit.mean(-1) < 0.9).mean() >= 0.5 and e64 < e8


# ---- arctic_fog_view --------------------------------------------------------------------------------------------------------------------------------------
def test_fog_view_against_the_matrices(pkg):
    """eye + D * zv projects to the pixel's centre within 1e-3 pixel and to `depth` within 1e-5 under the camera's matrix, and the light rows
    give the texel of the forward shader's shadow coordinates: uv = clip.xy * 0.5 + 0.5, v flipped, depth clip.z.  Points whose float64
    coordinate lies within 1e-3 texel of a texel's edge are left out: their share is stated and stays under 1 %"""
    import ao_scenes
    R = pkg.renderer
    width, height = 136, 72
    sc = ao_scenes.raster_scene(pkg)
    desc = pkg.scenes.SceneDesc(camera=dict(sc.desc.camera, aspect=width / height), ambient=0.1, sun=sc.desc.sun, objects=sc.desc.objects)
    pv, lpv, sd = (np.asarray(a, np.float64) for a in R.frame_constants(desc))
    view = R.fog_view(desc, width, height)
    v = view[0]
    zn, zf = (float(x) for x in desc.camera["z_near_far"])
    assert v["z_near"] == F(zn) and v["z_far"] == F(zf) and (v["eye"] == np.asarray(desc.camera["eye"], F)).all() and v["pad0"] == v["pad1"] == v["pad2"] == 0.0
    assert np.abs(v["sun_dir"].astype(np.float64) - sd / np.linalg.norm(sd)).max() <= 1e-6 and abs(np.linalg.norm(v["sun_dir"].astype(np.float64)) - 1.0) <= 1e-6
    rng = np.random.default_rng(4400)
    depth = rng.uniform(0.5, 0.9999, (height, width)).astype(F)
    zv = G.view_distance(depth, zn, zf).astype(np.float64)
    D, _, _ = rays64(view, width, height, depth, np.inf)
    P = np.stack([np.float64(v["eye"][a]) + D[a] * zv for a in range(3)] + [np.ones((height, width))], -1)
    clip = P @ pv                                                                 # pv is [col][row]: clip_r = sum_c P_c pv[c][r]
    ndc = clip[..., :3] / clip[..., 3:]
    py, px = np.mgrid[0:height, 0:width]
    ex = np.abs((ndc[..., 0] * 0.5 + 0.5) * width - (px + 0.5)).max()
    ey = np.abs((0.5 - 0.5 * ndc[..., 1]) * height - (py + 0.5)).max()
    ez = np.abs(ndc[..., 2] - depth).max()
    print(f"fog_view: the pixel's centre within {max(ex, ey):.2e} pixel, the depth within {ez:.2e}")
    assert ex <= 1e-3 and ey <= 1e-3 and ez <= 1e-5
    # the light rows on random world points, in fp32 as the kernel evaluates them, against float64 shadow coordinates
    S = 64
    pts = rng.uniform(-14.0, 14.0, (20000, 3))
    Pf = [pts[:, a].astype(F) for a in range(3)]
    P64 = [p.astype(np.float64) for p in Pf]
    lc = np.stack(P64 + [np.ones(len(pts))], -1) @ lpv
    u64, v64, w64 = lc[:, 0] * 0.5 + 0.5, 1.0 - (lc[:, 1] * 0.5 + 0.5), lc[:, 2]
    u, t, w = (G.row(v["light"][k], Pf) for k in range(3))
    near_edge = (np.abs(u64 * S - np.round(u64 * S)) < 1e-3) | (np.abs(v64 * S - np.round(v64 * S)) < 1e-3)
    share = near_edge.mean()
    print(f"fog_view: {share:.4f} of the points lie within 1e-3 texel of an edge and are left out")
    assert share < 0.01
    keep = ~near_edge
    assert (np.floor(u * F(S)) == np.floor(u64 * S))[keep].all() and (np.floor(t * F(S)) == np.floor(v64 * S))[keep].all()
    assert np.abs(w - w64).max() <= 1e-5 and ((u64 > 0) & (u64 < 1) & (v64 > 0) & (v64 < 1)).mean() >= 0.3
    with pytest.raises(R.ArcticError):
        R.fog_view(desc, 0, height)
    with pytest.raises(R.ArcticError):
        R.fog_view(desc, width, 16385)
