"""tests/shading_reference.py pinned without a GPU: against the C++ oracle where the two overlap (no spot / cube lights, ENV and MIP off),
by hand for the new terms, and -- for the inputs of every injected case of tests/test_gpu_extended_shading.py -- that a list of deliberate
defects moves the judged pixels far beyond the GPU bar and that the mask leaves few pixels out."""
import numpy as np
import pytest

import shading_reference as SR
import test_gpu_extended_shading as G

W, H, S = 96, 64, 64
# The reference arbitrates the kernels at 1e-4 on float LDR; it may disagree with the oracle by a tenth of that at most.  Measured here: 1.0e-7 at
# most with constant materials (0 / 1 / 5 / 16 lights, the three tonemappers; relative HDR 7e-8), 3.1e-8 with config 2's textures and 1.6e-6 with
# config 3's (whose oracle side filters its 102-texel noise textures in fp32): the fp32 rounding of the oracle's inputs and output.
ORACLE_GATE = 1e-5
MOVED_BY, MOVED_SHARE, LEFT_OUT = 10 * G.TOL, 0.01, 0.10


def _constant(rgb, nrm, rough, metal):
    px = lambda *c: np.array([[list(c) + [255]]], np.uint8)
    return px(*rgb), px(*nrm), px(255, rough, metal)


def _oracle_ldr_hdr(oracle, images, attrs, mat, shadow, lights, desc, settings):
    o = oracle.Oracle(W, H, S, 16)
    for d, n, m in images:
        o.create_material(d, n, m)
    o.update_lights(lights)
    o.write_shadow_map(shadow)
    out = o.shade_gbuffer(desc, settings, attrs, mat, want=("ldr", "hdr"))
    o.close()
    return out["ldr"].astype(np.float64), out["hdr"].astype(np.float64)


def _scene_bits(pkg, rng, n_materials):
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, n_materials, coverage=0.9)
    shadow = rng.random((S, S), dtype=np.float32) * 0.6 + 0.3
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0.0, 5.0, 0.0), rotation=(-15.0, 0.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 1000.0)),
                               ambient=0.1, sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([]))
    return attrs, mat, shadow, desc


def _distance(ref, ldr, hdr):
    cov = ref["covered"]
    return np.abs(ref["ldr"] - ldr)[cov].max(), (np.abs(ref["hdr"] - hdr) / (np.abs(ref["hdr"]) + 1e-3))[cov].max()


def test_reference_matches_oracle_constant_materials(pkg, oracle):
    """two separate float64 evaluations of ps_main + post_process: materials of constant 1 x 1 images, so filtering drops out"""
    rng = np.random.default_rng(41)
    mats = [_constant(rng.integers(20, 255, 3), (rng.integers(100, 156), rng.integers(100, 156), rng.integers(200, 256)), rough, 255 * (i % 2))
            for i, rough in enumerate((0, 26, 77, 128, 204, 255))]
    attrs, mat, shadow, desc = _scene_bits(pkg, rng, len(mats))
    lit = G.sun_lit(oracle, shadow, attrs, mat)
    cov = mat != SR.NO_MAT
    print(f"lit share {np.mean(lit[cov] == 1):.3f}, penumbra share {np.mean((lit[cov] > 0) & (lit[cov] < 1)):.4f}")
    assert (lit[cov] == 1).any() and (lit[cov] == 0).any() and ((lit[cov] > 0) & (lit[cov] < 1)).any()
    materials = G.host_materials(mats, mips=False)
    ch = SR.material_channels(materials, attrs, mat)
    worst = 0.0
    for n_lights in (0, 1, 5, 16):
        lights = pkg.scenes.random_lights(rng, n_lights, (-15, 0, -7), (15, 12, 7))
        for tm in (0, 1, 2):
            settings = (tm, 2.2, 1.0)
            ldr, hdr = _oracle_ldr_hdr(oracle, mats, attrs, mat, shadow, lights, desc, settings)
            ref = SR.shade(attrs, mat, ch, lit, desc.camera["eye"], desc.sun["rotation"], desc.sun["color"], desc.ambient, settings, points=lights)
            e_ldr, e_hdr = _distance(ref, ldr, hdr)
            print(f"reference - oracle, {n_lights} lights, tonemapper {tm}: ldr {e_ldr:.2e}, hdr relative {e_hdr:.2e}")
            assert ref["judged"].sum() == cov.sum()
            assert e_ldr <= ORACLE_GATE and e_hdr <= ORACLE_GATE, (n_lights, tm, e_ldr, e_hdr)
            worst = max(worst, e_ldr)
    print(f"reference - oracle, constant materials: largest ldr distance {worst:.2e}")


@pytest.mark.parametrize("cfg,scale", [(2, 0.25), (3, 0.1)])
def test_reference_matches_oracle_real_materials(pkg, oracle, cfg, scale):
    """the test-scale configs' own textures: the reference's bilinear channels against the oracle's fetch_surface, then the pixel"""
    rng = np.random.default_rng(42 + cfg)
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    attrs, mat, shadow, desc = _scene_bits(pkg, rng, len(sc.materials))
    lit = G.sun_lit(oracle, shadow, attrs, mat)
    cov = mat != SR.NO_MAT
    ch = SR.material_channels(G.host_materials(sc.materials, mips=False), attrs, mat)
    o = oracle.Oracle(W, H, S, 16)
    for d, n, m in sc.materials:
        o.create_material(d, n, m)
    surf = np.zeros(mat.shape + (8,))
    for y, x in zip(*np.nonzero(cov)):
        s = o.fetch_surface(int(mat[y, x]), attrs[y, x, 0], attrs[y, x, 1]).astype(np.float64)
        surf[y, x] = [s[0], s[1], s[2], (s[3] + 1) * 127.5, (1 - s[4]) * 127.5, (s[5] + 1) * 127.5, s[10], s[9]]
    o.close()
    d_ch = np.abs(ch - surf)[cov] / np.array([1, 1, 1, 255, 255, 255, 1, 1])
    print(f"config {cfg}: filtered channels, reference - oracle fetch_surface: {d_ch.max():.2e}")
    # fetch_surface filters in fp32: the scaled coordinate u W - 0.5 (below 128 here) carries up to two ulps of 128 = 1.5e-5 texels, and
    # neighbouring texels of the noise textures differ by up to the whole range
    assert d_ch.max() <= 2e-5
    lights = pkg.scenes.random_lights(rng, 5, (-15, 0, -7), (15, 12, 7))
    ldr, hdr = _oracle_ldr_hdr(oracle, sc.materials, attrs, mat, shadow, lights, desc, sc.settings)
    ref = SR.shade(attrs, mat, ch, lit, desc.camera["eye"], desc.sun["rotation"], desc.sun["color"], desc.ambient, sc.settings, points=lights)
    e_ldr, e_hdr = _distance(ref, ldr, hdr)
    print(f"reference - oracle, config {cfg}'s materials: ldr {e_ldr:.2e}, hdr relative {e_hdr:.2e}")
    assert e_ldr <= ORACLE_GATE and e_hdr <= ORACLE_GATE


# ---- known answers for the new terms, by hand ----------------------------------------------------------------------------------------
def _spot(pkg, position, direction, outer, inner, rng_, color=(10, 20, 30)):
    a = np.zeros(1, pkg.scene.SPOT_LIGHT_DTYPE)
    a["position"], a["direction"], a["color"], a["outer_cone_angle"], a["inner_cone_angle"], a["range"] = position, direction, color, outer, inner, rng_
    return a


def test_omnidirectional_spot_is_the_point_light(pkg, oracle):
    rng = np.random.default_rng(43)
    mats = [_constant((180, 90, 40), (120, 130, 250), 90, 0), _constant((60, 200, 220), (140, 120, 240), 200, 255)]
    attrs, mat, shadow, desc = _scene_bits(pkg, rng, len(mats))
    lit = G.sun_lit(oracle, shadow, attrs, mat)
    ch = SR.material_channels(G.host_materials(mats, False), attrs, mat)
    pts = pkg.scenes.random_lights(rng, 1, (-5, 2, -3), (5, 9, 3), intensity=40.0)
    omni = _spot(pkg, pts["position"][0], (0.3, -1.0, 0.2), np.float32(np.pi), 0.0, 0.0, pts["color"][0])
    args = (attrs, mat, ch, lit, desc.camera["eye"], desc.sun["rotation"], desc.sun["color"], desc.ambient, (2, 2.2, 1.0))
    a, b, none = SR.shade(*args, points=pts), SR.shade(*args, spots=omni), SR.shade(*args)
    np.testing.assert_array_equal(a["hdr"], b["hdr"])            # exactly, in float64
    assert np.abs(a["hdr"] - none["hdr"]).max() > 0.01


def test_cone_and_window_by_hand(pkg):
    outer, inner = 0.6, 0.3
    c = SR.spot_constants(_spot(pkg, (0, 0, 0), (2.0, 0, 0), outer, inner, 4.0))[0]
    np.testing.assert_allclose(c["s"], [1, 0, 0])
    assert c["ir2"] == 1 / 16 and abs(c["scale"] - 1 / (np.cos(inner) - np.cos(outer))) < 1e-6 and abs(c["offset"] + np.cos(outer) * c["scale"]) < 1e-6
    co, ci = np.cos(np.float64(np.float32(outer))), np.cos(np.float64(np.float32(inner)))
    mid = np.arccos((co + ci) / 2)
    world = np.array([[2.0, 0, 0],                                    # on the axis, half the range away: att 1, window 1 - (1/4)^2
                      [2 * np.cos(0.2), 2 * np.sin(0.2), 0],          # inside the inner cone
                      [2 * np.cos(0.7), 0, 2 * np.sin(0.7)],          # outside the outer cone
                      [2 * np.cos(mid), 2 * np.sin(mid), 0],          # halfway up the ramp: att 1/4
                      [4.0, 0, 0],                                    # at dist = range: window 0
                      [0, 0, 4.0]])
    f, _, d2, cd = SR.spot_factor(c, world)
    np.testing.assert_allclose(f[:4], [0.9375, 0.9375, 0.0, 0.25 * 0.9375], atol=2e-6)
    assert f[0] == 0.9375 and f[2] == 0 and f[4] == 0 and f[5] == 0
    # no range: the window is exactly 1; outer = pi: the cone factor is exactly 1 whatever the direction
    c = SR.spot_constants(_spot(pkg, (0, 0, 0), (1, 0, 0), outer, inner, 0.0))[0]
    assert c["ir2"] == 0 and SR.spot_factor(c, np.array([[100.0, 0, 0]]))[0][0] == 1
    c = SR.spot_constants(_spot(pkg, (0, 0, 0), (1, 0, 0), np.float32(np.pi), 0.1, 0.0))[0]
    assert (c["scale"], c["offset"]) == (0, 1) and (SR.spot_factor(c, np.array([[-3.0, 1, 2], [3, 0, 0]]))[0] == 1).all()
    # inner = outer: the clamped scale 1000, flagged as a hard cone
    c = SR.spot_constants(_spot(pkg, (0, 0, 0), (1, 0, 0), outer, outer, 0.0))[0]
    assert c["scale"] == 1000 and c["hard"]


# probe directions d = world - p, one per face, with the texel coordinates x = px F - 0.5, y = py F - 0.5 of an 8 x 8 face worked out by hand
# from the header's table (px = 0.5 + 0.5 (s.d) / m, py = 0.5 - 0.5 (u.d) / m):
FACE_PROBES = [((4, 1, 2), 0, 1.5, 4.5),     # +X: s = -z, u = -y: px = 0.5 - 2/8 = 0.25,  py = 0.5 + 1/8 = 0.625
               ((-4, 1, 2), 1, 5.5, 4.5),    # -X: s = +z, u = -y: px = 0.75,              py = 0.625
               ((1, 4, 2), 2, 4.5, 1.5),     # +Y: s = +x, u = +z: px = 0.5 + 1/8 = 0.625, py = 0.5 - 2/8 = 0.25
               ((1, -4, 2), 3, 4.5, 5.5),    # -Y: s = +x, u = -z: px = 0.625,             py = 0.75
               ((1, 2, 4), 4, 4.5, 5.5),     # +Z: s = +x, u = -y: px = 0.625,             py = 0.5 + 2/8 = 0.75
               ((1, 2, -4), 5, 2.5, 5.5)]    # -Z: s = -x, u = -y: px = 0.375,             py = 0.75


def test_cube_lookup_by_hand():
    Fh, zn, zf = 8, 1.0, 9.0
    p = np.array([0.5, -1.0, 2.0])
    for d, face, x, y in FACE_PROBES:
        d = np.asarray(d, np.float64)
        got = SR.cube_lookup(d[None], Fh, zn, zf)
        assert (int(got[0][0]), got[1][0], got[2][0]) == (face, x, y), (d, got[:3])
        assert got[3][0] == 9 / 8 * (1 - 1 / 4)                       # pz = zf / (zf - zn) (1 - zn / m), m = 4
        lo = np.zeros((6, Fh, Fh), np.float32)                       # everything casts, except the four texels the probe must read
        lo[face, int(y):int(y) + 2, int(x):int(x) + 2] = 1.0
        v, ok = SR.cube_visibility(lo, (p + d)[None], p, zn, zf)
        assert v[0] == 1 and ok[0], (face, v)
        v, _ = SR.cube_visibility(1 - lo, (p + d)[None], p, zn, zf)
        assert v[0] == 0, (face, v)
    # ties go to x, then y, then z
    assert [int(SR.cube_face(np.array([d], np.float64))[0][0]) for d in ((3, 3, 1), (3, 1, 3), (-3, 3, 3), (1, 3, 3), (1, -3, 3), (1, 2, 3))] == [0, 0, 1, 2, 3, 4]
    world = p + np.array([[0, 0, 4.0]])
    ones, zeros = np.ones((6, Fh, Fh), np.float32), np.zeros((6, Fh, Fh), np.float32)
    assert SR.cube_visibility(ones, world, p, zn, zf)[0][0] == 1 and SR.cube_visibility(zeros, world, p, zn, zf)[0][0] == 0
    # a face split down a texel column: x = 3.25 between a casting column 3 and a clear column 4 gives the bilinear fraction
    split = np.ones((6, Fh, Fh), np.float32)
    split[4, :, :4] = 0.0
    v, ok = SR.cube_visibility(split, p + np.array([[-0.25, 0.1, 4.0]]), p, zn, zf)   # px = 0.5 - 0.25/8 -> x = 3.75 - 0.5
    assert v[0] == 0.25 and ok[0]
    # inside the near plane and beyond the far plane: unshadowed, whatever the faces hold
    assert SR.cube_visibility(zeros, p + np.array([[0.2, 0.9, -0.3], [0, 10.0, 1.0]]), p, zn, zf)[0].tolist() == [1, 1]
    # a pixel within EPS of a compare, of a face change or of a plane is not judged
    pz = 9 / 8 * (1 - 1 / 4)
    near = np.full((6, Fh, Fh), np.float32(pz))
    assert not SR.cube_visibility(near, world, p, zn, zf)[1][0]
    assert not SR.cube_visibility(ones, p + np.array([[4.0, 4.0 + 1e-6, 1.0]]), p, zn, zf)[1][0]
    assert not SR.cube_visibility(ones, p + np.array([[0, 0, 1.0 + 1e-6]]), p, zn, zf)[1][0]


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_gpu_case_inputs_are_sensitive_and_mostly_judged(pkg, oracle, case):
    """for the inputs the GPU case injects: every deliberate defect of a term the case contains moves at least 1 % of the judged pixels by more
    than 10 x the GPU bar, and the mask leaves at most 10 % of the covered pixels out"""
    I = G.build_inputs(pkg, case)
    lit = G.sun_lit(oracle, I.shadow, I.attrs, I.mat)
    cov = I.mat != SR.NO_MAT
    if case.half_shadow:
        left = slice(0, case.width // 2)
        assert (lit[:, left][cov[:, left]] == 0).all() and (lit[:, case.width // 2:] == 1).mean() > 0.3
    # the edges every case carries: tiles of one material and tiles mixing all four, one of them with images of unequal sizes; a lambda plane with
    # exact integers, the longest chain's last level, values beyond it, negatives and a NaN; a cube light with pixels inside its near plane and others
    # beyond its far plane
    tiles = [set(I.mat[y:y + 8, x:x + 8].ravel().tolist()) - {SR.NO_MAT} for y in range(0, case.rows - 7, 8) for x in range(0, case.width - 7, 8)]
    assert any(len(t) == 1 for t in tiles) and any(len(t) == 4 for t in tiles)
    assert len({im.shape for im in I.images[2]}) == 3
    lam = I.lod[cov & ~np.isnan(I.lod)]
    assert (lam == 6).any() and (lam > 6).any() and (lam < 0).any() and ((lam == np.round(lam)) & (lam > 0) & (lam < 6)).any() and ((lam % 1) != 0).any()
    assert np.isnan(I.lod).sum() == 1
    m = np.abs(I.attrs[..., 11:14].astype(np.float64) - SR.f32(I.cubes[2]["position"])).max(-1)[cov]
    assert (m <= I.cubes[2]["z_near"]).mean() > 0.01 and (m > I.cubes[2]["z_far"]).mean() > 0.01, ((m <= 6).mean(), (m > 14).mean())
    materials = G.host_materials(I.images, "mip" in case.features)
    env = G.host_env_tables(I.env_map) if "env" in case.features else None
    truth = G.reference_for(case, I, lit, materials, env)
    left_out = 1 - truth["judged"].sum() / cov.sum()
    shares = G.sensitivity(case.features, case.n_points, truth, lambda m: G.reference_for(case, I, lit, materials, env, mutate=m))
    print(f"{case.name}: left out {left_out:.4f} ({ {k: int(v.sum()) for k, v in truth['reasons'].items()} }); moved by more than {MOVED_BY:g}: "
          + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert left_out <= LEFT_OUT, (case.name, left_out)
    for k, v in shares.items():
        assert v >= MOVED_SHARE, (case.name, k, v)
    # each feature of the case is seen at all: the GPU case asserts the same of the device, so it cannot pass by falling back
    for f in case.features:
        off = G.reference_for(case, I, lit, G.host_materials(I.images, "mip" in case.features - {f}), env, on=case.features - {f})
        assert np.abs(off["hdr"] - truth["hdr"])[truth["judged"]].max() > 1e-3, (case.name, f)


def test_every_launch_branch_and_mutation_is_covered():
    """the lattice takes each of the 8 kernel shapes with both loops, and every mutation is asked of some case"""
    shape = lambda fs: (next((f for f in ("mip", "cube", "spot") if f in fs), "material"), "env" in fs)   # launch_variant's order of tests
    assert len({(shape(c.features), c.light_path) for c in G.LATTICE}) == 16 and {c.light_path for c in G.LATTICE} == {1, 2}
    asked = set()
    for c in G.CASES:
        asked |= set(G.mutations_for(c.features, c.n_points))
    assert asked == set(SR.MUTATIONS)
