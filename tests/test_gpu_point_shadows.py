"""Shadow-casting point lights on the device (arctic_update_point_shadow_lights, kernels k_cubelit / k_cubelit_vis, the cube faces drawn by
the shadow pass's rasteriser): an unoccluded light adds the bits of a point light, injected faces against a float64 evaluation of the
documented lookup, drawn faces against the geometry, umbra and clear pixels in whole frames, stale scratch and culling, every path, shard
and option agreeing bit for bit, frames in flight, and the list's bookkeeping."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's standing bar on float LDR
W, H, S = 96, 64, 64
EPS = 1e-5   # distance to a compare or face-selection decision below which a pixel is not judged
DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
S_ROWS = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
U_ROWS = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)


def _cubes(pkg, positions, colors, z_near=0.05, z_far=40.0):
    a = np.zeros(len(positions), pkg.scene.POINT_SHADOW_LIGHT_DTYPE)
    if len(positions):
        a["position"], a["color"], a["z_near"], a["z_far"] = positions, colors, z_near, z_far
    return a


def _gbuffer_handle(hip, sc, attrs, mat, shadow, max_lights=16, F=32):
    r = hip.Renderer(W, H, S, max_lights)
    for d, n, m in sc.materials:
        r.create_material(d, n, m)
    r.write_gbuffer(attrs, mat)
    r.write_shadow_map(shadow)
    r.set_option("keep_float_output", 1)
    r.set_option("point_shadow_size", F)
    return r


def _random_inputs(pkg, sc, seed):
    rng = np.random.default_rng(seed)
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, len(sc.materials), coverage=0.9)
    shadow = rng.random((S, S), dtype=np.float32) * 0.6 + 0.3
    return rng, attrs, mat, shadow


def _frame_handle(hip, sc, cubes=None, F=128, **kw):
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    r.set_option("point_shadow_size", F)
    if cubes is not None:
        r.update_point_shadow_lights(cubes)
    return r


def visibility64(faces, world, p, zn, zf):
    """the documented lookup in float64: v per pixel, and whether the pixel is farther than EPS from every decision"""
    F = faces.shape[-1]
    d = world - p
    ad = np.abs(d)
    m = ad.max(-1)
    axis = np.where((ad[..., 0] >= ad[..., 1]) & (ad[..., 0] >= ad[..., 2]), 0, np.where(ad[..., 1] >= ad[..., 2], 1, 2))
    sign = np.take_along_axis(d, axis[..., None], -1)[..., 0] >= 0
    face = 2 * axis + np.where(sign, 0, 1)
    srt = np.sort(ad, -1)
    ok = (srt[..., 2] - srt[..., 1]) > EPS * np.maximum(m, 1.0)
    mm = np.where(m > 0, m, 1.0)
    sd = (S_ROWS[face] * d).sum(-1) / mm
    ud = (U_ROWS[face] * d).sum(-1) / mm
    A = float(np.float32(zf / (zf - zn)))
    pz = A * (1 - zn / mm)
    x, y = (0.5 + 0.5 * sd) * F - 0.5, (0.5 - 0.5 * ud) * F - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    c0, c1 = np.clip(x0, 0, F - 1).astype(int), np.clip(x0 + 1, 0, F - 1).astype(int)
    r0, r1 = np.clip(y0, 0, F - 1).astype(int), np.clip(y0 + 1, 0, F - 1).astype(int)
    t = [faces[face, r, c].astype(np.float64) for r, c in ((r0, c0), (r0, c1), (r1, c0), (r1, c1))]
    s = [(pz > ti).astype(np.float64) for ti in t]
    for ti in t:
        ok &= np.abs(pz - ti) > EPS
    sh = (s[0] + (s[1] - s[0]) * fx) + ((s[2] + (s[3] - s[2]) * fx) - (s[0] + (s[1] - s[0]) * fx)) * fy
    v = 1 - sh
    outside = (m <= zn) | (pz > 1)
    ok &= (np.abs(m - zn) > EPS) & (np.abs(pz - 1) > EPS)
    return np.where(outside, 1.0, v), ok


def test_unoccluded_light_equals_point_light_bit_for_bit(pkg, hip):
    """faces at 1.0: k shadow-casting lights add the bits of the same k lights appended to the point list (scalar light loop), over a
    random G-buffer and sun map with culling on and off; and whole frames of config 3 with z_far nearer than any geometry"""
    sc = pkg.scenes.config3(scale=0.1)
    rng, attrs, mat, shadow = _random_inputs(pkg, sc, 31)
    base = sc.lights[:3]
    for k in (1, 5, 12):
        pts = pkg.scenes.random_lights(rng, k, (-15, 0, -7), (15, 12, 7))
        a = _gbuffer_handle(hip, sc, attrs, mat, shadow)
        b = _gbuffer_handle(hip, sc, attrs, mat, shadow)
        for r in (a, b):
            r.set_option("light_path", 1)
        a.update_lights(np.concatenate([base, pts]))
        b.update_lights(base)
        b.update_point_shadow_lights(_cubes(pkg, pts["position"], pts["color"]))
        for culling in (1, 0):
            a.set_option("culling", culling); b.set_option("culling", culling)
            a.pass_shade(sc.desc, sc.settings); b.pass_shade(sc.desc, sc.settings)
            oa, ob = a.read_output(), b.read_output()
            for x, y in zip(oa, ob):
                np.testing.assert_array_equal(x, y)
            assert oa[1].max() > 0
        a.close(); b.close()
    pts = sc.lights[8:12]
    a = _frame_handle(hip, sc)
    b = _frame_handle(hip, sc, _cubes(pkg, pts["position"], pts["color"], z_near=1e-3, z_far=2e-3))
    for r in (a, b):
        r.set_option("light_path", 1); r.set_option("keep_float_output", 1)
    a.update_lights(sc.lights[:12])
    b.update_lights(sc.lights[:8])
    np.testing.assert_array_equal(a.render_frame(sc.desc, sc.settings), b.render_frame(sc.desc, sc.settings))
    for x, y in zip(a.read_output(), b.read_output()):
        np.testing.assert_array_equal(x, y)
    a.close(); b.close()


def test_injected_faces_against_float64(pkg, hip, oracle):
    sc = pkg.scenes.config3(scale=0.1)
    rng, attrs, mat, shadow = _random_inputs(pkg, sc, 32)
    shadow[:] = 1.0                                        # the sun's map lights every pixel: the cube term is seen everywhere
    F, n = 32, 3
    pos = rng.uniform((-8, 3, -3), (8, 9, 3), (n, 3)).astype(np.float32)
    cols = rng.uniform(10, 40, (n, 3)).astype(np.float32)
    cubes = _cubes(pkg, pos, cols, z_near=0.1, z_far=40.0)
    r = _gbuffer_handle(hip, sc, attrs, mat, shadow, F=F)
    r.update_lights(sc.lights[:0])
    r.update_point_shadow_lights(cubes)
    faces = []
    for i in range(n):   # blocks of 4 x 4 texels at depths around the pixels' pz: umbra, penumbra and light
        blocks = rng.uniform(0.975, 1.0, (6, F // 4, F // 4)).astype(np.float32)
        f = np.repeat(np.repeat(blocks, 4, 1), 4, 2)
        faces.append(np.ascontiguousarray(f))
        r.write_point_shadow(i, f)
        np.testing.assert_array_equal(r.read_point_shadow(i), f)
    desc = copy.deepcopy(sc.desc)
    r.pass_shade(desc, sc.settings)
    ldr, hdr, _ = r.read_output()
    world = r.read_gbuffer(want=("attrs",))[0][..., 11:14].astype(np.float64)
    o = _gbuffer_handle(hip, sc, attrs, mat, shadow, F=F)
    o.update_lights(sc.lights[:0])
    o.pass_shade(desc, sc.settings)
    base_hdr = o.read_output(want=("hdr",))[1]
    want = base_hdr.astype(np.float64)
    dark = copy.deepcopy(desc)
    dark.ambient = 0.0
    dark.sun = dict(dark.sun, color=(0.0, 0.0, 0.0))
    ok = mat != 0xFFFFFFFF
    vs = []
    for i in range(n):
        v, good = visibility64(faces[i], world, pos[i].astype(np.float64), 0.1, 40.0)
        ok &= good
        vs.append(v)
        o.update_lights(pkg.scene.make_lights(pos[i:i + 1], cols[i:i + 1]))
        o.pass_shade(dark, sc.settings)
        want += o.read_output(want=("hdr",))[1].astype(np.float64) * v[..., None]
    covered = mat != 0xFFFFFFFF
    assert ok.sum() > 0.9 * covered.sum(), ok.sum() / covered.sum()
    allv = np.concatenate([v[ok] for v in vs])
    assert (allv == 0).any() and (allv == 1).any() and ((allv > 0) & (allv < 1)).any()
    ys, xs = np.nonzero(ok)
    tm, gamma, exposure = sc.settings
    exp = np.array([oracle.tonemap(tm, gamma, exposure, want[y, x])[1] for y, x in zip(ys, xs)])
    err = np.abs(ldr[ys, xs] - exp)
    assert err.max() <= TOL, err.max()
    rel = np.abs(hdr[ys, xs] - want[ys, xs]) / (np.abs(want[ys, xs]) + 1e-3)
    assert rel.max() <= 1e-4, rel.max()
    r.close(); o.close()


def _quad_scene(pkg, quads):
    """meshes of the given quads (origin, eu, ev), one object each, identity transforms"""
    white, normal, mr = pkg.scenes.fallback_textures()
    meshes = [pkg.scenes.quad(o, eu, ev, 8, 8) + (0,) for o, eu, ev in quads]
    objs = pkg.scene.make_objects([(np.eye(4, dtype=np.float32), i) for i in range(len(meshes))])
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0, 0, 5), rotation=(0, -90), aspect=1.5, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.1, sun=dict(position=(0, 10, 0), rotation=(-60, 0), color=(0, 0, 0)), objects=objs)
    return [(white, normal, mr)], meshes, desc


def _upload(r, materials, meshes):
    for d, n, m in materials:
        r.create_material(d, n, m)
    for v, i, mat in meshes:
        r.create_mesh(v, i, mat)
    return r


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_raster_against_geometry(pkg, hip):
    F, zn, zf = 64, 0.1, 20.0
    P = np.array([0.25, 0.5, -0.25])
    # a wall at x = P.x + 3 (its back to the light: drawn), a tilted quad on the +Z side, and a floor facing the light (culled)
    wall = ((P[0] + 3, P[1] - 2, P[2] + 2), (0, 0, -4), (0, 4, 0))         # normal (0,0,-4) x (0,4,0) = +x: away from the light
    tilt_o = np.array([P[0] - 1.5, P[1] - 1.5, P[2] + 2 - 0.75])
    tilt = (tuple(tilt_o), (3.0, 0.0, 1.5), (0.0, 3.0, 0.0))                 # z - P.z = 2 + 0.5 (x - P.x); normal (-4.5, 0, 9): away
    floor_up = ((P[0] - 2, P[1] - 2, P[2] + 2), (4, 0, 0), (0, 0, -4))      # normal +y: facing the light (a front face: culled)
    floor_down = ((P[0] - 2, P[1] - 2, P[2] - 2), (4, 0, 0), (0, 0, 4))     # the same quad turned around
    planes = {0: (np.array([1.0, 0, 0]), P[0] + 3, wall), 4: (np.array([-0.5, 0, 1.0]), -0.5 * tilt_o[0] + tilt_o[2], tilt)}
    A = float(np.float32(zf / (zf - zn)))
    light = _cubes(pkg, [P], [(10, 10, 10)], zn, zf)

    def faces_of(quads):
        mats, meshes, desc = _quad_scene(pkg, quads)
        r = _upload(hip.Renderer(W, H, S, 16), mats, meshes)
        r.set_option("point_shadow_size", F)
        r.update_point_shadow_lights(light)
        r.pass_point_shadows(desc)
        f = r.read_point_shadow(0)
        r.close()
        return f

    def inside(q, w):
        o, eu, ev = (np.asarray(a, np.float64) for a in q)
        rel = w - o
        a = rel @ eu / (eu @ eu)
        b = rel @ ev / (ev @ ev)
        return (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1)

    faces = faces_of([wall, tilt, floor_up])
    ii, jj = np.meshgrid(np.arange(F), np.arange(F))
    judged = 0
    for k in range(6):
        hit_all, miss_all, depth = np.ones((F, F), bool), np.ones((F, F), bool), None
        for di, dj in ((0, 0), (1.5, 1.5), (-1.5, 1.5), (1.5, -1.5), (-1.5, -1.5)):   # (rays parallel to a plane give inf / nan: no hit)
            a = 2 * (ii + 0.5 + di) / F - 1
            b = 1 - 2 * (jj + 0.5 + dj) / F
            ray = DIRS[k] + a[..., None] * S_ROWS[k] + b[..., None] * U_ROWS[k]
            hit_any = np.zeros((F, F), bool)
            for kk, (n_, c_, q) in planes.items():
                t = (c_ - P @ n_) / (ray @ n_)
                w = P + t[..., None] * ray
                h = (t > 0) & inside(q, w)
                hit_any |= h
                if kk == k:
                    hit_all &= h
                    if di == 0:
                        depth = A * (1 - zn / t)
                else:
                    hit_all &= ~h
            miss_all &= ~hit_any
        if k in planes:
            judged += hit_all.sum()
            assert hit_all.sum() > 50
            np.testing.assert_allclose(faces[k][hit_all], depth[hit_all], rtol=0, atol=2e-6)
        else:
            hit_all[:] = False
        assert (faces[k][miss_all] == 1.0).all(), k
    assert judged > 1000
    # (the floor faces the light: a front face, culled -- the texels that see only it are among miss_all, asserted 1.0 above)
    turned = faces_of([floor_down])
    assert (turned[3] < 1.0).mean() > 0.5                   # turned around it casts
    np.testing.assert_allclose(turned[3][F // 2, F // 2], A * (1 - zn / 2.0), atol=2e-6)


def _floor_box_scene(pkg, n_grid=8):
    white, normal, mr = pkg.scenes.fallback_textures()
    floor = pkg.scenes.quad((-6, 0, 6), (12, 0, 0), (0, 0, -12), 24, 24) + (0,)
    box = pkg.scenes.box(1.0, 1.0, 1.0, n=n_grid) + (0,)
    objs = pkg.scene.make_objects([(np.eye(4, dtype=np.float32), 0), (pkg.scene.translation(0.0, 1.0, 0.0), 1)])
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0, 7, 7), rotation=(-45, -90), aspect=256 / 192, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.05, sun=dict(position=(0, 10, 0), rotation=(-60, 0), color=(0, 0, 0)), objects=objs)
    return [(white, normal, mr)], [floor, box], desc


def _segment_hits_box(w, p, lo, hi):
    """does the segment w -> p meet the box [lo, hi]?  (slab test, per pixel)"""
    d = p - w
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - w) / d, (hi - w) / d
    tmin = np.nanmax(np.minimum(t0, t1), -1)
    tmax = np.nanmin(np.maximum(t0, t1), -1)
    return (tmax >= np.maximum(tmin, 0)) & (tmin <= 1)


def test_umbra_and_clear_in_whole_frames(pkg, hip):
    mats, meshes, desc = _floor_box_scene(pkg)
    P = np.array([0.3, 3.2, -0.2], np.float32)
    col = np.array([[20, 18, 15]], np.float32)

    def frame(kind):
        r = _upload(hip.Renderer(256, 192, 0, 16), mats, meshes)
        r.set_option("point_shadow_size", 256)
        if kind == "cube":
            r.update_point_shadow_lights(_cubes(pkg, [P], col, 0.05, 20.0))
        elif kind == "point":
            r.update_lights(pkg.scene.make_lights([P], col))
        f = r.render_frame(desc, (2, 2.2, 1.0))
        world = r.read_gbuffer(want=("attrs",))[0][..., 11:14].astype(np.float64) if kind == "cube" else None
        mat = r.read_gbuffer(want=("material",))[0] if kind == "cube" else None
        r.close()
        return f, world, mat

    fc, world, mat = frame("cube")
    fn, _, _ = frame("none")
    fp, _, _ = frame("point")
    covered = mat != 0xFFFFFFFF
    margin = 0.1   # > 3 texels of a 256^2 face at the box's distance
    lo, hi = np.array([-0.5, 0.5, -0.5]), np.array([0.5, 1.5, 0.5])
    umbra = covered & _segment_hits_box(world, P.astype(np.float64), lo + margin, hi - margin)
    clear = covered & ~_segment_hits_box(world, P.astype(np.float64), lo - margin, hi + margin)
    assert umbra.sum() > 100 and clear.sum() > 2000, (umbra.sum(), clear.sum())
    np.testing.assert_array_equal(fc[umbra], fn[umbra])
    np.testing.assert_array_equal(fc[clear], fp[clear])
    assert not np.array_equal(fn[clear], fp[clear])


def test_stale_scratch_and_culling(pkg, hip):
    """meshes of more than 256 vertices and triangles: faces drawn for A, then B, then A again equal the first; culling 0, 1, 3 agree"""
    white, normal, mr = pkg.scenes.fallback_textures()
    box = pkg.scenes.box(1.0, 1.0, 1.0, n=16) + (0,)
    assert len(box[0]) > 256 and len(box[1]) // 3 > 256
    items = [(pkg.scene.translation(x, y, z), 0) for x, y, z in ((2, 0, 0), (-2, 0.5, 0), (0, 2, 0.3), (0, -2, 0), (0.4, 0, 2), (0, 0.2, -2.5),
                                                                (3, 3, 3), (-3, -1, 2))]
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0, 0, 8), rotation=(0, -90), aspect=1.5, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.1, sun=dict(position=(0, 10, 0), rotation=(-60, 0), color=(1, 1, 1)), objects=pkg.scene.make_objects(items))
    A = _cubes(pkg, [(0.1, 0.2, 0.05)], [(5, 5, 5)], 0.05, 30.0)
    B = _cubes(pkg, [(1.5, -1.0, 1.2)], [(5, 5, 5)], 0.05, 30.0)
    r = _upload(hip.Renderer(W, H, S, 16), [(white, normal, mr)], [box])
    r.set_option("point_shadow_size", 128)
    got = []
    for l in (A, B, A):
        r.update_point_shadow_lights(l)
        r.pass_point_shadows(desc)
        got.append(r.read_point_shadow(0))
    np.testing.assert_array_equal(got[0], got[2])
    assert not np.array_equal(got[0], got[1])
    assert (got[0] < 1).any()
    for cc in (0, 1):
        r.set_option("cluster_cull", cc)
        r.pass_point_shadows(desc)
        np.testing.assert_array_equal(r.read_point_shadow(0), got[0])
    r.close()


@pytest.mark.parametrize("cfg,scale", [(3, 0.1)])
def test_paths_shards_and_options_agree_bit_for_bit(pkg, hip, cfg, scale):
    from arctic_renderer_amd import sharding as sh
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    cubes = pkg.scenes.point_shadow_lights(3, seed=cfg)
    r = _frame_handle(hip, sc, cubes)
    ref = r.render_frame(sc.desc, sc.settings)
    plain = _frame_handle(hip, sc)
    assert not np.array_equal(ref, plain.render_frame(sc.desc, sc.settings))   # the lights are seen
    plain.close()
    r.set_option("visbuffer", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], ref)
    r.set_option("visbuffer", 1)
    r.set_option("culling", 0)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.set_option("culling", 1)
    r.set_option("tile_order", 1)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref)
    r.set_option("tile_order", 0)
    # shards: a row range, interleaved bands over 2 and 3 handles
    cut = sc.height // 3 + 3
    rs = _frame_handle(hip, sc, cubes, row_begin=cut, row_end=sc.height)
    np.testing.assert_array_equal(rs.render_frame(sc.desc, sc.settings), ref[cut:])
    rs.close()
    for world in (2, 3):
        for i in range(world):
            rb = _frame_handle(hip, sc, cubes, band_rows=16, shard=(i, world))
            np.testing.assert_array_equal(rb.render_frame(sc.desc, sc.settings), ref[sh.owned_rows(sc.height, i, world, 16)])
            rb.close()
    r.close()
    # the face cache on and off, over frames where the light sometimes moves
    moved = cubes.copy()
    moved[0]["position"] = moved[0]["position"] + np.float32([1.5, -0.5, 0.75])
    seq = [cubes, cubes, moved, moved, cubes]
    frames = {}
    for cache in (1, 0):
        h = _frame_handle(hip, sc, cubes)
        h.set_option("shadow_cache", cache)
        out, prev = [], seq[0]
        for c in seq:
            if c is not prev:   # (a new list always redraws: only a changed one is handed over)
                h.update_point_shadow_lights(c)
            prev = c
            out.append(h.render_frame(sc.desc, sc.settings))
        frames[cache] = out
        h.close()
    for a, b in zip(frames[0], frames[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(frames[1][0], ref)
    assert not np.array_equal(frames[1][2], ref)
    np.testing.assert_array_equal(frames[1][4], ref)


def test_combines_linearly_with_spots_and_env(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    env = np.ones((32, 64, 4), np.float32)
    env[..., :3] = np.linspace(0.8, 1.2, 64, dtype=np.float32)[None, :, None] * np.float32([0.5, 0.6, 0.7])
    sc.environment = env
    spots = pkg.scenes.spot_lights(3, seed=5)
    cubes = pkg.scenes.point_shadow_lights(3, seed=9)
    hdr = {}
    for env_on in (0, 1):
        r = _frame_handle(hip, sc)
        r.set_option("keep_float_output", 1)
        r.set_option("env_lighting", env_on)
        r.update_spot_lights(spots)
        for k, c in ((0, cubes[:0]), (1, cubes)):
            r.update_point_shadow_lights(c)
            r.render_frame(sc.desc, sc.settings)
            hdr[env_on, k] = r.read_output(want=("hdr",))[1].astype(np.float64)
        r.close()
    d_env, d_plain = hdr[1, 1] - hdr[1, 0], hdr[0, 1] - hdr[0, 0]
    assert np.abs(d_plain).max() > 1e-3
    scale = np.maximum(np.abs(hdr[1, 1]), np.abs(hdr[0, 1])) + 1e-30
    assert (np.abs(d_env - d_plain) <= 4 * np.finfo(np.float32).eps * scale).all(), np.abs(d_env - d_plain).max()


def test_frames_in_flight_equal_fresh_frames(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    base = pkg.scenes.point_shadow_lights(2, seed=4)
    lists = []
    for f in range(6):
        c = base.copy()
        c[0]["position"] = c[0]["position"] + np.float32([0.4 * f, 0.0, -0.2 * f])
        lists.append(c)
    fresh = []
    for c in lists:
        h = _frame_handle(hip, sc, c)
        fresh.append(h.render_frame(sc.desc, sc.settings))
        h.close()
    for fif in (1, 2, 3):
        h = _frame_handle(hip, sc, lists[0])
        h.set_option("frames_in_flight", fif)
        for f, c in enumerate(lists):
            h.update_point_shadow_lights(c)
            np.testing.assert_array_equal(h.render_frame(sc.desc, sc.settings), fresh[f])
        h.close()


def test_bookkeeping(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    never = _frame_handle(hip, sc)
    ref0 = never.render_frame(sc.desc, sc.settings)
    never.close()
    cubes = pkg.scenes.point_shadow_lights(3, seed=1)
    r = _frame_handle(hip, sc, cubes)
    with_cubes = r.render_frame(sc.desc, sc.settings)
    assert not np.array_equal(with_cubes, ref0)
    # an invalid light: ARCTIC_E_INVALID, the previous list keeps rendering
    for field, value in (("z_near", 0.0), ("z_far", 0.01), ("color", (np.nan, 1, 1))):
        bad = cubes.copy()
        bad[1][field] = value
        with pytest.raises(hip.ArcticError) as e:
            r.update_point_shadow_lights(bad)
        assert e.value.code == -1
        np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), with_cubes)
    # statistics and the tile trace do not apply
    for opt in ("count_light_evals", "tile_trace"):
        r.set_option(opt, 1)
        with pytest.raises(hip.ArcticError) as e:
            r.render_frame(sc.desc, sc.settings)
        assert e.value.code == -4
        r.set_option(opt, 0)
    # a bad size or light index
    for size in (0, 4, 12, 4104, 8192):
        with pytest.raises(hip.ArcticError) as e:
            r.set_option("point_shadow_size", size)
        assert e.value.code == -1
    for i in (3, 100):
        with pytest.raises(hip.ArcticError) as e:
            r.read_point_shadow(i)
        assert e.value.code == -1
        with pytest.raises(hip.ArcticError) as e:
            r.write_point_shadow(i, np.ones((6, 128, 128), np.float32))
        assert e.value.code == -1
    # arctic_resize keeps the faces
    before = r.read_point_shadow(2)
    assert (before < 1).any()
    r.resize(sc.width // 2, sc.height // 2)
    np.testing.assert_array_equal(r.read_point_shadow(2), before)
    r.resize(sc.width, sc.height)
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), with_cubes)
    # cleared: the frame of a handle that never had the list, bit for bit
    r.update_point_shadow_lights(cubes[:0])
    np.testing.assert_array_equal(r.render_frame(sc.desc, sc.settings), ref0)
    r.close()
    # the cap: max_lights lights are kept, the rest dropped
    cap = 2
    many = pkg.scenes.point_shadow_lights(5, seed=2)
    a = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, cap))
    b = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, cap))
    for h in (a, b):
        h.update_lights(sc.lights[:cap])
        h.set_option("point_shadow_size", 128)
    a.update_point_shadow_lights(many)
    b.update_point_shadow_lights(many[:cap])
    np.testing.assert_array_equal(a.render_frame(sc.desc, sc.settings), b.render_frame(sc.desc, sc.settings))
    a.close(); b.close()
