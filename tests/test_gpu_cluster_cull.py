"""ARCTIC_OPT_CLUSTER_CULL (round 5): the prepasses skip workgroups of 256 triangles / 256 vertices whose object-space box lies beyond a side
of the pass's scissor rectangle, the near or the far plane (needs an MI355X).

The reference draws every object and leaves the rest to the hardware's clipper and culler (src/renderer/forward_pass.cpp:212-224,
src/renderer/shadow_map_pass.cpp:157-167): there is one answer per pixel, so skipping must change nothing -- visibility plane, interpolated
attributes, shadow map, record and work-item counts, the frame shaded from the visibility plane (which reads the transformed vertices of every
surviving record: a vertex block skipped wrongly shows there) -- bit for bit, for cameras inside and outside the scene, shards, objects that
straddle the scissor's sides by fractions of a pixel, and meshes the host cannot bound.
"""
import copy

import numpy as np
import pytest

import cluster_cull_cases as CC

pytestmark = pytest.mark.gpu

COUNT = 1024     # ARCTIC_OPT_DEBUG bit 10: count what was skipped


def prepass(hip, sc, cull, desc=None, frame=True, jitter=None, **kw):
    """jitter: arctic_set_camera_jitter's (jx, jy) before anything is drawn; None: the call is never made"""
    desc = desc or sc.desc
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    r.set_option("cluster_cull", cull)
    if jitter is not None:
        r.set_camera_jitter(*jitter)
    r.set_option("debug", COUNT)
    if sc.shadow_size:
        r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    counts = [r.cull_counts(False).copy(), r.cull_counts(True).copy() if sc.shadow_size else np.zeros(4, np.uint32)]
    attrs, mat, depth, tri = r.read_gbuffer()
    out = [attrs.view(np.uint32).copy(), mat.copy(), depth.view(np.uint32).copy(), tri.copy(),
           r.read_shadow_map().view(np.uint32).copy() if sc.shadow_size else np.zeros(1, np.uint32), r.stats()[:4].copy()]
    if frame:
        out.append(r.render_frame(desc, sc.settings).copy())
        out.append(r.render_frame(desc, sc.settings).copy())     # (the second one with two frames in flight's other set of tables)
    r.close()
    return out, counts


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("cfg,scale", [(1, 0.5), (2, 0.25), (3, 0.2), (3, 0.5)])
def test_culling_changes_nothing(pkg, hip, cfg, scale):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    (off, c0), (setup_only, c1), (both, c3) = (prepass(hip, sc, m) for m in (0, 1, 3))
    assert (off[3] != 0xFFFFFFFF).mean() > 0.1
    same(off, setup_only)
    same(off, both)
    assert c0[0][1] == 0 and c0[0][3] == 0 and c1[0][3] == 0
    assert c1[0][1] == c3[0][1]
    print(f"config {cfg} x{scale}: forward pass skips {c3[0][1]} of {c3[0][0]} clusters and {c3[0][3]} of {c3[0][2]} vertex blocks, shadow pass {c3[1][1]} of {c3[1][0]} / {c3[1][3]} of {c3[1][2]}")
    if cfg == 3 and scale >= 0.5:      # not vacuous: the camera stands inside the atrium, most of it is behind it or beside the view
        assert c3[0][1] > 0.3 * c3[0][0] and c3[0][3] > 0.2 * c3[0][2]


def cameras(rng, n):
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:    # inside the hall, any direction
            eye = rng.uniform((-12, 0.5, -5), (12, 9, 5)); rot = (rng.uniform(-89, 89), rng.uniform(-180, 180))
        elif kind == 1:  # far outside, looking roughly at it (everything small, far plane close to mattering) or away from it (everything skipped)
            d = rng.normal(size=3); d /= np.linalg.norm(d); eye = d * rng.uniform(30, 400) + (0, 5, 0)
            yaw = np.degrees(np.arctan2(-d[0], -d[2])) + (180 if i % 8 == 1 else 0); rot = (rng.uniform(-30, 30), yaw)
        elif kind == 2:  # nose on a wall / the floor: the near plane cuts clusters, w <= 0 corners
            eye = (rng.uniform(-14, 14), rng.uniform(0.01, 0.3), rng.uniform(-6, 6)); rot = (rng.uniform(-60, 10), rng.uniform(-180, 180))
        else:            # straight up / down (degenerate yaw)
            eye = rng.uniform((-5, 1, -3), (5, 8, 3)); rot = (89.9 if i % 8 == 3 else -89.9, rng.uniform(-180, 180))
        out.append((tuple(float(x) for x in eye), tuple(float(x) for x in rot)))
    return out


def test_random_cameras(pkg, hip):
    sc = pkg.scenes.config3(scale=0.25)
    rng = np.random.default_rng(20251)
    skipped = []
    for k, (eye, rot) in enumerate(cameras(rng, 16)):
        desc = copy.deepcopy(sc.desc)
        desc.camera["eye"], desc.camera["rotation"] = eye, rot
        if k % 5 == 4:
            desc.camera["z_near_far"] = (0.5, 12.0)          # a far plane that cuts the hall
        if k % 3 == 2:
            desc.sun["rotation"] = (float(rng.uniform(-80, -20)), float(rng.uniform(-180, 180)))
        (a, _), (b, c) = prepass(hip, sc, 0, desc, frame=(k % 2 == 0)), prepass(hip, sc, 3, desc, frame=(k % 2 == 0))
        same(a, b)
        skipped.append(c[0][1] / c[0][0])
    print("fraction of the clusters skipped per camera:", " ".join(f"{x:.2f}" for x in skipped))
    assert max(skipped) > 0.5 and min(skipped) < max(skipped)


@pytest.mark.parametrize("kw", [dict(row_begin=0, row_end=48), dict(row_begin=96, row_end=160), dict(row_begin=263, row_end=264),
                                dict(band_rows=16, shard=(1, 3)), dict(band_rows=64, shard=(2, 4))], ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_shards(pkg, hip, kw):
    """a row-range shard's scissor is its rows: clusters above and below it go too; interleaved bands keep the whole frame's rectangle"""
    sc = pkg.scenes.config3(scale=0.25)
    (a, _), (b, c) = prepass(hip, sc, 0, **kw), prepass(hip, sc, 3, **kw)
    same(a, b)
    (_, whole) = prepass(hip, sc, 3, frame=False)
    if "row_begin" in kw:
        assert c[0][1] >= whole[0][1]
    else:
        assert c[0][1] == whole[0][1]


SWEEP_W, SWEEP_H = 256, 144
SWEEP_CAMERA = dict(eye=(0.0, 0.0, 3.0), rotation=(0.0, -90.0), aspect=SWEEP_W / SWEEP_H, fov_y=45.0, z_near_far=(0.1, 50.0))      # looks down -z
SWEEP_SIDES = ("right", "left", "top", "bottom")
SWEEP_STEPS = tuple(np.linspace(-2.5, 2.5, 11))


def sweep_offsets(steps=None):
    """[(side, d, translation)] of test_objects_on_the_scissors_sides: the quad of CC.small_quad with its near edge d pixels inside (negative) /
    outside each side of the frame (steps: {side: the values of d}, default SWEEP_STEPS for every side), then through the near plane, the far
    plane and behind the camera (side "depth", d = None)"""
    w, h = SWEEP_W, SWEEP_H
    # where does the quad's plane meet the frustum's sides?  half-extent of the view at the quad's distance
    half_h = 3.0 * np.tan(np.radians(22.5)); half_w = half_h * w / h
    px = 2 * half_w / w
    offsets = []
    for name, side, centre in (("right", "x", half_w), ("left", "x", -half_w), ("top", "y", half_h), ("bottom", "y", -half_h)):
        for d in (steps or {}).get(name, SWEEP_STEPS):
            t = centre + np.sign(centre) * (0.05 + d * px)      # the quad's near edge d pixels inside (negative) / outside the side
            offsets.append((name, float(d), (t, 0.0, 0.0) if side == "x" else (0.0, t, 0.0)))
    for z in (3.0 - 0.1 + 1e-4, 3.0 - 0.1 - 1e-4, 3.0 - 0.1, 3.0 - 50.0 + 1e-3, 3.0 - 50.0 - 1e-3, 3.0 + 5.0):      # at the near plane, the far plane, behind the camera
        offsets.append(("depth", None, (0.0, 0.0, z)))
    return offsets


def test_objects_on_the_scissors_sides(pkg, hip):
    """one small dense quad (several clusters) moved across every side of the frame in steps of a fraction of a pixel, and through the near and the
    far plane: whatever is skipped, the image's bits are those of the unculled prepass"""
    S = pkg.scenes
    rng = np.random.default_rng(7)
    mats = [S.make_material_textures(rng, 64)]
    meshes = [CC.small_quad(S) + (0,)]      # 1152 triangles: 5 clusters, strips of the quad
    w, h = SWEEP_W, SWEEP_H
    cam = SWEEP_CAMERA
    offsets = [off for _, _, off in sweep_offsets()]
    hits = seen = 0
    ra, rb = [hip.Renderer(w, h, 0, 16) for _ in range(2)]
    for r, cull in ((ra, 0), (rb, 3)):
        r.create_material(*mats[0]); r.create_mesh(*meshes[0][:2], 0)
        r.set_option("cluster_cull", cull); r.set_option("debug", COUNT)
    for off in offsets:
        desc = S.SceneDesc(camera=cam, ambient=0.1, sun=S.DEFAULT_SUN, objects=S.make_objects([(S.translation(*off), 0)]))
        out = []
        for r in (ra, rb):
            r.pass_gbuffer(desc)
            attrs, mat, depth, tri = r.read_gbuffer()
            out.append([attrs.view(np.uint32).copy(), mat.copy(), depth.view(np.uint32).copy(), tri.copy(), r.stats()[:2].copy()])
        same(out[0], out[1])
        n = rb.cull_counts(False)
        drawn = (out[0][3] != 0xFFFFFFFF).any()
        assert not (drawn and n[1] == n[0])
        seen += int(drawn)
        hits += int(drawn and n[1] > 0)      # partly in, and some of its strips skipped
    assert seen >= 12 and hits >= 4, (seen, hits)
    ra.close(); rb.close()


def test_meshes_the_host_cannot_bound(pkg, hip):
    """indices out of range draw nothing and bound nothing; a position that is not finite makes its blocks' boxes infinite (never skipped): the
    prepass is the unculled one's, whatever that draws"""
    S = pkg.scenes
    rng = np.random.default_rng(9)
    mats = [S.make_material_textures(rng, 64)]
    v, i = S.quad((-1, -1, 0), (2, 0, 0), (0, 2, 0), 40, 40)
    v = v.copy(); i = i.copy()
    i[5 * 3] = len(v) + 7                    # one triangle with an index out of range
    i[300 * 3 + 1] = 0xFFFFFFFF
    v["position"][len(v) // 2] = (np.nan, 0.0, np.inf)
    cam = dict(eye=(0.0, 0.0, 3.0), rotation=(0.0, -90.0), aspect=2.0, fov_y=45.0, z_near_far=(0.1, 50.0))
    out = []
    for cull in (0, 3):
        r = hip.Renderer(256, 128, 0, 16)
        r.create_material(*mats[0]); r.create_mesh(v, i, 0)
        r.set_option("cluster_cull", cull)
        frames = []
        for off in ((0, 0, 0), (4.0, 0, 0), (0, 0, 10.0)):
            desc = S.SceneDesc(camera=cam, ambient=0.1, sun=S.DEFAULT_SUN, objects=S.make_objects([(S.translation(*off), 0)]))
            r.pass_gbuffer(desc)
            _, mat, depth, tri = r.read_gbuffer()
            frames += [mat.copy(), depth.view(np.uint32).copy(), tri.copy()]
        out.append(frames)
        r.close()
    same(out[0], out[1])


def test_option_is_validated(pkg, hip):
    r = hip.Renderer(64, 64, 0, 16)
    for bad in (2, 4, -1):
        with pytest.raises(hip.ArcticError):
            r.set_option("cluster_cull", bad)
    with pytest.raises(hip.ArcticError):
        r.cull_counts(False)                # nothing counted yet
    r.close()


# ---- reused handles: what a skipped vertex block leaves in its slots is an EARLIER pass's coordinates --------------------------------------
# The tests above make a fresh handle per camera (a skipped block's slots then hold nothing plausible, or the very values the unculled run left in
# recycled memory) or move a quad of 6 pixels.  Here three handles -- cluster_cull 0, 1 and 3 -- live through a whole sequence of cameras or suns
# that differ by large steps, with meshes of many clusters and blocks that span hundreds of pixels, as generated and with their triangles
# permuted: a block skipped while a kept cluster still reads it shows the previous camera's triangle (tests/test_cluster_bounds.py counts, on
# the CPU, how many such reads each sequence has under a rule that allows them).  Everything is compared bit for bit with the cull-0 handle.
CULLS = (0, 1, 3)


class Mismatches:
    """every comparison of a sequence, so that a failure names each step and how many elements differ"""

    def __init__(self):
        self.found = []

    def compare(self, where, want, got):
        for name, a, b in zip(("plane 0", "plane 1", "plane 2", "plane 3"), want, got):
            assert a.shape == b.shape
            n = int((a != b).sum())
            if n:
                self.found.append(f"{where}, {name}: {n} of {a.size} elements differ")

    def check(self):
        for line in self.found:
            print(line)
        assert not self.found, f"{len(self.found)} comparisons differ from the unculled handle's; the first: {self.found[0]}"


def _planes(r, want=("attrs", "material", "depth", "tri")):
    return [np.ascontiguousarray(x).view(np.uint32).copy() for x in r.read_gbuffer(want=want) if x is not None]


@pytest.fixture(scope="module")
def hall(pkg):
    sc = pkg.scenes.config3(scale=0.5)
    return {False: sc, True: CC.permuted_scene(sc)}


def _handles(hip, sc, **options):
    out = []
    for cull in CULLS:
        r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
        for k, v in dict(options, cluster_cull=cull, debug=COUNT).items():
            r.set_option(k, v)
        out.append(r)
    return out


@pytest.mark.parametrize("permute", [False, True], ids=["as-generated", "permuted"])
def test_reused_handles_small_quad(pkg, hip, permute):
    """one 48 x 48 quad that fills camera A's frame (18 clusters, 10 vertex blocks), pass_gbuffer on the same table set for A, A tilted up, A, A
    raised, A, A raised and moved back: all four planes of the G-buffer"""
    S = pkg.scenes
    mats = S.make_material_textures(np.random.default_rng(7), 64)
    v, i = CC.permuted_meshes([CC.big_quad(S)])[0] if permute else CC.big_quad(S)
    rs = [hip.Renderer(CC.QUAD_W, CC.QUAD_H, 0, 16) for _ in CULLS]
    for r, cull in zip(rs, CULLS):
        r.create_material(*mats); r.create_mesh(v, i, 0)
        r.set_option("cluster_cull", cull); r.set_option("debug", COUNT)
    m = Mismatches()
    for k, cam in enumerate(CC.QUAD_CAMERAS):
        desc = CC.quad_desc(S, cam)
        out = []
        for r in rs:
            r.pass_gbuffer(desc)
            out.append(_planes(r))
        drawn = float((out[0][3] != 0xFFFFFFFF).mean())
        assert drawn > (0.75 if cam is CC.CAMERA_A else 0.05), (k, drawn)         # A sees the whole quad (0.82 of its frame); every other camera still sees part of it
        for cull, got in zip(CULLS[1:], out[1:]):
            m.compare(f"camera {k}, cluster_cull {cull}", out[0], got)
        n = rs[2].cull_counts(False)
        print(f"camera {k}: {drawn:.2f} of the frame drawn; cluster_cull 3 skips {n[1]} of {n[0]} clusters and {n[3]} of {n[2]} vertex blocks")
        if cam is CC.CAMERA_A:
            assert n[1] == 0 and n[3] == 0
        elif not permute:      # (a block of the permuted quad is read by every cluster: its box is the quad's, and the quad is in view)
            assert n[3] >= 1 and n[1] >= 1, (k, n)
    for r in rs:
        r.close()
    m.check()


@pytest.mark.parametrize("in_flight", [1, 2, 3])
@pytest.mark.parametrize("permute", [False, True], ids=["as-generated", "permuted"])
def test_reused_handles_whole_frames(pkg, hip, hall, permute, in_flight):
    """config 3 at 0.5, render_frame three times per camera -- so that every table set of the frames in flight has held the previous camera --
    for the camera turned on the spot by large steps: the RGBA8 frame each time, the triangle and depth planes after each camera's last frame;
    the second camera both through the visibility path (which reads the transformed vertices' attributes as well) and through the G-buffer"""
    sc = hall[permute]
    rs = _handles(hip, sc, frames_in_flight=in_flight, visbuffer=1)
    m = Mismatches()
    for k, rot in enumerate(CC.FRAME_ROTATIONS):
        desc = CC.with_camera_rotation(sc.desc, rot)
        for vis in ((1, 0) if k == 1 else (1,)):
            for r in rs:
                r.set_option("visbuffer", vis)
            for rep in range(3):
                frames = [r.render_frame(desc, sc.settings).copy() for r in rs]
                for cull, got in zip(CULLS[1:], frames[1:]):
                    m.compare(f"camera {k} {rot}, visbuffer {vis}, frame {rep}, cluster_cull {cull}: rgba8", [frames[0]], [got])
            out = [_planes(r, want=("depth", "tri")) for r in rs]
            for cull, got in zip(CULLS[1:], out[1:]):
                m.compare(f"camera {k} {rot}, visbuffer {vis}, cluster_cull {cull}: depth / tri", out[0], got)
            assert (out[0][1] != 0xFFFFFFFF).mean() > 0.3      # (the camera turned up sees the sky through the ceiling's opening)
        for r in rs:
            r.set_option("visbuffer", 1)
        n = rs[2].cull_counts(False)
        print(f"camera {k} {rot}: cluster_cull 3 skips {n[1]} of {n[0]} clusters and {n[3]} of {n[2]} vertex blocks")
        assert n[3] >= 1 and n[1] >= 1, (k, n)
    for r in rs:
        r.close()
    m.check()


@pytest.mark.parametrize("permute", [False, True], ids=["as-generated", "permuted"])
def test_reused_handles_sun_pass(pkg, hip, hall, permute):
    """the sun's pass for a sun whose frustum holds the hall, then two turned far away, then the first again: the shadow map's bits.  Then the
    same once more with a shadow-casting point light whose six faces are drawn in front of every sun's pass: they share the pass's vertex buffer
    and are drawn without block culling, so a skipped block's slots then hold the last face's coordinates"""
    sc = hall[permute]
    rs = _handles(hip, sc)
    m = Mismatches()
    for faces in (False, True):
        if faces:
            for r in rs:
                r.set_option("point_shadow_size", 64)
                r.update_point_shadow_lights(pkg.scenes.point_shadow_lights(1, seed=5))
        for k, rot in enumerate(CC.SUN_ROTATIONS):
            desc = CC.with_sun_rotation(sc.desc, rot)
            out = []
            for r in rs:
                if faces:
                    r.pass_point_shadows(desc)
                r.pass_shadow_map(desc)
                out.append([r.read_shadow_map().view(np.uint32).copy()])
            for cull, got in zip(CULLS[1:], out[1:]):
                m.compare(f"sun {k} {rot}, cube faces {faces}, cluster_cull {cull}: shadow map", out[0], got)
            n = rs[2].cull_counts(True)
            print(f"sun {k} {rot}, cube faces {faces}: {float((out[0][0] != 0x3F800000).mean()):.2f} of the map drawn; cluster_cull 3 skips {n[1]} of {n[0]} clusters and "
                  f"{n[3]} of {n[2]} vertex blocks")
            if k in (1, 2):
                assert n[3] >= 1 and n[1] >= 1, (k, n)
                assert (out[0][0] != 0x3F800000).any()
    for r in rs:
        r.close()
    m.check()


def test_reused_handles_box_through_the_eye_plane(pkg, hip):
    """a wall of ONE cluster and ONE vertex block (the same box) beside the eye, reaching far behind it; the camera looks at it, then turns in
    steps of 0.02 degrees through the directions at which the box's far corner, behind the eye, passes the side planes of box_outside --
    looking at the wall again before every step, so that its slots hold on-screen coordinates.  A block skipped while its cluster is kept
    draws the wall as the previous camera saw it."""
    S = pkg.scenes
    mats = S.make_material_textures(np.random.default_rng(7), 64)
    v, i = CC.wall(S)
    rs = [hip.Renderer(CC.QUAD_W, CC.QUAD_H, 0, 16) for _ in CULLS]
    for r, cull in zip(rs, CULLS):
        r.create_material(*mats); r.create_mesh(v, i, 0)
        r.set_option("cluster_cull", cull); r.set_option("debug", COUNT)
    m = Mismatches()
    states = []
    for k, rot in enumerate(CC.WALL_SWEEP):
        for step, rotation in (("wall in view", CC.WALL_VISIBLE), ("turned", rot)):
            desc = CC.quad_desc(S, CC.wall_camera(rotation))
            out = []
            for r in rs:
                r.pass_gbuffer(desc)
                out.append(_planes(r))
            for cull, got in zip(CULLS[1:], out[1:]):
                m.compare(f"camera {k} {rotation} ({step}), cluster_cull {cull}", out[0], got)
            n = rs[2].cull_counts(False)
            if step == "turned":
                states.append((int(n[3]), int(n[1])))
            else:
                assert (out[0][3] != 0xFFFFFFFF).mean() > 0.1 and n[1] == 0 and n[3] == 0
    for r in rs:
        r.close()
    print("vertex block skipped / cluster skipped per camera of the sweep:", " ".join(f"{b}{c}" for b, c in states))
    for line in m.found:
        print(line)
    assert all(c >= b for b, c in states), states              # never a block without its cluster
    assert (1, 1) in states and (0, 0) in states, states        # the sweep crosses the planes
    m.check()
