"""Morph targets on the device (needs an MI355X): arctic_set_mesh_morph_targets / arctic_set_mesh_morph_weights / arctic_read_mesh_vertices.

The blended vertex buffer is DEFINED bit for bit (include/arctic_hip.h; tests/morph_reference.py is the numpy arbiter), and nothing downstream
of it knows about morphing: a handle whose mesh is morphed must produce the bytes of a handle whose mesh was created from the arbiter's
vertices -- shadow map, visibility, G-buffer, image -- through the passes and through whole frames.  With a skin the buffer is
skin(morph(base)), both by their arbiters.  The parts of the renderer that keep state derived from a mesh's shape are checked one by one: the
cluster boxes, the shadow caches, the frames in flight.
"""
import copy

import numpy as np
import pytest

import morph_reference as M
import skin_reference as R

pytestmark = pytest.mark.gpu

W, H, S = 160, 96, 256
SETTINGS = (2, 2.2, 1.0)
NONE = 0xFFFFFFFF
COUNT = 1024          # ARCTIC_OPT_DEBUG bit 10: count what cluster culling skipped
UNROLL = 4            # csrc/morph.hip MORPH_UNROLL: active targets are taken four at a time, then one at a time
# csrc/morph.hip: a workgroup of 256 threads owns 256 sixteen-byte pieces = 85 1/3 vertices; 85 and 86 are the counts on either side
F = np.float32


def glm(m):
    return np.asarray(m, np.float64).astype(np.float32).T.reshape(16)


def rot_z(deg, pivot):
    a = np.radians(deg)
    r = np.eye(4); r[0, 0], r[0, 1], r[1, 0], r[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    t, u = np.eye(4), np.eye(4)
    t[:3, 3], u[:3, 3] = pivot, -np.asarray(pivot, float)
    return t @ r @ u


class Bar:
    """a tessellated bar along x above the floor with two morph targets (0: the middle rises and the normals lean, 1: the right half swells
    and twists its tangent frame) and a three-joint skin along x"""

    def __init__(self, pkg, offset=(0.0, 1.5, 0.0), n=12):
        v, i = pkg.scenes.box(4.0, 0.6, 0.6, n=n)
        v = v.copy()
        x = v["position"][:, 0].astype(np.float64)
        d = np.zeros((2, len(v)), M.MORPH_DTYPE)
        bump = np.cos(x * np.pi / 4.0) ** 2
        d["position"][0, :, 1] = bump.astype(F)
        d["normal"][0, :, 0] = (0.5 * np.sin(x * np.pi / 2.0)).astype(F)
        right = np.clip(x, 0.0, 2.0) / 2.0
        d["position"][1, :, 1] = (right * v["position"][:, 1]).astype(F)
        d["position"][1, :, 2] = (right * v["position"][:, 2]).astype(F)
        d["tangent"][1, :, 1] = (0.3 * right).astype(F)
        d["bitangent"][1, :, 0] = (-0.3 * right).astype(F)
        t = (x + 2.0) / 2.0
        k = np.clip(np.floor(t), 0, 1).astype(np.int64)
        f = (t - k).astype(F)
        s = np.zeros(len(v), R.SKIN_DTYPE)
        s["joints"][:, 0], s["joints"][:, 1] = k, k + 1
        s["weights"][:, 0], s["weights"][:, 1] = F(1) - f, f
        v["position"] += F(offset)
        self.vertices, self.indices, self.deltas, self.skin, self.offset = v, i, d, s, np.asarray(offset, float)

    def pose(self, angle):
        o = self.offset
        m1 = rot_z(angle, o)
        m2 = m1 @ rot_z(angle, o + (2.0, 0.0, 0.0))
        return np.stack([glm(m) for m in (np.eye(4), m1, m2)])


def make_scene(pkg, bar, with_floor=True):
    Sc = pkg.scenes
    rng = np.random.default_rng(3)
    mats = [Sc.make_material_textures(rng, 32), Sc.make_material_textures(rng, 32)]
    meshes = [(bar.vertices, bar.indices, 0)]
    objs = [(np.eye(4, dtype=np.float32), 0)]
    if with_floor:
        meshes.append(Sc.quad((-8, 0, 8), (16, 0, 0), (0, 0, -16), 8, 8) + (1,))
        objs.append((np.eye(4, dtype=np.float32), 1))
    cam = dict(eye=(0.0, 2.5, 7.0), rotation=(-8.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = Sc.SceneDesc(camera=cam, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=pkg.scene.make_objects(objs))
    lights = pkg.scene.make_lights([(1.5, 3.0, 2.0), (-2.0, 2.0, 1.0)], [(8.0, 6.0, 4.0), (3.0, 5.0, 8.0)])
    return mats, meshes, desc, lights


def handle(hip, scene, vertices=None, cubes=None, **opts):
    """a handle with the scene's materials and meshes; `vertices` replaces mesh 0's (a plain mesh made from the arbiter's)"""
    mats, meshes, desc, lights = scene
    r = hip.Renderer(W, H, S, 16)
    for m in mats:
        r.create_material(*m)
    for k, (v, i, mat) in enumerate(meshes):
        r.create_mesh(vertices if (k == 0 and vertices is not None) else v, i, mat)
    r.update_lights(lights)
    if cubes is not None:
        r.set_option("point_shadow_size", 64)
        r.update_point_shadow_lights(cubes)
    for name, value in opts.items():
        r.set_option(name, value)
    return r


def cube_lights(pkg):
    a = np.zeros(2, pkg.scene.POINT_SHADOW_LIGHT_DTYPE)
    a["position"], a["color"], a["z_near"], a["z_far"] = [(0.5, 4.0, 1.0), (-1.5, 3.0, -1.0)], [(6, 6, 6), (4, 3, 2)], 0.05, 30.0
    return a


def through_passes(r, desc, cubes):
    r.pass_shadow_map(desc)
    if cubes:
        r.pass_point_shadows(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, SETTINGS)
    attrs, mat, depth, tri = r.read_gbuffer()
    out = [r.read_shadow_map().view(np.uint32).copy(), attrs.view(np.uint32).copy(), mat.copy(), depth.view(np.uint32).copy(), tri.copy(),
           r.read_output(want=("rgba8",))[2].copy(), r.stats()[:4].copy()]
    return out + [r.read_point_shadow(k).view(np.uint32).copy() for k in range(cubes)]


def through_frames(r, desc, cubes):
    out = [r.render_frame(desc, SETTINGS).copy(), r.render_frame(desc, SETTINGS).copy(), r.read_shadow_map().view(np.uint32).copy()]
    out += [r.read_point_shadow(k).view(np.uint32).copy() for k in range(cubes)]
    _, mat, depth, tri = r.read_gbuffer(want=("material", "depth", "tri"))
    return out + [mat.copy(), depth.view(np.uint32).copy(), tri.copy()]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- read-back: the kernel against the arbiter ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bench_handle(pkg, hip):
    r = hip.Renderer(W, H, S, 16)
    r.create_material(*pkg.scenes.make_material_textures(np.random.default_rng(1), 8))
    yield r
    r.close()


def active_sets(w):
    """the random weights as they are (zeros of both signs, negatives, above 1, a denormal), then: none, all, first only, last only, every other"""
    n = len(w)
    full = np.where(w == 0, F(0.625), w).astype(F)
    first, last, other = np.zeros(n, F), np.zeros(n, F), full.copy()
    first[0], last[-1] = F(-1.75), F(2.5)
    other[1::2] = F(-0.0)
    return [w, np.zeros(n, F), full, first, last, other]


@pytest.mark.parametrize("n_targets", [1, 2, UNROLL - 1, UNROLL, UNROLL + 1, 64, 65])
@pytest.mark.parametrize("n_vertices", [1, 2, 63, 64, 65, 85, 86, 255, 256, 257, 1000])
def test_read_back_equals_the_arbiter(pkg, hip, bench_handle, n_vertices, n_targets):
    r = bench_handle
    rng = np.random.default_rng(77 * n_targets + n_vertices)
    v, d, w = M.random_case(rng, n_vertices, n_targets, pkg.scene.VERTEX_DTYPE)
    mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
    r.set_mesh_morph_targets(mesh, d)
    assert r.read_mesh_vertices(mesh, n_vertices).tobytes() == v.tobytes()          # targets alone change nothing
    for weights in active_sets(w):
        r.set_mesh_morph_weights(mesh, weights)                                      # (every call overwrites the same buffer)
        got = r.read_mesh_vertices(mesh, n_vertices)
        assert got.tobytes() == M.morph_vertices(v, d, weights).tobytes()
        if not (weights == 0).all():
            assert got.tobytes() != v.tobytes()
    r.set_mesh_morph_weights(mesh, None)
    assert r.read_mesh_vertices(mesh, n_vertices).tobytes() == v.tobytes()
    r.set_mesh_morph_targets(mesh, None)                                             # (the module's handle does not keep every case's arrays)


def test_the_sum_keeps_the_ascending_order(pkg, hip, bench_handle):
    """weights of equal magnitude whose products differ hugely: (1 + 2^-24) - 1 = 0 in float32, (1 - 1) + 2^-24 = 2^-24.  The same two arrays
    attached in the other order give the other result; a kernel that reordered its sums would give the same for both."""
    r = bench_handle
    n = 300
    v = np.zeros(n, pkg.scene.VERTEX_DTYPE)
    for name in M.VERTEX_FIELDS:
        v[name] = 1.0
    tiny, one = np.zeros(n, M.MORPH_DTYPE), np.zeros(n, M.MORPH_DTYPE)
    for name in M.VERTEX_FIELDS:
        tiny[name], one[name] = F(2.0 ** -24), F(1.0)
    results = []
    for d, w in ((np.stack([tiny, one]), np.array([1.0, -1.0], F)), (np.stack([one, tiny]), np.array([-1.0, 1.0], F))):
        mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
        r.set_mesh_morph_targets(mesh, d)
        r.set_mesh_morph_weights(mesh, w)
        got = r.read_mesh_vertices(mesh, n)
        assert got.tobytes() == M.morph_vertices(v, d, w).tobytes()
        results.append(got["position"][7, 0])
        r.set_mesh_morph_targets(mesh, None)
    assert results[0] == 0.0 and results[1] == F(2.0 ** -24)
    # ... and in a longer sum: eight targets, weights +-1.5, against the arbiter in the defined order and in the reverse order
    v, d, _ = M.random_case(np.random.default_rng(8), 300, 8, pkg.scene.VERTEX_DTYPE)
    w = np.array([1.5, -1.5, 1.5, 1.5, -1.5, -1.5, 1.5, -1.5], F)
    mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
    r.set_mesh_morph_targets(mesh, d)
    r.set_mesh_morph_weights(mesh, w)
    got = r.read_mesh_vertices(mesh, 300).tobytes()
    assert got == M.morph_vertices(v, d, w).tobytes() and got != M.morph_vertices(v, d[::-1], w[::-1]).tobytes()
    r.set_mesh_morph_targets(mesh, None)


def test_refusals_leave_the_mesh_as_it_was(pkg, hip):
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc, v, d = scene[2], bar.vertices, bar.deltas
    r = handle(hip, scene)

    def refused(code, fn, *a):
        with pytest.raises(hip.ArcticError) as e:
            fn(*a)
        assert e.value.code == code

    before = r.render_frame(desc, SETTINGS).copy()
    refused(-4, r.set_mesh_morph_weights, 0, [0.5, 0.5])                              # no targets yet: ARCTIC_E_STATE
    refused(-1, r.set_mesh_morph_targets, 0, d[:, :-1])                               # not the mesh's vertex count
    refused(-1, r.set_mesh_morph_targets, 0, d[:0])                                   # 0 targets
    bad = d.copy(); bad["normal"][1, 5, 2] = np.nan
    refused(-1, r.set_mesh_morph_targets, 0, bad)
    refused(-1, r.set_mesh_morph_targets, 10 ** 6, d)                                 # no such mesh
    refused(-4, r.set_mesh_morph_weights, 0, [0.5, 0.5])                              # still no targets
    np.testing.assert_array_equal(r.render_frame(desc, SETTINGS), before)
    r.set_mesh_morph_targets(0, d)
    np.testing.assert_array_equal(r.render_frame(desc, SETTINGS), before)             # targets with zero weights: the mesh's own bytes
    w = np.array([0.8, -0.4], F)
    r.set_mesh_morph_weights(0, w)
    morphed = M.morph_vertices(v, d, w).tobytes()
    frame = r.render_frame(desc, SETTINGS).copy()
    assert not np.array_equal(frame, before)
    refused(-1, r.set_mesh_morph_weights, 0, [0.5])                                   # wrong count
    refused(-1, r.set_mesh_morph_weights, 0, [0.5, 0.5, 0.5])
    refused(-1, r.set_mesh_morph_weights, 0, [0.5, np.nan])
    refused(-1, r.set_mesh_morph_weights, 0, [np.inf, 0.0])
    refused(-1, r.set_mesh_morph_weights, 10 ** 6, w)                                 # a mesh index out of range
    refused(-4, r.set_mesh_morph_weights, 1, w)                                       # the floor has no targets
    assert r.read_mesh_vertices(0, len(v)).tobytes() == morphed                       # the previous weights are kept
    refused(-1, r.set_mesh_morph_targets, 0, bad)                                     # a refused replacement keeps targets and weights
    refused(-1, r.set_mesh_morph_targets, 0, d[:, :-1])
    assert r.read_mesh_vertices(0, len(v)).tobytes() == morphed
    np.testing.assert_array_equal(r.render_frame(desc, SETTINGS), frame)              # the next frame is the one before
    r.set_mesh_morph_targets(0, None)                                                 # detach: targets and weights go
    assert r.read_mesh_vertices(0, len(v)).tobytes() == v.tobytes()
    np.testing.assert_array_equal(r.render_frame(desc, SETTINGS), before)
    refused(-4, r.set_mesh_morph_weights, 0, w)
    r.close()


# ---- a morphed mesh against a plain mesh of the arbiter's vertices ------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [3, 0], ids=["cluster-cull", "no-cluster-cull"])
@pytest.mark.parametrize("cubes", [0, 2], ids=["default", "point-shadows"])
def test_morphed_mesh_equals_plain_mesh(pkg, hip, cubes, cull):
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    w = np.array([0.9, 1.4], F)
    want_vertices = M.morph_vertices(bar.vertices, bar.deltas, w)
    assert np.abs(want_vertices["position"] - bar.vertices["position"]).max() > 0.5
    lights = cube_lights(pkg) if cubes else None
    for run in (through_passes, through_frames):
        morphed = handle(hip, scene, cubes=lights, cluster_cull=cull)
        plain = handle(hip, scene, vertices=want_vertices, cubes=lights, cluster_cull=cull)
        rest = handle(hip, scene, cubes=lights, cluster_cull=cull)
        morphed.set_mesh_morph_targets(0, bar.deltas)
        morphed.set_mesh_morph_weights(0, w)
        a, b, c = run(morphed, desc, cubes), run(plain, desc, cubes), run(rest, desc, cubes)
        same(a, b)
        assert not np.array_equal(a[0], c[0])                                         # and the morph is visible: not the neutral shape's frame
        for r in (morphed, plain, rest):
            r.close()


def test_a_handle_without_morph_targets_renders_what_it_rendered(pkg, hip):
    """the same process, the same library: a handle no morph call was made on, one with targets at rest, one whose weights came back to zero"""
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    plain, rest = handle(hip, scene), handle(hip, scene)
    want_p, want_f = through_passes(plain, desc, 0), through_frames(plain, desc, 0)
    rest.set_mesh_morph_targets(0, bar.deltas)
    same(through_passes(rest, desc, 0), want_p)
    same(through_frames(rest, desc, 0), want_f)
    rest.set_mesh_morph_weights(0, [0.0, -0.0])
    same(through_frames(rest, desc, 0), want_f)
    rest.set_mesh_morph_weights(0, [1.0, 1.0])
    assert not np.array_equal(through_frames(rest, desc, 0)[0], want_f[0])
    rest.set_mesh_morph_weights(0, None)
    same(through_frames(rest, desc, 0), want_f)
    same(through_passes(rest, desc, 0), want_p)
    rest.set_mesh_morph_weights(0, [1.0, 1.0])
    rest.set_mesh_morph_targets(0, None)                                              # the targets detached while morphed
    same(through_frames(rest, desc, 0), want_f)
    plain.close(); rest.close()


# ---- morph and skin together ------------------------------------------------------------------------------------------------------------------
def test_morph_then_skin(pkg, hip):
    """every order of the calls leaves skin(morph(base)): vertices bit for bit, and the frame of a plain mesh made from them"""
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc, v, d, s = scene[2], bar.vertices, bar.deltas, bar.skin
    w1, w2 = np.array([0.7, 0.0], F), np.array([-0.3, 1.2], F)
    J1, J2 = bar.pose(30.0), bar.pose(-25.0)
    d2 = d[::-1].copy()
    d2["position"] *= F(0.5)

    def check(r, want, what):
        assert r.read_mesh_vertices(0, len(v)).tobytes() == want.tobytes(), what
        plain = handle(hip, scene, vertices=want)
        same(through_frames(r, desc, 0), through_frames(plain, desc, 0))
        plain.close()

    r = handle(hip, scene)
    r.set_mesh_skin(0, s, 3)
    r.set_mesh_morph_targets(0, d)
    r.set_mesh_pose(0, J1); r.set_mesh_morph_weights(0, w1)
    check(r, R.skin_vertices(M.morph_vertices(v, d, w1), s, J1), "pose, then weights")
    r.set_mesh_morph_weights(0, w2)
    check(r, R.skin_vertices(M.morph_vertices(v, d, w2), s, J1), "new weights under a standing pose")
    r.set_mesh_morph_weights(0, [0.0, 0.0])
    check(r, R.skin_vertices(v, s, J1), "weights back to zero under a standing pose")
    r.set_mesh_pose(0, None)
    check(r, v, "neither")
    r.set_mesh_morph_weights(0, w1); r.set_mesh_pose(0, J2)
    check(r, R.skin_vertices(M.morph_vertices(v, d, w1), s, J2), "weights, then pose")
    r.set_mesh_pose(0, None)
    check(r, M.morph_vertices(v, d, w1), "pose removed under standing weights")
    r.set_mesh_pose(0, J1)
    r.set_mesh_morph_targets(0, d2)                                                   # replaced: all weights zero, the pose stands on the mesh's own vertices
    check(r, R.skin_vertices(v, s, J1), "targets replaced under a standing pose")
    r.set_mesh_morph_weights(0, w2)
    check(r, R.skin_vertices(M.morph_vertices(v, d2, w2), s, J1), "the new targets under the standing pose")
    r.set_mesh_skin(0, None)
    check(r, M.morph_vertices(v, d2, w2), "skin detached under standing weights")
    r.set_mesh_morph_targets(0, None)
    check(r, v, "everything detached")
    r.close()


# ---- cluster boxes ----------------------------------------------------------------------------------------------------------------------------
def test_a_morphed_mesh_is_never_skipped_and_rest_gets_its_boxes_back(pkg, hip):
    """a mesh of many clusters most of which are outside the view: skipped at rest, none skipped while a weight is non-zero (the target lifts a
    far corner of the sheet into view, which the rest shape's boxes would cull), skipped again afterwards"""
    Sc = pkg.scenes
    v, i = Sc.quad((-40, 0, 40), (80, 0, 0), (0, 0, -80), 48, 48)
    d = np.zeros((1, len(v)), M.MORPH_DTYPE)
    far = (v["position"][:, 0] < -30) & (v["position"][:, 2] > 30)                     # behind the camera, to its left
    d["position"][0, far] = (30.0, 1.0, -40.0)                                        # ... moved in front of it
    mats = [Sc.make_material_textures(np.random.default_rng(2), 32)]
    cam = dict(eye=(0.0, 2.5, 7.0), rotation=(-8.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = Sc.SceneDesc(camera=cam, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=pkg.scene.make_objects([(np.eye(4, dtype=np.float32), 0)]))
    scene = (mats, [(v, i, 0)], desc, pkg.scene.make_lights([(0, 3, 0)], [(5, 5, 5)]))
    r = handle(hip, scene, debug=COUNT)
    first = through_passes(r, desc, 0)
    counts = [r.cull_counts(False).copy(), r.cull_counts(True).copy()]
    assert counts[0][1] > 0 and counts[0][3] > 0 and counts[1][1] > 0
    r.set_mesh_morph_targets(0, d)
    same(through_passes(r, desc, 0), first)
    np.testing.assert_array_equal(r.cull_counts(False), counts[0])                    # targets at rest keep the boxes
    r.set_mesh_morph_weights(0, [1.0])
    plain = handle(hip, (mats, [(M.morph_vertices(v, d, [1.0]), i, 0)], desc, scene[3]))
    got = through_passes(r, desc, 0)
    same(got, through_passes(plain, desc, 0))
    assert not np.array_equal(got[4], first[4])                                       # the lifted corner is seen
    plain.close()
    for shadow_pass in (False, True):
        n = r.cull_counts(shadow_pass)
        assert n[0] == counts[int(shadow_pass)][0] and n[1] == 0 and n[3] == 0        # nothing skipped for the morphed mesh
    r.set_mesh_morph_weights(0, [-0.0])
    same(through_passes(r, desc, 0), first)
    np.testing.assert_array_equal(r.cull_counts(False), counts[0])
    np.testing.assert_array_equal(r.cull_counts(True), counts[1])
    r.close()


# ---- shadow caches ----------------------------------------------------------------------------------------------------------------------------
def test_the_shadow_caches_see_a_weights_call(pkg, hip):
    """static sun, static objects, ARCTIC_OPT_SHADOW_CACHE on: the only thing that changes between the frames is the caster's shape.  The maps
    after each call are those of a fresh handle; that a repeated frame does NOT redraw the sun's map shows in arctic_read_cull_counts, which
    refuses while the latest shadow pass ran before counting was switched on."""
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc, cubes = scene[2], cube_lights(pkg)
    weights = [np.array([1.0, 0.0], F), np.array([-0.5, 1.5], F)]
    fresh = []
    for w in weights:
        h = handle(hip, scene, cubes=cubes)
        h.set_mesh_morph_targets(0, bar.deltas); h.set_mesh_morph_weights(0, w)
        fresh.append(through_frames(h, desc, 2))
        h.close()
    r = handle(hip, scene, cubes=cubes)
    r.set_mesh_morph_targets(0, bar.deltas)
    got = []
    for w in weights:
        r.set_mesh_morph_weights(0, w)
        got.append(through_frames(r, desc, 2))
    same(got[0], fresh[0])
    same(got[1], fresh[1])
    for k in (2, 3, 4):                                                               # the sun's map and both lights' faces did change
        assert not np.array_equal(got[0][k], got[1][k])
    r.set_option("debug", COUNT)                                                      # from here on a shadow pass that runs counts
    r.render_frame(desc, SETTINGS)                                                    # a repeated frame without a call: the map is not redrawn
    with pytest.raises(hip.ArcticError) as e:
        r.cull_counts(True)
    assert e.value.code == -4
    r.set_mesh_morph_weights(0, weights[1])                                           # the same weights again are a call all the same
    r.render_frame(desc, SETTINGS)
    assert r.cull_counts(True)[0] > 0                                                 # redrawn
    r.set_option("debug", 0)
    r.set_mesh_morph_weights(0, None)                                                 # ... and the way back to rest is a change too
    plain = handle(hip, scene, cubes=cubes)
    same(through_frames(r, desc, 2), through_frames(plain, desc, 2))
    r.close(); plain.close()


# ---- frames in flight -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [2, 3])
def test_frames_in_flight_alternating_weights(pkg, hip, in_flight):
    """eight frames, each enqueued behind new weights without a flush in between: k_morph must follow the prepass that still reads the buffer
    it overwrites and precede the next one, whichever stream that runs on; frames 4..7 have a pose on top"""
    import torch
    bar = Bar(pkg)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    weights = [np.array([1.0, 0.2], F), np.array([-0.6, 1.3], F), None]
    J = bar.pose(30.0)
    alone = []
    for w in weights[:2]:
        h = handle(hip, scene, frames_in_flight=1)
        h.set_mesh_morph_targets(0, bar.deltas); h.set_mesh_morph_weights(0, w)
        alone.append(h.render_frame(desc, SETTINGS).copy())
        h.close()
    assert not np.array_equal(alone[0], alone[1])
    descs = []
    for k in range(8):                                                                # the camera moves a little as well: no frame is a repeat
        c = copy.deepcopy(desc)
        c.camera["eye"] = (0.05 * k, 2.5, 7.0)
        descs.append(c)

    def enqueue(r, k, out=None):
        if k == 4:
            r.set_mesh_pose(0, J)
        r.set_mesh_morph_weights(0, weights[k % 3])
        if out is None:
            return r.render_frame(descs[k], SETTINGS)
        r.render_frame_device(descs[k], SETTINGS, out.data_ptr())

    r = handle(hip, scene, frames_in_flight=in_flight)
    r.set_mesh_morph_targets(0, bar.deltas)
    r.set_mesh_skin(0, bar.skin, 3)
    outs = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    for k in range(8):
        enqueue(r, k, outs[k])
    r.flush()
    got = [o.cpu().numpy() for o in outs]
    r.close()
    h = handle(hip, scene, frames_in_flight=1)
    h.set_mesh_morph_targets(0, bar.deltas)
    h.set_mesh_skin(0, bar.skin, 3)
    for k in range(8):
        np.testing.assert_array_equal(got[k], enqueue(h, k), err_msg=f"frame {k}")
    np.testing.assert_array_equal(got[0], alone[0])
    h.close()
    # frame 7 (weights[1] under the pose) against a plain mesh of the two arbiters' vertices
    want = R.skin_vertices(M.morph_vertices(bar.vertices, bar.deltas, weights[1]), bar.skin, J)
    plain = handle(hip, scene, vertices=want, frames_in_flight=1)
    np.testing.assert_array_equal(got[7], plain.render_frame(descs[7], SETTINGS))
    plain.close()


# ---- glTF ------------------------------------------------------------------------------------------------------------------------------------
def test_gltf_file_end_to_end(pkg, hip, tmp_path):
    """a glTF file written here with two targets, an animated weights channel and a skin -> loader -> GltfScene.upload + GltfScene.pose ->
    frames, at three times: the vertices are skin(morph(base)) by the two arbiters for the loader's weights and joint matrices, and the frame
    is that of a plain mesh made from them"""
    from importlib import import_module
    from gltf_morph_files import write_morphed
    gltf = import_module("arctic_renderer_amd.gltf")
    gltf.build()
    path, _ = write_morphed(tmp_path, storage="sparse", index_type=5123, skin=True)
    sc = gltf.load(path)
    cam = dict(eye=(0.0, 0.5, 6.0), rotation=(0.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = pkg.scenes.SceneDesc(camera=cam, ambient=0.3, sun=dict(pkg.scenes.DEFAULT_SUN, position=(2.0, 6.0, 12.0), rotation=(-25.0, -100.0)), objects=sc.objects)
    v, idx, mat = sc.meshes[0]
    skin, _, n_joints = sc.mesh_skins[0]
    d = sc.mesh_morphs[0]
    r = sc.upload(hip.Renderer(W, H, S, 16))
    rest = r.render_frame(desc, SETTINGS).copy()
    frames = []
    for animation, t in ((0, 0.75), (0, 1.0), (0, 1.6), (1, 1.6), (-1, 0.0)):
        sc.pose(r, animation, t)
        w, J = sc.morph_weights(0, animation, t), sc.joint_matrices(0, animation, t)
        want = R.skin_vertices(M.morph_vertices(v, d, w), skin, J)
        assert r.read_mesh_vertices(0, len(v)).tobytes() == want.tobytes()
        plain = hip.Renderer(W, H, S, 16)
        plain.create_material(*sc.materials[0]); plain.create_mesh(want, idx, mat)
        frames.append(r.render_frame(desc, SETTINGS).copy())
        np.testing.assert_array_equal(frames[-1], plain.render_frame(desc, SETTINGS))
        plain.close()
    assert (rest[..., :3] != 0).any() and not np.array_equal(frames[0], rest) and not np.array_equal(frames[0], frames[1])
    assert not np.array_equal(frames[2], frames[3])                                   # LINEAR against STEP at the same time
    for animation, word in ((2, "CUBICSPLINE"), (3, "weights")):
        with pytest.raises(ValueError, match=word):
            sc.pose(r, animation, 0.0)
    np.testing.assert_array_equal(r.render_frame(desc, SETTINGS), frames[-1])         # a refused animation changed nothing
    r.close()
