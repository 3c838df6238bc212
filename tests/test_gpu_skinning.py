"""Skeletal skinning on the device (needs an MI355X): arctic_set_mesh_skin / arctic_set_mesh_pose / arctic_read_mesh_vertices.

The posed vertex buffer is DEFINED bit for bit (include/arctic_hip.h; tests/skin_reference.py is the numpy arbiter), and nothing downstream of
it knows about skinning: a handle whose mesh is posed must produce the bytes of a handle whose mesh was created from the arbiter's vertices --
shadow map, visibility, G-buffer, image -- through the passes and through whole frames.  The parts of the renderer that keep state derived from
a mesh's shape are checked one by one: the cluster boxes, the shadow caches, the frames in flight.
"""
import copy

import numpy as np
import pytest

import skin_reference as R

pytestmark = pytest.mark.gpu

W, H, S = 160, 96, 256
SETTINGS = (2, 2.2, 1.0)
NONE = 0xFFFFFFFF
COUNT = 1024          # ARCTIC_OPT_DEBUG bit 10: count what cluster culling skipped
LDS_JOINTS = 256      # csrc/common.h SKIN_LDS_JOINTS: up to here the kernel stages the joint table in LDS, beyond it gathers from global memory


def glm(m):
    return np.asarray(m, np.float64).astype(np.float32).T.reshape(16)


def rot_z(deg, pivot):
    a = np.radians(deg)
    r = np.eye(4); r[0, 0], r[0, 1], r[1, 0], r[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    t, u = np.eye(4), np.eye(4)
    t[:3, 3], u[:3, 3] = pivot, -np.asarray(pivot, float)
    return t @ r @ u


def shift(x, y=0.0, z=0.0):
    m = np.eye(4); m[:3, 3] = (x, y, z)
    return m


class Bar:
    """a tessellated bar along x with three joints at x = -2, 0, 2 (or the same three poses spread over n_joints joints)"""

    def __init__(self, pkg, n_joints=3, offset=(0.0, 1.5, 0.0), n=12):
        v, i = pkg.scenes.box(4.0, 0.6, 0.6, n=n)
        v = v.copy()
        x = v["position"][:, 0].astype(np.float64)
        t = (x + 2.0) / 2.0
        k = np.clip(np.floor(t), 0, 1).astype(np.int64)
        f = (t - k).astype(np.float32)
        spread = 3 * ((np.arange(len(v)) * 7) % (n_joints // 3)) if n_joints >= 6 else 0
        s = np.zeros(len(v), R.SKIN_DTYPE)
        s["joints"][:, 0], s["joints"][:, 1] = k + spread, k + 1 + spread
        s["weights"][:, 0], s["weights"][:, 1] = np.float32(1) - f, f
        v["position"] += np.float32(offset)
        self.vertices, self.indices, self.skin, self.n_joints, self.offset = v, i, s, n_joints, np.asarray(offset, float)

    def pose(self, angle, move=(0.0, 0.0, 0.0)):
        o = self.offset
        m1 = rot_z(angle, o)
        m2 = m1 @ rot_z(angle, o + (2.0, 0.0, 0.0))
        three = [shift(*move) @ m for m in (np.eye(4), m1, m2)]
        return np.stack([glm(three[j % 3]) for j in range(self.n_joints)])


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


# ---- read-back ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bench_handle(pkg, hip):
    r = hip.Renderer(W, H, S, 16)
    r.create_material(*pkg.scenes.make_material_textures(np.random.default_rng(1), 8))
    yield r
    r.close()


@pytest.mark.parametrize("n_joints", [1, 2, 300, LDS_JOINTS, LDS_JOINTS + 1])
@pytest.mark.parametrize("n_vertices", [1, 63, 64, 65, 257, 1000])
def test_read_back_equals_the_arbiter(pkg, hip, bench_handle, n_vertices, n_joints):
    r = bench_handle
    rng = np.random.default_rng(77 * n_joints + n_vertices)
    v, s, J = R.random_case(rng, n_vertices, n_joints, pkg.scene.VERTEX_DTYPE)
    mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
    r.set_mesh_skin(mesh, s, n_joints)
    assert r.read_mesh_vertices(mesh, n_vertices).tobytes() == v.tobytes()          # a skin alone changes nothing
    r.set_mesh_pose(mesh, J)
    got = r.read_mesh_vertices(mesh, n_vertices)
    assert got.tobytes() == R.skin_vertices(v, s, J).tobytes()
    J2 = J[::-1].copy()                                                              # a second pose overwrites the same buffer
    r.set_mesh_pose(mesh, J2)
    assert r.read_mesh_vertices(mesh, n_vertices).tobytes() == R.skin_vertices(v, s, J2).tobytes()
    r.set_mesh_pose(mesh, None)
    assert r.read_mesh_vertices(mesh, n_vertices).tobytes() == v.tobytes()


def test_refusals_leave_the_mesh_as_it_was(pkg, hip, bench_handle):
    r = bench_handle
    v, s, J = R.random_case(np.random.default_rng(4), 130, 4, pkg.scene.VERTEX_DTYPE)
    mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)

    def refused(code, fn, *a):
        with pytest.raises(hip.ArcticError) as e:
            fn(*a)
        assert e.value.code == code

    refused(-4, r.set_mesh_pose, mesh, J)                                            # no skin yet: ARCTIC_E_STATE
    refused(-1, r.set_mesh_skin, mesh, s[:-1], 4)                                    # not the mesh's vertex count
    refused(-1, r.set_mesh_skin, mesh, s, 0)
    refused(-1, r.set_mesh_skin, mesh, s, 65536)
    refused(-1, r.set_mesh_skin, mesh, s, int(s["joints"].max()))                    # an index at n_joints
    bad = s.copy(); bad["weights"][5, 3] = np.inf
    refused(-1, r.set_mesh_skin, mesh, bad, 4)
    refused(-1, r.set_mesh_skin, 10 ** 6, s, 4)                                      # no such mesh
    refused(-4, r.set_mesh_pose, mesh, J)                                            # still no skin
    r.set_mesh_skin(mesh, s, 4)
    r.set_mesh_pose(mesh, J)
    posed = R.skin_vertices(v, s, J).tobytes()
    refused(-1, r.set_mesh_pose, mesh, J[:3])                                        # wrong joint count
    Jb = J.copy(); Jb[1, 7] = np.nan
    refused(-1, r.set_mesh_pose, mesh, Jb)
    refused(-1, r.set_mesh_pose, 10 ** 6, J)
    assert r.read_mesh_vertices(mesh, len(v)).tobytes() == posed                     # the previous pose is kept
    refused(-1, r.set_mesh_skin, mesh, bad, 4)                                       # a refused replacement keeps skin and pose
    assert r.read_mesh_vertices(mesh, len(v)).tobytes() == posed
    refused(-1, r.read_mesh_vertices, mesh, len(v) + 1)
    r.set_mesh_skin(mesh, None)                                                      # detach: the skin and the pose go
    assert r.read_mesh_vertices(mesh, len(v)).tobytes() == v.tobytes()
    refused(-4, r.set_mesh_pose, mesh, J)


# ---- a posed mesh against a plain mesh of the arbiter's vertices ---------------------------------------------------------------------------
@pytest.mark.parametrize("cubes", [0, 2], ids=["default", "point-shadows"])
@pytest.mark.parametrize("n_joints", [3, 300])
def test_posed_mesh_equals_plain_mesh(pkg, hip, n_joints, cubes):
    bar = Bar(pkg, n_joints)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    J = bar.pose(35.0)
    want_vertices = R.skin_vertices(bar.vertices, bar.skin, J)
    assert np.abs(want_vertices["position"] - bar.vertices["position"]).max() > 0.5
    lights = cube_lights(pkg) if cubes else None
    for run in (through_passes, through_frames):
        posed, plain, bind = handle(hip, scene, cubes=lights), handle(hip, scene, vertices=want_vertices, cubes=lights), handle(hip, scene, cubes=lights)
        posed.set_mesh_skin(0, bar.skin, n_joints)
        posed.set_mesh_pose(0, J)
        a, b, c = run(posed, desc, cubes), run(plain, desc, cubes), run(bind, desc, cubes)
        same(a, b)
        assert not np.array_equal(a[0], c[0])                                         # and the pose is visible: not the bind pose's frame
        for r in (posed, plain, bind):
            r.close()


# ---- cluster boxes -------------------------------------------------------------------------------------------------------------------------
def test_a_pose_moves_the_mesh_onto_and_off_the_screen(pkg, hip):
    """the boxes made at arctic_create_mesh bound the bind pose: used for a posed mesh they would cull what the pose brought into view"""
    on = Bar(pkg, 3)
    off = Bar(pkg, 3, offset=(60.0, 1.5, 0.0))                                        # bind pose far beyond the right side of the frame
    for cull in (3, 1):
        # off-screen -> on-screen
        scene = make_scene(pkg, off, with_floor=False)
        r = handle(hip, scene, cluster_cull=cull, debug=COUNT)
        r.pass_gbuffer(scene[2])
        assert (r.read_gbuffer(want=("tri",))[3] == NONE).all()
        n = r.cull_counts(False)
        assert n[1] == n[0] > 1                                                       # every cluster skipped in the bind pose
        r.set_mesh_skin(0, off.skin, 3)
        J = off.pose(0.0, move=(-60.0, 0.0, 0.0))
        r.set_mesh_pose(0, J)
        plain = handle(hip, scene, vertices=R.skin_vertices(off.vertices, off.skin, J), cluster_cull=cull)
        a, b = through_passes(r, scene[2], 0), through_passes(plain, scene[2], 0)
        same(a, b)
        assert (a[4] != NONE).mean() > 0.02
        assert r.cull_counts(False)[1] == 0 and r.cull_counts(False)[3] == 0          # a posed mesh's boxes are never skipped
        same(through_frames(r, scene[2], 0), through_frames(plain, scene[2], 0))
        r.close(); plain.close()
        # on-screen -> off-screen: the frame is empty; back to the bind pose: the original frame and the original counts
        scene = make_scene(pkg, on, with_floor=False)
        r = handle(hip, scene, cluster_cull=cull, debug=COUNT)
        first = through_passes(r, scene[2], 0)
        counts = [r.cull_counts(False).copy(), r.cull_counts(True).copy()]
        assert (first[4] != NONE).mean() > 0.02
        r.set_mesh_skin(0, on.skin, 3)
        r.set_mesh_pose(0, on.pose(0.0, move=(60.0, 0.0, 0.0)))
        gone = through_passes(r, scene[2], 0)
        assert (gone[4] == NONE).all() and (gone[2] == NONE).all()
        assert (r.render_frame(scene[2], SETTINGS)[..., :3] == 0).all()               # no geometry, no environment map: black
        r.set_mesh_pose(0, None)
        same(through_passes(r, scene[2], 0), first)
        np.testing.assert_array_equal(r.cull_counts(False), counts[0])
        np.testing.assert_array_equal(r.cull_counts(True), counts[1])
        r.close()


def test_bind_pose_gets_its_real_boxes_back(pkg, hip):
    """a mesh of many clusters most of which are outside the view: skipped in the bind pose, none skipped while posed, skipped again afterwards"""
    Sc = pkg.scenes
    v, i = Sc.quad((-40, 0, 40), (80, 0, 0), (0, 0, -80), 48, 48)
    s = np.zeros(len(v), R.SKIN_DTYPE); s["weights"][:, 0] = 1
    mats = [Sc.make_material_textures(np.random.default_rng(2), 32)]
    cam = dict(eye=(0.0, 2.5, 7.0), rotation=(-8.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = Sc.SceneDesc(camera=cam, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=pkg.scene.make_objects([(np.eye(4, dtype=np.float32), 0)]))
    scene = (mats, [(v, i, 0)], desc, pkg.scene.make_lights([(0, 3, 0)], [(5, 5, 5)]))
    r = handle(hip, scene, debug=COUNT)
    first = through_passes(r, desc, 0)
    counts = [r.cull_counts(False).copy(), r.cull_counts(True).copy()]
    assert counts[0][1] > 0 and counts[0][3] > 0 and counts[1][1] > 0
    r.set_mesh_skin(0, s, 1)
    same(through_passes(r, desc, 0), first)
    np.testing.assert_array_equal(r.cull_counts(False), counts[0])                    # a skin without a pose keeps the boxes
    identity = glm(np.eye(4))[None]
    r.set_mesh_pose(0, identity)                                                      # the identity pose: the same shape, but no box may be trusted
    plain = handle(hip, (mats, [(R.skin_vertices(v, s, identity), i, 0)], desc, scene[3]))    # (the arithmetic turns a -0.0 of the mesh into +0.0)
    same(through_passes(r, desc, 0), through_passes(plain, desc, 0))
    plain.close()
    for shadow_pass in (False, True):
        n = r.cull_counts(shadow_pass)
        assert n[0] == counts[int(shadow_pass)][0] and n[1] == 0 and n[3] == 0
    r.set_mesh_pose(0, None)
    same(through_passes(r, desc, 0), first)
    np.testing.assert_array_equal(r.cull_counts(False), counts[0])
    np.testing.assert_array_equal(r.cull_counts(True), counts[1])
    r.close()


# ---- shadow caches -------------------------------------------------------------------------------------------------------------------------
def test_the_shadow_caches_see_a_pose(pkg, hip):
    """static sun, static objects, ARCTIC_OPT_SHADOW_CACHE on: the only thing that changes between the two frames is the caster's shape"""
    bar = Bar(pkg, 3)
    scene = make_scene(pkg, bar)
    desc, cubes = scene[2], cube_lights(pkg)
    poses = [bar.pose(20.0), bar.pose(-40.0)]
    fresh = []
    for J in poses:
        h = handle(hip, scene, cubes=cubes)
        h.set_mesh_skin(0, bar.skin, 3); h.set_mesh_pose(0, J)
        fresh.append(through_frames(h, desc, 2))
        h.close()
    r = handle(hip, scene, cubes=cubes)
    r.set_mesh_skin(0, bar.skin, 3)
    got = []
    for J in poses:
        r.set_mesh_pose(0, J)
        got.append(through_frames(r, desc, 2))
    same(got[0], fresh[0])
    same(got[1], fresh[1])
    for k in (2, 3, 4):                                                               # the sun's map and both lights' faces did change
        assert not np.array_equal(got[0][k], got[1][k])
    r.set_mesh_pose(0, None)                                                          # ... and the way back to the bind pose is a change too
    plain = handle(hip, scene, cubes=cubes)
    same(through_frames(r, desc, 2), through_frames(plain, desc, 2))
    r.close(); plain.close()


# ---- frames in flight ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [2, 3])
def test_frames_in_flight_alternating_poses(pkg, hip, in_flight):
    """eight frames, each enqueued behind a new pose without a flush in between: k_skin must follow the prepass that still reads the buffer it
    overwrites and precede the next one, whichever stream that runs on"""
    import torch
    bar = Bar(pkg, 3)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    poses = [bar.pose(30.0), bar.pose(-30.0, move=(0.0, 0.5, 0.0))]
    alone = []
    for J in poses:
        h = handle(hip, scene, frames_in_flight=1)
        h.set_mesh_skin(0, bar.skin, 3); h.set_mesh_pose(0, J)
        alone.append(h.render_frame(desc, SETTINGS).copy())
        h.close()
    assert not np.array_equal(alone[0], alone[1])
    r = handle(hip, scene, frames_in_flight=in_flight)
    r.set_mesh_skin(0, bar.skin, 3)
    descs = []
    for k in range(8):                                                                # the camera moves a little as well: no frame is a repeat
        d = copy.deepcopy(desc)
        d.camera["eye"] = (0.05 * k, 2.5, 7.0)
        descs.append(d)
    outs = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    for k in range(8):
        r.set_mesh_pose(0, poses[k % 2])
        r.render_frame_device(descs[k], SETTINGS, outs[k].data_ptr())
    r.flush()
    got = [o.cpu().numpy() for o in outs]
    r.close()
    h = handle(hip, scene, frames_in_flight=1)
    h.set_mesh_skin(0, bar.skin, 3)
    for k in range(8):
        h.set_mesh_pose(0, poses[k % 2])
        np.testing.assert_array_equal(got[k], h.render_frame(descs[k], SETTINGS), err_msg=f"frame {k}")
    np.testing.assert_array_equal(got[0], alone[0])
    h.set_mesh_pose(0, poses[1])
    np.testing.assert_array_equal(h.render_frame(descs[0], SETTINGS), alone[1])
    h.close()


def test_frames_in_flight_on_a_callers_stream(pkg, hip):
    """a handle on a caller's stream with three frames in flight: its own stream serves as the second prepass stream.  Eight frames without a flush,
    a new pose before every second one, the sun moved on frames 2, 3 and 6 (the other shadow map, drawn on the shadow stream behind the latest
    k_skin); after frame 4 the handle goes back to its own stream, so the second prepass stream is another one and waits for the latest k_skin
    again.  Every frame is the frame of a handle with one frame in flight on its own stream that is given the same calls."""
    import torch
    bar = Bar(pkg, 3)
    scene = make_scene(pkg, bar)
    poses = [bar.pose(30.0), bar.pose(-30.0, move=(0.0, 0.5, 0.0)), bar.pose(15.0), bar.pose(-45.0, move=(0.0, 0.3, 0.0))]
    descs, sun = [], pkg.scenes.DEFAULT_SUN
    for k in range(8):                                                                # the camera moves a little as well: no frame is a repeat
        d = copy.deepcopy(scene[2])
        d.camera["eye"] = (0.05 * k, 2.5, 7.0)
        if k in (2, 3, 6):
            sun = dict(sun, rotation=(-70.0 + 4.0 * k, 12.0 + 3.0 * k))
        d.sun = sun
        descs.append(d)
    stream = torch.cuda.Stream()
    r = handle(hip, scene, frames_in_flight=3)
    r.set_mesh_skin(0, bar.skin, 3)
    r.set_stream(stream.cuda_stream)
    outs = [torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    for k in range(8):
        if k % 2 == 0:
            r.set_mesh_pose(0, poses[k // 2])
        r.render_frame_device(descs[k], SETTINGS, outs[k].data_ptr())
        if k == 4:
            r.set_stream(None)
    r.flush()
    got = [o.cpu().numpy() for o in outs]
    r.close()
    h = handle(hip, scene, frames_in_flight=1)
    h.set_mesh_skin(0, bar.skin, 3)
    for k in range(8):
        if k % 2 == 0:
            h.set_mesh_pose(0, poses[k // 2])
        np.testing.assert_array_equal(got[k], h.render_frame(descs[k], SETTINGS), err_msg=f"frame {k}")
    h.close()
    for k in range(7):
        assert not np.array_equal(got[k], got[k + 1]), f"frames {k} and {k + 1} are the same"
    assert all((g[..., :3] != 0).any() for g in got)


# ---- skin state----------------------------------------------------------------------------------------------------------------------------
def test_a_skin_without_a_pose_changes_nothing(pkg, hip):
    bar = Bar(pkg, 3)
    scene = make_scene(pkg, bar)
    desc = scene[2]
    plain, skinned = handle(hip, scene), handle(hip, scene)
    skinned.set_mesh_skin(0, bar.skin, 3)
    want_p, want_f = through_passes(plain, desc, 0), through_frames(plain, desc, 0)
    same(through_passes(skinned, desc, 0), want_p)
    same(through_frames(skinned, desc, 0), want_f)
    skinned.set_mesh_pose(0, bar.pose(50.0))
    assert not np.array_equal(through_frames(skinned, desc, 0)[0], want_f[0])
    skinned.set_mesh_pose(0, None)                                                    # the pose cleared
    same(through_frames(skinned, desc, 0), want_f)
    same(through_passes(skinned, desc, 0), want_p)
    skinned.set_mesh_pose(0, bar.pose(50.0))
    skinned.set_mesh_skin(0, None)                                                    # the skin detached while posed
    same(through_frames(skinned, desc, 0), want_f)
    plain.close(); skinned.close()


# ---- glTF ------------------------------------------------------------------------------------------------------------------------------------
def test_gltf_file_end_to_end(pkg, hip, tmp_path):
    """a skinned glTF file written here -> loader -> GltfScene.upload + GltfScene.pose -> frames: the posed vertices are the arbiter's for the
    loader's joint matrices, and the frame is that of a plain mesh made from them"""
    from importlib import import_module
    from gltf_skin_files import write_skinned
    gltf = import_module("arctic_renderer_amd.gltf")
    gltf.build()
    path, rig, _ = write_skinned(tmp_path, parent=False, edit=lambda d: d["nodes"][4].pop("translation"))
    sc = gltf.load(path)
    cam = dict(eye=(0.0, 0.5, 6.0), rotation=(0.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = pkg.scenes.SceneDesc(camera=cam, ambient=0.3, sun=dict(pkg.scenes.DEFAULT_SUN, position=(2.0, 6.0, 12.0), rotation=(-25.0, -100.0)), objects=sc.objects)
    v, idx, mat = sc.meshes[0]
    skin, _, n_joints = sc.mesh_skins[0]
    r = sc.upload(hip.Renderer(W, H, S, 16))
    bind = r.render_frame(desc, SETTINGS).copy()
    frames = []
    for animation, t in ((0, 1.0), (0, 1.6), (1, 0.5), (-1, 0.0)):
        sc.pose(r, animation, t)
        J = sc.joint_matrices(0, animation, t)
        want = R.skin_vertices(v, skin, J)
        assert r.read_mesh_vertices(0, len(v)).tobytes() == want.tobytes()
        plain = hip.Renderer(W, H, S, 16)
        plain.create_material(*sc.materials[0]); plain.create_mesh(want, idx, mat)
        frames.append(r.render_frame(desc, SETTINGS).copy())
        np.testing.assert_array_equal(frames[-1], plain.render_frame(desc, SETTINGS))
        plain.close()
    assert (bind[..., :3] != 0).any() and not np.array_equal(frames[0], bind) and not np.array_equal(frames[0], frames[1])
    with pytest.raises(ValueError, match="CUBICSPLINE"):
        sc.pose(r, 2, 0.0)
    r.close()
