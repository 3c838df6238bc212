"""The refit of the ray structure on the device (needs an MI355X): ARCTIC_OPT_RAY_REFIT = 1, arctic_ray_refit_info, arctic_ray_scene_reset,
arctic_read_ray_structure -- ray_refit.hip's kernels against the definition in include/arctic_hip.h ("a refitted structure").

Every comparison is of bytes (boxes: of values, the sign of a zero bound is not defined): the hits after a refit against the loop over every
triangle of the MOVED scene, and the device's structure against the host arbiter arctic_refit_triangles, which tests/test_ray_refit_reference.py
pins to numpy.  Sizes: 1 triangle (one leaf), 5 (a root and two leaves), 257 (65 leaves: two stages), 1000, 16385 (4097 leaves: three stages),
as one to three objects; 64 x 64 handles."""
import numpy as np
import pytest

import ray_reference as R
import ray_refit_reference as RR
from test_gpu_ray_query import soup_meshes, transforms

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
N_OBJECTS = {1: 1, 5: 3, 257: 2, 1000: 3, 16385: 3}
CAMERA = dict(eye=(0, 0, 9), rotation=(0, -90), aspect=1.0, fov_y=60.0, z_near_far=(0.1, 50.0))


def brute(pkg, tris, prims, rays, any_hit):
    """the loop over every triangle: numpy for the small scenes, the library's host loop (pinned to numpy by tests/test_ray_query_abi.py) for 16385"""
    if len(tris) <= 1000:
        return R.brute(tris, rays, any_hit=any_hit, prims=prims)
    h = pkg.renderer.trace_triangles(tris, rays, any_hit=any_hit, brute=True)
    if not any_hit:
        hit = h["prim"] != NONE
        h["prim"][hit] = prims[h["prim"][hit]]                                           # (ascending with the index: ties break the same way)
    return h


def soup_scene(pkg, hip, n_tris, refit=1):
    rng = np.random.default_rng(17000 + n_tris)
    n_objects = N_OBJECTS[n_tris]
    meshes = soup_meshes(pkg, rng, n_tris, n_objects)
    desc = pkg.scenes.SceneDesc(camera=CAMERA, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN,
                                objects=pkg.scene.make_objects([(m, k) for k, m in enumerate(transforms()[:n_objects])]))
    r = hip.Renderer(64, 64, 64, 16)
    r.create_material(*pkg.scenes.fallback_textures())
    for v, i in meshes:
        r.create_mesh(v, i, 0)
    r.set_option("ray_refit", refit)
    return r, desc, meshes


def check_hits(pkg, r, desc, meshes, rng, n_rays=257):
    tris, prims = R.world_triangles(desc.objects, meshes)
    live = tris[np.isfinite(tris).all(1)]
    rays = R.soup_rays(rng, live if len(live) else np.zeros((1, 9), F), n_rays)
    want = {}
    for any_hit in (False, True):
        want[any_hit] = brute(pkg, tris, prims, rays, any_hit)
        assert r.trace_rays(desc, rays, any_hit=any_hit).tobytes() == want[any_hit].tobytes(), any_hit
    return tris, prims, rays, want[False]


def check_structure(pkg, r, tris_build, tris_now, prims):
    """the device's structure against the arbiter's: slots by bytes, boxes by value, skip / leaf exactly"""
    nodes, slots = r.read_ray_structure()
    _, want_nodes, want_slots = pkg.renderer.refit_triangles(tris_build, tris_now, np.zeros(0, R.RAY_DTYPE), structure=True)
    assert len(nodes) == len(want_nodes) and len(slots) == len(want_slots) == r.ray_scene_info()[0]
    assert (nodes["skip"] == want_nodes["skip"]).all() and (nodes["leaf"] == want_nodes["leaf"]).all()
    assert (nodes["bmin"] == want_nodes["bmin"]).all() and (nodes["bmax"] == want_nodes["bmax"]).all()
    assert (slots["prim"] == prims[want_slots["prim"]]).all() and not slots["pad"].any()
    for f in ("p0", "p1", "p2"):
        assert slots[f].tobytes() == want_slots[f].tobytes(), f
    return nodes, slots


@pytest.mark.parametrize("n_tris", [1, 5, 257, 1000, 16385])
def test_a_moved_object_is_followed_by_a_refit(pkg, hip, n_tris):
    r, desc, meshes = soup_scene(pkg, hip, n_tris)
    rng = np.random.default_rng(n_tris)
    built, prims, _, _ = check_hits(pkg, r, desc, meshes, rng)                           # 1. the first query builds
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info() == (0, 1, 0, 0)
    check_structure(pkg, r, built, built, prims)
    k = len(desc.objects) - 1                                                            # 2. an object moves: a turn, a scale and a shift
    c, s = np.cos(0.4), np.sin(0.4)
    turn = np.array([[c, 0, s, 0.5], [0, 1.25, 0, -0.75], [-s, 0, c, 0.25], [0, 0, 0, 1]])
    desc.objects["trs"][k] = (turn @ desc.objects["trs"][k].reshape(4, 4).T.astype(np.float64)).T.astype(F).reshape(16)
    moved, prims2, _, want = check_hits(pkg, r, desc, meshes, rng)
    assert moved.tobytes() != built.tobytes() and (prims2 == prims).all()
    assert (want["prim"] != NONE).sum() * 4 >= len(want)                                 # not vacuous
    refits, refittable, launches, zero = r.ray_refit_info()
    stages = {1: 1, 5: 1, 257: 2, 1000: 2, 16385: 3}[n_tris]
    assert r.ray_scene_info()[2] == 1 and (refits, refittable, launches, zero) == (1, 1, stages, 0)
    check_structure(pkg, r, built, moved, prims)                                         # 3. the structure is the arbiter's
    check_hits(pkg, r, desc, meshes, rng)                                                # 4. nothing changed: nothing counted
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info() == (1, 1, stages, 0)
    r.close()


def test_the_cached_structure_follows_morphs_skins_and_poses_by_refits(pkg, hip):
    """tests/test_gpu_ray_query.py's cached-structure scenario under the option: the same hits, one build, the refits counted"""
    import morph_reference as M
    import skin_reference as S
    Sc = pkg.scenes
    v, i = Sc.box(2.0, 1.0, 1.0, n=3)
    fv, fi = Sc.quad((-6, -1, 6), (12, 0, 0), (0, 0, -12), 2, 2)
    r = hip.Renderer(64, 64, 64, 16)
    r.create_material(*Sc.fallback_textures())
    r.create_mesh(v, i, 0)
    r.create_mesh(fv, fi, 0)
    r.set_option("ray_refit", 1)
    objs = pkg.scene.make_objects([(transforms()[1], 0), (np.eye(4, dtype=F), 1), (transforms()[2], 0)])
    desc = Sc.SceneDesc(camera=CAMERA, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=objs)
    rng = np.random.default_rng(5)

    def check(expect_builds, expect_refits):
        meshes = [(r.read_mesh_vertices(0, len(v)), i), (r.read_mesh_vertices(1, len(fv)), fi)]
        tris, prims = R.world_triangles(desc.objects, meshes)
        rays = R.soup_rays(rng, tris, 257)
        for any_hit in (False, True):
            want = R.brute(tris, rays, any_hit=any_hit, prims=prims)
            assert r.trace_rays(desc, rays, any_hit=any_hit).tobytes() == want.tobytes()
            assert (want["prim"] != NONE).sum() * 4 >= len(rays)
        assert (r.ray_scene_info()[2], r.ray_refit_info()[0]) == (expect_builds, expect_refits)
        return tris, prims

    base, prims = check(1, 0)
    check(1, 0)
    desc.objects["trs"][0, 12] += 0.5                                                    # an object moves
    moved, _ = check(1, 1)
    assert moved.tobytes() != base.tobytes()
    check(1, 1)
    d = np.zeros((2, len(v)), M.MORPH_DTYPE)
    d["position"][0] = rng.uniform(-0.2, 0.2, (len(v), 3)).astype(F)
    d["position"][1, :, 1] = 0.5
    r.set_mesh_morph_targets(0, d)
    check(1, 2)                                                                          # (all weights zero: a targets call counts as a change)
    r.set_mesh_morph_weights(0, [0.75, -0.5])
    morphed, _ = check(1, 3)
    assert morphed.tobytes() != moved.tobytes()
    s = np.zeros(len(v), S.SKIN_DTYPE)
    s["joints"][:, 1] = 1
    w = ((v["position"][:, 0] + 1.0) / 2.0).astype(F)
    s["weights"][:, 0], s["weights"][:, 1] = F(1) - w, w
    r.set_mesh_skin(0, s, 2)
    check(1, 4)
    lift = np.eye(4, dtype=F); lift[1, 3] = 0.8; lift[0, 1] = 0.25
    r.set_mesh_pose(0, np.stack([np.eye(4, dtype=F).T.reshape(16), lift.T.reshape(16)]))
    posed, _ = check(1, 5)
    assert posed.tobytes() != morphed.tobytes()
    check_structure(pkg, r, base, posed, prims)
    r.set_mesh_pose(0, None)
    back, _ = check(1, 6)
    assert back.tobytes() == morphed.tobytes()
    check_structure(pkg, r, base, morphed, prims)
    desc.objects = desc.objects[1:2].copy()                                              # the object list shrinks: a full build
    floor, _ = check(2, 6)
    assert len(floor) == len(fi) // 3 and r.ray_refit_info()[1] == 1
    r.close()


def test_dead_and_back(pkg, hip):
    r, desc, meshes = soup_scene(pkg, hip, 257)
    rng = np.random.default_rng(12)
    built, prims, rays, before = check_hits(pkg, r, desc, meshes, rng)
    first = len(meshes[0][1]) // 3                                                       # object 0's prims: [0, first)
    assert (before["prim"] < first).any() and (before["prim"][before["prim"] != NONE] >= first).any()
    keep = desc.objects["trs"][0, 12]
    desc.objects["trs"][0, 12] = np.inf                                                  # every vertex of object 0 leaves the finite numbers
    gone, _, _, _ = check_hits(pkg, r, desc, meshes, rng)
    assert not np.isfinite(gone[:first]).all(1).any() and np.isfinite(gone[first:]).all()
    for any_hit in (False, True):                                                        # the rays that hit it before: none of its triangles now
        now = r.trace_rays(desc, rays, any_hit=any_hit)
        assert now.tobytes() == brute(pkg, gone, prims, rays, any_hit).tobytes()
    assert not (r.trace_rays(desc, rays)["prim"] < first).any()
    nodes, slots = check_structure(pkg, r, built, gone, prims)
    raw = np.concatenate([slots["p0"], slots["p1"], slots["p2"]], 1).view(np.uint32)
    assert (raw[slots["prim"] < first] == RR.DEAD_BITS).all() and (nodes["bmin"][:, 0] == np.inf).any() and np.isfinite(nodes["bmin"][0]).all()
    assert r.ray_refit_info()[:2] == (1, 1) and r.ray_scene_info()[2] == 1
    desc.objects["trs"][0, 12] = keep                                                    # and back: hit again
    assert r.trace_rays(desc, rays).tobytes() == before.tobytes()
    check_structure(pkg, r, built, built, prims)
    assert r.ray_refit_info()[:2] == (2, 1) and r.ray_scene_info()[2] == 1
    r.close()


def test_a_build_that_left_a_triangle_out_is_not_refittable(pkg, hip):
    rng = np.random.default_rng(21)
    meshes = soup_meshes(pkg, rng, 40, 1)
    meshes[0][0]["position"][7, 1] = np.nan                                              # one triangle with a vertex that is not finite
    desc = pkg.scenes.SceneDesc(camera=CAMERA, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([(transforms()[1], 0)]))
    r = hip.Renderer(64, 64, 64, 16)
    r.create_material(*pkg.scenes.fallback_textures())
    r.create_mesh(*meshes[0], 0)
    r.set_option("ray_refit", 1)
    check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_scene_info()[0] == 39 and r.ray_scene_info()[2] == 1 and r.ray_refit_info() == (0, 0, 0, 0)
    desc.objects["trs"][0, 13] -= 0.5
    check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_scene_info()[2] == 2 and r.ray_refit_info() == (0, 0, 0, 0)             # the change was followed by a full build
    r.close()


def test_scene_reset_and_option_zero(pkg, hip):
    r, desc, meshes = soup_scene(pkg, hip, 1000)
    rng = np.random.default_rng(4)
    with pytest.raises(hip.ArcticError) as e:
        r.set_option("ray_refit", 2)
    assert e.value.code == -1
    with pytest.raises(hip.ArcticError) as e:
        r.read_ray_structure()                                                           # no structure yet
    assert e.value.code == -4
    _, _, rays, _ = check_hits(pkg, r, desc, meshes, rng)
    desc.objects["trs"][1, 14] += 1.5
    moved, prims, _, _ = check_hits(pkg, r, desc, meshes, rng)
    refitted = r.trace_rays(desc, rays)
    assert (r.ray_scene_info()[2], r.ray_refit_info()[0]) == (1, 1)
    r.ray_scene_reset()                                                                  # the next query builds in full; the hits do not change
    assert r.ray_refit_info()[1] == 0
    assert r.trace_rays(desc, rays).tobytes() == refitted.tobytes()
    assert (r.ray_scene_info()[2], r.ray_refit_info()[:2]) == (2, (1, 1))
    check_structure(pkg, r, moved, moved, prims)
    # option 0 from here on: the structure in place was built under 1 and still refits; after a reset everything is as without the feature
    r.set_option("ray_refit", 0)
    desc.objects["trs"][1, 14] -= 0.5
    check_hits(pkg, r, desc, meshes, rng)
    assert (r.ray_scene_info()[2], r.ray_refit_info()[0]) == (2, 2)
    r.ray_scene_reset()
    check_hits(pkg, r, desc, meshes, rng)
    assert (r.ray_scene_info()[2], r.ray_refit_info()) == (3, (2, 0, 2, 0))
    desc.objects["trs"][1, 14] -= 0.5
    check_hits(pkg, r, desc, meshes, rng)
    assert (r.ray_scene_info()[2], r.ray_refit_info()) == (4, (2, 0, 2, 0))              # a full build per change, as ever
    r.close()
    # a handle that never saw the option: the counters tests/test_gpu_ray_query.py expects, and no refit
    r, desc, meshes = soup_scene(pkg, hip, 5, refit=0)
    check_hits(pkg, r, desc, meshes, rng)
    desc.objects["trs"][0, 12] += 0.5
    check_hits(pkg, r, desc, meshes, rng)
    check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_scene_info()[2] == 2 and r.ray_refit_info() == (0, 0, 0, 0)
    r.close()


def test_sun_visibility_after_a_refit_equals_the_arbiter(pkg, hip):
    bias = 1e-3
    sc = pkg.scenes.CONFIGS[1](scale=0.5)
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_option("ray_refit", 1)
    r.pass_gbuffer(sc.desc)
    before = r.trace_sun_visibility(sc.desc, bias)
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[:2] == (0, 1)
    sc.desc.objects["trs"][:, 12] += F(0.375)                                             # the scene moves; the G-buffer is drawn again
    sc.desc.objects["trs"][0, 13] += F(0.25)
    r.pass_gbuffer(sc.desc)
    mask = r.trace_sun_visibility(sc.desc, bias)
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 1
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    tris, prims = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    rays = R.sun_rays(attrs, pkg.renderer.frame_constants(sc.desc)[2], bias)
    covered = mat.reshape(-1) != NONE
    hits, _ = R.walk(R.build_bvh(tris, prims), rays[covered], any_hit=True)
    want = np.full(sc.height * sc.width, 255, np.uint8)
    want[covered] = np.where(hits["prim"] == 0, 0, 255)
    assert mask.reshape(-1).tobytes() == want.tobytes()
    assert 0.05 <= (want[covered] == 0).mean() <= 0.95 and mask.tobytes() != before.tobytes()
    r.close()


def test_device_buffers_after_a_refit_with_one_flush_at_the_end(pkg, hip):
    import torch
    r, desc, meshes = soup_scene(pkg, hip, 1000)
    rng = np.random.default_rng(8)
    check_hits(pkg, r, desc, meshes, rng)
    n_rays, out, want, d_rays, trs = 1000, [], [], [], []
    start = desc.objects["trs"].copy()
    for step in range(3):                                                                # three moves, three refits, three queries: nothing waits in between
        desc.objects["trs"][step, 12 + step] += F(0.625)
        trs.append(desc.objects["trs"].copy())
        tris, prims = R.world_triangles(desc.objects, meshes)
        rays = R.soup_rays(rng, tris, n_rays)
        want.append(R.brute(tris, rays, prims=prims))
        d_rays.append(torch.from_numpy(rays.view(np.uint8).copy()).cuda())
        out.append(torch.full((n_rays * 16,), 0xCD, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    desc.objects["trs"][:] = start
    for step in range(3):
        desc.objects["trs"][:] = trs[step]
        r.trace_rays_device(desc, d_rays[step].data_ptr(), n_rays, out[step].data_ptr())
    r.flush()
    for step in range(3):
        assert out[step].cpu().numpy().tobytes() == want[step].tobytes(), step
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[:2] == (3, 1)
    r.close()
