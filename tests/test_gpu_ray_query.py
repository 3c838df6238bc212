"""Ray queries on the device (needs an MI355X): arctic_trace_rays / arctic_trace_rays_device / arctic_trace_sun_visibility / arctic_ray_scene_info.

The answer to a ray is DEFINED bit for bit (include/arctic_hip.h, "ray queries"; tests/ray_reference.py is the numpy arbiter, pinned by
tests/test_ray_reference.py), so every comparison here is of bytes: the device's hits against the arbiter's loop over every triangle of the
scene, for the smallest shapes at which the kernel can still go wrong -- 1, 4 and 5 triangles (one leaf, a full leaf, the first split), 1000 (a
tree of 511 nodes, depth 9) in one to three objects with transforms of their own; 1, 63, 64, 65, 257 and 1000 rays (a lane, a wave short of one,
a wave, a wave and a lane, a workgroup and a lane, four workgroups).

These rays come from soup_rays, a quarter of which have a zero direction component, so nearly every wave here takes the walk that looks for
0 * inf.  tests/test_gpu_ray_paths.py has the per-wave cases: waves without such a ray, edge rays, subnormal directions, the sun's grid tails.
The scenes are tests/ray_scenes.py's, shared with that file."""
import numpy as np
import pytest

import ray_reference as R
from ray_scenes import Scene, soup_meshes, transforms   # noqa: F401 (the refit and re-split tests import the latter two from this module)

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
TRI_COUNTS = [1, 4, 5, 1000]
RAY_COUNTS = [1, 63, 64, 65, 257, 1000]


@pytest.fixture(scope="module")
def scenes(pkg, hip):
    made = {}

    def get(n_tris):
        if n_tris not in made:
            made[n_tris] = Scene(pkg, hip, n_tris)
        return made[n_tris]
    yield get
    for s in made.values():
        s.r.close()


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
@pytest.mark.parametrize("n_tris", TRI_COUNTS)
def test_device_matches_the_arbiter_bit_for_bit(scenes, n_tris, n_rays):
    s = scenes(n_tris)
    rays, want = s.case(n_rays)
    for any_hit in (False, True):
        got = s.r.trace_rays(s.desc, rays, any_hit=any_hit)
        assert got.tobytes() == want[any_hit].tobytes(), any_hit
    stored, nodes, builds, depth = s.r.ray_scene_info()
    assert builds == 1 and stored <= len(s.tris) and (depth >= 9 if n_tris == 1000 else depth <= 2)
    if n_tris > 1:
        assert s.n_prims == n_tris + 1 and len(s.tris) == n_tris                         # the triangle with the bad index took a number
    if n_rays >= 63:
        hit = want[False]["prim"] != NONE
        assert hit.sum() * 4 >= n_rays and (want[False]["prim"][hit] < s.n_prims).all()   # not vacuous
        assert ((want[True]["prim"] == 0) == hit).all()


def test_the_large_case_has_ties_and_a_tree(scenes):
    s = scenes(1000)
    rays, want = s.case(1000)
    hit, tie = R.tied(s.tris, rays)
    assert tie.sum() >= 1 and s.r.ray_scene_info()[1] > 255
    assert len(np.unique(want[False]["prim"][hit] // 334)) >= 3                            # every object is hit


@pytest.mark.parametrize("n_tris", TRI_COUNTS)
def test_device_buffers_through_torch(scenes, hip, n_tris):
    import torch
    s = scenes(n_tris)
    for n_rays in (65, 1000):
        rays, want = s.case(n_rays)
        d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
        for any_hit in (False, True):
            d_hits = torch.full((n_rays * 16,), 0xCD, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            s.r.trace_rays_device(s.desc, d_rays.data_ptr(), n_rays, d_hits.data_ptr(), any_hit=any_hit)
            s.r.flush()
            assert d_hits.cpu().numpy().tobytes() == want[any_hit].tobytes()
    with pytest.raises(hip.ArcticError) as e:
        s.r.trace_rays_device(s.desc, d_rays.data_ptr() + 4, 1, d_hits.data_ptr())      # not 16-byte aligned: refused, nothing launched
    assert e.value.code == -1


def test_an_empty_scene_misses_every_ray(pkg, hip):
    r = hip.Renderer(64, 64, 64, 16)
    desc = pkg.scenes.SceneDesc(camera=dict(eye=(0, 0, 9), rotation=(0, -90), aspect=1.0, fov_y=60.0, z_near_far=(0.1, 50.0)), ambient=0.1,
                                sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([]))
    rays = R.soup_rays(np.random.default_rng(1), R.soup_triangles(np.random.default_rng(2), 8), 257)
    for any_hit in (False, True):
        got = r.trace_rays(desc, rays, any_hit=any_hit)
        assert (got["prim"] == NONE).all() and not got["t"].any() and not got["u"].any() and not got["v"].any()
    assert r.ray_scene_info() == (0, 0, 1, 0)
    assert len(r.trace_rays(desc, rays[:0])) == 0
    with pytest.raises(hip.ArcticError) as e:
        r.trace_sun_visibility(desc, 1e-3)                                               # no G-buffer yet
    assert e.value.code == -4
    r.close()


def test_the_structure_is_cached_and_follows_the_scene(pkg, hip):
    import morph_reference as M
    import skin_reference as S
    Sc = pkg.scenes
    v, i = Sc.box(2.0, 1.0, 1.0, n=3)
    fv, fi = Sc.quad((-6, -1, 6), (12, 0, 0), (0, 0, -12), 2, 2)
    r = hip.Renderer(64, 64, 64, 16)
    r.create_material(*Sc.fallback_textures())
    r.create_mesh(v, i, 0)
    r.create_mesh(fv, fi, 0)
    objs = pkg.scene.make_objects([(transforms()[1], 0), (np.eye(4, dtype=F), 1), (transforms()[2], 0)])
    desc = Sc.SceneDesc(camera=dict(eye=(0, 0, 9), rotation=(0, -90), aspect=1.0, fov_y=60.0, z_near_far=(0.1, 50.0)), ambient=0.1, sun=Sc.DEFAULT_SUN, objects=objs)
    rng = np.random.default_rng(5)

    def check(expect_builds):
        meshes = [(r.read_mesh_vertices(0, len(v)), i), (r.read_mesh_vertices(1, len(fv)), fi)]
        tris, prims = R.world_triangles(desc.objects, meshes)
        rays = R.soup_rays(rng, tris, 257)
        for any_hit in (False, True):
            want = R.brute(tris, rays, any_hit=any_hit, prims=prims)
            assert r.trace_rays(desc, rays, any_hit=any_hit).tobytes() == want.tobytes()
            assert (want["prim"] != NONE).sum() * 4 >= len(rays)
        assert r.ray_scene_info()[2] == expect_builds
        return tris

    base = check(1)
    check(1)                                                                             # nothing changed: the same structure
    desc.objects["trs"][0, 12] += 0.5                                                    # an object moves
    moved = check(2)
    assert moved.tobytes() != base.tobytes()
    check(2)
    # morph targets and weights
    d = np.zeros((2, len(v)), M.MORPH_DTYPE)
    d["position"][0] = rng.uniform(-0.2, 0.2, (len(v), 3)).astype(F)
    d["position"][1, :, 1] = 0.5
    r.set_mesh_morph_targets(0, d)
    check(3)                                                                             # (all weights zero: the mesh's own vertices, but a targets call counts)
    r.set_mesh_morph_weights(0, [0.75, -0.5])
    morphed = check(4)
    assert morphed.tobytes() != moved.tobytes()
    check(4)
    # a skin and a pose on top (morph first, then skin)
    s = np.zeros(len(v), S.SKIN_DTYPE)
    s["joints"][:, 1] = 1
    w = ((v["position"][:, 0] + 1.0) / 2.0).astype(F)
    s["weights"][:, 0], s["weights"][:, 1] = F(1) - w, w
    r.set_mesh_skin(0, s, 2)
    check(5)
    lift = np.eye(4, dtype=F); lift[1, 3] = 0.8; lift[0, 1] = 0.25
    r.set_mesh_pose(0, np.stack([np.eye(4, dtype=F).T.reshape(16), lift.T.reshape(16)]))
    posed = check(6)
    assert posed.tobytes() != morphed.tobytes()
    r.set_mesh_pose(0, None)
    assert check(7).tobytes() == morphed.tobytes()
    # the object list shrinks: the floor alone
    desc.objects = desc.objects[1:2].copy()
    assert len(check(8)) == len(fi) // 3
    r.close()


def sun_case(pkg, hip, cfg, scale, bias, rows=None):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    kw = {} if rows is None else dict(row_begin=rows[0], row_end=rows[1])
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    r.pass_gbuffer(sc.desc)
    mask = r.trace_sun_visibility(sc.desc, bias)
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    r.close()
    return sc, mask, attrs, mat


# config 1 and config 3 at the sizes tests/test_gpu_parity.py renders them; bias = 1 mm on scenes of metres
@pytest.mark.parametrize("cfg,scale", [(1, 0.5), (3, 0.1)])
def test_sun_visibility_equals_the_arbiter_byte_for_byte(pkg, hip, cfg, scale):
    bias = 1e-3
    sc, mask, attrs, mat = sun_case(pkg, hip, cfg, scale, bias)
    assert mask.shape == (sc.height, sc.width) and mask.dtype == np.uint8
    tris, prims = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    sun = pkg.renderer.frame_constants(sc.desc)[2]
    rays = R.sun_rays(attrs, sun, bias)
    covered = mat.reshape(-1) != NONE
    assert covered.any() and (cfg != 1 or not covered.all())                             # (config 3 is an interior: every pixel has geometry; config 1 has sky)
    # the arbiter: its pruned walk for every covered pixel (tests/test_ray_reference.py shows it is the loop over every triangle) ...
    hits, _ = R.walk(R.build_bvh(tris, prims), rays[covered], any_hit=True)
    want = np.full(sc.height * sc.width, 255, np.uint8)                                  # a pixel without geometry is 255
    want[covered] = np.where(hits["prim"] == 0, 0, 255)
    assert mask.reshape(-1).tobytes() == want.tobytes()
    # ... and the loop itself for a sample of them
    pick = np.random.default_rng(cfg).choice(np.nonzero(covered)[0], 512, replace=False)
    loop = R.brute(tris, rays[pick], any_hit=True, prims=prims)
    assert (np.where(loop["prim"] == 0, 0, 255) == mask.reshape(-1)[pick]).all()
    occluded = (want[covered] == 0).mean()
    print(f"config {cfg} x{scale}: {covered.sum()} covered pixels, {100 * occluded:.2f} % occluded")
    assert 0.05 <= occluded <= 0.95                                                      # both answers are there
    assert (mask.reshape(-1)[~covered] == 255).all()
    # a row-range shard answers for its own rows (a range that cuts 8-row tiles at both ends)
    lo, hi = 13, sc.height - 19
    _, part, _, _ = sun_case(pkg, hip, cfg, scale, bias, rows=(lo, hi))
    assert part.shape == (hi - lo, sc.width) and part.tobytes() == mask[lo:hi].tobytes()


def test_sun_visibility_from_a_frame_and_left_on_the_device(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.pass_gbuffer(sc.desc)
    want = r.trace_sun_visibility(sc.desc, 1e-3)
    r.render_frame(sc.desc, sc.settings)                     # shaded from the visibility plane: the G-buffer is resolved on demand
    assert r.trace_sun_visibility(sc.desc, 1e-3, read=False) is None
    assert r.trace_sun_visibility(sc.desc, 1e-3).tobytes() == want.tobytes()
    assert r.ray_scene_info()[2] == 1
    with pytest.raises(hip.ArcticError) as e:
        r.trace_sun_visibility(sc.desc, float("nan"))
    assert e.value.code == -1
    r.close()
