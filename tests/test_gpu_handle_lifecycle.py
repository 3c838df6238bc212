"""What a handle owns, on the device (needs an MI355X): meshes that hold device buffers, pinned rings and events are MOVED when the handle's mesh
list grows, and everything a handle ever allocated goes when it is closed -- streams first (csrc/device_resources.h, DESIGN.md "Ownership").

Moving and the order of destruction are what can go wrong on a device; the owners' own rules (what is released, once; which runtime calls a ring
makes) are checked on the CPU by tests/test_device_resources.py.  Neither test measures free device memory: that figure belongs to everybody on
the machine.  64 x 64 target, 64^2 shadow map, a bar of 48 triangles and a floor of 8."""
import copy

import numpy as np
import pytest

import morph_reference as M
import skin_reference as R
from test_gpu_morph import Bar

pytestmark = pytest.mark.gpu

W = H = S = 64
SETTINGS = (2, 2.2, 1.0)
F = np.float32


def small_scene(pkg):
    Sc = pkg.scenes
    rng = np.random.default_rng(11)
    bar = Bar(pkg, n=2)
    mats = [Sc.make_material_textures(rng, 16), Sc.make_material_textures(rng, 16)]
    meshes = [(bar.vertices, bar.indices, 0), Sc.quad((-8, 0, 8), (16, 0, 0), (0, 0, -16), 2, 2) + (1,)]
    cam = dict(eye=(0.0, 2.5, 7.0), rotation=(-8.0, -90.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = Sc.SceneDesc(camera=cam, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=pkg.scene.make_objects([(np.eye(4, dtype=F), 0), (np.eye(4, dtype=F), 1)]))
    lights = pkg.scene.make_lights([(1.5, 3.0, 2.0), (-2.0, 2.0, 1.0)], [(8.0, 6.0, 4.0), (3.0, 5.0, 8.0)])
    assert len(bar.indices.ravel()) // 3 == 48
    return bar, mats, meshes, desc, lights


def deform(r, bar, pose, weights, times=1):
    for _ in range(times):
        r.set_mesh_pose(0, pose)
        r.set_mesh_morph_weights(0, weights)


def test_meshes_survive_the_growth_of_the_mesh_list(pkg, hip):
    """mesh 0 is skinned, posed and morphed, with all three slots of both rings pending; nine more meshes make the list reallocate; the next pose and
    weights take a slot that was filled before the move, and nothing the frame or the vertex buffer shows has changed"""
    bar, mats, meshes, desc, lights = small_scene(pkg)
    r = hip.Renderer(W, H, S, 16)
    for m in mats:
        r.create_material(*m)
    for v, i, mat in meshes:
        r.create_mesh(v, i, mat)
    r.update_lights(lights)
    pose, weights = bar.pose(30.0), np.array([0.7, -0.3], F)
    r.set_mesh_skin(0, bar.skin, 3)
    r.set_mesh_morph_targets(0, bar.deltas)
    deform(r, bar, pose, weights, times=3)                                               # slots 0, 1, 2 of the joint ring and of the weight ring
    before, v_before = r.render_frame(desc, SETTINGS).copy(), r.read_mesh_vertices(0, len(bar.vertices))
    want = R.skin_vertices(M.morph_vertices(bar.vertices, bar.deltas, weights), bar.skin, pose)
    assert v_before.tobytes() == want.tobytes() and v_before.tobytes() != bar.vertices.tobytes()
    assert len(np.unique(before.reshape(-1, 4), axis=0)) > 16                           # (a picture, not a clear colour)
    spare = pkg.scenes.quad((-1, 5, 0), (1, 0, 0), (0, 1, 0), 2, 2)
    for k in range(9):                                                                   # 2 -> 11 meshes: the list's storage moves (more than once)
        assert r.create_mesh(spare[0], spare[1], k % 2) == 2 + k
    deform(r, bar, pose, weights)                                                        # slot 0 again: waits for its own event, in its moved owner
    after, v_after = r.render_frame(desc, SETTINGS), r.read_mesh_vertices(0, len(bar.vertices))
    assert v_after.tobytes() == v_before.tobytes()
    assert after.tobytes() == before.tobytes()
    r.flush()
    r.close()


def everything_once(pkg, hip):
    """one handle through every family of lazily allocated resources, then closed; returns what it produced on the way"""
    Sc = pkg.scenes
    bar, mats, meshes, desc, lights = small_scene(pkg)
    out = {}
    r = hip.Renderer(W, H, S, 16)
    r.set_option("texture_mips", 1)                                                      # chains and their level tables
    for m in mats:
        r.create_material(*m)
    for v, i, mat in meshes:
        r.create_mesh(v, i, mat)
    r.update_lights(lights)
    # the tile order and the tile trace first: the trace is refused once mip chains, extras, an environment or point shadows take part in the shading
    r.set_option("texture_mips", 0)
    r.set_option("tile_order", 1)
    r.set_option("tile_trace", 1)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)                                                                 # tile classes, order lists, the order
    r.pass_shade(desc, SETTINGS)                                                         # the tile trace
    out["passes"] = r.read_output(want=("rgba8",))[2].copy()
    order, classes = r.tile_order()
    out["order"], out["classes"] = order.copy(), classes.copy()
    assert r.tile_trace().shape == (H // 8, W // 8, 4) and r.tile_trace().any()
    r.set_option("tile_trace", 0)
    r.set_option("texture_mips", 1)
    rng = np.random.default_rng(5)
    params = np.zeros(1, pkg.scene.MATERIAL_PARAMS_DTYPE)
    params["base_color_factor"], params["metallic_factor"], params["roughness_factor"], params["normal_scale"] = (0.9, 0.8, 0.7), 0.5, 0.75, 1.0
    params["occlusion_strength"], params["emissive_factor"] = 0.5, (0.5, 0.25, 1.0)
    r.set_material_extras(0, params, emissive=rng.integers(0, 256, (16, 16, 4), np.uint8))                                    # the packed image
    r.set_material_extras(1, None, emissive=rng.integers(0, 256, (8, 8, 4), np.uint8), occlusion=rng.integers(0, 256, (4, 8, 4), np.uint8))   # two plain ones
    r.create_hdri(Sc.synthetic_hdri(w=32, h=16))
    r.set_option("env_lighting", 1)
    cube = np.zeros(1, pkg.scene.POINT_SHADOW_LIGHT_DTYPE)
    cube["position"], cube["color"], cube["z_near"], cube["z_far"] = [(0.5, 4.0, 1.0)], [(6, 6, 6)], 0.05, 30.0
    r.set_option("point_shadow_size", 8)                                                 # the smallest cube
    r.update_point_shadow_lights(cube)
    r.set_mesh_skin(0, bar.skin, 3)
    r.set_mesh_morph_targets(0, bar.deltas)
    deform(r, bar, bar.pose(20.0), np.array([0.5, 0.25], F))
    r.set_option("antialias", 1)
    r.set_option("frames_in_flight", 3)
    out["frames"] = [r.render_frame(desc, SETTINGS).copy() for _ in range(4)]            # 3 frames in flight, 4 frames: every set and both prepass streams
    r.set_option("ray_refit", 1)
    rays = np.zeros(64, pkg.scene.RAY_DTYPE)
    rays["origin"], rays["t_max"] = (0.0, 6.0, 0.5), np.inf
    rays["direction"] = np.stack([np.linspace(-0.8, 0.8, 64), np.full(64, -1.0), np.tile([0.1, -0.1], 32)], 1)
    out["hits"] = [r.trace_rays(desc, rays).copy()]
    moved = copy.deepcopy(desc)
    moved.objects["trs"][0][12:15] += F(0.5)                                             # the bar shifts: the structure is refitted ...
    out["hits"].append(r.trace_rays(moved, rays).copy())
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 1
    moved.objects["trs"][0][12:15] -= F(1.25)
    r.ray_scene_resplit(moved)                                                           # ... and split again
    assert r.ray_resplit_info()[0] == 1 and r.ray_resplit_info()[2] == 0
    out["hits"].append(r.trace_rays(moved, rays).copy())
    assert (out["hits"][0]["prim"] != 0xFFFFFFFF).any() and out["hits"][0].tobytes() != out["hits"][2].tobytes()
    dirs = pkg.renderer.ao_directions(4, 2)                                              # (the frames left no G-buffer: it is resolved under the tile order)
    out["ao"] = r.trace_ambient_occlusion(moved, dirs, radius=3.0, filter=True).copy()   # table, hits plane, result
    assert out["ao"].min() < 255
    r.flush()
    r.close()
    return out


def test_everything_allocated_then_destroyed_twice_over(pkg, hip):
    """a handle that used every option that allocates -- the tile order and tile trace among them -- is closed, and a second handle of the same
    description in the same process produces the first one's bytes, from the first frame on"""
    a = everything_once(pkg, hip)
    b = everything_once(pkg, hip)
    assert len(np.unique(a["frames"][0].reshape(-1, 4), axis=0)) > 16
    assert b["frames"][0].tobytes() == a["frames"][0].tobytes()
    for x, y in zip(a["frames"] + a["hits"] + [a["passes"], a["order"], a["classes"], a["ao"]], b["frames"] + b["hits"] + [b["passes"], b["order"], b["classes"], b["ao"]]):
        assert x.tobytes() == y.tobytes()
