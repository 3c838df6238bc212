"""The re-split of the ray structure on the device (needs an MI355X): arctic_ray_scene_resplit, arctic_ray_resplit_info -- ray_resplit.hip's
kernels and sorts against the definition in include/arctic_hip.h ("a re-split structure").

Every comparison is of bytes (boxes: of values, the sign of a zero bound is not defined).  After a re-split the device's structure must be the
host arbiter's (arctic_resplit_triangles, which tests/test_ray_resplit_reference.py pins to numpy and to a build of the moved triangles) AND the
one a second handle builds from scratch at that pose; the hits must be the loop's over every triangle of the moved scene.  Stored triangles:
9 (two levels of splits), 257 (65 leaves: more than one treelet of the refit), 16385 (a third refit stage), in two or three objects, the second
of which carries a skipped triangle, so prims are not slot numbers; 64 x 64 handles."""
import numpy as np
import pytest

import ray_reference as R
import ray_refit_reference as RR
from test_gpu_ray_query import soup_meshes, transforms
from test_gpu_ray_refit import CAMERA, brute

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
N_OBJECTS = {9: 3, 257: 2, 16385: 3}
NO_RAYS = np.zeros(0, R.RAY_DTYPE)


def handle(pkg, hip, meshes, refit=1):
    r = hip.Renderer(64, 64, 64, 16)
    r.create_material(*pkg.scenes.fallback_textures())
    for v, i in meshes:
        r.create_mesh(v, i, 0)
    r.set_option("ray_refit", refit)
    return r


def soup_scene(pkg, hip, n_tris, refit=1, extra=()):
    rng = np.random.default_rng(23000 + n_tris)
    n_objects = N_OBJECTS.get(n_tris, 2)
    meshes = soup_meshes(pkg, rng, n_tris, n_objects) + list(extra)
    places = (transforms() + transforms())[:len(meshes)]
    desc = pkg.scenes.SceneDesc(camera=CAMERA, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([(m, k) for k, m in enumerate(places)]))
    return handle(pkg, hip, meshes, refit), desc, meshes


def split_info(r):
    """(device re-splits so far, 1 if the latest call fell back); a device re-split has launched something"""
    count, launches, fell_back, zero = r.ray_resplit_info()
    assert zero == 0 and (launches > 0) == (count > 0)
    return count, fell_back


def move(desc, step):
    """every object turns, scales and shifts, each its own way: the order of the triangles in space changes thoroughly"""
    for k in range(len(desc.objects)):
        ang = 0.9 + 0.7 * k + 1.3 * step
        c, s = np.cos(ang), np.sin(ang)
        turn = np.array([[c, 0, s, 1.5 - 1.25 * k - 0.5 * step], [0, 1.0 + 0.25 * k, 0, 0.75 * step - 0.5], [-s, 0, c, 0.25 + 0.5 * k], [0, 0, 0, 1]])
        desc.objects["trs"][k] = (turn @ desc.objects["trs"][k].reshape(4, 4).T.astype(np.float64)).T.astype(F).reshape(16)


def world(desc, meshes):
    return R.world_triangles(desc.objects, meshes)


def check_hits(pkg, r, desc, meshes, rng, n_rays=257):
    tris, prims = world(desc, meshes)
    live = tris[np.isfinite(tris).all(1)]
    rays = R.soup_rays(rng, live, n_rays)                                                # (with zero direction components and axis-parallel rays)
    assert (rays["direction"] == 0).any(1).sum() >= n_rays // 10
    for any_hit in (False, True):
        want = brute(pkg, tris, prims, rays, any_hit)
        assert r.trace_rays(desc, rays, any_hit=any_hit).tobytes() == want.tobytes(), any_hit
        if not any_hit and len(tris) >= 200:
            assert (want["prim"] != NONE).sum() * 4 >= len(rays)                         # not vacuous
    return tris, prims


def same_as_arbiter(pkg, r, tris_build, tris_now, prims):
    """the device's structure against arctic_resplit_triangles': slots by bytes, boxes by value, skip / leaf exactly"""
    nodes, slots = r.read_ray_structure()
    _, want_nodes, want_slots = pkg.renderer.resplit_triangles(tris_build, tris_now, NO_RAYS, structure=True)
    assert len(nodes) == len(want_nodes) and len(slots) == len(want_slots) == r.ray_scene_info()[0]
    assert (nodes["skip"] == want_nodes["skip"]).all() and (nodes["leaf"] == want_nodes["leaf"]).all()
    assert (slots["prim"] == prims[want_slots["prim"]]).all() and not slots["pad"].any()
    for f in ("p0", "p1", "p2"):
        assert slots[f].tobytes() == want_slots[f].tobytes(), f
    assert (nodes["bmin"] == want_nodes["bmin"]).all() and (nodes["bmax"] == want_nodes["bmax"]).all()
    return nodes, slots


def same_structure(a, b):
    (nodes, slots), (wn, ws) = a, b
    assert slots.tobytes() == ws.tobytes() and nodes["skip"].tobytes() == wn["skip"].tobytes() and nodes["leaf"].tobytes() == wn["leaf"].tobytes()
    assert (nodes["bmin"] == wn["bmin"]).all() and (nodes["bmax"] == wn["bmax"]).all()


def refitted_in_place(nodes, slots, order_nodes, order_slots, tris_now, prims):
    """arctic_refit_triangles' definition applied to the order a re-split left: the prims stay where they are, every slot is its prim's triangle
    now, every box the union below it"""
    by_prim = np.full((int(prims.max()) + 1, 9), np.nan, F)
    by_prim[prims] = tris_now
    return RR.check_structure(nodes, slots, order_nodes, order_slots, by_prim)


@pytest.mark.parametrize("n_tris", [9, 257, 16385])
def test_a_resplit_is_a_fresh_build_of_the_moved_scene(pkg, hip, n_tris):
    r, desc, meshes = soup_scene(pkg, hip, n_tris)
    rng = np.random.default_rng(n_tris)
    built, prims = check_hits(pkg, r, desc, meshes, rng)                                 # 1. the first query builds
    assert len(built) == n_tris and r.ray_scene_info()[2] == 1 and r.ray_resplit_info() == (0, 0, 0, 0)
    if n_tris > 9:
        assert not (prims == np.arange(n_tris)).all()                                    # (the skipped triangle took a prim number)
    move(desc, 0)                                                                        # 2. the scene moves; the structure is split again
    r.ray_scene_resplit(desc)
    count, launches, fell_back, zero = r.ray_resplit_info()
    assert (count, fell_back, zero) == (1, 0, 0) and launches > 0
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 0                      # neither a build nor a refit
    moved, _ = world(desc, meshes)
    nodes, slots = same_as_arbiter(pkg, r, built, moved, prims)                          # 3. the arbiter's structure ...
    _, _, refit_only = pkg.renderer.refit_triangles(built, moved, NO_RAYS, structure=True)
    assert n_tris == 9 or (prims[refit_only["prim"]] != slots["prim"]).any()             # (and not the order a refit would have kept)
    fresh = handle(pkg, hip, meshes)                                                     # 4. ... and the one a second handle builds at this pose
    fresh.trace_rays(desc, NO_RAYS)
    same_structure((nodes, slots), fresh.read_ray_structure())
    check_hits(pkg, r, desc, meshes, rng)                                                # 5. hits: the loop over every triangle of the moved scene
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 0 and r.ray_resplit_info()[0] == 1
    r.pass_gbuffer(desc); fresh.pass_gbuffer(desc)                                       # 6. the sun's mask
    assert r.trace_sun_visibility(desc, 1e-3).tobytes() == fresh.trace_sun_visibility(desc, 1e-3).tobytes()
    fresh.close()
    move(desc, 1)                                                                        # 7. a refit behind the re-split keeps ITS order: the source records moved with the prims
    again, _ = check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_refit_info()[0] == 1 and r.ray_scene_info()[2] == 1
    n2, s2 = r.read_ray_structure()
    assert refitted_in_place(n2, s2, nodes, slots, again, prims) == 0
    r.ray_scene_resplit(desc)                                                            # 8. and a second re-split, of a structure whose order is no longer the build's
    same_as_arbiter(pkg, r, built, again, prims)
    assert r.ray_resplit_info()[:3] == (2, launches, 0)
    r.close()


def test_a_resplit_at_the_builds_own_pose_changes_nothing(pkg, hip):
    r, desc, meshes = soup_scene(pkg, hip, 257)
    r.trace_rays(desc, NO_RAYS)
    before = r.read_ray_structure()
    r.ray_scene_resplit(desc)
    assert split_info(r) == (1, 0) and r.ray_scene_info()[2] == 1
    same_structure(r.read_ray_structure(), before)
    r.close()


def test_skinned_and_morphed_meshes(pkg, hip):
    import morph_reference as M
    import skin_reference as S
    Sc = pkg.scenes
    v, i = Sc.box(2.0, 1.0, 1.0, n=3)
    bv, bi = Sc.box(1.0, 1.5, 1.0, n=2)
    fv, fi = Sc.quad((-6, -1, 6), (12, 0, 0), (0, 0, -12), 3, 3)
    meshes0 = [(v, i), (bv, bi), (fv, fi)]
    r = handle(pkg, hip, meshes0)
    objs = pkg.scene.make_objects([(transforms()[1], 0), (transforms()[2], 1), (np.eye(4, dtype=F), 2)])
    desc = Sc.SceneDesc(camera=CAMERA, ambient=0.1, sun=Sc.DEFAULT_SUN, objects=objs)
    rng = np.random.default_rng(9)
    s = np.zeros(len(v), S.SKIN_DTYPE)                                                    # mesh 0: skinned; mesh 1: morphed
    s["joints"][:, 1] = 1
    w = ((v["position"][:, 0] + 1.0) / 2.0).astype(F)
    s["weights"][:, 0], s["weights"][:, 1] = F(1) - w, w
    r.set_mesh_skin(0, s, 2)
    d = np.zeros((2, len(bv)), M.MORPH_DTYPE)
    d["position"][0] = rng.uniform(-0.3, 0.3, (len(bv), 3)).astype(F)
    d["position"][1, :, 0] = 2.5
    r.set_mesh_morph_targets(1, d)

    def now():
        return [(r.read_mesh_vertices(0, len(v)), i), (r.read_mesh_vertices(1, len(bv)), bi), (fv, fi)]

    built, prims = check_hits(pkg, r, desc, now(), rng)
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[1] == 1
    lift = np.eye(4, dtype=F); lift[1, 3] = 1.8; lift[0, 1] = 0.25; lift[2, 3] = -2.0
    r.set_mesh_pose(0, np.stack([np.eye(4, dtype=F).T.reshape(16), lift.T.reshape(16)]))
    r.set_mesh_morph_weights(1, [0.75, 1.0])
    r.ray_scene_resplit(desc)
    assert split_info(r) == (1, 0) and r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 0
    posed, _ = world(desc, now())
    assert posed.tobytes() != built.tobytes()
    nodes, slots = same_as_arbiter(pkg, r, built, posed, prims)
    check_hits(pkg, r, desc, now(), rng)
    lift[1, 3] = -0.7                                                                    # a pose change, then a weight change: refits of the re-split order
    r.set_mesh_pose(0, np.stack([np.eye(4, dtype=F).T.reshape(16), lift.T.reshape(16)]))
    t2, _ = check_hits(pkg, r, desc, now(), rng)
    assert refitted_in_place(*r.read_ray_structure(), nodes, slots, t2, prims) == 0 and r.ray_refit_info()[0] == 1
    r.set_mesh_morph_weights(1, [-0.5, 0.25])
    t3, _ = check_hits(pkg, r, desc, now(), rng)
    assert refitted_in_place(*r.read_ray_structure(), nodes, slots, t3, prims) == 0 and r.ray_refit_info()[0] == 2
    assert t3.tobytes() != t2.tobytes() != posed.tobytes()
    r.ray_scene_resplit(desc)                                                            # ... and the re-split of that equals the full build a reset forces
    mine = same_as_arbiter(pkg, r, built, t3, prims)
    r.ray_scene_reset()
    r.trace_rays(desc, NO_RAYS)
    assert r.ray_scene_info()[2] == 2
    same_structure(mine, r.read_ray_structure())
    r.close()


def test_back_to_back_with_one_flush_at_the_end(pkg, hip):
    import torch
    r, desc, meshes = soup_scene(pkg, hip, 257)
    rng = np.random.default_rng(8)
    built, prims = check_hits(pkg, r, desc, meshes, rng)
    n_rays, poses, want, d_rays, out = 500, [], [], [], []
    for step in range(2):
        move(desc, step)
        poses.append(desc.objects["trs"].copy())
    for k, pose in enumerate((0, 1, 1)):                                                 # query 0 at pose 0; queries 1 and 2 at pose 1
        desc.objects["trs"][:] = poses[pose]
        tris, _ = world(desc, meshes)
        rays = R.soup_rays(rng, tris, n_rays)
        want.append(R.brute(tris, rays, prims=prims))
        d_rays.append(torch.from_numpy(rays.view(np.uint8).copy()).cuda())
        out.append(torch.full((n_rays * 16,), 0xCD, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    desc.objects["trs"][:] = poses[0]
    r.ray_scene_resplit(desc)                                                            # re-split, query,
    r.trace_rays_device(desc, d_rays[0].data_ptr(), n_rays, out[0].data_ptr())
    desc.objects["trs"][:] = poses[1]
    r.trace_rays_device(desc, d_rays[1].data_ptr(), n_rays, out[1].data_ptr())           # move, query (a refit),
    r.ray_scene_resplit(desc)                                                            # re-split, query: nothing waited in between
    r.trace_rays_device(desc, d_rays[2].data_ptr(), n_rays, out[2].data_ptr())
    r.flush()
    for k in range(3):
        assert out[k].cpu().numpy().tobytes() == want[k].tobytes(), k
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 1 and r.ray_resplit_info()[0] == 2
    same_as_arbiter(pkg, r, built, world(desc, meshes)[0], prims)
    r.close()


def test_fallbacks_build_in_full_and_say_so(pkg, hip):
    rng = np.random.default_rng(3)
    # never built: the call builds
    r, desc, meshes = soup_scene(pkg, hip, 257)
    r.ray_scene_resplit(desc)
    assert r.ray_resplit_info() == (0, 0, 1, 0) and r.ray_scene_info()[2] == 1
    check_hits(pkg, r, desc, meshes, rng)
    # a changed object count
    desc.objects = desc.objects[:1].copy()
    r.ray_scene_resplit(desc)
    assert r.ray_resplit_info() == (0, 0, 1, 0) and r.ray_scene_info()[2] == 2
    tris, prims = check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_scene_info()[2] == 2
    move(desc, 0)                                                                        # ... and from that build on the device does it again
    r.ray_scene_resplit(desc)
    assert split_info(r) == (1, 0) and r.ray_scene_info()[2] == 2
    same_as_arbiter(pkg, r, tris, world(desc, meshes)[0], prims)
    r.close()
    # a mesh that is gone from the scene: the object's mesh_idx names none of the handle's meshes
    r, desc, meshes = soup_scene(pkg, hip, 257)
    check_hits(pkg, r, desc, meshes, rng)
    desc.objects["mesh_idx"][1] = 7
    r.ray_scene_resplit(desc)
    assert r.ray_resplit_info() == (0, 0, 1, 0) and r.ray_scene_info()[2] == 2 and r.ray_refit_info()[1] == 0
    tris, _ = check_hits(pkg, r, desc, meshes, rng)
    assert len(tris) == len(meshes[0][1]) // 3
    r.close()
    # the option at 0: a structure that cannot be refitted
    r, desc, meshes = soup_scene(pkg, hip, 257, refit=0)
    check_hits(pkg, r, desc, meshes, rng)
    move(desc, 0)
    r.ray_scene_resplit(desc)
    assert r.ray_resplit_info() == (0, 0, 1, 0) and r.ray_scene_info()[2] == 2 and r.ray_refit_info() == (0, 0, 0, 0)
    check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_scene_info()[2] == 2
    r.close()


def test_dead_and_back(pkg, hip):
    one = np.zeros(3, pkg.scene.VERTEX_DTYPE)                                            # an object of ONE triangle: its trs decides that triangle alone
    one["position"] = [(-1, -1, 0.5), (1.5, -1, 0.25), (0, 1.5, 0.75)]
    one["normal"], one["tangent"], one["bitangent"] = (0, 1, 0), (1, 0, 0), (0, 0, 1)
    r, desc, meshes = soup_scene(pkg, hip, 256, extra=[(one, np.arange(3, dtype=np.uint32))])
    rng = np.random.default_rng(12)
    built, prims = check_hits(pkg, r, desc, meshes, rng)
    assert len(built) == 257 and len(desc.objects) == 3
    lone = int(prims[-1])
    keep = desc.objects["trs"][2].copy()
    move(desc, 0)
    desc.objects["trs"][2, 13] = np.nan                                                  # the one triangle leaves the finite numbers
    r.ray_scene_resplit(desc)
    assert split_info(r) == (1, 0)
    gone, _ = check_hits(pkg, r, desc, meshes, rng)                                      # hits: brute force, which never reports it
    assert not np.isfinite(gone[-1]).all() and np.isfinite(gone[:-1]).all()    # (its y coordinates are NaN)
    nodes, slots = same_as_arbiter(pkg, r, built, gone, prims)
    at = int(np.nonzero(slots["prim"] == lone)[0][0])
    assert at >= 254                                                                     # behind every live one: in the last leaf (3 slots)
    raw = np.concatenate([slots["p0"], slots["p1"], slots["p2"]], 1).view(np.uint32)
    assert (raw[at] == RR.DEAD_BITS).all() and np.isfinite(np.delete(raw, at, 0).view(F)).all()
    desc.objects["trs"][2] = keep                                                        # a finite pose and a refit: the slot is alive again, where the re-split put it
    back, _ = check_hits(pkg, r, desc, meshes, rng)
    assert r.ray_refit_info()[0] == 1 and r.ray_scene_info()[2] == 1
    n2, s2 = r.read_ray_structure()
    assert refitted_in_place(n2, s2, nodes, slots, back, prims) == 0
    assert s2["prim"][at] == lone and np.concatenate([s2["p0"], s2["p1"], s2["p2"]], 1)[at].tobytes() == back[-1].tobytes()
    r.close()
