"""Cost of splitting the ray structure again on the device (arctic_ray_scene_resplit, csrc/ray_resplit.hip) on one MI355X; the numbers of
DESIGN.md 6m / profiles/ray_resplit_cost.json.  Config 3 at 3840 x 2160 with the skinned mesh and the moderate motion of DESIGN.md 6l (b)
(tools/ray_refit_time.py): every object shifted, one turned, the skinned mesh bent.

    ray_resplit_time.py cost       (a) one re-split (host wall clock around the call and a flush; device time between torch events) against
                                   arctic_ray_scene_reset + the rebuild of the next query, in the same process
                                   (b) closest hit for the camera rays and for 4 Mi random rays on three trees for that pose: REFITTED (the order of the
                                   rest pose), RE-SPLIT, and BUILT on the host -- with the hits compared bit for bit and the last two structures by bytes
    ray_resplit_time.py kernels    a few re-splits and nothing else: run it under a kernel trace for the per-kernel times

Frames without ray queries against the parent's library: tools/ray_query_time.py's `ab` mode, run as DESIGN.md 6k (b) describes.
Each mode prints one JSON line and, with --out FILE, stores it under its mode in that JSON file.  Clocks are not read: assumed."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry
from ray_query_time import camera_rays, summary, timed_ms
from ray_refit_time import handle, pose, stats

pkg = entry.load_package()
F = np.float32


def moderate_motion(sc, r, rng):
    """DESIGN.md 6l (b)'s motion, from the same generator state"""
    obj = sc.desc.objects
    obj["trs"][:, 12] += rng.uniform(-0.5, 0.5, len(obj)).astype(F)
    obj["trs"][:, 14] += rng.uniform(-0.5, 0.5, len(obj)).astype(F)
    c, s = np.cos(0.5), np.sin(0.5)
    turn = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    obj["trs"][1] = (obj["trs"][1].reshape(4, 4).T.astype(np.float64) @ turn).T.astype(F).reshape(16)
    r.set_mesh_pose(0, pose(0.6, 0.3))


def ray_sets(sc, rng):
    pts = []
    for ob in sc.desc.objects:                                                   # bounds of the rest pose are good enough for the random origins
        v = sc.meshes[int(ob["mesh_idx"])][0]["position"]
        m = ob["trs"].reshape(4, 4).T
        pts.append(v @ m[:3, :3].T + m[:3, 3])
    pts = np.concatenate(pts)
    lo, hi = pts.min(0), pts.max(0)
    n_rand = 4 << 20
    return {"camera_rays_coherent": camera_rays(sc),
            "random_rays_4Mi_incoherent": pkg.scene.make_rays(rng.uniform(lo, hi, (n_rand, 3)).astype(F), rng.normal(size=(n_rand, 3)).astype(F))}


def wall_ms(fn, samples=7, warm=2):
    out = []
    for k in range(warm + samples):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[warm:]


def cost_mode():
    sc = pkg.scenes.config3()
    r = handle(sc, 1)
    r.set_mesh_pose(0, pose(0.0, 0.0))
    r.trace_rays_device(sc.desc, None, 0, None)                                  # the build, for the rest pose
    r.flush()
    rng = np.random.default_rng(11)
    moderate_motion(sc, r, rng)
    sets = ray_sets(sc, rng)
    dev = {name: (torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda(), torch.empty(len(rays) * 16, dtype=torch.uint8, device="cuda")) for name, rays in sets.items()}
    walk = {name: {"rays": len(rays)} for name, rays in sets.items()}
    hits, structure, res = {}, {}, {"config": 3, "size": [sc.width, sc.height]}

    def walks(tree):
        for name, rays in sets.items():
            n, (d_rays, d_hits) = len(rays), dev[name]
            ms = timed_ms(lambda: r.trace_rays_device(sc.desc, d_rays.data_ptr(), n, d_hits.data_ptr()), reps=5)
            walk[name][tree] = dict(summary(ms, n), builds_refits_resplits_so_far=[r.ray_scene_info()[2], r.ray_refit_info()[0], r.ray_resplit_info()[0]])
            hits[name, tree] = d_hits.cpu().numpy().tobytes()

    walks("refitted")                                                            # the first query refits the tree split for the rest pose

    def resplit_and_wait():
        r.ray_scene_resplit(sc.desc)
        r.flush()

    res["resplit_call_and_flush_wall"] = stats(wall_ms(resplit_and_wait))
    res["resplit_device"] = stats(timed_ms(lambda: r.ray_scene_resplit(sc.desc), reps=3))
    res["resplit_info"] = list(r.ray_resplit_info())
    walks("re_split")
    structure["re_split"] = r.read_ray_structure()

    def reset_and_rebuild():
        r.ray_scene_reset()
        r.trace_rays_device(sc.desc, None, 0, None)
        r.flush()

    res["reset_and_rebuild_wall"] = stats(wall_ms(reset_and_rebuild))
    walks("built_for_the_pose")
    structure["built"] = r.read_ray_structure()
    (n1, s1), (n2, s2) = structure["re_split"], structure["built"]
    res["structure_equals_the_host_build"] = bool(s1.tobytes() == s2.tobytes() and n1["skip"].tobytes() == n2["skip"].tobytes() and n1["leaf"].tobytes() == n2["leaf"].tobytes()
                                                  and (n1["bmin"] == n2["bmin"]).all() and (n1["bmax"] == n2["bmax"]).all())
    for name in sets:
        walk[name]["same_hits_bit_for_bit"] = hits[name, "refitted"] == hits[name, "re_split"] == hits[name, "built_for_the_pose"]
        walk[name]["rays_that_hit"] = int((np.frombuffer(hits[name, "built_for_the_pose"], pkg.scene.HIT_DTYPE)["prim"] != 0xFFFFFFFF).sum())
    stored, nodes, builds, depth = r.ray_scene_info()
    res.update(walk=walk, triangles_stored=stored, nodes=nodes, depth=depth, builds=builds, refit_info=list(r.ray_refit_info()))
    r.close()
    return {"mode": "cost", "how": "wall: host clock around the call(s) and arctic_flush, 7 samples after 2 warm-ups; device and walks: torch events on torch's stream around "
            "back-to-back calls (3 re-splits, 5 walks), median of 7 rounds; clocks assumed, not read", "results": res}


def kernels_mode():
    sc = pkg.scenes.config3()
    r = handle(sc, 1)
    r.set_mesh_pose(0, pose(0.0, 0.0))
    r.trace_rays_device(sc.desc, None, 0, None)
    moderate_motion(sc, r, np.random.default_rng(11))
    for k in range(5):
        sc.desc.objects["trs"][0, 12] += F(0.01)
        r.ray_scene_resplit(sc.desc)
    r.flush()
    info = r.ray_resplit_info()
    r.close()
    return {"mode": "kernels", "resplit_info": list(info)}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    mode = args[0]
    result = cost_mode() if mode == "cost" else kernels_mode()
    print(json.dumps(result))
    if out_file:
        doc = json.load(open(out_file)) if os.path.exists(out_file) else {}
        doc[mode] = result
        json.dump(doc, open(out_file, "w"), indent=1)
