"""Cost of following a moving scene with the ray structure (ARCTIC_OPT_RAY_REFIT, csrc/ray_refit.hip) on one MI355X; the numbers of DESIGN.md 6l /
profiles/ray_refit_cost.json.  Config 3 at 3840 x 2160; mesh 0 gets a two-joint skin so that it can be re-posed.

    ray_refit_time.py cost         (a) one query call (one ray, host to host) after one object moved, and after one mesh was re-posed, under option 1
                                   and under option 0 in the same process; the device time of the refit alone (torch events around a query of no rays)
                                   (b) closest hit for the camera rays and for 4 Mi random rays on a tree REFITTED after a moderate motion -- every object
                                   shifted, one turned, the skinned mesh bent -- and on a tree BUILT for that very pose (arctic_ray_scene_reset)
    ray_refit_time.py kernels      a few refits and nothing else: run it under a kernel trace for the per-kernel times of the stages

(c), frames without queries against the parent's library, is tools/ray_query_time.py's `ab` mode run as DESIGN.md 6k (b) describes.
Each mode prints one JSON line and, with --out FILE, stores it under its mode in that JSON file.  Clocks are not read: assumed."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry
from ray_query_time import camera_rays, summary, timed_ms

pkg = entry.load_package()
F = np.float32


def handle(sc, option):
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.set_option("ray_refit", option)
    v = sc.meshes[0][0]
    s = np.zeros(len(v), pkg.scene.SKIN_VERTEX_DTYPE)
    x = v["position"][:, 0]
    w = ((x - x.min()) / max(float(x.max() - x.min()), 1e-6)).astype(F)
    s["joints"][:, 1] = 1
    s["weights"][:, 0], s["weights"][:, 1] = F(1) - w, w
    r.set_mesh_skin(0, s, 2)
    return r


def pose(angle, lift):
    c, s = np.cos(angle), np.sin(angle)
    m = np.array([[c, -s, 0, 0], [s, c, 0, lift], [0, 0, 1, 0], [0, 0, 0, 1]], F)
    return np.stack([np.eye(4, dtype=F).T.reshape(16), m.T.reshape(16)])


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def cost_mode():
    res = {"config": 3}
    one = pkg.scene.make_rays(np.array([[0, 1, 0]], F), np.array([[0, 0, -1]], F))
    for option in (1, 0):
        sc = pkg.scenes.config3()
        res["size"] = [sc.width, sc.height]
        r = handle(sc, option)
        r.set_mesh_pose(0, pose(0.0, 0.0))
        t0 = time.perf_counter()
        r.trace_rays(sc.desc, one)
        first = (time.perf_counter() - t0) * 1e3
        moved, posed, device = [], [], []
        for k in range(9):
            sc.desc.objects["trs"][0, 12] += F(0.01)
            t0 = time.perf_counter()
            r.trace_rays(sc.desc, one)
            moved.append((time.perf_counter() - t0) * 1e3)
        for k in range(9):
            r.set_mesh_pose(0, pose(0.02 * (k + 1), 0.01 * k))
            t0 = time.perf_counter()
            r.trace_rays(sc.desc, one)
            posed.append((time.perf_counter() - t0) * 1e3)
        if option == 1:
            def nudge():
                sc.desc.objects["trs"][0, 13] += F(0.001)
                r.trace_rays_device(sc.desc, None, 0, None)             # no ray: the refit alone, enqueued
            device = timed_ms(nudge, reps=5)
        stored, nodes, builds, depth = r.ray_scene_info()
        res["option_%d" % option] = {"first_query_ms": round(first, 2), "query_after_an_object_moved": stats(moved[2:]), "query_after_a_mesh_was_reposed": stats(posed[2:]),
                                     "builds": builds, "refit_info": list(r.ray_refit_info()), "triangles_stored": stored, "nodes": nodes}
        if device:
            res["option_1"]["refit_alone_device_ms"] = stats(device)
        if option == 1:
            res["walk"] = walk_cost(sc, r)
        r.close()
    try:
        parent = json.load(open(os.path.join(ROOT, "profiles", "ray_query_cost.json")))["trace"]["results"]["structure"]["host_build_ms"]
    except Exception:
        parent = None
    res["parent_recorded_host_build_ms"] = parent
    return {"mode": "cost", "how": "query calls: host wall clock around arctic_trace_rays with one ray (it synchronises), 7 samples after 2 warm-ups; refit alone and walks: "
            "torch events on torch's stream around 5 back-to-back calls, median of 7 rounds; clocks assumed, not read", "results": res}


def walk_cost(sc, r):
    """(b): the same rays on a tree refitted to a moved pose and on a tree built for it"""
    rng = np.random.default_rng(11)
    obj = sc.desc.objects
    obj["trs"][:, 12] += rng.uniform(-0.5, 0.5, len(obj)).astype(F)             # every object shifted by up to half a metre
    obj["trs"][:, 14] += rng.uniform(-0.5, 0.5, len(obj)).astype(F)
    c, s = np.cos(0.5), np.sin(0.5)
    turn = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    obj["trs"][1] = (obj["trs"][1].reshape(4, 4).T.astype(np.float64) @ turn).T.astype(F).reshape(16)
    r.set_mesh_pose(0, pose(0.6, 0.3))
    tris = []
    for ob in obj:                                                               # bounds of the rest pose are good enough for the random origins
        v = sc.meshes[int(ob["mesh_idx"])][0]["position"]
        m = ob["trs"].reshape(4, 4).T
        tris.append(v @ m[:3, :3].T + m[:3, 3])
    pts = np.concatenate(tris)
    lo, hi = pts.min(0), pts.max(0)
    n_rand = 4 << 20
    sets = {"camera_rays_coherent": camera_rays(sc),
            "random_rays_4Mi_incoherent": pkg.scene.make_rays(rng.uniform(lo, hi, (n_rand, 3)).astype(F), rng.normal(size=(n_rand, 3)).astype(F))}
    out = {name: {"rays": len(rays)} for name, rays in sets.items()}
    dev = {name: (torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda(), torch.empty(len(rays) * 16, dtype=torch.uint8, device="cuda")) for name, rays in sets.items()}
    hits = {}
    for tree in ("refitted", "built_for_the_pose"):                              # the handle's tree was split for the rest pose; the first query below refits it
        if tree == "built_for_the_pose":
            r.ray_scene_reset()
        for name, rays in sets.items():
            n, (d_rays, d_hits) = len(rays), dev[name]
            ms = timed_ms(lambda: r.trace_rays_device(sc.desc, d_rays.data_ptr(), n, d_hits.data_ptr()), reps=5)
            out[name][tree] = dict(summary(ms, n), builds_and_refits_so_far=[r.ray_scene_info()[2], r.ray_refit_info()[0]])
            hits[name, tree] = d_hits.cpu().numpy().tobytes()
    for name in sets:
        out[name]["same_hits_bit_for_bit"] = hits[name, "refitted"] == hits[name, "built_for_the_pose"]
        out[name]["rays_that_hit"] = int((np.frombuffer(hits[name, "refitted"], pkg.scene.HIT_DTYPE)["prim"] != 0xFFFFFFFF).sum())
    return out


def kernels_mode():
    sc = pkg.scenes.config3()
    r = handle(sc, 1)
    r.set_mesh_pose(0, pose(0.0, 0.0))
    r.trace_rays_device(sc.desc, None, 0, None)
    for k in range(20):
        r.set_mesh_pose(0, pose(0.02 * (k + 1), 0.0))
        sc.desc.objects["trs"][0, 12] += F(0.01)
        r.trace_rays_device(sc.desc, None, 0, None)
    r.flush()
    info = r.ray_refit_info()
    r.close()
    return {"mode": "kernels", "refit_info": list(info)}


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
