"""Cost of the ray queries (arctic_trace_rays / arctic_trace_sun_visibility, csrc/trace.hip) on one MI355X; the numbers of DESIGN.md 6k /
profiles/ray_query_cost.json.

    ray_query_time.py trace        config 3 at 3840 x 2160: the structure (triangles, nodes, depth, host build time); closest hit for the camera rays
                                   through the pixel centres (coherent) and for 8 Mi uniformly random rays inside the scene's bounds (incoherent),
                                   any hit for the same two sets, the sun mask from the resident G-buffer; nodes fetched and triangles tested per ray
                                   from the reference walk (tests/ray_reference.py: the same median-split tree) on a sample of the same rays
    ray_query_time.py ab LABEL     config 3 whole frames, no ray query anywhere, with the library ARCTIC_HIP_LIBRARY names (default: this tree's); run it
                                   in separate processes for this tree, for a library built from the parent commit (ARCTIC_HIP_LIBRARY_OLDER=1) and for
                                   that parent library once more -- the control that shows the noise --, the three alternating

Each mode prints one JSON line and, with --out FILE, stores it under its mode (ab: its label) in that JSON file."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry

pkg = entry.load_package()


def timed_ms(fn, reps, rounds=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def summary(ms, n_rays):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "Mrays_per_s": round(n_rays / med / 1e3, 1)}


def camera_rays(sc):
    """one ray per pixel centre from the eye: the directions that unproject the centres through the library's own proj_view (binary64, rounded once)"""
    pv = pkg.renderer.frame_constants(sc.desc)[0].astype(np.float64).T            # [col][row] -> a math matrix
    inv = np.linalg.inv(pv)
    x = (np.arange(sc.width) + 0.5) / sc.width * 2 - 1
    y = 1 - (np.arange(sc.height) + 0.5) / sc.height * 2
    X, Y = np.meshgrid(x, y)
    far = np.stack([X, Y, np.ones_like(X), np.ones_like(X)], -1) @ inv.T
    far = far[..., :3] / far[..., 3:]
    eye = np.asarray(sc.desc.camera["eye"], np.float64)
    d = far - eye
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return pkg.scene.make_rays(np.broadcast_to(eye, d.shape).reshape(-1, 3), d.reshape(-1, 3))


def trace_mode():
    import ray_reference as R
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    res = {"config": 3, "size": [sc.width, sc.height]}
    builds = []
    for k in range(3):                                     # the host build, three times (an object moved by nothing but a rounding step)
        sc.desc.objects["trs"][0, 12] = np.nextafter(sc.desc.objects["trs"][0, 12], np.float32(np.inf))
        t0 = time.perf_counter()
        r.trace_rays(sc.desc, np.zeros(0, pkg.scene.RAY_DTYPE))
        builds.append((time.perf_counter() - t0) * 1e3)
    stored, nodes, n_builds, depth = r.ray_scene_info()
    res["structure"] = {"triangles_in_scene": sc.n_triangles, "triangles_stored": stored, "nodes": nodes, "depth": depth, "bytes": nodes * 32 + stored * 48,
                        "host_build_ms": [round(b, 1) for b in builds], "what_the_build_time_covers": "draining the stream, reading vertices and indices of every mesh in use back, world transform, median-split build, validation, upload"}
    tris, prims = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    rng = np.random.default_rng(11)
    n_rand = 8 << 20
    o = rng.uniform(lo, hi, (n_rand, 3)).astype(np.float32)
    d = rng.normal(size=(n_rand, 3)).astype(np.float32)
    sets = {"camera_rays_coherent": camera_rays(sc), "random_rays_8Mi_incoherent": pkg.scene.make_rays(o, d)}
    ref = R.build_bvh(tris, prims)
    for name, rays in sets.items():
        n = len(rays)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
        d_hits = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        entry_ = {"rays": n}
        for any_hit in (False, True):
            ms = timed_ms(lambda: r.trace_rays_device(sc.desc, d_rays.data_ptr(), n, d_hits.data_ptr(), any_hit=any_hit), reps=5)
            entry_["any_hit" if any_hit else "closest_hit"] = summary(ms, n)
            hits = d_hits.cpu().numpy().view(pkg.scene.HIT_DTYPE)
            entry_["any_hit" if any_hit else "closest_hit"]["rays_that_hit"] = int((hits["prim"] != 0xFFFFFFFF).sum())
            # the reference walk on a sample of the same rays: what a ray fetches and tests, and that the device agrees with it
            pick = rng.choice(n, 16384, replace=False)
            want, visits, tested = R.walk(ref, rays[pick], any_hit=any_hit, count_triangles=True)
            entry_["any_hit" if any_hit else "closest_hit"].update({
                "sample_agrees_with_the_arbiter": bool(want.tobytes() == hits[pick].tobytes()),
                "nodes_fetched_per_ray_mean_max": [round(float(visits.mean()), 2), int(visits.max())],
                "triangles_tested_per_ray_mean_max": [round(float(tested.mean()), 2), int(tested.max())],
                "bytes_fetched_per_ray_mean": round(float(visits.mean() * 32 + tested.mean() * 48 + 48), 1)})
        res[name] = entry_
        del d_rays, d_hits
    # the sun mask from the resident G-buffer
    r.pass_gbuffer(sc.desc)
    ms = timed_ms(lambda: r.trace_sun_visibility(sc.desc, 1e-3, read=False), reps=5)
    mask = r.trace_sun_visibility(sc.desc, 1e-3)
    res["sun_mask_any_hit"] = dict(summary(ms, sc.width * sc.height), pixels=sc.width * sc.height, occluded_fraction=round(float((mask == 0).mean()), 4),
                                   for_context_ms={"shadow_pass_DESIGN_6": 0.104})
    res["scalar_fast_path"] = "not built: the plain walk is the only variant (DESIGN.md 6k)"
    r.close()
    return {"mode": "trace", "how": "torch events on torch's stream (arctic_set_stream) around 5 back-to-back calls, median of 7 rounds after 2 warm-up calls; rays and hits resident on the device", "results": res}


def frame_loop(r, sc, outs, n):
    t0 = time.perf_counter()
    for k in range(n):
        r.render_frame_device(sc.desc, sc.settings, outs[k % len(outs)].data_ptr())
    r.flush(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ab_mode(label):
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    outs = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    frame_loop(r, sc, outs, 100)
    static = [frame_loop(r, sc, outs, 400) for _ in range(5)]
    r.flush()
    img = outs[0].cpu().numpy()
    r.close()
    import hashlib
    return {"mode": "ab", "label": label, "library": os.environ.get("ARCTIC_HIP_LIBRARY", "this build"), "frame_ms": [round(x, 4) for x in static],
            "frame_sha256_16": hashlib.sha256(img.tobytes()).hexdigest()[:16]}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    mode = args[0]
    result = trace_mode() if mode == "trace" else ab_mode(args[1])
    print(json.dumps(result))
    if out_file:
        doc = json.load(open(out_file)) if os.path.exists(out_file) else {}
        doc[mode if mode != "ab" else "ab_" + args[1]] = result
        json.dump(doc, open(out_file, "w"), indent=1)
