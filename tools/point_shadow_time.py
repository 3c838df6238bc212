"""Shadow-casting point lights at 4K config 3 (its 64 point lights stay), faces of F = 1024: for K = 0, 1 and 4 lights
(scenes.point_shadow_lights) the shading pass over a resident G-buffer (time_shade), the same with the sun's map at 1.0 (every pixel lit,
each takes K cube lookups: the analogue of bench.py's roofline.all_pixels_lit), whole frames with static lights (faces cached) and with
one light moving every frame (faces redrawn; each frame then also synchronises in arctic_update_point_shadow_lights), and the face
passes alone (arctic_pass_point_shadows, host-timed between two flushes).  --faces-only N: only N face passes of K = 4 (a kernel-trace run
of their own: rocprofv3 --kernel-trace --stats -- python tools/point_shadow_time.py --faces-only 20).  Prints one JSON object.
usage: python tools/point_shadow_time.py [--out FILE] [--iters N] [--faces-only N]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as e
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--faces-only", type=int, default=0)
args = ap.parse_args()
pkg = e.load_package()
sc = pkg.scenes.config3(scale=1.0)
F = 1024
r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
r.set_option("point_shadow_size", F)
if args.faces_only:
    r.update_point_shadow_lights(pkg.scenes.point_shadow_lights(4))
    for i in range(args.faces_only): r.pass_point_shadows(sc.desc)
    r.flush(); r.close()
    sys.exit(0)
out = torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
res = {"config": 3, "width": sc.width, "height": sc.height, "point_lights": int(len(sc.lights)), "face_size": F, "iters": args.iters}
ones = np.ones((sc.shadow_size, sc.shadow_size), np.float32)


def frames(n, move=None):
    r.flush(); t = time.perf_counter()
    for i in range(n):
        if move is not None: r.update_point_shadow_lights(move(i))
        r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush()
    return (time.perf_counter() - t) / n * 1e3


for K in (0, 1, 4):
    lights = pkg.scenes.point_shadow_lights(K)
    r.update_point_shadow_lights(lights)
    frames(3)
    static = frames(args.iters)
    row = {"n_lights": K, "frame_ms_static": static}
    r.pass_gbuffer(sc.desc)
    ms = r.time_shade(sc.desc, sc.settings, warmup=3, iters=args.iters)
    row["shade_ms_median"], row["shade_ms_min"] = float(np.median(ms)), float(np.min(ms))
    r.write_shadow_map(ones)
    ms = r.time_shade(sc.desc, sc.settings, warmup=3, iters=args.iters)
    row["shade_all_lit_ms_median"], row["shade_all_lit_ms_min"] = float(np.median(ms)), float(np.min(ms))
    r.pass_shadow_map(sc.desc)
    if K:
        def move(i, base=lights):
            m = base.copy()
            m[0]["position"] = m[0]["position"] + np.float32([0.01 * (i + 1), 0.0, 0.0])
            return m
        row["frame_ms_one_light_moving"] = frames(args.iters, move)
        r.update_point_shadow_lights(lights)
        for i in range(3): r.pass_point_shadows(sc.desc)
        r.flush(); t = time.perf_counter()
        for i in range(args.iters): r.pass_point_shadows(sc.desc)
        r.flush()
        row["face_pass_ms"] = (time.perf_counter() - t) / args.iters * 1e3
    res[f"k{K}"] = row
    print(f"K={K}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items() if k != "n_lights"), flush=True)
for K in (1, 4):
    res[f"shade_ratio_k{K}"] = res[f"k{K}"]["shade_ms_median"] / res["k0"]["shade_ms_median"]
    res[f"shade_all_lit_ratio_k{K}"] = res[f"k{K}"]["shade_all_lit_ms_median"] / res["k0"]["shade_all_lit_ms_median"]
r.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
