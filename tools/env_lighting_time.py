"""ARCTIC_OPT_ENV_LIGHTING at 4K config 3: the shading pass over a resident G-buffer (time_shade) and whole frames in mode 0 and mode 1,
and the one-off precompute of the tables for a 2048 x 1024 map.  Prints one JSON object.
usage: python tools/env_lighting_time.py [--out FILE] [--iters N]"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as e
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
pkg = e.load_package()
sc = pkg.scenes.config3(scale=1.0)
sc.environment = pkg.scenes.synthetic_hdri(2048, 1024)
r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
out = torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
res = {"config": 3, "width": sc.width, "height": sc.height, "env": [2048, 1024], "iters": args.iters}
# the precompute: enqueued by the option (the map is already there), measured to the end of the stream; then once more for a new map
r.flush()
t = time.perf_counter(); r.set_option("env_lighting", 1); r.flush(); res["precompute_ms_first"] = (time.perf_counter() - t) * 1e3
t = time.perf_counter(); r.create_hdri(sc.environment); r.flush(); res["precompute_ms_create_hdri"] = (time.perf_counter() - t) * 1e3
for mode in (0, 1):
    r.set_option("env_lighting", mode)
    for i in range(3): r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush(); t = time.perf_counter()
    for i in range(args.iters): r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush(); frame = (time.perf_counter() - t) / args.iters * 1e3
    r.pass_gbuffer(sc.desc)
    ms = r.time_shade(sc.desc, sc.settings, warmup=3, iters=args.iters)
    res[f"mode{mode}"] = {"shade_ms_median": float(np.median(ms)), "shade_ms_min": float(np.min(ms)), "frame_ms": frame}
    print(f"mode {mode}: shading pass {np.median(ms):.4f} ms (min {np.min(ms):.4f}), whole frame {frame:.4f} ms", flush=True)
res["shade_ratio"] = res["mode1"]["shade_ms_median"] / res["mode0"]["shade_ms_median"]
r.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
