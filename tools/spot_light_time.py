"""Spot lights at 4K config 3 (its 64 point lights stay): the shading pass over a resident G-buffer (time_shade) and whole frames with
0, 4 and 16 spot lights (scenes.spot_lights), plus one spot light that no pixel sees (range 0.01 far outside the hall: culled in every
wave) -- the cost of sending every tile through the general tile code (k_spotlit) with next to no light work.  Prints one JSON object.
usage: python tools/spot_light_time.py [--out FILE] [--iters N]"""
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
r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
out = torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
res = {"config": 3, "width": sc.width, "height": sc.height, "point_lights": int(len(sc.lights)), "iters": args.iters}
unseen = np.zeros(1, pkg.scene.SPOT_LIGHT_DTYPE)
unseen["position"], unseen["direction"], unseen["range"] = (0.0, 1000.0, 0.0), (0.0, -1.0, 0.0), 0.01
unseen["outer_cone_angle"], unseen["color"] = 0.5, (1.0, 1.0, 1.0)
cases = [("spots0", np.zeros(0, pkg.scene.SPOT_LIGHT_DTYPE)), ("spots1_unseen", unseen),
         ("spots4", pkg.scenes.spot_lights(4)), ("spots16", pkg.scenes.spot_lights(16))]
for name, spots in cases:
    r.update_spot_lights(spots)
    for i in range(3): r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush(); t = time.perf_counter()
    for i in range(args.iters): r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush(); frame = (time.perf_counter() - t) / args.iters * 1e3
    r.pass_gbuffer(sc.desc)
    ms = r.time_shade(sc.desc, sc.settings, warmup=3, iters=args.iters)
    res[name] = {"n_spots": int(len(spots)), "shade_ms_median": float(np.median(ms)), "shade_ms_min": float(np.min(ms)), "frame_ms": frame}
    print(f"{name}: shading pass {np.median(ms):.4f} ms (min {np.min(ms):.4f}), whole frame {frame:.4f} ms", flush=True)
for name, _ in cases[1:]:
    res[f"shade_ratio_{name}"] = res[name]["shade_ms_median"] / res["spots0"]["shade_ms_median"]
r.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
