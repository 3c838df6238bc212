"""How far a cheap estimate of the indirect diffuse light is from a converged one, on one MI355X; the numbers of DESIGN.md 6aa /
profiles/gi_quality.json.

The scene of tests/hit_scenes.py at 64 x 64 pixels, camera still.  The reference is a 256-ray estimate of the same definition: 16 calls of
arctic_trace_gi at 16 rays per pixel and P = 1, each with a table of its own seed, averaged in float64.  Against it, the mean absolute
difference of E.rgb over the pixels that had rays, for: 1 ray per pixel (P = 4); the same filtered; the same filtered after 16 frames of
arctic_accumulate_gi with the table turned per frame (a new seed) and max_history = 16.  Every figure is of ONE run of this program.

    gi_quality.py [--out FILE]      prints one JSON line and, with --out, writes it there"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import __graft_entry__ as entry
    import hit_scenes as HS
    pkg = entry.load_package()
    R = pkg.renderer
    size = 64
    c = HS.scene(pkg, list(HS.ASSIGNMENTS)[0])
    desc = pkg.scenes.SceneDesc(camera=dict(c.desc.camera, aspect=1.0), ambient=HS.AMBIENT, sun=c.desc.sun, objects=c.g.objects)
    r = HS.upload(pkg, R.Renderer(size, size, HS.SHADOW, HS.MAX_LIGHTS), c)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    kw = dict(max_distance=float("inf"), bias=2e-3, clamp_max=64.0)
    flt = dict(filter=True, normal_cos=0.9, plane_dist=0.1)
    ref = np.zeros((size, size, 3))
    for k in range(16):
        E = r.trace_gi(desc, R.gi_directions(16, 1, seed=1000 + k), **kw)
        ref += E[..., :3].astype(np.float64) / 16
    had = E[..., 3] > 0
    mad = lambda x: round(float(np.abs(x[..., :3].astype(np.float64) - ref)[had].mean()), 5)
    res = {"scene": "tests/hit_scenes.py, " + list(HS.ASSIGNMENTS)[0], "size": [size, size], "pixels_with_rays": int(had.sum()), "reference_rays_per_pixel": 256,
           "mean_reference_rgb": [round(float(x), 4) for x in ref[had].mean(0)], "clamp_max": kw["clamp_max"]}
    res["mean_abs_difference_1_ray"] = mad(r.trace_gi(desc, R.gi_directions(1, 4, seed=0), **kw))
    res["mean_abs_difference_1_ray_filtered"] = mad(r.trace_gi(desc, R.gi_directions(1, 4, seed=0), **kw, **flt))
    out = None
    for k in range(16):
        out = r.accumulate_gi(desc, r.trace_gi(desc, R.gi_directions(1, 4, seed=k), **kw, **flt), max_history=16.0, normal_cos=0.9, plane_dist=0.1)
    res["mean_abs_difference_1_ray_filtered_16_accumulated_frames"] = mad(out)
    res["history_count_mean"] = round(float(out[..., 3][had].mean()), 3)
    a = np.zeros_like(ref)
    for k in range(8):
        a += r.trace_gi(desc, R.gi_directions(16, 1, seed=1000 + k), **kw)[..., :3].astype(np.float64) / 8
    res["for_scale_mean_abs_difference_of_the_first_128_rays_from_all_256"] = round(float(np.abs(a - ref)[had].mean()), 5)
    r.close()
    return {"how": "arctic_trace_gi and arctic_accumulate_gi on one handle, camera still; one run of this program", "results": res}


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main()
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
