"""Cost of the extended hit model (ARCTIC_OPT_HIT_MODEL = 1; csrc/hit_shade_ext.hip: k_shade_hits_ext) against the base model of the same commit
(option 0: k_shade_hits) on one MI355X; the numbers of DESIGN.md 6ab / profiles/hit_model_cost.json.

Config 3 at 3840 x 2160 with its 64 point lights plus 8 spot lights, 2 shadow-casting point lights (faces drawn by arctic_pass_point_shadows),
material extras on every material (factors off neutral, an emissive and an occlusion image of the packed size: the fast layout) and
ARCTIC_OPT_ENV_LIGHTING = 1 on a 2048 x 1024 synthetic map; the sun's map drawn, the frame shaded under ARCTIC_OPT_KEEP_FLOAT_OUTPUT and the G-buffer resident.  The handle is
the same under both settings: option 0 ignores everything the extended model reads.

    hit_model_time.py [--scale S] [--out FILE]      call times without a profiler: torch events on torch's stream around back-to-back calls, median of
                                                    7 rounds after 2 warm-up calls -- arctic_trace_reflections and arctic_pass_gi (1 ray, P = 4, filter
                                                    and history on) under option 0, under option 1, and under option 1 with ARCTIC_OPT_ENV_LIGHTING 0
    hit_model_time.py --kernels 0|1|1-noenv [--scale S]   20 reflection planes under that setting (1-noenv: option 1 with ARCTIC_OPT_ENV_LIGHTING 0) and nothing else, for a kernel trace in a process of its own:
                                                    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/hit_model_time.py --kernels 1
    hit_model_time.py --stats DIR0 DIR1 [DIR1N] [--out FILE]   the traces' kernel_stats.csv as JSON, merged into FILE when it holds the call times already

Every figure is of ONE run of this program."""
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_shade_hits_ext", "k_shade_hits", "k_trace", "k_reflect_rays")
N_SPOTS, N_CUBES, CUBE_FACE = 8, 2, 1024


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


def figures(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def resident(scale):
    global np, torch, pkg
    import numpy as np
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    sc = pkg.scenes.config3(scale)
    sc.environment = pkg.scenes.synthetic_hdri(2048, 1024)
    r = pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
    r.set_option("point_shadow_size", CUBE_FACE)
    sc.upload(r)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.set_option("keep_float_output", 1)
    r.set_option("env_lighting", 1)
    r.update_spot_lights(pkg.scenes.spot_lights(N_SPOTS))
    r.update_point_shadow_lights(pkg.scenes.point_shadow_lights(N_CUBES))
    rng = np.random.default_rng(71)
    params = pkg.scene.neutral_material_params(1)
    params["base_color_factor"], params["metallic_factor"], params["roughness_factor"] = (0.9, 0.8, 0.7), 0.8, 0.9
    params["normal_scale"], params["occlusion_strength"], params["emissive_factor"] = 1.2, 0.8, (0.5, 0.4, 0.3)
    n_materials = len(sc.materials)
    for m, (d, _, _) in enumerate(sc.materials):
        img = rng.integers(0, 256, d.shape, dtype=np.uint8)
        r.set_material_extras(m, params[0], img, img)
    r.pass_shadow_map(sc.desc)
    r.pass_point_shadows(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    return sc, r, n_materials


def calls(sc, r):
    R = pkg.renderer
    dirs, gi = R.gi_directions(1, 4), dict(max_distance=float("inf"), bias=1e-3, clamp_max=64.0)
    hist, comp = R.gi_history_arguments(max_history=16.0), R.gi_compose_arguments(1.0, 1.0)   # (ambient_scale 1: what the composition accepts under image-based ambient and occlusion)
    return {"arctic_trace_reflections": lambda: r.trace_reflections(sc.desc, 1e-3, read=False),
            "arctic_pass_gi_1_ray_P4_filter_history": lambda: r.pass_gi(sc.desc, sc.settings, dirs, hist=hist, compose=comp, filter=True, **gi)}


def main(scale):
    sc, r, n_materials = resident(scale)
    res = {"config": 3, "size": [sc.width, sc.height], "point_lights": len(sc.lights), "spot_lights": N_SPOTS, "cube_lights": N_CUBES, "cube_face": CUBE_FACE,
           "materials_with_extras": n_materials, "env_lighting": 1, "shadow_size": sc.shadow_size}
    planes = {}
    for model in (0, 1):
        r.set_option("hit_model", model)
        for name, fn in calls(sc, r).items():
            res[f"{name}_hit_model_{model}"] = figures(timed_ms(fn, reps=3))
        planes[model] = r.trace_reflections(sc.desc, 1e-3)
    r.set_option("env_lighting", 0)                                   # option 1 on a handle without image-based ambient: the same kernel, the block not entered
    for name, fn in calls(sc, r).items():
        res[f"{name}_hit_model_1_env_lighting_0"] = figures(timed_ms(fn, reps=3))
    r.set_option("env_lighting", 1)
    hit = planes[0][..., 3] == 1
    res["reflection_pixels_that_show_geometry"] = round(float(hit.mean()), 4)
    res["of_them_moved_by_the_extended_model"] = round(float((planes[1][hit] != planes[0][hit]).any(-1).mean()), 4)
    for model in (0, 1):   # (colours that are not numbers are counted and left out of the mean)
        rgb = planes[model][hit][:, :3].astype(np.float64)
        ok = np.isfinite(rgb).all(1)
        res[f"mean_rgb_hit_model_{model}"] = [round(float(x), 4) for x in rgb[ok].mean(0)]
        res[f"colours_not_finite_hit_model_{model}"] = int((~ok).sum())
    r.close()
    import __graft_entry__ as entry
    return {"source": entry.source_id(), "how": "torch events on torch's stream (arctic_set_stream) around 3 back-to-back calls, median of 7 rounds after 2 warm-up calls; sun map, cube faces, "
                   "G-buffer, shaded HDR plane and structure resident; no profiler; one run of this program", "results": res}


def kernels_mode(scale, which):
    sc, r, _ = resident(scale)
    r.set_option("hit_model", int(which[0]))
    if which.endswith("-noenv"):
        r.set_option("env_lighting", 0)
    fn = calls(sc, r)["arctic_trace_reflections"]
    for _ in range(20):
        fn()
    r.flush()
    r.close()


def kernel_stats(directory):
    import csv
    import glob
    rows = {}
    for p in glob.glob(directory + "/**/*kernel_stats.csv", recursive=True):
        for row in csv.DictReader(open(p)):
            for k in KERNELS:                                        # (the whole name, mangled or not: k_shade_hits is not k_shade_hits_ext)
                if re.search(r"(?<![A-Za-z_])" + k + r"(?![a-z_])", row["Name"]):
                    e = rows.setdefault(k, {"calls": 0, "total_ns": 0.0, "min_us": None, "max_us": None})
                    e["calls"] += int(row["Calls"]); e["total_ns"] += float(row["TotalDurationNs"])
                    e["min_us"] = round(min(x for x in (e["min_us"], float(row["MinNs"]) / 1e3) if x is not None), 1)
                    e["max_us"] = round(max(x for x in (e["max_us"], float(row["MaxNs"]) / 1e3) if x is not None), 1)
                    break
    for e in rows.values():
        e["avg_us"] = round(e.pop("total_ns") / e["calls"] / 1e3, 1)
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    scale = float(args[args.index("--scale") + 1]) if "--scale" in args else 1.0
    if "--kernels" in args:
        kernels_mode(scale, args[args.index("--kernels") + 1])
        sys.exit(0)
    out = args[args.index("--out") + 1] if "--out" in args else None
    if "--stats" in args:
        i = args.index("--stats")
        result = json.load(open(out)) if out and os.path.exists(out) else {}
        result["kernel_trace"] = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/hit_model_time.py --kernels 0|1 (20 reflection planes, "
                                             "a process per setting)", "hit_model_0": kernel_stats(args[i + 1]), "hit_model_1": kernel_stats(args[i + 2])}
        if len(args) > i + 3 and not args[i + 3].startswith("--"):
            result["kernel_trace"]["hit_model_1_env_lighting_0"] = kernel_stats(args[i + 3])
    else:
        result = main(scale)
    print(json.dumps(result))
    if out:
        json.dump(result, open(out, "w"), indent=1)
