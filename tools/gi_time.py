"""Cost of the indirect diffuse light (arctic_trace_gi, arctic_accumulate_gi_device, arctic_gi_compose_device, arctic_pass_gi; csrc/gi.hip) on
one MI355X; the numbers of DESIGN.md 6aa / profiles/gi_cost.json.

Config 3 (64 point lights) with the sun's map drawn, the frame shaded under ARCTIC_OPT_KEEP_FLOAT_OUTPUT and the G-buffer resident, on a
3840 x 2160 handle and on a 1920 x 1080 handle of the same scene.

    gi_time.py [--scale S] [--out FILE]     call times: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up
                                            calls -- arctic_trace_gi at 1 ray per pixel (P = 4) unfiltered and filtered, arctic_pass_gi with the
                                            filter and the history on, and as yardsticks the reflection plane and arctic_pass_ray_effects_temporal
    gi_time.py --kernels gi|yardsticks [--scale S]   20 frames of the indirect light's calls above, or of the yardsticks', and nothing else, for a
                                            kernel trace of its own, so that k_trace and k_shade_hits of the one are not averaged with the other's:
                                            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/gi_time.py --kernels gi
    gi_time.py --stats DIR [--out FILE]     that trace's kernel_stats.csv as JSON, with the counted bytes per pixel of the three streaming kernels
                                            and their share of the 8 TB/s roof

Every figure is of ONE run of this program."""
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_gi_rays", "k_gi_add", "k_gi_estimate_window", "k_gi_estimate", "k_gi_accumulate", "k_gi_compose", "k_trace", "k_shade_hits", "k_reflect_rays", "k_ao_accumulate",
           "k_compose", "k_trace_ao", "k_ao_filter")
# what a streaming kernel has to move per pixel, counted from its definition: k_gi_add a record's second half, a colour, S in and out (the first round
# reads no S: 48); k_gi_estimate S in, E out; k_gi_compose the colour, the material word, uv, E in, RGBA8, LDR and HDR out (texels not counted)
STREAM_BYTES = {"k_gi_add": 64, "k_gi_estimate": 32, "k_gi_compose": 12 + 4 + 16 + 16 + 4 + 12 + 12}
ROOF_BYTES_PER_S = 8.0e12


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
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.set_option("keep_float_output", 1)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    return sc, r


def calls(sc, r):
    """the calls that are timed and traced, by name"""
    R = pkg.renderer
    dirs, gi = R.gi_directions(1, 4), dict(max_distance=float("inf"), bias=1e-3, clamp_max=64.0)
    hist, comp = R.gi_history_arguments(max_history=16.0), R.gi_compose_arguments(1.0, 0.0)
    return {
        "arctic_trace_gi_1_ray_unfiltered": lambda: r.trace_gi(sc.desc, dirs, read=False, **gi),
        "arctic_trace_gi_1_ray_filtered": lambda: r.trace_gi(sc.desc, dirs, read=False, filter=True, **gi),
        "arctic_pass_gi_1_ray_P4_filter_history": lambda: r.pass_gi(sc.desc, sc.settings, dirs, hist=hist, compose=comp, filter=True, **gi),
        "yardstick_arctic_trace_reflections": lambda: r.trace_reflections(sc.desc, 1e-3, read=False),
        "yardstick_arctic_pass_ray_effects_temporal_1_ray_P4_filter": lambda: r.pass_ray_effects_temporal(sc.desc, sc.settings, R.ao_directions(1, 4), filter=True, read=False),
    }


def main(scale):
    sc, r = resident(scale)
    res = {"config": 3, "size": [sc.width, sc.height], "point_lights": len(sc.lights), "shadow_size": sc.shadow_size}
    for name, fn in calls(sc, r).items():
        res[name] = figures(timed_ms(fn, reps=3))
    E = r.trace_gi(sc.desc, pkg.renderer.gi_directions(1, 4), max_distance=float("inf"), bias=1e-3, clamp_max=64.0)
    res["covered_pixels_fraction"] = round(float((E[..., 3] > 0).mean()), 4)
    res["mean_E_rgb_of_covered_pixels"] = [round(float(x), 4) for x in E[E[..., 3] > 0][:, :3].mean(0)]
    res["gi_info"] = dict(zip(("device_bytes", "launches", "calls", "history_bytes"), r.gi_info()))
    res["hit_shading_info_device_bytes"] = r.hit_shading_info()[0]
    res["structure"] = dict(zip(("triangles_stored", "nodes", "builds", "depth"), r.ray_scene_info()))
    r.close()
    return {"how": "torch events on torch's stream (arctic_set_stream) around 3 back-to-back calls, median of 7 rounds after 2 warm-up calls; sun map, G-buffer, shaded "
                   "HDR plane and structure resident; one run of this program", "results": res}


def kernels_mode(scale, which):
    sc, r = resident(scale)
    todo = {k: fn for k, fn in calls(sc, r).items() if k.startswith("yardstick") == (which == "yardsticks")}
    for _ in range(20):
        for fn in todo.values():
            fn()
    r.flush()
    r.close()


def kernel_stats(directory, pixels):
    import csv
    import glob
    rows = {}
    for p in glob.glob(directory + "/**/*kernel_stats.csv", recursive=True):
        for row in csv.DictReader(open(p)):
            for k in KERNELS:                                        # (the whole name, mangled or not: k_gi_estimate is not k_gi_estimate_window, k_trace not k_trace_ao)
                if re.search(r"(?<![A-Za-z_])" + k + r"(?![a-z_])", row["Name"]):
                    e = rows.setdefault(k, {"calls": 0, "total_ns": 0.0, "min_us": None, "max_us": None})
                    e["calls"] += int(row["Calls"]); e["total_ns"] += float(row["TotalDurationNs"])
                    e["min_us"] = round(min(x for x in (e["min_us"], float(row["MinNs"]) / 1e3) if x is not None), 1)
                    e["max_us"] = round(max(x for x in (e["max_us"], float(row["MaxNs"]) / 1e3) if x is not None), 1)
                    break
    for k, e in rows.items():
        e["avg_us"] = round(e.pop("total_ns") / e["calls"] / 1e3, 1)
        if k in STREAM_BYTES and pixels:
            e["counted_bytes_per_pixel"] = STREAM_BYTES[k]
            e["GB_per_s"] = round(STREAM_BYTES[k] * pixels / (e["avg_us"] * 1e-6) / 1e9, 1)
            e["share_of_the_8_TB_per_s_roof"] = round(STREAM_BYTES[k] * pixels / (e["avg_us"] * 1e-6) / ROOF_BYTES_PER_S, 3)
    return {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/gi_time.py --kernels gi|yardsticks (20 frames of the timed calls of that group)", "pixels": pixels, "kernels": rows}


if __name__ == "__main__":
    args = sys.argv[1:]
    scale = float(args[args.index("--scale") + 1]) if "--scale" in args else 1.0
    if "--kernels" in args:
        kernels_mode(scale, args[args.index("--kernels") + 1])
        sys.exit(0)
    if "--stats" in args:
        result = kernel_stats(args[args.index("--stats") + 1], int(round(3840 * scale)) * int(round(2160 * scale)))
    else:
        result = main(scale)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
