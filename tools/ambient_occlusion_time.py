"""Cost of the ambient occlusion (arctic_trace_ambient_occlusion, csrc/ray_ao.hip) on one MI355X; the numbers of DESIGN.md 6n /
profiles/ambient_occlusion_cost.json.

Config 3 at 3840 x 2160 with the G-buffer resident: n_rays 1, 4 and 16 with pattern 4 and ao_directions' cosine hemisphere, a radius of a tenth of
the scene's diagonal and +inf, filter off and on.  Per case: milliseconds (torch events on torch's stream around back-to-back calls with out ==
NULL, median of 7 rounds after 2 warm-up calls), rays per second over the covered pixels' rays, and -- from the reference walk
(tests/ray_reference.py: the same median-split tree) on a sample of the same pixels -- nodes fetched and triangles tested per ray, checked against
the device's bytes.  The filter kernel alone is the difference between the call with the filter and the call without it (the trace kernel does the
same work in both), against the bytes it has to move: per pixel 12 + 16 + 16 bytes of planes b, c, e and the hits byte once, one byte written.

    ambient_occlusion_time.py [--out FILE]                  the cases above: prints one JSON line and, with --out, writes it there
    ambient_occlusion_time.py --kernels                     a program for a kernel trace of its own: 20 filtered calls with 4 rays and the finite radius
                                                            (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/ambient_occlusion_time.py --kernels)
    ambient_occlusion_time.py --kernel-stats DIR --out FILE adds the two kernels' rows of that trace's statistics to FILE (needs no GPU)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def resident():
    global np, torch, pkg
    import numpy as np
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.pass_gbuffer(sc.desc)
    return sc, r


def kernels_mode():
    sc, r = resident()
    dirs = pkg.renderer.ao_directions(4, 4)
    for _ in range(20):
        r.trace_ambient_occlusion(sc.desc, dirs, radius=3.521, bias=1e-3, filter=True, read=False)
    r.flush()
    r.close()


def kernel_stats(directory):
    import csv
    import glob
    rows = {}
    for p in glob.glob(directory + "/**/*kernel_stats.csv", recursive=True):
        for row in csv.DictReader(open(p)):
            for k in ("k_trace_ao", "k_ao_filter"):
                if k in row["Name"]:
                    rows[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 1), "min_us": round(float(row["MinNs"]) / 1e3, 1), "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
    return {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python3 tools/ambient_occlusion_time.py --kernels (4 rays, pattern 4, radius 3.521, filter on)", "kernels": rows}


def main():
    import ao_reference as A
    import ray_reference as R
    sc, r = resident()
    attrs, material, _, _ = r.read_gbuffer(want=("attrs", "material"))
    tris, prims = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo))
    ref = R.build_bvh(tris, prims)
    pixels = sc.width * sc.height
    rng = np.random.default_rng(17)
    pick = rng.choice(pixels, 2048, replace=False)
    P, bias = 4, 1e-3
    points, sets, geometry = A.image_points(attrs, material, P)
    _, ok = A.normal(points[:, 3:6])
    covered = int((ok & geometry).sum())
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "covered_pixels": covered, "scene_diagonal": round(diagonal, 3), "pattern": P, "bias": bias,
           "cases": []}
    for n_rays in (1, 4, 16):
        dirs = pkg.renderer.ao_directions(n_rays, P)
        for radius in (0.1 * diagonal, float("inf")):
            case = {"n_rays": n_rays, "radius": "inf" if radius == float("inf") else round(radius, 3)}
            ms = {}
            for filt in (False, True):
                call = lambda: r.trace_ambient_occlusion(sc.desc, dirs, radius=radius, bias=bias, filter=filt, read=False)
                t = timed_ms(call, reps=3)
                ms[filt] = statistics.median(t)
                case["filter_on" if filt else "filter_off"] = {"ms_median": round(ms[filt], 4), "ms_min_max": [round(min(t), 4), round(max(t), 4)],
                                                               "Grays_per_s": round(covered * n_rays / ms[filt] / 1e6, 3)}
            extra = ms[True] - ms[False]
            moved = pixels * (12 + 16 + 16 + 1 + 1)
            case["filter_kernel_alone_by_difference"] = {"ms": round(extra, 4), "bytes_it_has_to_move": moved, "GB_per_s": round(moved / extra / 1e6, 1) if extra > 0 else None}
            got = r.trace_ambient_occlusion(sc.desc, dirs, radius=radius, bias=bias)
            case["mean_visibility_of_covered_pixels"] = round(float(got.reshape(-1)[ok & geometry].mean()) / 255.0, 4)
            # the reference walk for the sampled pixels: what a ray fetches and tests, and that the device agrees with it
            ry, okp = A.point_rays(points[pick], sets[pick], dirs, n_rays, radius, bias)
            act = okp & geometry[pick]
            flat = ry[act].reshape(-1)
            found, visits, tested = R.walk(ref, flat, any_hit=True, count_triangles=True)
            hits = np.zeros(len(pick), np.int64)
            hits[act] = (found["prim"] != R.NO_PRIM).reshape(-1, n_rays).sum(1)
            want = A.result(hits, n_rays, act)
            case["sample"] = {"pixels": len(pick), "agrees_with_the_arbiter": bool((got.reshape(-1)[pick] == want).all()),
                              "rays_that_hit_fraction": round(float((found["prim"] != R.NO_PRIM).mean()), 4),
                              "nodes_fetched_per_ray_mean_max": [round(float(visits.mean()), 2), int(visits.max())],
                              "triangles_tested_per_ray_mean_max": [round(float(tested.mean()), 2), int(tested.max())]}
            res["cases"].append(case)
    res["structure"] = dict(zip(("triangles_stored", "nodes", "builds", "depth"), r.ray_scene_info()))
    ms = timed_ms(lambda: r.trace_sun_visibility(sc.desc, 1e-3, read=False), reps=5)
    res["for_context"] = {"sun_mask_ms_this_run": round(statistics.median(ms), 4), "sun_mask_Grays_per_s_this_run": round(pixels / statistics.median(ms) / 1e6, 2),
                          "DESIGN_6k": {"sun_mask_Grays_per_s": 11.0, "incoherent_any_hit_Grays_per_s": 1.64}}
    r.close()
    return {"how": "torch events on torch's stream (arctic_set_stream) around 3 back-to-back calls with out == NULL, median of 7 rounds after 2 warm-up calls; G-buffer, "
                   "structure and direction table resident", "results": res}


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--kernels" in args:
        kernels_mode()
    elif "--kernel-stats" in args:
        out = args[args.index("--out") + 1]
        result = json.load(open(out))
        result["kernel_trace"] = kernel_stats(args[args.index("--kernel-stats") + 1])
        bytes_moved = result["results"]["pixels"] * (12 + 16 + 16 + 1 + 1)
        f = result["kernel_trace"]["kernels"].get("k_ao_filter")
        if f:
            f["bytes_it_has_to_move"] = bytes_moved
            f["GB_per_s_at_avg"] = round(bytes_moved / f["avg_us"] / 1e3, 1)
        print(json.dumps(result["kernel_trace"]))
        json.dump(result, open(out, "w"), indent=1)
    else:
        result = main()
        print(json.dumps(result))
        if "--out" in args:
            json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
