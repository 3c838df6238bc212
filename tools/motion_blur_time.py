"""Cost of the motion blur (arctic_motion_blur_device, arctic_pass_motion_blur; csrc/motion_blur.hip) on one MI355X; the numbers of DESIGN.md 6t /
profiles/motion_blur_cost.json.

Config 3 at 3840 x 2160 under a CAMERA PAN: a frame is drawn, the motion call is made, the camera turns by 0.5 degrees, the next frame is drawn and
the motion call made again -- velocity2 is then the pan (about 26 pixels across the frame), so nearly every tile moves and every pixel takes the
whole gather.  On a still scene the gather is a copy, and its figure (recorded too, as `still`) would flatter the kernel.
  arctic_depth_plane_device             k_mb_depth alone
  arctic_motion_blur_device             k_mb_tile_max + k_mb_neighbour_max + k_motion_blur on the handle's HDR plane, at 7, 15 and 31 samples,
                                        with and without the dither, and on a zero velocity plane
  arctic_pass_motion_blur per frame     behind arctic_render_frame_device with the camera alternating between the two poses, next to the frames
                                        alone in the same run
Beside each figure the bytes per pixel COUNTED from the layout: what the kernels must move when every plane is read once (the floor), and what
the taps request through the cache.  Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up
calls.  Every figure is of ONE run.

    motion_blur_time.py [--out FILE] [--bench FILE] [--kernel-stats NAME=FILE.csv ...]
        prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py result lines of this build and the parent's
        library, recorded beside the figures as given; --kernel-stats: kernel statistics (csv) of a profiler's run of `--only SAMPLES`, whose rows
        for this unit's kernels are recorded under NAME -- the split of the chain into its kernels
    motion_blur_time.py --only SAMPLES     20 calls of the depth plane and of the blur at SAMPLES taps under the pan, nothing timed: the run a
                                           profiler's kernel trace is taken of"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
DITHER = 1
KW = dict(shutter=1.0, max_radius=16.0, depth_extent=0.05)


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


def figure(ms, floor_bytes, requested_bytes, pixels):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "floor_bytes_per_pixel": round(floor_bytes, 2),
            "requested_bytes_per_pixel": round(requested_bytes, 2), "ms_at_the_roof": round(floor_bytes * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4),
            "fraction_of_the_roof": round(floor_bytes * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4)}


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def kernel_rows(path):
    """the rows of a kernel statistics csv that name this unit's kernels: {kernel: {calls, average_ns}}"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "k_mb_" in name or "k_motion_blur" in name:
            short = "k_motion_blur_history" if "HistoryColor" in name else [k for k in ("k_mb_depth", "k_mb_tile_max", "k_mb_neighbour_max", "k_motion_blur") if k in name][0]
            out[short] = {"calls": int(float(row.get("Calls", 0))), "average_ns": round(float(row.get("AverageNs") or row.get("Average") or 0.0), 1)}
    return out


def panned(pkg, desc, degrees=0.5):
    c = dict(desc.camera)
    c["rotation"] = (c["rotation"][0], c["rotation"][1] + degrees)
    return pkg.scenes.SceneDesc(camera=c, ambient=desc.ambient, sun=desc.sun, objects=desc.objects, point_lights=desc.point_lights)


def main(bench=None, stats=(), only=None):
    global torch
    import numpy as np
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_option("keep_float_output", 1)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    pixels = sc.width * sc.height
    d_pw = torch.zeros((sc.height, sc.width, 4), dtype=torch.float32, device="cuda")
    d_vel = torch.zeros((sc.height, sc.width, 2), dtype=torch.float32, device="cuda")
    d_zero = torch.zeros((sc.height, sc.width, 2), dtype=torch.float32, device="cuda")
    d_z = torch.zeros((sc.height, sc.width), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    poses = (sc.desc, panned(pkg, sc.desc))
    for desc in poses:                                                           # the second call sees what the first saw from the other pose: the pan
        r.render_frame_device(desc, sc.settings, d_out.data_ptr())
        r.motion_vectors_device(desc, d_pw.data_ptr(), d_vel.data_ptr())
    r.depth_plane_device(d_z.data_ptr())
    blur = lambda samples, vel=d_vel, flags=0: r.motion_blur_device(sc.settings, None, vel.data_ptr(), d_z.data_ptr(), d_out.data_ptr(), samples=samples, flags=flags, **KW)
    if only is not None:
        for _ in range(20):
            r.depth_plane_device(d_z.data_ptr())
            blur(only)
        torch.cuda.synchronize()
        r.close()
        return {"only": only}
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "pan_degrees": 0.5, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S, "settings": KW}

    # ---- k_mb_depth: the key 8 in, the float 4 out
    res["k_mb_depth"] = figure(timed_ms(lambda: r.depth_plane_device(d_z.data_ptr()), reps=10), 12, 12, pixels)
    # ---- the chain.  Counted per pixel, every plane once: k_mb_tile_max velocity2 8 and depth 4 in, P 8 out; the tile planes 3 x 8 / 64;
    # k_motion_blur C 12 and P 8 in, out 12, RGBA8 4 and float LDR 12 out: 68.4.  Requested through the cache on top of that: per tap P 8 and,
    # where the weight enters, C 12
    floor = (8 + 4 + 8) + 3 * 8 / 64 + (12 + 8) + (12 + 4 + 12)
    for samples in (7, 15, 31):
        res[f"chain_{samples}_samples"] = figure(timed_ms(lambda: blur(samples), reps=5), floor, floor + samples * 20, pixels)
        res[f"chain_{samples}_samples_dither"] = figure(timed_ms(lambda: blur(samples, flags=DITHER), reps=5), floor, floor + samples * 20, pixels)
    blur(15)
    _, hdr, _, _, near, _ = r.read_motion_blur(want=("hdr", "neighbour_max"))
    res["tiles_that_gather_fraction"] = round(float((np.hypot(near[..., 0], near[..., 1]) > 0.5).mean()), 4)
    res["neighbour_max_length_median_px"] = round(float(np.median(np.hypot(near[..., 0], near[..., 1]))), 3)
    res["still_chain_15_samples"] = figure(timed_ms(lambda: blur(15, vel=d_zero), reps=5), floor, floor, pixels)

    # ---- the one call per frame, the camera alternating between the two poses so that every frame pans
    state = {"k": 0}
    def frame(then_blur, samples=15):
        desc = poses[state["k"] & 1]
        state["k"] += 1
        r.render_frame_device(desc, sc.settings, d_out.data_ptr())
        if then_blur:
            r.pass_motion_blur(desc, sc.settings, d_out.data_ptr(), samples=samples, **KW)
    res["render_frame"] = med(timed_ms(lambda: frame(False), reps=6))
    for samples in (7, 15, 31):
        res[f"render_frame_then_pass_motion_blur_{samples}_samples"] = med(timed_ms(lambda: frame(True, samples), reps=6))
    res["render_frame_again"] = med(timed_ms(lambda: frame(False), reps=6))
    res["motion_blur_info"] = dict(zip(("device_bytes", "k_motion_blur_launches", "calls"), r.motion_blur_info()[:3]))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded, its HDR plane, the pan's velocity2 and the depth plane resident; bytes counted from the layout, not measured; one run of this "
                  "program: single figures",
           "results": res}
    if stats:
        out["kernels_by_a_profilers_trace"] = {name: kernel_rows(path) for name, path in stats}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    stats = [a.split("=", 1) for a in args[args.index("--kernel-stats") + 1:] if "=" in a] if "--kernel-stats" in args else []
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None, stats, int(args[args.index("--only") + 1]) if "--only" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
