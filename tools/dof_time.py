"""Cost of depth of field (arctic_dof_device, arctic_pass_dof; csrc/dof.hip) on one MI355X; the numbers of DESIGN.md 6u / profiles/dof_cost.json.

Config 3 at 3840 x 2160, a frame drawn and its depth plane extracted, the focus put on the scene's middle (arctic_dof_focus_at of the centre
pixel) and coc_scale that of a 50 mm lens at f/2 on a 24 mm sensor (arctic_dof_coc_scale), max_radius 16 -- what is not at the middle's distance
is then out of focus by up to max_radius pixels, and the fraction of tiles that gather and their median radius are recorded.
  arctic_dof_device             k_dof_prepare + k_dof_neighbour_max + k_dof_gather on the handle's HDR plane, at 16, 32 and 48 samples, and
                                with coc_scale = 0, where nothing is out of focus and the gather is a copy; and again with a lens
                                eight times as wide, where the discs reach max_radius over much of the frame
  arctic_pass_dof per frame     behind arctic_render_frame_device, next to the frames alone in the same run
Beside each figure the bytes per pixel COUNTED from the layout: what the kernels must move when every plane is read once (the floor), and what
the taps request through the cache.  A rate of requested bytes above the HBM roof -- counting P alone for a tap, since C is read only where the
weight enters -- shows that the taps hit in cache; a rate below it shows nothing either way.  The per-tap cost -- the chain at 48 samples less the chain at 16, over 32 -- is put next to the motion blur's from
profiles/motion_blur_cost.json (31 less 7 samples, over 24).  Milliseconds: torch events on torch's stream around back-to-back calls, median of
7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    dof_time.py [--out FILE] [--bench FILE] [--kernel-stats NAME=FILE.csv ...]
        prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py result lines of this build and the parent's
        library, recorded beside the figures as given; --kernel-stats: kernel statistics (csv) of a profiler's run of `--only SAMPLES`, whose rows
        for this unit's kernels are recorded under NAME -- the split of the chain into its kernels
        --counters: counter collections (csv) of a profiler's run of `--only SAMPLES`, a run of its own, whose FETCH_SIZE per launch of this
        unit's kernels is recorded under NAME next to the bytes the layout counts -- whether the taps hit in cache, measured
    dof_time.py --only SAMPLES [--wide]     20 calls of the chain at SAMPLES taps (--wide: with the wide lens), nothing timed: the run a
                                            profiler's kernel trace or counter collection is taken of"""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
LENS = dict(f_number=2.0, focal_length_mm=50.0, sensor_height_mm=24.0)


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
    """requested_bytes counts P (8) and C (12) for every tap; C is read only where the weight enters, so the rate that decides whether the taps
    must have hit in cache counts P alone: it is the least the taps can have requested"""
    m = statistics.median(ms)
    rate = requested_bytes * pixels / (m * 1e-3)
    least = (floor_bytes + (requested_bytes - floor_bytes) * 8 / 20) * pixels / (m * 1e-3)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "floor_bytes_per_pixel": round(floor_bytes, 2),
            "requested_bytes_per_pixel": round(requested_bytes, 2), "ms_at_the_roof": round(floor_bytes * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4),
            "fraction_of_the_roof": round(floor_bytes * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4), "requested_tb_per_s": round(rate / 1e12, 3),
            "requested_tb_per_s_p_alone": round(least / 1e12, 3), "taps_hit_in_cache": True if least > HBM_ROOF_BYTES_PER_S else "not shown by this figure"}


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def kernel_rows(path):
    """the rows of a kernel statistics csv that name this unit's kernels: {kernel: {calls, average_ns}}"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "k_dof_" in name:
            short = "k_dof_gather_history" if "HistoryColor" in name else [k for k in ("k_dof_prepare", "k_dof_neighbour_max", "k_dof_gather") if k in name][0]
            out[short] = {"calls": int(float(row.get("Calls", 0))), "average_ns": round(float(row.get("AverageNs") or row.get("Average") or 0.0), 1)}
    return out


def counter_rows(path, pixels):
    """FETCH_SIZE per launch of this unit's kernels from a counter collection csv, in bytes per pixel: {kernel: {launches, fetch_bytes_per_pixel}}.
    The counter is in KiB and on gfx950 counts a 128-byte request as 64 bytes (profile_config.sh): reads are doubled, as there"""
    total, launches = {}, {}
    for row in csv.DictReader(open(path)):
        name = row.get("Kernel_Name") or row.get("KernelName") or ""
        if "k_dof_" not in name or row.get("Counter_Name") != "FETCH_SIZE":
            continue
        short = "k_dof_gather_history" if "HistoryColor" in name else [k for k in ("k_dof_prepare", "k_dof_neighbour_max", "k_dof_gather") if k in name][0]
        total[short] = total.get(short, 0.0) + float(row["Counter_Value"])
        launches.setdefault(short, set()).add(row.get("Dispatch_Id"))
    return {k: {"launches": len(launches[k]), "fetch_bytes_per_pixel": round(2 * 1024 * total[k] / len(launches[k]) / pixels, 2)} for k in total}


def motion_blur_per_tap():
    """the motion blur's per-tap cost from its own profile: the chain at 31 samples less the chain at 7, over 24; None without the file"""
    try:
        res = json.load(open(os.path.join(ROOT, "profiles", "motion_blur_cost.json")))["results"]
        return round((res["chain_31_samples"]["ms_median"] - res["chain_7_samples"]["ms_median"]) / 24, 5)
    except (OSError, KeyError, ValueError):
        return None


def main(bench=None, stats=(), only=None, wide=False, counters=()):
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
    d_z = torch.zeros((sc.height, sc.width), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    zn, zf = (float(x) for x in sc.desc.camera["z_near_far"])
    r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    r.depth_plane_device(d_z.data_ptr())
    focus = r.dof_focus_at(sc.width // 2, sc.height // 2, zn, zf)
    scale = min(pkg.renderer.dof_coc_scale(focus_distance=focus, height_px=sc.height, **LENS), 4096.0)
    kw = dict(focus_distance=focus, coc_scale=scale, max_radius=16.0, depth_extent=0.5)
    tables = {n: pkg.renderer.dof_taps(n) for n in (16, 32, 48)}
    chain = lambda samples, coc=scale: r.dof_device(sc.settings, None, d_z.data_ptr(), tables[samples], d_out.data_ptr(), samples=samples, z_near=zn, z_far=zf,
                                                    **dict(kw, coc_scale=coc))
    if only is not None:
        for _ in range(20):
            chain(only, coc=min(8.0 * scale, 4096.0) if wide else scale)
        torch.cuda.synchronize()
        r.close()
        return {"only": only}
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S, "lens": LENS, "z_near_far": [zn, zf],
           "settings": {k: round(float(v), 4) for k, v in kw.items()}}

    # ---- the chain.  Counted per pixel, every plane once: k_dof_prepare depth 4 in, P 8 out; the tile planes 3 x 4 / 64; k_dof_gather C 12 and P 8
    # in, out 12, RGBA8 4 and float LDR 12 out: 60.2.  Requested through the cache on top of that: per tap P 8 and, where the weight enters, C 12
    floor = (4 + 8) + 3 * 4 / 64 + (12 + 8) + (12 + 4 + 12)
    for samples in (16, 32, 48):
        res[f"chain_{samples}_samples"] = figure(timed_ms(lambda: chain(samples), reps=5), floor, floor + samples * 20, pixels)
    def spread(into):
        _, _, _, _, near, prep = r.read_dof(want=("neighbour_max", "prepared"))
        into["tiles_that_gather_fraction"] = round(float((near > 0.5).mean()), 4)
        into["neighbour_max_median_px"] = round(float(np.median(near)), 3)
        into["pixels_out_of_focus_by_more_than_a_pixel_fraction"] = round(float((np.abs(prep[..., 0]) > 1.0).mean()), 4)
    chain(16)
    spread(res)
    # ---- the same with a lens eight times as wide: the discs reach max_radius over much of the frame, so a wave's taps spread over more lines
    wide = res["wide_lens"] = {"coc_scale": round(min(8.0 * scale, 4096.0), 4)}
    for samples in (16, 32, 48):
        wide[f"chain_{samples}_samples"] = figure(timed_ms(lambda: chain(samples, coc=wide["coc_scale"]), reps=5), floor, floor + samples * 20, pixels)
    chain(16, coc=wide["coc_scale"])
    spread(wide)
    wide["per_tap_ms_48_less_16_over_32"] = round((wide["chain_48_samples"]["ms_median"] - wide["chain_16_samples"]["ms_median"]) / 32, 5)
    res["in_focus_chain_16_samples"] = figure(timed_ms(lambda: chain(16, coc=0.0), reps=5), floor, floor, pixels)
    per_tap = (res["chain_48_samples"]["ms_median"] - res["chain_16_samples"]["ms_median"]) / 32
    res["per_tap_ms"] = {"dof_48_less_16_over_32": round(per_tap, 5), "motion_blur_31_less_7_over_24": motion_blur_per_tap()}

    # ---- the one call per frame
    def frame(then_dof, samples=16):
        r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
        if then_dof:
            r.pass_dof(sc.desc, sc.settings, d_out.data_ptr(), tables[samples], samples=samples, **kw)
    res["render_frame"] = med(timed_ms(lambda: frame(False), reps=6))
    for samples in (16, 32, 48):
        res[f"render_frame_then_pass_dof_{samples}_samples"] = med(timed_ms(lambda: frame(True, samples), reps=6))
    res["render_frame_again"] = med(timed_ms(lambda: frame(False), reps=6))
    res["dof_info"] = dict(zip(("device_bytes", "k_dof_gather_launches", "calls"), r.dof_info()[:3]))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded, its HDR plane and the depth plane resident; bytes counted from the layout, not measured; one run of this program: single figures",
           "results": res}
    if stats:
        out["kernels_by_a_profilers_trace"] = {name: kernel_rows(path) for name, path in stats}
    if counters:
        out["fetch_size_by_a_profilers_counters"] = {"how": "rocprofv3 --pmc FETCH_SIZE, a run of its own per case, 20 launches; KiB doubled (gfx950 counts a 128-byte request "
                                                            "as 64 bytes); next to it the layout's count of what each kernel must read once",
                                                     "must_read_once_bytes_per_pixel": {"k_dof_prepare": 4, "k_dof_neighbour_max": round(4 / 64, 3), "k_dof_gather": 20},
                                                     **{name: counter_rows(path, pixels) for name, path in counters}}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    def pairs(flag):
        """NAME=FILE arguments behind `flag`, up to the next option"""
        out = []
        for a in args[args.index(flag) + 1:] if flag in args else []:
            if a.startswith("--"):
                break
            out.append(a.split("=", 1))
        return out
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None, pairs("--kernel-stats"), int(args[args.index("--only") + 1]) if "--only" in args else None,
                  "--wide" in args, pairs("--counters"))
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
