"""Cost of auto-exposure (arctic_exposure_device; csrc/exposure.hip) on one MI355X; the numbers of DESIGN.md 6w / profiles/exposure_cost.json.

Config 3 at 3840 x 2160, a frame drawn with the float HDR plane kept.  Three planes are metered: that frame, a constant plane (every lane of every
wave on one bin: the worst case of an LDS atomic) and a plane that cycles all 256 bins along a row (no two neighbouring lanes on one bin).
Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Beside each figure the bytes
COUNTED from the layout -- the meter reads 12 B per pixel, the apply reads 12 and writes 12 + 4 + 12 -- and that floor's time at 8 TB/s.  Every
figure is of ONE run.

How k_exposure_meter meets contention and how many workgroups it gets are chosen by measurement: exposure.hip, exposure.cpp and
exposure_calls.cpp built with -DARCTIC_EXPOSURE_METER_VARIANT=V -DARCTIC_EXPOSURE_MAX_GROUPS=G into a library of their own, which only this
tool does; each library is timed in a process of its own (ARCTIC_HIP_LIBRARY) with `--meter`.

    exposure_time.py --build-variant FILE.so V G    (no GPU) builds that library from the objects of a built tree, with the Makefile's flags, and
                                                    leaves FILE.json beside it, which `--meter` records
    exposure_time.py --meter                        meter + resolve (ARCTIC_EXPOSURE_METER_ONLY) on the three planes, one JSON line
    exposure_time.py --only                         20 calls of each kind and 20 of bloom's chain at one level, nothing timed: the run a
                                                    profiler's kernel trace is taken of (k_bloom_composite is the apply's yardstick)
    exposure_time.py [--out FILE] [--variants FILE.json ...] [--bench FILE] [--kernel-stats NAME=FILE.csv ...]
        prints one JSON line and, with --out, writes it there; --variants: outputs of `--meter` under the variant libraries; --bench: a JSON
        file of bench.py result lines of the parent's library and this build; --kernel-stats: kernel statistics (csv) of a profiler's run of
        `--only`, whose rows for this unit's kernels and k_bloom_composite are recorded under NAME next to each kernel's floor"""
import csv
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
METER_ONLY, HOLD = 256, 128
RECORD = dict(low=0.5, high=0.95, key_value=0.18, rate_up=0.1, rate_down=0.05)


def build_variant(out, variant, groups):
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    objs = []
    for line in make.splitlines():
        if line.startswith("OBJS"):
            objs += line.split("=", 1)[1].split()
    missing = [o for o in objs if not os.path.exists(os.path.join(csrc, o))]
    if missing:
        raise SystemExit(f"build the library first (make -C {csrc}): {missing[:3]} ... are not there")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    stem = os.path.splitext(os.path.abspath(out))[0]
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    var = {"ARCH": "gfx950"}                                                     # the Makefile's own flags: COMMON, and EXACT where the unit is built with it
    for line in make.splitlines():
        m = re.match(r"(ARCH|COMMON|EXACT)\s*[:?]?=\s*(.*)", line)
        if m:
            var[m.group(1)] = m.group(2)
    flags = lambda name: re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var[name]).split()
    common = [hipcc] + flags("COMMON") + [f"-DARCTIC_EXPOSURE_METER_VARIANT={int(variant)}", f"-DARCTIC_EXPOSURE_MAX_GROUPS={int(groups)}"]
    swap = {}
    for obj, src, exact in (("exposure.o", "exposure.hip", True), ("exposure_host.o", "exposure.cpp", True), ("exposure_calls.o", "exposure_calls.cpp", False)):
        swap[obj] = f"{stem}_{obj}"
        subprocess.run(common + (flags("EXACT") if exact else []) + ["-c", src, "-o", swap[obj]], check=True, cwd=csrc)
    subprocess.run([hipcc, f"--offload-arch={var['ARCH']}", "-shared", "-fPIC", "-o", os.path.abspath(out)] + [swap.get(o, o) for o in objs], check=True, cwd=csrc)
    json.dump({"variant": int(variant), "max_groups": int(groups)}, open(stem + ".json", "w"))      # beside the library: `--meter` records it
    return {"built": out, "variant": int(variant), "max_groups": int(groups)}


def built_as():
    """what the library under ARCTIC_HIP_LIBRARY was built with: the record `--build-variant` left beside it, else the sources' defaults"""
    beside = os.path.splitext(os.environ.get("ARCTIC_HIP_LIBRARY", ""))[0] + ".json"
    if os.environ.get("ARCTIC_HIP_LIBRARY") and os.path.exists(beside):
        return json.load(open(beside))
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    default = lambda unit, name: int(re.search(r"#define " + name + r" (\d+)", open(os.path.join(csrc, unit)).read()).group(1))
    return {"variant": default("exposure.hip", "ARCTIC_EXPOSURE_METER_VARIANT"), "max_groups": default("exposure.h", "ARCTIC_EXPOSURE_MAX_GROUPS")}


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


def med(ms, floor_bytes=None):
    out = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    if floor_bytes:
        out.update(floor_bytes=floor_bytes, ms_at_the_roof=round(floor_bytes / HBM_ROOF_BYTES_PER_S * 1e3, 4),
                   fraction_of_the_roof=round(floor_bytes / (statistics.median(ms) * 1e-3) / HBM_ROOF_BYTES_PER_S, 4))
    return out


def kernel_rows(path, floor):
    """the rows of a kernel statistics csv that name this unit's kernels and k_bloom_composite: {kernel: {calls, average_ns, floor}}"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        short = [k for k in ("k_exposure_meter", "k_exposure_resolve", "k_exposure_apply", "k_bloom_composite") if k in name][:1]
        if not short:
            continue
        key = short[0] + ("_history" if "HistoryColor" in name else "")
        out[key] = {"calls": int(float(row.get("Calls", 0))), "average_ns": round(float(row.get("AverageNs") or row.get("Average") or 0.0), 1)}
        if short[0] in floor:
            out[key].update(floor_bytes=floor[short[0]], floor_ns_at_the_roof=round(floor[short[0]] / HBM_ROOF_BYTES_PER_S * 1e9, 1))
    return out


def main(mode=None, variants=(), bench=None, stats=()):
    global torch
    import numpy as np
    import torch
    import __graft_entry__ as entry
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    W, H = sc.width, sc.height
    pixels = W * H
    r = sc.upload(pkg.Renderer(W, H, sc.shadow_size, sc.max_lights))
    r.set_option("keep_float_output", 1)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    constant = torch.full((H, W, 3), 0.37, dtype=torch.float32, device="cuda")
    keys = ((np.arange(W, dtype=np.uint32) % 256 + 888) << 20 | (1 << 19)).view(np.float32)
    cycle = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(keys[None, :, None], (H, W, 3)))).cuda()
    torch.cuda.synchronize()
    planes = {"rendered_frame": None, "constant_plane": constant.data_ptr(), "bin_cycle_plane": cycle.data_ptr()}
    lay = pkg.renderer.exposure_layout(W, H)
    library = os.path.basename(os.environ.get("ARCTIC_HIP_LIBRARY", "libarctic_hip.so"))
    floor = {"k_exposure_meter": 12 * pixels, "k_exposure_resolve": lay["table_bytes"] + 1024 + 64, "k_exposure_apply": (12 + 12 + 4 + 12) * pixels,
             "k_bloom_composite": (12 + 3 + 12 + 4 + 12) * pixels}
    meter = lambda ptr: (lambda: r.exposure_device(sc.settings, ptr, None, flags=METER_ONLY, **RECORD))
    hold = lambda: r.exposure_device(sc.settings, None, d_out.data_ptr(), flags=HOLD, **RECORD)
    full = lambda: r.exposure_device(sc.settings, None, d_out.data_ptr(), **RECORD)
    bloom1 = lambda: r.bloom_device(sc.settings, None, d_out.data_ptr(), threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=0.75, levels=1)
    if mode == "only":
        for fn in [meter(p) for p in planes.values()] + [hold, full, bloom1]:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        r.close()
        return {"only": True, "library": library}
    metered = {name: med(timed_ms(meter(ptr), reps=20), floor["k_exposure_meter"]) for name, ptr in planes.items()}
    worst = max(v["ms_median"] for v in metered.values())
    if mode == "meter":
        r.close()
        return dict(built_as(), library=library, layout=lay, meter_and_resolve=metered, worst_ms=worst)
    res = {"built_as": built_as(), "config": 3, "size": [W, H], "pixels": pixels, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S, "record": RECORD, "layout": lay,
           "meter_and_resolve": metered, "meter_and_resolve_worst_ms": worst}
    res["floor_by_kernel"] = {k: {"bytes": v, "ms_at_the_roof": round(v / HBM_ROOF_BYTES_PER_S * 1e3, 5)} for k, v in floor.items()}
    full()
    res["apply_alone_HOLD"] = med(timed_ms(hold, reps=20), floor["k_exposure_apply"])
    res["whole_call"] = med(timed_ms(full, reps=20), floor["k_exposure_meter"] + floor["k_exposure_apply"])
    res["bloom_one_level_two_launches"] = med(timed_ms(bloom1, reps=20))

    def frame(then_exposure):
        r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
        if then_exposure:
            full()
    res["render_frame"] = med(timed_ms(lambda: frame(False), reps=6))
    res["render_frame_then_exposure"] = med(timed_ms(lambda: frame(True), reps=6))
    res["render_frame_again"] = med(timed_ms(lambda: frame(False), reps=6))
    r.exposure_device(sc.settings, None, None, **dict(RECORD, flags=64))
    state = r.read_exposure(want=("state",))[4]
    res["state_of_the_rendered_frame"] = {k: (float(state[k][0]) if state[k].dtype.kind == "f" else int(state[k][0])) for k in state.dtype.names}
    res["exposure_info"] = dict(zip(("device_bytes", "k_exposure_apply_launches", "calls", "k_exposure_meter_launches"), r.exposure_info()))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded and its HDR plane resident; bytes counted from the layout, not measured; one run of this program: single figures",
           "results": res}
    if variants:
        rows = [json.load(open(p)) for p in variants]
        out["meter_variants"] = {"how": "the same three planes under libraries built with -DARCTIC_EXPOSURE_METER_VARIANT (0: one histogram per workgroup, plain LDS adds; 1: one per wave; "
                                        "2: a wave whose lanes share one bin adds their count once) and -DARCTIC_EXPOSURE_MAX_GROUPS, a process each; ms are meter + resolve",
                                 "rows": rows}
    if stats:
        out["kernels_by_a_profilers_trace"] = {name: kernel_rows(path, floor) for name, path in stats}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--build-variant" in args:
        at = args.index("--build-variant")
        print(json.dumps(build_variant(args[at + 1], args[at + 2], args[at + 3])))
        sys.exit(0)

    def behind(flag):
        """the arguments behind `flag`, up to the next option"""
        out = []
        for a in args[args.index(flag) + 1:] if flag in args else []:
            if a.startswith("--"):
                break
            out.append(a)
        return out
    result = main("only" if "--only" in args else "meter" if "--meter" in args else None, behind("--variants"), args[args.index("--bench") + 1] if "--bench" in args else None,
                  [a.split("=", 1) for a in behind("--kernel-stats")])
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
