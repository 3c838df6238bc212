"""Cost of bloom (arctic_bloom_device; csrc/bloom.hip) on one MI355X; the numbers of DESIGN.md 6v / profiles/bloom_cost.json.

Config 3 at 3840 x 2160, a frame drawn with the float HDR plane kept, then the chain of 2 L = 12 launches at L = 6 levels on that plane into a
device RGBA8 buffer; the fraction of pixels above the threshold is recorded, since the work does not depend on it (every pixel is prefiltered
and every level is written whatever it holds).  Beside each figure the bytes COUNTED from the layout (arctic_bloom_layout): what each kernel
must move when every plane is read once and written once -- the floor -- and that floor's time at 8 TB/s.  The taps on top of it (36 per pixel
of a level on the way down, 16 on the way up) go through LDS in k_bloom_down_first and through the cache elsewhere.  Milliseconds: torch events
on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

k_bloom_down_first against its unstaged variant (the prefilter per tap through the cache, no LDS): bloom.hip built with -DARCTIC_BLOOM_UNSTAGED
into a library of its own, which only this tool does; the two libraries are timed in a process each (ARCTIC_HIP_LIBRARY) and split into kernels
by a profiler's trace of `--only`.

    bloom_time.py --build-unstaged FILE.so      (no GPU) builds that library from the objects of a built tree
    bloom_time.py [--out FILE] [--unstaged FILE.json] [--bench FILE] [--kernel-stats NAME=FILE.csv ...]
        prints one JSON line and, with --out, writes it there; --unstaged: the output of `--chain` under the unstaged library; --bench: a JSON file
        of bench.py result lines of this build and the parent's library, recorded beside the figures as given; --kernel-stats: kernel statistics
        (csv) of a profiler's run of `--only`, whose rows for this unit's kernels are recorded under NAME next to each kernel's floor
    bloom_time.py --chain                       the chain's time alone, as one JSON line
    bloom_time.py --only                        20 calls of the chain, nothing timed: the run a profiler's kernel trace is taken of"""
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
LEVELS = 6
RECORD = dict(threshold=1.0, soft_knee=0.5, clamp_max=65504.0, intensity=0.5, spread=0.75, levels=LEVELS)


def build_unstaged(out):
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    objs = [o for o in make.split("OBJS")[1].split("\n")[0].replace(":=", "").split()]
    missing = [o for o in objs if not os.path.exists(os.path.join(csrc, o))]
    if missing:
        raise SystemExit(f"build the library first (make -C {csrc}): {missing[:3]} ... are not there")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.splitext(out)[0] + "_bloom.o"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "--offload-arch=gfx950", "-ffp-contract=off", "-DARCTIC_BLOOM_UNSTAGED", "-c", "bloom.hip", "-o",
                    os.path.abspath(obj)], check=True, cwd=csrc)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.abspath(out)] + [os.path.abspath(obj) if o == "bloom.o" else o for o in objs], check=True, cwd=csrc)
    return {"built": out}


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


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def floors(lay, width, height):
    """bytes each kernel must move when every plane is read once and written once, from the layout: {kernel: bytes} summed over its launches"""
    px = [width * height] + [w * h for w, h in lay["sizes"]]                   # pixels of level 0 .. L
    L = len(lay["sizes"])
    return {"k_bloom_down_first": 12 * px[0] + 12 * px[1],
            "k_bloom_down": sum(12 * px[k - 1] + 12 * px[k] for k in range(2, L + 1)),
            "k_bloom_up": sum(12 * px[k] + 12 * px[k + 1] + 12 * px[k] for k in range(1, L)),
            "k_bloom_composite": 12 * px[1] + 12 * px[0] + (12 + 4 + 12) * px[0]}


def kernel_rows(path, floor):
    """the rows of a kernel statistics csv that name this unit's kernels: {kernel: {calls, average_ns, per-call floor and its time at the roof}}.
    k_bloom_down and k_bloom_up run L - 1 levels of falling size: their row averages over them, and so does the floor beside it"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        short = [k for k in ("k_bloom_down_first", "k_bloom_composite", "k_bloom_up", "k_bloom_down") if k in name][:1]   # (the longer name first)
        if "k_bloom_" not in name or not short:
            continue
        key = short[0] + ("_history" if "HistoryColor" in name else "")
        calls = int(float(row.get("Calls", 0)))
        per_chain = {"k_bloom_down": LEVELS - 1, "k_bloom_up": LEVELS - 1}.get(short[0], 1)
        out[key] = {"calls": calls, "average_ns": round(float(row.get("AverageNs") or row.get("Average") or 0.0), 1), "launches_per_chain": per_chain,
                    "floor_bytes_per_launch": round(floor[short[0]] / per_chain), "floor_ns_per_launch_at_the_roof": round(floor[short[0]] / per_chain / HBM_ROOF_BYTES_PER_S * 1e9, 1)}
    return out


def main(bench=None, stats=(), mode=None, unstaged=None):
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
    d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    chain = lambda: r.bloom_device(sc.settings, None, d_out.data_ptr(), **RECORD)
    library = os.path.basename(os.environ.get("ARCTIC_HIP_LIBRARY", "libarctic_hip.so"))
    if mode == "only":
        for _ in range(20):
            chain()
        torch.cuda.synchronize()
        r.close()
        return {"only": LEVELS, "library": library}
    if mode == "chain":
        out = {"library": library, "chain": med(timed_ms(chain, reps=5))}
        r.close()
        return out
    lay = pkg.renderer.bloom_layout(sc.width, sc.height, LEVELS)
    floor = floors(lay, sc.width, sc.height)
    total = sum(floor.values())
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S, "record": RECORD, "launches_per_chain": 2 * LEVELS,
           "levels": lay["sizes"], "pyramid_floats": [lay["down_floats"], lay["up_floats"]]}
    ms = timed_ms(chain, reps=5)
    res["chain"] = dict(med(ms), floor_bytes=total, floor_bytes_per_pixel=round(total / pixels, 2), ms_at_the_roof=round(total / HBM_ROOF_BYTES_PER_S * 1e3, 4),
                        fraction_of_the_roof=round(total / (statistics.median(ms) * 1e-3) / HBM_ROOF_BYTES_PER_S, 4))
    res["floor_by_kernel"] = {k: {"bytes": v, "ms_at_the_roof": round(v / HBM_ROOF_BYTES_PER_S * 1e3, 5)} for k, v in floor.items()}

    # ---- behind a frame
    def frame(then_bloom):
        r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
        if then_bloom:
            chain()
    res["render_frame"] = med(timed_ms(lambda: frame(False), reps=6))
    res["render_frame_then_bloom"] = med(timed_ms(lambda: frame(True), reps=6))
    res["render_frame_again"] = med(timed_ms(lambda: frame(False), reps=6))
    r.render_frame(sc.desc, sc.settings)                                         # (into the handle's own buffers, which read_output reads)
    chain()
    hdr, out = r.read_output(want=("hdr",))[1], r.read_bloom(LEVELS, want=("hdr",))[1]
    res["pixels_above_the_threshold_fraction"] = round(float((np.nanmax(hdr, -1) > RECORD["threshold"]).mean()), 4)
    res["pixels_changed_fraction"] = round(float((out != hdr).any(-1).mean()), 4)
    res["bloom_info"] = dict(zip(("device_bytes", "k_bloom_composite_launches", "calls"), r.bloom_info()[:3]))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded and its HDR plane resident; bytes counted from the layout, not measured; one run of this program: single figures",
           "results": res}
    if unstaged:
        other = json.load(open(unstaged))
        out["k_bloom_down_first_unstaged"] = {"how": "the same chain under a library whose bloom.hip was built with -DARCTIC_BLOOM_UNSTAGED (prefilter per tap, no LDS), a process of its own; "
                                                     "the chains differ in that one kernel alone", "unstaged": other, "staged_chain": res["chain"]["ms_median"],
                                              "staged_less_unstaged_ms": round(res["chain"]["ms_median"] - other["chain"]["ms_median"], 4)}
    if stats:
        out["kernels_by_a_profilers_trace"] = {name: kernel_rows(path, floor) for name, path in stats}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--build-unstaged" in args:
        print(json.dumps(build_unstaged(args[args.index("--build-unstaged") + 1])))
        sys.exit(0)

    def pairs(flag):
        """NAME=FILE arguments behind `flag`, up to the next option"""
        out = []
        for a in args[args.index(flag) + 1:] if flag in args else []:
            if a.startswith("--"):
                break
            out.append(a.split("=", 1))
        return out
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None, pairs("--kernel-stats"), "only" if "--only" in args else "chain" if "--chain" in args else None,
                  args[args.index("--unstaged") + 1] if "--unstaged" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
