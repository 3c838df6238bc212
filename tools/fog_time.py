"""Cost of volumetric fog (arctic_fog_device, arctic_pass_fog; csrc/fog.hip) on one MI355X; the numbers of DESIGN.md 6x / profiles/fog_cost.json.

Config 3 at 3840 x 2160, a frame drawn (which draws the sun's map), its depth plane extracted and the scene's view record built
(arctic_fog_view); density 0.05, g 0.5, max_distance 60, the shuffled offset table.
  arctic_fog_device             k_fog_march on the handle's HDR plane at 16, 32 and 64 steps, and with density 0 (the march still runs: the
                                lookups do not depend on the density), and with a hostile view whose samples all fall outside the map (no
                                lookup is made: the arithmetic alone)
  arctic_pass_fog per frame     behind arctic_render_frame_device, next to the frames alone in the same run
Beside each figure the bytes per pixel COUNTED from the layout: colour 12 and depth 4 in, HDR 12, RGBA8 4 and float LDR 12 out = 44, the floor;
and the lookups the march requests through the cache, 4 bytes each.  Milliseconds: torch events on torch's stream around back-to-back calls,
median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    fog_time.py [--out FILE] [--bench FILE] [--variant NAME=FILE.json ...]
        prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py result lines of this build and the parent's
        library, recorded beside the figures as given; --variant: the output of `--chain` under another library, recorded under NAME
    fog_time.py --chain         the march at 16, 32 and 64 steps alone, under the library ARCTIC_HIP_LIBRARY names: one JSON line
    fog_time.py --only STEPS    20 calls of the march at STEPS steps, nothing timed: the run a profiler's kernel trace is taken of
    fog_time.py --build-table FILE.so [--every-call]   (no GPU) builds a library whose k_fog_march asks a min/max table of 4 x 4 texel blocks
                                first and reads the map only where the table does not decide (-DARCTIC_FOG_TABLE_VARIANT=1, set by this
                                tool alone: the table is built once from the map of the first call; --every-call: =2, built again in
                                front of every march)"""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
FOG = dict(density=0.05, anisotropy=0.5, max_distance=60.0, bias=0.002, scatter_color=(4.0, 3.6, 3.0), ambient_color=(0.02, 0.03, 0.05))
FLOOR = 12 + 4 + 12 + 4 + 12


def build_table(out, every_call=False):
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    objs = [o for line in re.findall(r"^OBJS\s*[:+]=(.*)$", make, flags=re.M) for o in line.split()]
    missing = [o for o in objs if not os.path.exists(os.path.join(csrc, o))]
    if missing:
        raise SystemExit(f"build the library first (make -C {csrc}): {missing[:3]} ... are not there")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    common = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "--offload-arch=gfx950", "-DARCTIC_FOG_TABLE_VARIANT=" + ("2" if every_call else "1")]
    stem = os.path.splitext(os.path.abspath(out))[0]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    subprocess.run([hipcc] + common + ["-ffp-contract=off", "-c", "fog.hip", "-o", stem + "_fog.o"], check=True, cwd=csrc)
    subprocess.run([hipcc] + common + ["-c", "fog_calls.cpp", "-o", stem + "_fog_calls.o"], check=True, cwd=csrc)
    swap = {"fog.o": stem + "_fog.o", "fog_calls.o": stem + "_fog_calls.o"}
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.abspath(out)] + [swap.get(o, o) for o in objs], check=True, cwd=csrc)
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


def figure(ms, steps, pixels):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "floor_bytes_per_pixel": FLOOR, "lookups_per_pixel": steps,
            "ms_at_the_roof": round(FLOOR * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4), "fraction_of_the_roof": round(FLOOR * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4),
            "lookups_per_ns": round(steps * pixels / (m * 1e6), 2)}


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def main(bench=None, variants=(), only=None, chain_only=False):
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
    r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    r.depth_plane_device(d_z.data_ptr())
    view = pkg.renderer.fog_view(sc.desc, sc.width, sc.height)
    offsets = pkg.renderer.fog_offsets(1)
    march = lambda steps, v=view, **kw: r.fog_device(sc.settings, v, None, d_z.data_ptr(), None, d_out.data_ptr(), offsets, steps=steps, **dict(FOG, **kw))
    if only is not None:
        for _ in range(20):
            march(only)
        torch.cuda.synchronize()
        r.close()
        return {"only": only}
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "shadow_size": sc.shadow_size, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S,
           "settings": {k: v for k, v in FOG.items()}, "library": os.environ.get("ARCTIC_HIP_LIBRARY", "this build")}
    for steps in (16, 32, 64):
        res[f"march_{steps}_steps"] = figure(timed_ms(lambda: march(steps), reps=5), steps, pixels)
    res["per_step_ms_64_less_16_over_48"] = round((res["march_64_steps"]["ms_median"] - res["march_16_steps"]["ms_median"]) / 48, 5)
    if chain_only:
        r.close()
        return {"results": res}
    # what the march met: the share of the frame the fog changed, and the share whose march met a shadow
    r.fog_device(sc.settings, view, None, d_z.data_ptr(), None, d_out.data_ptr(), offsets, steps=32, **dict(FOG, density=0.0))
    shaded = r.read_fog(want=("hdr",))[1]                                        # (density 0 returns the colour by bits)
    r.fog_device(sc.settings, view, None, d_z.data_ptr(), None, d_out.data_ptr(), offsets, steps=32, **FOG)
    fogged = r.read_fog(want=("hdr",))[1]
    res["pixels_changed_fraction_32_steps"] = round(float((fogged != shaded).any(-1).mean()), 4)
    lit = dict(FOG, bias=1.0)                                                    # every compare passes: what the shadowed samples took out of the in-scattering
    r.fog_device(sc.settings, view, None, d_z.data_ptr(), None, d_out.data_ptr(), offsets, steps=32, **lit)
    all_lit = r.read_fog(want=("hdr",))[1]
    res["pixels_with_a_shadowed_sample_fraction_32_steps"] = round(float((all_lit != fogged).any(-1).mean()), 4)
    res["density_0_32_steps"] = figure(timed_ms(lambda: march(32, density=0.0), reps=5), 32, pixels)
    hostile = view.copy()
    hostile["light"][0][0][3] = -8.0                                             # every u is far below 0: no sample is inside, no lookup is made
    res["no_lookup_32_steps"] = figure(timed_ms(lambda: march(32, v=hostile), reps=5), 0, pixels)
    res["no_lookup_64_steps"] = figure(timed_ms(lambda: march(64, v=hostile), reps=5), 0, pixels)

    # ---- the one call per frame
    def frame(then_fog, steps=32):
        r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
        if then_fog:
            r.pass_fog(sc.desc, sc.settings, d_out.data_ptr(), offsets, steps=steps, **FOG)
    res["render_frame"] = med(timed_ms(lambda: frame(False), reps=6))
    for steps in (16, 32, 64):
        res[f"render_frame_then_pass_fog_{steps}_steps"] = med(timed_ms(lambda: frame(True, steps), reps=6))
    res["render_frame_again"] = med(timed_ms(lambda: frame(False), reps=6))
    res["fog_info"] = dict(zip(("device_bytes", "k_fog_march_launches", "calls", "table_uploads"), r.fog_info()))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded, its HDR plane, the depth plane and the sun's map resident; bytes counted from the layout, not measured; one run of this program: single figures",
           "results": res}
    if variants:
        out["variants"] = {name: json.load(open(path)) for name, path in variants}
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
    if "--build-table" in args:
        print(json.dumps(build_table(args[args.index("--build-table") + 1], "--every-call" in args)))
        sys.exit(0)
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None, pairs("--variant"), int(args[args.index("--only") + 1]) if "--only" in args else None, "--chain" in args)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
