"""ARCTIC_OPT_TEXTURE_MIPS at config 2 (1080p, 2048^2 textures: the config the one-level minification bounds) and config 3 (4K): the shading
pass over a resident G-buffer (time_shade) and whole frames, mode 0 against mode 1 ALTERNATING on one box, each mode over three handles in
turn (own G-buffer, shadow map, textures and output each: the rotation bench.py uses for config 2, so that the cache flatters neither);
the chain's build time per material (create_material under the option minus without it); and, with --asm-log, the new kernels' register
and scratch figures from the compiler's resource remarks (make -C arctic-renderer_amd/csrc asm OUT=dir > log 2>&1).
--pass-only MODE / --frames-only MODE: the program for a counter or kernel-trace run of its own (one handle, the shading pass / whole frames of
that mode, --iters times).
usage: python tools/texture_mips_time.py [--config 2|3] [--out FILE] [--iters N] [--rounds N] [--asm-log FILE] [--pass-only 0|1] [--frames-only 0|1]"""
import argparse, json, os, re, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as e
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=2, choices=(2, 3))
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--asm-log", default=None)
ap.add_argument("--pass-only", type=int, default=None, choices=(0, 1))
ap.add_argument("--frames-only", type=int, default=None, choices=(0, 1))
args = ap.parse_args()
pkg = e.load_package()
sc = pkg.scenes.CONFIGS[args.config](scale=1.0)
N_SETS = 3


def handle(mips):
    r = pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
    r.set_option("texture_mips", mips)
    return sc.upload(r)


if args.pass_only is not None:
    r = handle(args.pass_only)
    r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
    for i in range(args.iters): r.pass_shade(sc.desc, sc.settings)
    r.flush(); r.close()
    sys.exit(0)

if args.frames_only is not None:
    r = handle(args.frames_only)
    out = torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    for i in range(args.iters): r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush(); r.close()
    sys.exit(0)

res = {"config": args.config, "width": sc.width, "height": sc.height, "texture_side": int(sc.materials[0][0].shape[0]), "materials": len(sc.materials),
       "point_lights": int(len(sc.lights)), "iters": args.iters, "rounds": args.rounds, "handles_per_mode": N_SETS}
# the chain's build time: create_material with and without the option, one 2048^2 material (the copy and the packing are in both)
d, n, m = pkg.scenes.make_material_textures(np.random.default_rng(1), 2048)
build = {}
for mips in (0, 1, 0, 1):
    r = pkg.Renderer(64, 64, 0, 16); r.set_option("texture_mips", mips)
    t = time.perf_counter(); r.create_material(d, n, m); build.setdefault(mips, []).append((time.perf_counter() - t) * 1e3)
    r.close()
res["create_material_2048_ms"] = {"mode0": min(build[0]), "mode1": min(build[1]), "chain_build_ms": min(build[1]) - min(build[0])}
print("create_material 2048^2:", res["create_material_2048_ms"], flush=True)

sets = {mips: [handle(mips) for _ in range(N_SETS)] for mips in (0, 1)}
outs = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in range(N_SETS)]
for hs in sets.values():
    for r in hs:
        r.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for every handle (as bench.py does): the passes run one after the other
        r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
shade = {mips: [r.prepared_pass_shade(sc.desc, sc.settings) for r in hs] for mips, hs in sets.items()}
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pass_ms, frame_ms = {0: [], 1: []}, {0: [], 1: []}
for rnd in range(args.rounds):
    for mips in (0, 1):   # alternating
        for i in range(N_SETS): shade[mips][i](outs[i].data_ptr())
        for r in sets[mips]: r.flush()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(args.iters * N_SETS): shade[mips][i % N_SETS](outs[i % N_SETS].data_ptr())
        for r in sets[mips]: r.flush()
        pass_ms[mips].append((time.perf_counter() - t) / (args.iters * N_SETS) * 1e3)
    for mips in (0, 1):
        for i in range(N_SETS): sets[mips][i].render_frame_device(sc.desc, sc.settings, outs[i].data_ptr())
        for r in sets[mips]: r.flush()
        t = time.perf_counter()
        for i in range(args.iters * N_SETS): sets[mips][i % N_SETS].render_frame_device(sc.desc, sc.settings, outs[i % N_SETS].data_ptr())
        for r in sets[mips]: r.flush()
        frame_ms[mips].append((time.perf_counter() - t) / (args.iters * N_SETS) * 1e3)
    print(f"round {rnd}: pass {pass_ms[0][-1]:.4f} / {pass_ms[1][-1]:.4f} ms, frame {frame_ms[0][-1]:.4f} / {frame_ms[1][-1]:.4f} ms (mode 0 / mode 1)", flush=True)
# one handle, back to back (warm caches): arctic_time_shade's own events
for mips in (0, 1):
    ms = sets[mips][0].time_shade(sc.desc, sc.settings, warmup=3, iters=args.iters)
    res[f"mode{mips}"] = {"pass_ms_rotating_median": float(np.median(pass_ms[mips])), "pass_ms_rotating_all": pass_ms[mips],
                          "frame_ms_rotating_median": float(np.median(frame_ms[mips])), "frame_ms_rotating_all": frame_ms[mips],
                          "pass_ms_one_handle_median": float(np.median(ms)), "pass_ms_one_handle_min": float(np.min(ms))}
res["pass_ratio_mode1_over_mode0"] = res["mode1"]["pass_ms_rotating_median"] / res["mode0"]["pass_ms_rotating_median"]
res["frame_ratio_mode1_over_mode0"] = res["mode1"]["frame_ms_rotating_median"] / res["mode0"]["frame_ms_rotating_median"]
lod = sets[1][0].read_lod()
res["lod_plane"] = {"mean": float(lod.mean()), "median": float(np.median(lod)), "max": float(lod.max()), "share_above_1": float((lod > 1).mean())}
for hs in sets.values():
    for r in hs: r.close()
if args.asm_log:
    regs, name = {}, None
    for line in open(args.asm_log):
        mm = re.search(r"Function Name: (\S+)", line)
        if mm: name = mm.group(1)
        mm = re.search(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if mm and name and ("k_miplit" in name or "k_resolve_lod" in name or "k_mip_reduce" in name):
            regs.setdefault(name, {})[mm.group(1)] = int(mm.group(2))
    res["kernel_resources"] = regs
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
