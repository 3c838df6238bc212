"""What arctic_set_material_extras costs the shading pass at config 3 (4K, 64 point lights), through arctic_time_shade on ONE handle whose
materials are switched between four states, in turn and repeatedly (one box, one G-buffer, one shadow map):
  default             every material neutral: k_material, the fast tile
  one_extended        ONE material with factors only: every tile through k_pbrlit, neutral records for the rest
  all_same_size       every material with an emissive and an occlusion image of its own size (the fast path: one 4-byte texel)
  all_other_size      every material with an emissive and an occlusion image of other sizes (the cold path: two plain images)
and, with --asm-log, the new kernels' register, scratch and occupancy figures from the compiler's resource remarks
(make -C arctic-renderer_amd/csrc asm OUT=dir > log 2>&1).
usage: python tools/material_extras_time.py [--out FILE] [--iters N] [--rounds N] [--lights N] [--scale S] [--asm-log FILE]"""
import argparse, json, os, re, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as e

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--lights", type=int, default=64)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--asm-log", default=None)
args = ap.parse_args()
pkg = e.load_package()
res = {"config": 3, "iters": args.iters, "rounds": args.rounds}
if args.asm_log:
    regs, name = {}, None
    for line in open(args.asm_log):
        mm = re.search(r"Function Name: (\S+)", line)
        if mm: name = mm.group(1)
        mm = re.search(r"(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if mm and name and "k_pbrlit" in name:
            regs.setdefault(name, {})[mm.group(1)] = int(mm.group(2))
    res["kernel_resources"] = regs

sc = pkg.scenes.CONFIGS[3](scale=args.scale)
n_lights = max(args.lights, len(sc.lights))
r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, n_lights))
rng = np.random.default_rng(3)
if len(sc.lights) != args.lights:   # (config 3 carries 64 of its own)
    r.update_lights(pkg.scenes.random_lights(rng, args.lights, (-14, 1, -6), (14, 11, 6), intensity=30.0))
r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
side = int(sc.materials[0][0].shape[0])
res.update(width=sc.width, height=sc.height, point_lights=args.lights, materials=len(sc.materials), texture_side=side)


def image(w, h):
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., 3] = 255
    return a


factors = pkg.scene.neutral_material_params()
factors["base_color_factor"], factors["metallic_factor"], factors["roughness_factor"], factors["normal_scale"] = (0.9, 0.8, 0.7), 0.8, 0.9, 1.2
factors["occlusion_strength"], factors["emissive_factor"] = 0.8, (0.2, 0.1, 0.3)
same = (image(side, side), image(side, side))
other = (image(side // 2, side // 4), image(side // 4, side // 2))
M = range(len(sc.materials))


def state(name):
    for m in M:
        if name == "default" or (name == "one_extended" and m != 0): r.set_material_extras(m)
        elif name == "one_extended": r.set_material_extras(m, factors[0])
        elif name == "all_same_size": r.set_material_extras(m, factors[0], *same)
        else: r.set_material_extras(m, factors[0], *other)


STATES = ("default", "one_extended", "all_same_size", "all_other_size")
ms = {s: [] for s in STATES}
for rnd in range(args.rounds):
    for s in STATES:
        state(s)
        t = r.time_shade(sc.desc, sc.settings, warmup=5, iters=args.iters)
        ms[s].append(float(np.median(t)))
    print(f"round {rnd}: " + ", ".join(f"{s} {ms[s][-1]:.4f} ms" for s in STATES), flush=True)
for s in STATES:
    res[s] = {"pass_ms_median": float(np.median(ms[s])), "pass_ms_all": ms[s]}
for s in STATES[1:]:
    res[s]["ratio_to_default"] = res[s]["pass_ms_median"] / res["default"]["pass_ms_median"]
r.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
