"""Cost of composing ray-traced occlusion and reflections into the shaded frame (arctic_compose_planes_device, arctic_pass_ray_effects;
csrc/compose.hip) on one MI355X; the numbers of DESIGN.md 6p / profiles/compose_cost.json.

Config 3 at 3840 x 2160 with the sun's map drawn, the G-buffer resident and the frame shaded under ARCTIC_OPT_KEEP_FLOAT_OUTPUT.  The two planes
are traced once into buffers of the caller's (4 occlusion rays per pixel over 4 x 4 pixels, radius a tenth of the scene's diagonal; the reflection
plane at a bias of 1e-3 of the diagonal); then k_compose alone on those planes with each flag and with both, into a device buffer of the
caller's; then the one call, which traces both planes again every time.  Per case: milliseconds (torch events on torch's stream around
back-to-back calls, median of 7 rounds after 2 warm-up calls).  Beside each k_compose figure stand the bytes per pixel the algorithm needs --
counted from the layout below, not measured -- and the fraction of the 8 TB/s HBM roof they amount to at the measured time.  Every figure is of
ONE run of this program.

    compose_time.py [--out FILE] [--bench FILE]      prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py
                                                     result lines of this build and the parent's library, recorded beside the figures as given"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_ROOF_BYTES_PER_S = 8e12


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


def bytes_per_pixel(ao, refl, covered, reflecting):
    """what k_compose has to move per pixel, from the layout: hdr in (12), RGBA8 + float LDR + composed HDR out (4 + 12 + 12), the material word of
    plane b (12: the plane's stride) for every pixel; for a covered pixel with a term to add plane a (16); the occlusion byte (1); the
    reflection (16) and, where refl.a > 0, planes c and e (32).  Texels and descriptors are not counted (a 2 x 2 footprint of 8-byte texels that
    neighbouring pixels share)"""
    b = 12 + 28 + 12
    b += (1 if ao else 0) + (16 if refl else 0)
    b += 16 * (covered if ao else reflecting)
    b += 32 * reflecting if refl else 0
    return b


def main(bench=None):
    global np, torch
    import numpy as np
    import torch
    import __graft_entry__ as entry
    import ray_reference as R
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.set_option("keep_float_output", 1)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    _, material, _, _ = r.read_gbuffer(want=("material",))
    tris, _ = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo))
    pixels = sc.width * sc.height
    covered = float((material != 0xFFFFFFFF).mean())
    dirs = pkg.renderer.ao_directions(4, 4, seed=3)
    ao_kw = dict(radius=0.1 * diagonal, bias=1e-3 * diagonal)
    bias = 1e-3 * diagonal
    d_ao = torch.zeros((sc.height, sc.width), dtype=torch.uint8, device="cuda")
    d_refl = torch.zeros((sc.height, sc.width, 4), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.trace_ambient_occlusion_device(sc.desc, dirs, d_ao.data_ptr(), **ao_kw)
    r.trace_reflections_device(sc.desc, bias, d_refl.data_ptr())
    r.flush()
    reflecting = float(((d_refl[..., 3] > 0).float().mean()).item())
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "covered_fraction": round(covered, 4), "reflecting_fraction": round(reflecting, 4),
           "mean_visibility": round(float(d_ao.float().mean().item()) / 255.0, 4), "scene_diagonal": round(diagonal, 3), "point_lights": len(sc.lights),
           "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S}
    cases = {"k_compose_ao": (d_ao.data_ptr(), None), "k_compose_reflections": (None, d_refl.data_ptr()), "k_compose_both": (d_ao.data_ptr(), d_refl.data_ptr())}
    for name, (pa, pr) in cases.items():
        ms = timed_ms(lambda: r.compose_planes_device(sc.desc, sc.settings, pa, pr, d_out_ptr=d_out.data_ptr()), reps=5)
        m = statistics.median(ms)
        bpp = bytes_per_pixel(pa is not None, pr is not None, covered, reflecting)
        res[name] = {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "algorithmic_bytes_per_pixel": round(bpp, 2),
                     "ms_at_the_roof": round(bpp * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4), "fraction_of_the_roof": round(bpp * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4)}
    frame = d_out.cpu().numpy()
    shaded = r.read_output(want=("rgba8",))[2]
    res["pixels_the_composition_changes_fraction"] = round(float((frame != shaded).any(-1).mean()), 4)
    one = lambda: r.pass_ray_effects(sc.desc, sc.settings, dirs=dirs, reflection_bias=bias, d_out_ptr=d_out.data_ptr(), **ao_kw)
    ms = timed_ms(one, reps=2)
    res["arctic_pass_ray_effects_4_rays_per_pixel"] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    t_ao = timed_ms(lambda: r.trace_ambient_occlusion_device(sc.desc, dirs, d_ao.data_ptr(), **ao_kw), reps=2)
    t_refl = timed_ms(lambda: r.trace_reflections_device(sc.desc, bias, d_refl.data_ptr()), reps=2)
    t_pass = timed_ms(lambda: r.pass_shade(sc.desc, sc.settings), reps=3)
    res["for_context"] = {"arctic_trace_ambient_occlusion_device_ms": round(statistics.median(t_ao), 4), "arctic_trace_reflections_device_ms": round(statistics.median(t_refl), 4),
                          "arctic_pass_shade_ms_keeping_float_planes": round(statistics.median(t_pass), 4)}
    res["compose_info"] = dict(zip(("device_bytes", "launches", "passes"), r.compose_info()))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers (5 for k_compose, 2 for the one call), median of 7 "
                  "rounds after 2 warm-up calls; sun map, G-buffer, HDR plane, structure and source table resident; bytes per pixel counted from the layout, "
                  "not measured; one run of this program: single figures", "results": res}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
