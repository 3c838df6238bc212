"""Cost of the temporal upscaler (arctic_taa_upscale_device, arctic_pass_taa_upscale; csrc/taa_upscale.hip) on one MI355X; the numbers of
DESIGN.md 6y / profiles/taa_upscale_cost.json.

  k_taa_upscale alone at 1920 x 1080 -> 3840 x 2160 and at 2560 x 1440 -> 3840 x 2160, next to k_taa_resolve at 3840 x 2160 in the same run:
    bare handles on synthetic device planes (random HDR colours, velocity2 = -j as a still scene has it), a warm history, a Halton jitter, so
    the four taps are four different entries.  Beside each figure the bytes per OUTPUT pixel the algorithm needs, COUNTED from the layout, and
    the fraction of the 8 TB/s roof.
  The whole frame this stage exists for, config 3 with arctic_pass_ray_effects at four occlusion rays per pixel and the reflection plane:
    a 3840 x 2160 handle (frame + ray effects) against a 1920 x 1080 handle (frame + ray effects + arctic_pass_taa_upscale to 3840 x 2160
    from the composition's plane), per frame, in the same run.
Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    taa_upscale_time.py [--out FILE] [--kernels-only] [--frames-only]   prints one JSON line and, with --out, writes it there (merging into
                                                                        what FILE holds, so that the two halves may come from two runs)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from taa_time import HBM_ROOF_BYTES_PER_S, figure, med   # noqa: E402
import taa_time                                            # noqa: E402

OUT_SIZE = (3840, 2160)
SETTINGS = (2, 2.2, 1.0)
GATHER = 16 * 81 / 64   # the history's taps when they are the tile and its apron, bytes per output pixel


def kernels(pkg, torch):
    res = {}
    W, H = OUT_SIZE
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    for w, h in ((1920, 1080), (2560, 1440)):
        r = pkg.Renderer(w, h, 64, 16)
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        j = pkg.renderer.taa_upscale_jitter(1, (w, h), OUT_SIZE)
        d_c = torch.rand((h, w, 3), dtype=torch.float32, device="cuda", generator=gen) * 4.0
        d_v = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
        d_v[..., 0], d_v[..., 1] = -float(j[0]), -float(j[1])
        torch.cuda.synchronize()
        ratio = (w * h) / (W * H)
        for name, vel, flags in (("with_velocity", True, 0), ("without_velocity", False, 0), ("with_velocity_luma_weight", True, 1), ("with_velocity_no_clamp", True, 4)):
            call = lambda: r.taa_upscale_device(SETTINGS, OUT_SIZE, d_c.data_ptr(), d_v.data_ptr() if vel else None, d_out.data_ptr(), jitter=j, max_history=8.0, sharpness=1.0,
                                                flags=flags)
            # counted per OUTPUT pixel: C 12 and velocity2 8 per INPUT pixel in; U 16, RGBA8 4 and float LDR 12 out; the gather of the taps
            res[f"k_taa_upscale_{w}x{h}_{name}"] = figure(taa_time.timed_ms(call, reps=10), ratio * (12 + (8 if vel else 0)) + 16 + 4 + 12 + GATHER, W * H)
        res[f"taa_upscale_info_{w}x{h}"] = dict(zip(("device_bytes", "k_taa_upscale_launches", "calls", "size"), r.taa_upscale_info()))
        r.close()
    r = pkg.Renderer(W, H, 64, 16)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    j = pkg.renderer.taa_jitter(1)
    d_c = torch.rand((H, W, 3), dtype=torch.float32, device="cuda", generator=gen) * 4.0
    d_v = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    d_v[..., 0], d_v[..., 1] = -j[0], -j[1]
    torch.cuda.synchronize()
    call = lambda: r.taa_resolve_device(SETTINGS, d_c.data_ptr(), d_v.data_ptr(), d_out.data_ptr(), jitter=j, max_history=8.0)
    res["k_taa_resolve_3840x2160_with_velocity"] = figure(taa_time.timed_ms(call, reps=10), 12 + 8 + 16 + 4 + 12 + GATHER, W * H)
    # ... and the upscaler at ratio 1, the same bytes as the resolve: what the footprint and the confidence cost by themselves
    call = lambda: r.taa_upscale_device(SETTINGS, OUT_SIZE, d_c.data_ptr(), d_v.data_ptr(), d_out.data_ptr(), jitter=j, max_history=8.0, sharpness=0.0)
    res["k_taa_upscale_3840x2160_ratio_1_with_velocity"] = figure(taa_time.timed_ms(call, reps=10), 12 + 8 + 16 + 4 + 12 + GATHER, W * H)
    r.close()
    return res


def frames(pkg, torch):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ray_reference as R
    res = {}
    W, H = OUT_SIZE
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    dirs = pkg.renderer.ao_directions(4, 4, seed=3)
    sc = pkg.scenes.config3()                                                    # ONE scene: the same meshes, textures and 4000 x 4000 sun map on both handles
    tris, _ = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    diagonal = float(np.linalg.norm(tris.reshape(-1, 3).max(0).astype(np.float64) - tris.reshape(-1, 3).min(0)))
    ao_kw, bias = dict(radius=0.1 * diagonal, bias=1e-3 * diagonal), 1e-3 * diagonal
    for scale, name in ((1.0, "handle_3840x2160"), (0.5, "handle_1920x1080_upscaled_to_3840x2160")):
        width, height = int(sc.width * scale), int(sc.height * scale)
        r = sc.upload(pkg.Renderer(width, height, sc.shadow_size, sc.max_lights))
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        r.set_option("keep_float_output", 1)
        j = pkg.renderer.taa_upscale_jitter(1, (width, height), OUT_SIZE) if scale != 1.0 else (0.0, 0.0)
        r.set_camera_jitter(float(j[0]), float(j[1]))
        frame = lambda: r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
        rays = lambda: r.pass_ray_effects(sc.desc, sc.settings, dirs=dirs, reflection_bias=bias, d_out_ptr=d_out.data_ptr(), **ao_kw)
        up = lambda: r.pass_taa_upscale(sc.desc, sc.settings, OUT_SIZE, d_out.data_ptr(), jitter=j, max_history=8.0, sharpness=1.0, flags=2)

        def whole():
            frame()
            rays()
            if scale != 1.0:
                up()
        entry = {"size": [width, height], "triangles": sc.n_triangles, "render_frame": med(taa_time.timed_ms(frame, reps=3)),
                 "render_frame_then_pass_ray_effects_4_rays_and_reflections" + ("_then_pass_taa_upscale" if scale != 1.0 else ""): med(taa_time.timed_ms(whole, reps=2))}
        if scale != 1.0:
            frame(); rays()
            entry["pass_taa_upscale_alone"] = med(taa_time.timed_ms(up, reps=5))
        res[name] = entry
        r.close()
    return res


def main(want_kernels=True, want_frames=True):
    import torch
    import __graft_entry__ as entry
    taa_time.torch = torch
    pkg = entry.load_package()
    res = {"output_size": list(OUT_SIZE), "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S}
    if want_kernels:
        res["kernels"] = kernels(pkg, torch)
    if want_frames:
        res["frames_config3"] = frames(pkg, torch)
    return {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; the kernels on "
                   "bare handles with synthetic planes and a warm history; the frames on config 3 with everything resident; bytes counted from the layout, not measured; one run "
                   "of this program per half: single figures",
            "results": res}


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main("--frames-only" not in args, "--kernels-only" not in args)
    print(json.dumps(result))
    if "--out" in args:
        path = args[args.index("--out") + 1]
        if os.path.exists(path):
            held = json.load(open(path))
            held.get("results", {}).update(result["results"])
            result["results"] = held.get("results", result["results"])
        json.dump(result, open(path, "w"), indent=1)
