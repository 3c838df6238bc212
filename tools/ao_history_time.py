"""Cost and effect of the temporal accumulation of the occlusion plane (arctic_accumulate_ambient_occlusion_device; csrc/ao_history.hip) on one
MI355X; the numbers of DESIGN.md 6q / profiles/ao_history_cost.json.

Config 3 at 3840 x 2160 with the G-buffer resident; the occlusion at a radius of a tenth of the scene's diagonal over 4 x 4 direction sets, as in
tools/compose_time.py and profiles/ambient_occlusion_cost.json.
  k_ao_accumulate alone, between two device planes of the caller's: under a still camera (every call's matrix is the previous call's) and under
    a moving one (the calls alternate between the frame's camera and one moved and turned a little, over the same resident G-buffer: the taps
    land where a moving camera puts them -- across tiles, at fractional weights, some outside, some rejected -- which is what the kernel's time
    depends on).  Beside each figure the bytes per pixel the algorithm needs, counted from the layout, and the fraction of the 8 TB/s roof.
  the per-frame chain: one ray per pixel with a NEW direction table every frame (its upload included), the occlusion's filter, the accumulation
    in place; next to it the same call with 4 and with 16 rays per pixel, measured here, and the parent's figures as recorded.
  what it is for: the mean absolute difference (in bytes, 0..255) of the accumulated plane from a 64-ray reference plane after 1, 4, 16 and 32
    frames under a still camera (max_history 32, table seed = frame), over the covered pixels; beside it the difference of ONE unfiltered 1-ray plane,
    one filtered 4-ray plane and one filtered 16-ray plane.
Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    ao_history_time.py [--out FILE] [--bench FILE]   prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py
                                                     result lines of this build and the parent's library, recorded beside the figures as given"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_ROOF_BYTES_PER_S = 8e12
HIST = dict(max_history=32.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.1)


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


def bytes_per_pixel(covered, with_history):
    """what k_ao_accumulate has to move per pixel, from the layout: the material word of plane b (12: the plane's stride), plane e (16) and
    plane c (16), the byte in and out (2) and the two history planes written (32) for every pixel, and -- with a history, for a covered pixel --
    the gather: 32 bytes per entry, a 9 x 9 block of entries per 8 x 8 tile when the taps are the tile and its apron (81 / 64 entries per pixel)"""
    return 12 + 16 + 16 + 2 + 32 + covered * (32 * 81 / 64 if with_history else 0)


def figure(ms, bpp, pixels):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "algorithmic_bytes_per_pixel": round(bpp, 2),
            "ms_at_the_roof": round(bpp * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4), "fraction_of_the_roof": round(bpp * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4)}


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
    r.pass_gbuffer(sc.desc)
    _, material, _, _ = r.read_gbuffer(want=("material",))
    tris, _ = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo))
    pixels = sc.width * sc.height
    geometry = material != 0xFFFFFFFF
    covered = float(geometry.mean())
    ao_kw = dict(radius=0.1 * diagonal, bias=1e-3 * diagonal)
    hist = dict(HIST, plane_dist=2e-3 * diagonal)
    cam = dict(sc.desc.camera)
    cam["eye"] = tuple(float(e) + d * diagonal for e, d in zip(cam["eye"], (2e-3, 5e-4, -1e-3)))
    cam["rotation"] = (cam["rotation"][0] - 0.3, cam["rotation"][1] + 0.8)
    moved = pkg.scenes.SceneDesc(camera=cam, ambient=sc.desc.ambient, sun=sc.desc.sun, objects=sc.desc.objects, point_lights=sc.desc.point_lights)
    d_in = torch.zeros((sc.height, sc.width), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((sc.height, sc.width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(1, 4, seed=0), d_in.data_ptr(), filter=True, **ao_kw)
    r.flush()
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "covered_fraction": round(covered, 4), "scene_diagonal": round(diagonal, 3),
           "history": hist, "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S}

    # ---- the kernel alone
    r.ao_history_reset()
    still = lambda: r.accumulate_ambient_occlusion_device(sc.desc, d_in.data_ptr(), d_out.data_ptr(), **hist)
    res["k_ao_accumulate_still_camera"] = figure(timed_ms(still, reps=5), bytes_per_pixel(covered, True), pixels)
    count = r.read_ao_history(want=("count",))[1]
    res["k_ao_accumulate_still_camera"]["pixels_that_used_their_history_fraction"] = round(float((count[geometry] > 1).mean()), 4)
    turn = [0]
    def moving():
        turn[0] ^= 1
        r.accumulate_ambient_occlusion_device(moved if turn[0] else sc.desc, d_in.data_ptr(), d_out.data_ptr(), **hist)
    res["k_ao_accumulate_moving_camera"] = figure(timed_ms(moving, reps=6), bytes_per_pixel(covered, True), pixels)
    count = r.read_ao_history(want=("count",))[1]
    res["k_ao_accumulate_moving_camera"]["pixels_that_used_their_history_fraction"] = round(float((count[geometry] > 1).mean()), 4)
    def first():
        r.ao_history_reset()
        r.accumulate_ambient_occlusion_device(sc.desc, d_in.data_ptr(), d_out.data_ptr(), **hist)
    res["k_ao_accumulate_empty_history"] = figure(timed_ms(first, reps=5), bytes_per_pixel(covered, False), pixels)

    # ---- the per-frame chain
    tables = {n: [pkg.renderer.ao_directions(n, 4, seed=s) for s in range(16)] for n in (1, 4, 16)}
    frame = [0]
    def chain():
        frame[0] += 1
        r.trace_ambient_occlusion_device(sc.desc, tables[1][frame[0] % 16], d_in.data_ptr(), filter=True, **ao_kw)
        r.accumulate_ambient_occlusion_device(sc.desc, d_in.data_ptr(), d_in.data_ptr(), **hist)
    def traced(n):
        frame[0] += 1
        r.trace_ambient_occlusion_device(sc.desc, tables[n][frame[0] % 16], d_in.data_ptr(), filter=True, **ao_kw)
    med = lambda ms: {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    res["per_frame_chain_1_ray_filter_accumulate"] = med(timed_ms(chain, reps=4))
    res["trace_1_ray_filtered_alone"] = med(timed_ms(lambda: traced(1), reps=4))
    res["trace_4_rays_filtered"] = med(timed_ms(lambda: traced(4), reps=2))
    res["trace_16_rays_filtered"] = med(timed_ms(lambda: traced(16), reps=1))
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "ambient_occlusion_cost.json")))["results"]["cases"]
        res["parent_recorded_filter_on_ms"] = {str(c["n_rays"]): c["filter_on"]["ms_median"] for c in rec if c["radius"] != "inf"}
    except (OSError, KeyError):
        pass

    # ---- what it is for
    d_ref = torch.zeros_like(d_in)
    r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(64, 4, seed=1000), d_ref.data_ptr(), **ao_kw)
    r.flush()
    ref = d_ref.cpu().numpy().astype(np.float64)
    mad = lambda plane: round(float(np.abs(plane.cpu().numpy().astype(np.float64) - ref)[geometry].mean()), 3)
    quality = {"reference": "64 rays per pixel, unfiltered", "mean_reference_byte": round(float(ref[geometry].mean()), 2)}
    r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(1, 4, seed=500), d_in.data_ptr(), **ao_kw)
    r.flush()
    quality["one_plane_1_ray_unfiltered"] = mad(d_in)
    r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(4, 4, seed=500), d_in.data_ptr(), filter=True, **ao_kw)
    r.flush()
    quality["one_plane_4_rays_filtered"] = mad(d_in)
    r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(16, 4, seed=500), d_in.data_ptr(), filter=True, **ao_kw)
    r.flush()
    quality["one_plane_16_rays_filtered"] = mad(d_in)
    r.ao_history_reset()
    acc = {}
    for k in range(1, 33):
        r.trace_ambient_occlusion_device(sc.desc, pkg.renderer.ao_directions(1, 4, seed=k), d_in.data_ptr(), filter=True, **ao_kw)
        r.accumulate_ambient_occlusion_device(sc.desc, d_in.data_ptr(), d_out.data_ptr(), **hist)
        if k in (1, 4, 16, 32):
            r.flush()
            acc[str(k)] = mad(d_out)
    quality["accumulated_1_ray_filtered_after_frames"] = acc
    res["mean_absolute_difference_from_the_reference_in_bytes"] = quality
    res["ao_history_info"] = dict(zip(("device_bytes", "launches", "calls"), r.ao_history_info()))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "G-buffer, structure and history resident; bytes per pixel counted from the layout, not measured; the moving camera alternates between two "
                  "cameras over one resident G-buffer; one run of this program: single figures", "results": res}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
