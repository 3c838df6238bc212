"""Cost of the temporal anti-aliasing resolve (arctic_taa_resolve_device, arctic_pass_taa; csrc/taa.hip) on one MI355X; the numbers of DESIGN.md 6s /
profiles/taa_cost.json.

Config 3 at 3840 x 2160 with the frame shaded and its float HDR plane resident.
  k_taa_resolve alone, on the handle's HDR plane, a warm history: with and without velocity2 (the plane arctic_motion_vectors_device wrote for
    the still scene), with and without ARCTIC_TAA_LUMA_WEIGHT; the jitter is a Halton point, so the four taps are four different entries.
  arctic_pass_taa per frame (k_motion + k_taa_resolve), alone and behind arctic_render_frame_device, next to the frame alone in the same run.
Beside each kernel's figure the bytes per pixel the algorithm needs, COUNTED from the layout, and the fraction of the 8 TB/s roof.
Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    taa_time.py [--out FILE] [--bench FILE]   prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py
                                              result lines of this build and the parent's library, recorded beside the figures as given"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF_BYTES_PER_S = 8e12
LUMA_WEIGHT = 1


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


def figure(ms, bytes_per_pixel, pixels):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "algorithmic_bytes_per_pixel": round(bytes_per_pixel, 2),
            "ms_at_the_roof": round(bytes_per_pixel * pixels / HBM_ROOF_BYTES_PER_S * 1e3, 4),
            "fraction_of_the_roof": round(bytes_per_pixel * pixels / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4)}


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def main(bench=None):
    global torch
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
    d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    j = pkg.renderer.taa_jitter(1)
    r.set_camera_jitter(*j)
    r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    for _ in range(2):                                                           # the second call sees the scene the first saw: velocity2 = -j where there is geometry
        r.motion_vectors_device(sc.desc, d_pw.data_ptr(), d_vel.data_ptr())
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "jitter": [round(x, 4) for x in j], "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S}

    # ---- k_taa_resolve alone.  Counted per pixel: C 12 and velocity2 8 in; T 16, RGBA8 4 and float LDR 12 out; the gather of the history's taps,
    # 81 / 64 entries of 16 bytes when the taps are the tile and its apron.  The box's apron (100 / 64 colours per pixel into LDS) overlaps the
    # neighbouring tiles' and is counted once, as the 12 bytes of C
    gather = 16 * 81 / 64
    for name, vel, flags in (("k_taa_resolve_with_velocity", True, 0), ("k_taa_resolve_without_velocity", False, 0),
                             ("k_taa_resolve_with_velocity_luma_weight", True, LUMA_WEIGHT), ("k_taa_resolve_without_velocity_luma_weight", False, LUMA_WEIGHT)):
        call = lambda: r.taa_resolve_device(sc.settings, None, d_vel.data_ptr() if vel else None, d_out.data_ptr(), jitter=j if vel else (0.25, -0.25), max_history=8.0, flags=flags)
        res[name] = figure(timed_ms(call, reps=10), 12 + (8 if vel else 0) + 16 + 4 + 12 + gather, pixels)
    _, _, count, _ = r.read_taa(want=("count",))
    res["pixels_at_the_history_cap_fraction"] = round(float((count == 8.0).mean()), 4)

    # ---- the one call per frame
    one_call = lambda: r.pass_taa(sc.desc, sc.settings, d_out.data_ptr(), jitter=j, max_history=8.0)
    res["pass_taa_alone"] = med(timed_ms(one_call, reps=5))
    frame = lambda: r.render_frame_device(sc.desc, sc.settings, d_out.data_ptr())
    def frame_and_taa():
        frame()
        one_call()
    res["render_frame"] = med(timed_ms(frame, reps=5))
    res["render_frame_then_pass_taa"] = med(timed_ms(frame_and_taa, reps=5))
    res["render_frame_again"] = med(timed_ms(frame, reps=5))
    res["taa_info"] = dict(zip(("device_bytes", "k_taa_resolve_launches", "calls"), r.taa_info()[:3]))
    r.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "the frame shaded, its HDR plane and the history resident; bytes counted from the layout, not measured; one run of this program: single figures",
           "results": res}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
