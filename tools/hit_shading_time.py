"""Cost of shading ray hits (arctic_shade_hits, arctic_trace_reflections; csrc/hit_shade.hip) on one MI355X; the numbers of DESIGN.md 6o /
profiles/hit_shading_cost.json.

Config 3 at 3840 x 2160 with the sun's map drawn and the G-buffer resident.  Camera rays -- from the eye through the G-buffer's world position
of every covered pixel, in row-major order -- are traced alone (k_trace), then traced and shaded (k_trace, k_shade_hits), between device
buffers; then the reflection plane (k_reflect_rays, k_trace, k_shade_hits over every pixel of the frame) at a bias of 1e-3 of the scene's
diagonal; next to them the shading pass of the same frame (arctic_pass_shade); last, with a 2048 x 1024 environment map created for it,
k_shade_hits on the same rays with every hit record a miss -- the sky path alone, which the plane of this scene almost never takes.  Per case: milliseconds (torch events on torch's stream around
back-to-back calls, median of 7 rounds after 2 warm-up calls) and rays per second.  Every figure is of ONE run of this program.

    hit_shading_time.py [--out FILE]      prints one JSON line and, with --out, writes it there"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def figures(ms, rays):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "Grays_per_s": round(rays / m / 1e6, 3)}


def main():
    global np, torch
    import numpy as np
    import torch
    import __graft_entry__ as entry
    import ray_reference as R
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    attrs, material, _, _ = r.read_gbuffer(want=("attrs", "material"))
    tris, _ = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo))
    pixels = sc.width * sc.height
    covered = (material != 0xFFFFFFFF).reshape(-1)
    eye = np.asarray(sc.desc.camera["eye"], np.float32)
    world = attrs.reshape(-1, 18)[covered, 11:14]
    rays = pkg.scene.make_rays(np.broadcast_to(eye, world.shape), world - eye)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    d_rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    trace = lambda: r.trace_rays_device(sc.desc, d_rays.data_ptr(), n, d_hits.data_ptr())
    shade = lambda: r.shade_hits_device(sc.desc, d_rays.data_ptr(), d_hits.data_ptr(), n, d_rgba.data_ptr())

    def both():
        trace()
        shade()
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "camera_rays": n, "scene_diagonal": round(diagonal, 3), "point_lights": len(sc.lights),
           "shadow_size": sc.shadow_size}
    t_trace = timed_ms(trace, reps=3)
    t_both = timed_ms(both, reps=3)
    res["k_trace_on_camera_rays"] = figures(t_trace, n)
    res["k_trace_then_k_shade_hits"] = figures(t_both, n)
    res["k_shade_hits_alone_by_difference_ms"] = round(statistics.median(t_both) - statistics.median(t_trace), 4)
    hits = d_hits.cpu().numpy().view(np.uint32)
    rgba = d_rgba.cpu().numpy()
    res["camera_rays_that_hit_fraction"] = round(float((hits[:, 3] != 0xFFFFFFFF).mean()), 4)
    res["mean_shaded_rgb"] = [round(float(x), 4) for x in rgba[rgba[:, 3] == 1, :3].mean(0)]
    bias = 1e-3 * diagonal
    t_refl = timed_ms(lambda: r.trace_reflections(sc.desc, bias, read=False), reps=3)
    res["reflection_plane"] = dict(figures(t_refl, pixels), bias=round(bias, 5))
    plane = r.trace_reflections(sc.desc, bias)
    res["reflection_plane"]["pixels_whose_reflection_shows_geometry_fraction"] = round(float((plane[..., 3] == 1).mean()), 4)
    t_pass = timed_ms(lambda: r.pass_shade(sc.desc, sc.settings), reps=3)
    res["for_context"] = {"arctic_pass_shade_ms_this_run": round(statistics.median(t_pass), 4), "README": {"camera_Grays_per_s": 5.4}}
    res["structure"] = dict(zip(("triangles_stored", "nodes", "builds", "depth"), r.ray_scene_info()))
    # the sky path: config 3 has no environment map, so one is made now; the camera rays again, every record a miss
    r.create_hdri(pkg.scenes.synthetic_hdri(2048, 1024))
    d_miss = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")           # prim = 0xFFFFFFFF
    d_sky = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t_sky = timed_ms(lambda: r.shade_hits_device(sc.desc, d_rays.data_ptr(), d_miss.data_ptr(), n, d_sky.data_ptr()), reps=3)
    sky = d_sky.cpu().numpy()
    res["k_shade_hits_every_ray_a_miss"] = dict(figures(t_sky, n), environment_map=[2048, 1024], alpha_zero_fraction=round(float((sky[:, 3] == 0).mean()), 4),
                                                mean_rgb=[round(float(x), 4) for x in sky[:, :3].mean(0)])
    res["hit_shading_info"] = dict(zip(("device_bytes", "pinned_bytes", "prims", "tables_made"), r.hit_shading_info()))
    r.close()
    return {"how": "torch events on torch's stream (arctic_set_stream) around 3 back-to-back calls between device buffers, median of 7 rounds after 2 warm-up "
                   "calls; sun map, G-buffer, structure and source table resident; one run of this program", "results": res}


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main()
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
