"""Cost of the motion vectors and of the accumulation's motion form (arctic_motion_vectors_device, arctic_accumulate_ambient_occlusion_motion_device,
arctic_pass_ray_effects_motion; csrc/motion.hip) on one MI355X; the numbers of DESIGN.md 6r / profiles/motion_cost.json.

Config 3 at 3840 x 2160 with the visibility plane and the G-buffer resident.
  k_motion alone, into two device planes of the caller's: on a rigid scene (every call sees the scene the previous call saw), and with one
    object moved (the calls alternate between the scene and the scene with its first object elsewhere, over the same resident visibility plane:
    the object's pixels go through another trs every call, which is all the kernel sees of a move).
  k_motion_snapshot per million vertices: a handle of its own with one morphed grid of 1024 x 1024 vertices; the call behind a change of
    weights (k_morph, k_motion, k_motion_snapshot) minus the change of weights alone (k_morph) minus the call alone (k_motion).
  k_ao_accumulate_motion next to k_ao_accumulate, in the same run, still camera, the prev_world4 plane of a rigid scene.
  the one call per frame: arctic_pass_ray_effects_motion next to arctic_pass_ray_effects_temporal, one ray per pixel with the filter.
Beside each kernel's figure the bytes per pixel (or vertex) the algorithm needs, COUNTED from the layout, and the fraction of the 8 TB/s roof.
Milliseconds: torch events on torch's stream around back-to-back calls, median of 7 rounds after 2 warm-up calls.  Every figure is of ONE run.

    motion_time.py [--out FILE] [--bench FILE]   prints one JSON line and, with --out, writes it there; --bench: a JSON file of bench.py
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
GRID = 1023   # cells a side: 1024 x 1024 vertices


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


def figure(ms, bytes_per_item, items, what="algorithmic_bytes_per_pixel"):
    m = statistics.median(ms)
    return {"ms_median": round(m, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)], what: round(bytes_per_item, 2),
            "ms_at_the_roof": round(bytes_per_item * items / HBM_ROOF_BYTES_PER_S * 1e3, 4),
            "fraction_of_the_roof": round(bytes_per_item * items / (m * 1e-3) / HBM_ROOF_BYTES_PER_S, 4)}


def med(ms):
    return {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def main(bench=None):
    global np, torch
    import numpy as np
    import torch
    import __graft_entry__ as entry
    import ray_reference as R
    pkg = entry.load_package()
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.set_option("keep_float_output", 1)
    r.set_stream(torch.cuda.current_stream().cuda_stream)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    _, material, _, _ = r.read_gbuffer(want=("material",))
    tris, _ = R.world_triangles(sc.desc.objects, [(v, i) for v, i, _ in sc.meshes])
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    diagonal = float(np.linalg.norm(hi.astype(np.float64) - lo))
    pixels = sc.width * sc.height
    geometry = material != 0xFFFFFFFF
    covered = float(geometry.mean())
    objects = sc.desc.objects.copy()
    objects["trs"][0][12:15] += np.float32(0.01 * diagonal)
    moved = pkg.scenes.SceneDesc(camera=sc.desc.camera, ambient=sc.desc.ambient, sun=sc.desc.sun, objects=objects, point_lights=sc.desc.point_lights)
    d_pw = torch.zeros((sc.height, sc.width, 4), dtype=torch.float32, device="cuda")
    d_vel = torch.zeros((sc.height, sc.width, 2), dtype=torch.float32, device="cuda")
    d_in = torch.zeros((sc.height, sc.width), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((sc.height, sc.width), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"config": 3, "size": [sc.width, sc.height], "pixels": pixels, "covered_fraction": round(covered, 4), "scene_diagonal": round(diagonal, 3),
           "objects": int(len(objects)), "hbm_roof_bytes_per_s": HBM_ROOF_BYTES_PER_S}

    # ---- k_motion alone.  Counted per pixel: the visibility key (8) in, prev_world4 (16) and velocity2 (8) out: 32 streamed bytes.  The gather of a
    # covered pixel -- rec_of 4, the SetupRec and RasterRec (128 each), the prepass's object record (112), three indices (12), the call's object
    # record (96), three positions (36): 516 bytes if nothing were shared -- is per TRIANGLE and object, shared by the pixels of a tile
    streamed, gather = 8 + 16 + 8, 4 + 128 + 128 + 112 + 12 + 96 + 36
    rigid = lambda: r.motion_vectors_device(sc.desc, d_pw.data_ptr(), d_vel.data_ptr())
    res["k_motion_rigid_scene"] = figure(timed_ms(rigid, reps=5), streamed, pixels)
    turn = [0]
    def one_moved():
        turn[0] ^= 1
        r.motion_vectors_device(moved if turn[0] else sc.desc, d_pw.data_ptr(), d_vel.data_ptr())
    res["k_motion_one_object_moved"] = figure(timed_ms(one_moved, reps=6), streamed, pixels)
    r.flush()
    vel = d_vel.cpu().numpy()
    res["k_motion_one_object_moved"]["pixels_with_a_velocity_above_a_hundredth_fraction"] = round(float((np.abs(vel).max(-1) > 0.01).mean()), 4)
    no_velocity = lambda: r.motion_vectors_device(sc.desc, d_pw.data_ptr(), None)
    res["k_motion_rigid_scene_without_the_velocity_plane"] = figure(timed_ms(no_velocity, reps=5), streamed - 8, pixels)
    res["k_motion_gather_bytes_per_covered_pixel_if_nothing_were_shared"] = gather

    # ---- k_ao_accumulate_motion next to k_ao_accumulate: ao_history_time.py's count, and 16 bytes of prev_world4 more
    r.motion_vectors_device(sc.desc, d_pw.data_ptr(), None)
    hist = dict(HIST, plane_dist=2e-3 * diagonal)
    plain_bytes = 12 + 16 + 16 + 2 + 32 + covered * 32 * 81 / 64
    r.ao_history_reset()
    plain = lambda: r.accumulate_ambient_occlusion_device(sc.desc, d_in.data_ptr(), d_out.data_ptr(), **hist)
    with_motion = lambda: r.accumulate_ambient_occlusion_motion_device(sc.desc, d_pw.data_ptr(), d_in.data_ptr(), d_out.data_ptr(), **hist)
    res["k_ao_accumulate_still_camera"] = figure(timed_ms(plain, reps=5), plain_bytes, pixels)
    res["k_ao_accumulate_motion_still_camera"] = figure(timed_ms(with_motion, reps=5), plain_bytes + 16, pixels)
    res["k_ao_accumulate_still_camera_again"] = figure(timed_ms(plain, reps=5), plain_bytes, pixels)
    count = r.read_ao_history(want=("count",))[1]
    res["k_ao_accumulate_motion_still_camera"]["pixels_that_used_their_history_fraction"] = round(float((count[geometry] > 1).mean()), 4)

    # ---- the one call per frame
    ao_kw = dict(radius=0.1 * diagonal, bias=1e-3 * diagonal, filter=True)
    hist_kw = dict(max_history=hist["max_history"], history_normal_cos=hist["normal_cos"], history_plane_dist=hist["plane_dist"], min_weight=hist["min_weight"])
    tables = [pkg.renderer.ao_directions(1, 4, seed=s) for s in range(16)]
    frame = [0]
    def one_call(motion):
        frame[0] += 1
        call = r.pass_ray_effects_motion if motion else r.pass_ray_effects_temporal
        call(sc.desc, sc.settings, tables[frame[0] % 16], read=False, **ao_kw, **hist_kw)
    res["pass_ray_effects_temporal_1_ray_filtered"] = med(timed_ms(lambda: one_call(False), reps=4))
    res["pass_ray_effects_motion_1_ray_filtered"] = med(timed_ms(lambda: one_call(True), reps=4))
    res["motion_info"] = dict(zip(("device_bytes", "k_motion_launches", "k_motion_snapshot_launches", "calls"), r.motion_info()))
    r.close()

    # ---- k_motion_snapshot per million vertices.  Counted per vertex: the position's 12 bytes lie in a 56-byte vertex (the lines are touched whole:
    # 56 in) and a float4 goes out (16)
    small = pkg.Renderer(256, 256, 64, 16)
    small.set_stream(torch.cuda.current_stream().cuda_stream)
    small.create_material(*pkg.scenes.fallback_textures())
    v, ix = pkg.scenes.quad((-2, -2, 0), (4, 0, 0), (0, 4, 0), GRID, GRID)
    small.create_mesh(v, ix, 0)
    deltas = np.zeros((1, len(v)), pkg.scene.MORPH_DELTA_DTYPE)
    deltas["position"][0, :, 2] = 0.1
    small.set_mesh_morph_targets(0, deltas)
    cam = dict(eye=(0.0, 0.0, 6.0), rotation=(0.0, -90.0), aspect=1.0, fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = pkg.scenes.SceneDesc(camera=cam, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([(np.eye(4, dtype=np.float32), 0)]))
    small.set_mesh_morph_weights(0, np.float32([0.5]))
    small.pass_gbuffer(desc)
    s_pw = torch.zeros((256, 256, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    weight = [0]
    def change():
        weight[0] += 1
        small.set_mesh_morph_weights(0, np.float32([0.25 + 0.5 * (weight[0] & 1)]))
    def change_and_call():
        change()
        small.motion_vectors_device(desc, s_pw.data_ptr(), None)
    call_alone = lambda: small.motion_vectors_device(desc, s_pw.data_ptr(), None)
    a, b, c = timed_ms(change_and_call, reps=4), timed_ms(change, reps=4), timed_ms(call_alone, reps=4)
    snap_ms = statistics.median(a) - statistics.median(b) - statistics.median(c)
    n_vertices = len(v)
    res["k_motion_snapshot"] = {"vertices": n_vertices, "weights_then_call_ms": med(a), "weights_alone_ms": med(b), "call_alone_ms": med(c), "ms_by_difference": round(snap_ms, 4),
                                "ms_per_million_vertices": round(snap_ms / (n_vertices / 1e6), 4), "algorithmic_bytes_per_vertex": 72,
                                "fraction_of_the_roof": round(72 * n_vertices / (max(snap_ms, 1e-6) * 1e-3) / HBM_ROOF_BYTES_PER_S, 4),
                                "motion_info": dict(zip(("device_bytes", "k_motion_launches", "k_motion_snapshot_launches", "calls"), small.motion_info()))}
    small.close()
    out = {"how": "torch events on torch's stream (arctic_set_stream) around back-to-back calls between device buffers, median of 7 rounds after 2 warm-up calls; "
                  "visibility plane, G-buffer, structure and history resident; bytes counted from the layout, not measured; k_motion_snapshot by the difference of three "
                  "chains; one run of this program: single figures", "results": res}
    if bench:
        out["bench_py_steps20_warmup5"] = json.load(open(bench))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    result = main(args[args.index("--bench") + 1] if "--bench" in args else None)
    print(json.dumps(result))
    if "--out" in args:
        json.dump(result, open(args[args.index("--out") + 1], "w"), indent=1)
