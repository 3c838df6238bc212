"""Cost of skeletal skinning (arctic_set_mesh_pose, csrc/skin.hip) on one MI355X; the numbers of DESIGN.md 6i / profiles/skinning_cost.json.

    skinning_cost.py kernel         k_skin on 1 Mi and 4 Mi vertices (64 and 300 joints) against a device-to-device copy of the same 56 B per vertex
    skinning_cost.py frames         config 3 with its largest mesh posed before every frame against the same frames unposed (shadow cache on / off)
    skinning_cost.py ab LABEL       config 3 whole frames, no skin anywhere, with the library ARCTIC_HIP_LIBRARY names (default: this tree's); run it in
                                    separate processes for this tree, for a library built from the parent commit (with ARCTIC_HIP_LIBRARY_OLDER=1) and for
                                    that parent library once more -- the control that shows the noise --, the three alternating

Each mode prints one JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry

pkg = entry.load_package()
SKIN = np.dtype([("joints", "<u2", 4), ("weights", "<f4", 4)])


def skin_for(v, n_joints, rng):
    s = np.zeros(len(v), SKIN)
    s["joints"] = rng.integers(0, n_joints, size=(len(v), 4))
    w = rng.uniform(size=(len(v), 4)).astype(np.float32)
    s["weights"] = w / w.sum(axis=1, keepdims=True)
    return s


def poses(n_joints, k):
    out = np.zeros((n_joints, 4, 4), np.float32)
    for j in range(n_joints):
        a = 0.002 * (k + 1) * ((j % 7) - 3)
        out[j] = np.eye(4)
        out[j, 0, 0], out[j, 0, 2], out[j, 2, 0], out[j, 2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(n_joints, 16)


def kernel_mode():
    rng = np.random.default_rng(1)
    res = {}
    for n in (1 << 20, 1 << 22):
        v = np.zeros(n, pkg.scene.VERTEX_DTYPE)
        v["position"] = rng.normal(size=(n, 3)).astype(np.float32)
        v["normal"] = rng.normal(size=(n, 3)).astype(np.float32)
        r = pkg.Renderer(64, 64, 0, 16)
        r.create_material(*pkg.scenes.make_material_textures(rng, 8))
        r.set_stream(torch.cuda.current_stream().cuda_stream)
        src = torch.empty(n * 56, dtype=torch.uint8, device="cuda").random_(0, 255)
        dst = torch.empty_like(src)
        for nj in (64, 300):
            mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
            r.set_mesh_skin(mesh, skin_for(v, nj, rng), nj)
            P = [poses(nj, k) for k in range(4)]

            def timed(fn, reps=40):
                for _ in range(5):
                    fn(0)
                torch.cuda.synchronize()
                out = []
                for _ in range(7):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for k in range(reps):
                        fn(k)
                    e1.record()
                    torch.cuda.synchronize()
                    out.append(e0.elapsed_time(e1) / reps * 1e3)
                return out
            skin_us = timed(lambda k: r.set_mesh_pose(mesh, P[k % 4]))
            copy_us = timed(lambda k: dst.copy_(src))
            res[f"{n}_vertices_{nj}_joints"] = {"k_skin_us": round(statistics.median(skin_us), 2), "k_skin_us_min_max": [round(min(skin_us), 2), round(max(skin_us), 2)],
                                                "d2d_copy_56B_per_vertex_us": round(statistics.median(copy_us), 2), "copy_us_min_max": [round(min(copy_us), 2), round(max(copy_us), 2)],
                                                "ratio_skin_over_copy": round(statistics.median(skin_us) / statistics.median(copy_us), 3),
                                                "skin_bytes_moved": n * (56 + 24 + 56), "copy_bytes_moved": n * 112}
        r.close()
    print(json.dumps({"mode": "kernel", "how": "torch events around 40 back-to-back arctic_set_mesh_pose calls (each: a 64 B x joints host-to-device copy + k_skin) on torch's stream, median of 7; the copy is torch's dst.copy_(src) of the same 56 B per vertex", "results": res}))


def frame_loop(r, sc, outs, n, before=None):
    t0 = time.perf_counter()
    for k in range(n):
        if before:
            before(k)
        r.render_frame_device(sc.desc, sc.settings, outs[k % len(outs)].data_ptr())
    r.flush(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def frames_mode():
    sc = pkg.scenes.config3()
    rng = np.random.default_rng(2)
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    outs = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    big = max(range(len(sc.meshes)), key=lambda i: len(sc.meshes[i][0]))
    nv, nj = len(sc.meshes[big][0]), 32
    P = [poses(nj, k) for k in range(8)]
    runs = {"unposed_shadow_cache_on": [], "unposed_shadow_cache_off": [], "posed_every_frame": []}
    r.set_mesh_skin(big, skin_for(sc.meshes[big][0], nj, rng), nj)
    for rep in range(6):
        r.set_mesh_pose(big, None)
        r.set_option("shadow_cache", 1)
        frame_loop(r, sc, outs, 30)
        a = frame_loop(r, sc, outs, 300)
        r.set_option("shadow_cache", 0)
        frame_loop(r, sc, outs, 30)
        b = frame_loop(r, sc, outs, 300)
        r.set_option("shadow_cache", 1)
        pose = lambda k: r.set_mesh_pose(big, P[k % 8])
        frame_loop(r, sc, outs, 30, pose)
        c = frame_loop(r, sc, outs, 300, pose)
        if rep:
            runs["unposed_shadow_cache_on"].append(a); runs["unposed_shadow_cache_off"].append(b); runs["posed_every_frame"].append(c)
    r.close()
    out = {k: {"ms_per_frame_median": round(statistics.median(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in runs.items()}
    print(json.dumps({"mode": "frames", "config": 3, "size": [sc.width, sc.height], "posed_mesh_vertices": nv, "joints": nj,
                      "how": "300 arctic_render_frame_device calls enqueued back to back, host clock to the flush, 5 repetitions alternating the three cases; a pose per frame also redraws the sun's shadow map every frame (the cache sees the caster change), so 'unposed, cache off' is the like-for-like comparison", "results": out}))


def ab_mode(label):
    sc = pkg.scenes.config3()
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    outs = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
    frame_loop(r, sc, outs, 100)
    static = [frame_loop(r, sc, outs, 400) for _ in range(5)]
    r.set_option("shadow_cache", 0)
    frame_loop(r, sc, outs, 50)
    redraw = [frame_loop(r, sc, outs, 400) for _ in range(5)]
    r.flush()
    img = outs[0].cpu().numpy()
    r.close()
    print(json.dumps({"mode": "ab", "label": label, "library": os.environ.get("ARCTIC_HIP_LIBRARY", "this build"), "static_sun_ms": [round(x, 4) for x in static],
                      "shadow_redrawn_ms": [round(x, 4) for x in redraw], "frame_checksum": int(img.astype(np.uint64).sum())}))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernel":
        kernel_mode()
    elif mode == "frames":
        frames_mode()
    else:
        ab_mode(sys.argv[2])
