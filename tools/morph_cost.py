"""Cost of morph targets (arctic_set_mesh_morph_weights, csrc/morph.hip) on one MI355X; the numbers of DESIGN.md 6j / profiles/morph_cost.json.

    morph_cost.py kernel         k_morph on 1 Mi and 4 Mi vertices with 1, 4 and 16 active targets of 64 against a device-to-device copy of the same
                                 112 + 48 A bytes per vertex; and 1 active of 64 against 1 active of 1 (targets at rest must cost nothing)
    morph_cost.py frames         config 3 with its largest mesh morphed before every frame against the same frames unmorphed (shadow cache on / off)
    morph_cost.py ab LABEL       config 3 whole frames, no morph anywhere, with the library ARCTIC_HIP_LIBRARY names (default: this tree's); run it in
                                 separate processes for this tree, for a library built from the parent commit (with ARCTIC_HIP_LIBRARY_OLDER=1) and for
                                 that parent library once more -- the control that shows the noise --, the three alternating

Each mode prints one JSON line and, with --out FILE, stores it under its mode (ab: its label) in that JSON file (profiles/morph_cost.json)."""
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
N_TARGETS = 64


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


def deltas_for(n, n_targets, rng):
    """(n_targets, n) records: zeros but for a random stretch per target (the time of a streaming blend does not depend on the values; filling
    gigabytes with random numbers on the host would only take long)"""
    d = np.zeros((n_targets, n), pkg.scene.MORPH_DELTA_DTYPE)
    m = min(n, 4096)
    for name in ("position", "normal", "tangent", "bitangent"):
        d[name][:, :m] = rng.normal(scale=0.1, size=(n_targets, m, 3)).astype(np.float32)
    return d


def weight_sets(n_targets, active):
    """four weight vectors with `active` non-zero entries spread over the targets, values changing from call to call"""
    out = []
    for k in range(4):
        w = np.zeros(n_targets, np.float32)
        w[np.linspace(0, n_targets - 1, active).astype(int)] = 0.1 * (k + 1)
        out.append(w)
    return out


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
        for n_targets, actives in ((N_TARGETS, (1, 4, 16)), (1, (1,))):
            mesh = r.create_mesh(v, np.zeros(3, np.uint32), 0)
            r.set_mesh_morph_targets(mesh, deltas_for(n, n_targets, rng))
            for a in actives:
                W = weight_sets(n_targets, a)
                per_vertex = 112 + 48 * a
                src = torch.empty(n * per_vertex // 2, dtype=torch.uint8, device="cuda").random_(0, 255)
                dst = torch.empty_like(src)
                morph_us = timed(lambda k: r.set_mesh_morph_weights(mesh, W[k % 4]))
                copy_us = timed(lambda k: dst.copy_(src))
                res[f"{n}_vertices_{a}_active_of_{n_targets}"] = {
                    "k_morph_us": round(statistics.median(morph_us), 2), "k_morph_us_min_max": [round(min(morph_us), 2), round(max(morph_us), 2)],
                    "d2d_copy_same_bytes_us": round(statistics.median(copy_us), 2), "copy_us_min_max": [round(min(copy_us), 2), round(max(copy_us), 2)],
                    "ratio_morph_over_copy": round(statistics.median(morph_us) / statistics.median(copy_us), 3),
                    "bytes_moved": n * per_vertex, "morph_GB_per_s": round(n * per_vertex / statistics.median(morph_us) / 1e3, 1)}
                del src, dst
            r.set_mesh_morph_targets(mesh, None)
        r.close()
    return {"mode": "kernel", "how": "torch events around 40 back-to-back arctic_set_mesh_morph_weights calls (each: an 8 B x active-targets host-to-device copy + k_morph) on torch's stream, median of 7; the copy is torch's dst.copy_(src) moving the same 112 + 48 A bytes per vertex (read + written)", "results": res}


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
    nv, nt, active = len(sc.meshes[big][0]), 8, 4
    d = np.zeros((nt, nv), pkg.scene.MORPH_DELTA_DTYPE)
    d["position"] = rng.normal(scale=0.002, size=(nt, nv, 3)).astype(np.float32)
    W = []
    for k in range(8):
        w = np.zeros(nt, np.float32); w[:active] = 0.1 * (k + 1)
        W.append(w)
    runs = {"unmorphed_shadow_cache_on": [], "unmorphed_shadow_cache_off": [], "morphed_every_frame": []}
    r.set_mesh_morph_targets(big, d)
    for rep in range(6):
        r.set_mesh_morph_weights(big, None)
        r.set_option("shadow_cache", 1)
        frame_loop(r, sc, outs, 30)
        a = frame_loop(r, sc, outs, 300)
        r.set_option("shadow_cache", 0)
        frame_loop(r, sc, outs, 30)
        b = frame_loop(r, sc, outs, 300)
        r.set_option("shadow_cache", 1)
        morph = lambda k: r.set_mesh_morph_weights(big, W[k % 8])
        frame_loop(r, sc, outs, 30, morph)
        c = frame_loop(r, sc, outs, 300, morph)
        if rep:
            runs["unmorphed_shadow_cache_on"].append(a); runs["unmorphed_shadow_cache_off"].append(b); runs["morphed_every_frame"].append(c)
    r.close()
    out = {k: {"ms_per_frame_median": round(statistics.median(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)]} for k, v in runs.items()}
    return {"mode": "frames", "config": 3, "size": [sc.width, sc.height], "morphed_mesh_vertices": nv, "targets": nt, "active_targets": active,
            "how": "300 arctic_render_frame_device calls enqueued back to back, host clock to the flush, 5 repetitions alternating the three cases; weights per frame also redraw the sun's shadow map every frame (the cache sees the caster change), so 'unmorphed, cache off' is the like-for-like comparison", "results": out}


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
    return {"mode": "ab", "label": label, "library": os.environ.get("ARCTIC_HIP_LIBRARY", "this build"), "static_sun_ms": [round(x, 4) for x in static],
            "shadow_redrawn_ms": [round(x, 4) for x in redraw], "frame_checksum": int(img.astype(np.uint64).sum())}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out")
        out_file = args[i + 1]
        del args[i:i + 2]
    mode = args[0]
    result = kernel_mode() if mode == "kernel" else frames_mode() if mode == "frames" else ab_mode(args[1])
    print(json.dumps(result))
    if out_file:
        doc = json.load(open(out_file)) if os.path.exists(out_file) else {}
        doc[mode if mode != "ab" else "ab_" + args[1]] = result
        json.dump(doc, open(out_file, "w"), indent=1)
