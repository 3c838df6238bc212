"""What the edge anti-aliasing pass (ARCTIC_OPT_ANTIALIAS, csrc/antialias.hip) costs at config 3, 3840 x 2160, in ONE process on one box, every
comparison alternating its two sides round by round after a warm-up:
  (a) whole frames with the option 0: this tree's library against the parent commit's (--parent-lib: a libarctic_hip.so built from the parent
      commit, e.g. in a `git worktree`); the shading and prepass kernels are untouched, so the two should sit within the alternation's spread
  (b) whole frames with the option 1 against 0 (this tree's library, one handle)
  (c) the filter alone on that frame's RGBA8 (device events around arctic_antialias_device) next to a device-to-device copy of the same bytes
      on the same stream and to the filter on a flat image of that size (no edge pixel: what the copy-with-stencil part costs), and the share
      of the frame's pixels that go past the filter's early exit (computed here from the frame)
Frame times are host-clock times of `--frames` frames enqueued back to back and ended by arctic_flush; (c) uses events on the stream the handle
is put on.  usage: python tools/antialias_time.py [--out profiles/antialias_cost.json] [--parent-lib FILE] [--rounds N] [--frames N] [--scale S]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as e

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--scale", type=float, default=1.0)
args = ap.parse_args()

import torch
if not torch.cuda.is_available():
    sys.exit("antialias_time: no HIP device (there is nothing to measure without one)")
pkg = e.load_package()
binding = pkg.binding
sc = pkg.scenes.CONFIGS[3](scale=args.scale)
res = {"config": 3, "width": sc.width, "height": sc.height, "rounds": args.rounds, "frames_per_round": args.frames, "source": e.source_id()}


def handle(lib=None):
    """a config-3 handle on `lib` (a second build in the same process: the Renderer keeps the library it was created with)"""
    saved = binding._lib
    if lib is not None:
        binding._lib = lib
    try:
        return sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    finally:
        binding._lib = saved


def load(path):
    L = C.CDLL(os.path.abspath(path))
    for name, (rt, at) in binding.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = rt, at
    return L


d_out = torch.zeros((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda")
scene_c, settings_c = pkg.Renderer._scene(sc.desc), pkg.Renderer._settings(sc.settings)


def frames_ms(r, n):
    """n whole frames into d_out, back to back; host clock around enqueue + flush"""
    fn, h, ps, pst, p = r.L.arctic_render_frame_device, r.h, C.byref(scene_c), C.byref(settings_c), C.c_void_p(d_out.data_ptr())
    r.flush()
    t0 = time.perf_counter()
    for _ in range(n):
        rc = fn(h, ps, pst, p)
        if rc < 0:
            r._check(rc)
    r.flush()
    return (time.perf_counter() - t0) * 1e3 / n


def alternate(sides, prepare=None):
    """sides: name -> handle; returns name -> per-round ms per frame, the sides taking turns inside every round"""
    ms = {k: [] for k in sides}
    for k, r in sides.items():
        if prepare:
            prepare(k, r)
        frames_ms(r, 20)                      # warm-up: code objects, tables, the shadow map, clocks
    for rnd in range(args.rounds):
        for k, r in (list(sides.items()) if rnd % 2 == 0 else list(sides.items())[::-1]):   # who goes first takes turns too
            if prepare:
                prepare(k, r)
            ms[k].append(frames_ms(r, args.frames))
        print(f"round {rnd}: " + ", ".join(f"{k} {ms[k][-1]:.4f} ms" for k in sides), flush=True)
    return ms


def summary(v):
    return {"ms_per_frame_median": float(np.median(v)), "ms_per_frame_min": float(np.min(v)), "ms_per_frame_max": float(np.max(v)), "ms_per_frame_all": [float(x) for x in v]}


r = handle()
# (a) option 0: this library against the parent's
if args.parent_lib:
    rp = handle(load(args.parent_lib))
    ms = alternate({"this": r, "parent": rp})
    res["a_option_off_this_vs_parent"] = {"this": summary(ms["this"]), "parent": summary(ms["parent"]),
                                          "ratio_this_to_parent": float(np.median(ms["this"]) / np.median(ms["parent"])),
                                          "parent_version": int(rp.L.arctic_version()), "this_version": int(r.L.arctic_version())}
    mine = d_out.clone()
    frames_ms(rp, 1)
    res["a_option_off_this_vs_parent"]["same_bytes"] = bool(torch.equal(mine, d_out))
    rp.close()
else:
    res["a_option_off_this_vs_parent"] = "not measured (no --parent-lib)"

# (b) option 1 against 0, one handle
ms = alternate({"off": r, "on": r}, prepare=lambda k, h: h.set_option("antialias", 1 if k == "on" else 0))
res["b_option_on_vs_off"] = {"off": summary(ms["off"]), "on": summary(ms["on"]), "ratio_on_to_off": float(np.median(ms["on"]) / np.median(ms["off"])),
                             "added_ms_per_frame": float(np.median(ms["on"]) - np.median(ms["off"]))}

# (c) the filter alone against a device-to-device copy, on one stream, events around each
r.set_option("antialias", 0)
frames_ms(r, 1)
frame = d_out.clone()
filtered, copied = torch.empty_like(frame), torch.empty_like(frame)
r.set_stream(torch.cuda.current_stream().cuda_stream)
w, h = sc.width, sc.height


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def do_filter():
    r.antialias_device(frame.data_ptr(), filtered.data_ptr(), w, h)


def do_copy():
    copied.copy_(frame)


flat = torch.full_like(frame, 128)          # no pixel past the early exit: the copy-with-stencil part of the pass alone


def do_flat():
    r.antialias_device(flat.data_ptr(), filtered.data_ptr(), w, h)


for _ in range(10):
    do_filter(); do_copy(); do_flat()
t_f, t_c, t_0 = [], [], []
for rnd in range(args.rounds):
    t_f.append(float(np.median([timed(do_filter) for _ in range(args.iters)])))
    t_c.append(float(np.median([timed(do_copy) for _ in range(args.iters)])))
    t_0.append(float(np.median([timed(do_flat) for _ in range(args.iters)])))
    print(f"round {rnd}: filter {t_f[-1]:.4f} ms, copy {t_c[-1]:.4f} ms, filter on a flat image {t_0[-1]:.4f} ms", flush=True)
do_filter()
torch.cuda.synchronize()
r.set_stream(None)
img = frame.cpu().numpy()
c = img.astype(np.int64)
Y = 77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]
P = np.pad(Y, 1, mode="edge")
five = np.stack([Y, P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]])
hi, lo = five.max(0), five.min(0)
edge = (hi - lo) >= np.maximum(4096, hi >> 3)
bytes_moved = int(frame.numel())
res["c_filter_alone"] = {"filter_ms_median": float(np.median(t_f)), "filter_ms_all": t_f, "copy_ms_median": float(np.median(t_c)), "copy_ms_all": t_c,
                         "ratio_filter_to_copy": float(np.median(t_f) / np.median(t_c)), "image_bytes": bytes_moved,
                         "filter_flat_image_ms_median": float(np.median(t_0)), "filter_flat_image_ms_all": t_0,
                         "ratio_flat_filter_to_copy": float(np.median(t_0) / np.median(t_c)), "edge_pixels_cost_ms": float(np.median(t_f) - np.median(t_0)),
                         "filter_read_plus_write_GBps": float(2 * bytes_moved / (np.median(t_f) * 1e-3) / 1e9),
                         "copy_read_plus_write_GBps": float(2 * bytes_moved / (np.median(t_c) * 1e-3) / 1e9),
                         "share_of_pixels_past_early_exit": float(edge.mean()), "pixels_changed": float((filtered.cpu().numpy() != img).any(-1).mean())}
r.close()
print(json.dumps(res))
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
