"""Host-visible times of one build of the library, for comparing two builds whose kernels are the same (profiles/resource_owners_frame_times.json):
whole frames of config 3 at 3840 x 2160 -- bench.py --full's loop, five rounds of 20 frames, wall clock -- and the ambient-occlusion call with its
direction table resident (tools/ambient_occlusion_time.py's set-up and timing) and with a table that changes every call, which takes the staged
upload every time.  Run it once per build in processes of their own, the builds alternating on one box; ARCTIC_HIP_LIBRARY names the other build's
library.  Prints one line: "AB " + JSON."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))   # (ambient_occlusion_time puts tests/ there too)
import numpy as np
import torch
import ambient_occlusion_time as T
T.torch = torch

sc, r = T.resident()                       # config 3 at 3840 x 2160 on torch's stream, G-buffer resident
pkg = T.pkg
out = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in range(3)]
res = {"library": os.environ.get("ARCTIC_HIP_LIBRARY", "in-tree"), "whole_frame_ms": {}, "ambient_occlusion_ms": {}}
for name, cache in (("static_sun", 1), ("moving_sun", 0)):
    r.set_option("shadow_cache", cache)
    rounds = []
    for _ in range(5):
        for k in range(3 + 20):
            if k == 3:
                r.flush(); torch.cuda.synchronize(); t0 = time.perf_counter()
            r.render_frame_device(sc.desc, sc.settings, out[k % 3].data_ptr())
        r.flush(); torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / 20 * 1e3)
    res["whole_frame_ms"][name] = [round(x, 4) for x in rounds]
r.set_option("shadow_cache", 1)
r.pass_gbuffer(sc.desc)
a, b = pkg.renderer.ao_directions(4, 4), pkg.renderer.ao_directions(4, 4, seed=1)
call = lambda: r.trace_ambient_occlusion(sc.desc, a, radius=3.521, bias=1e-3, filter=True, read=False)
res["ambient_occlusion_ms"]["table_resident"] = [round(x, 4) for x in T.timed_ms(call, reps=3)]
flip = [0]
def changing():
    flip[0] ^= 1
    r.trace_ambient_occlusion(sc.desc, b if flip[0] else a, radius=3.521, bias=1e-3, filter=True, read=False)
res["ambient_occlusion_ms"]["table_sent_every_call"] = [round(x, 4) for x in T.timed_ms(changing, reps=3)]
# host time alone of the staged call: 200 calls enqueued, wall clock per call before the flush
r.flush(); t0 = time.perf_counter()
for _ in range(200):
    changing()
res["ambient_occlusion_ms"]["host_enqueue_per_call_table_sent"] = round((time.perf_counter() - t0) / 200 * 1e3, 4)
r.flush()
r.close()
print("AB " + json.dumps(res), flush=True)
