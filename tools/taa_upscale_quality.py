"""The quality figures of the temporal upscaler that the tests' thresholds stand on: profiles/taa_upscale_quality.json.

  "cpu"  the numpy reference alone (tests/taa_upscale_reference.py; no GPU, no library): the analytic scene at 48 x 32 -> 96 x 64, 16 jittered
         frames -- mean absolute error through Reinhard against the supersampled 96 x 64 frame of one frame stretched bilinearly, of the same
         frames through the low-resolution resolve then stretched, and of the upscaler (tests/test_taa_upscale_reference.py: measure_quality)
  "gpu"  one MI355X: config 1's scene on a half-size handle under the exact four-phase jitter through arctic_pass_taa_upscale against a handle
         that renders the output size directly, next to one half-size frame stretched (tests/test_gpu_taa_upscale.py: chain)

    taa_upscale_quality.py [--gpu] [--out FILE]   measures the "cpu" part, with --gpu the "gpu" part instead; merges it into FILE (default:
                                                  profiles/taa_upscale_quality.json) and prints the part as one JSON line"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(gpu, path):
    if gpu:
        import __graft_entry__ as entry
        import test_gpu_taa_upscale as TG
        pkg = entry.load_package()
        part, _ = TG.chain(pkg, pkg.renderer, **TG.CHAIN)
        part = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in part.items()}
    else:
        import test_taa_upscale_reference as TR
        part = {k: (list(v) if isinstance(v, tuple) else v) for k, v in TR.QUALITY_CASE.items()}
        part.update({k: round(v, 6) for k, v in TR.measure_quality(**TR.QUALITY_CASE).items()})
    whole = json.load(open(path)) if os.path.exists(path) else {}
    whole["gpu" if gpu else "cpu"] = part
    json.dump(whole, open(path, "w"), indent=1)
    return part


if __name__ == "__main__":
    args = sys.argv[1:]
    print(json.dumps(main("--gpu" in args, args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "taa_upscale_quality.json"))))
