"""What the runs of the packed light loop's pair table (ARCTIC_OPT_LIGHT_PAIR_RUNS, csrc/shade.hip: accumulate_pair<SKIP>) are worth on one MI355X;
the numbers of DESIGN.md 4.2 / profiles/light_pair_runs_cost.json.

    light_pair_runs_time.py ab --parent LIB [--rounds 16]   bench.py --gpus 1 --steps 20 --warmup 5 in child processes, alternating three labels
                                   `rounds` times each: this tree's library, a library built from the parent commit (LIB, loaded with
                                   ARCTIC_HIP_LIBRARY_OLDER=1) and that parent library once more -- the control that shows the noise.  Stores
                                   ms_per_step of every run, the medians, the control's spread (the standard error of its median, from the
                                   scatter of its single runs, which is stored next to it) and the verdict: a gain only if the median improvement over
                                   the parent exceeds twice the control's spread
    light_pair_runs_time.py shade LABEL   one process, the library ARCTIC_HIP_LIBRARY names (default: this tree's): arctic_time_shade of config 3
                                   at 3840 x 2160 with its 64 lights and with the first 16, then whole frames (arctic_render_frame_device, static sun), the option at 1 and at 0 where the
                                   library has it, the settings alternating
    light_pair_runs_time.py counters LABEL DIR   per-launch averages of k_material's counters from a rocprofv3 --pmc pass over tools/prof_shade.py

Every mode prints one JSON line and, with --out FILE, stores it under its mode (shade, counters: mode_label) in that JSON file."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def store(out, key, value):
    if out:
        data = json.load(open(out)) if os.path.exists(out) else {}
        data[key] = value
        json.dump(data, open(out, "w"), indent=1)
    print(json.dumps({key: value}))


def judge(runs, key="ms_per_step"):
    """the issue's rule on the medians of n runs per label.  What is compared is a median of n, so the control's spread is the standard error of ITS
    median, from the scatter of its single runs: 1.2533 * stdev / sqrt(n) (the large-sample value for a normal scatter).  The plain scatter of
    single runs (stdev, range) is stored next to it, and so is the verdict a reader gets who takes that for the spread."""
    med = {name: statistics.median(r[key] for r in runs[name]) for name in runs}
    vals = [r[key] for r in runs["control"]]
    sd = statistics.stdev(vals)
    se = 1.2533 * sd / len(vals) ** 0.5
    gain = med["parent"] - med["this"]
    return {key: {"median": {k: round(v, 5) for k, v in med.items()},
                  "min_max": {name: [min(r[key] for r in runs[name]), max(r[key] for r in runs[name])] for name in runs},
                  "control_stdev_of_single_runs": round(sd, 5), "control_range_of_single_runs": round(max(vals) - min(vals), 5),
                  "control_spread": round(se, 5), "control_spread_is": "standard error of the control's median, 1.2533 * stdev / sqrt(n)",
                  "parent_median_minus_control_median": round(med["parent"] - med["control"], 5),
                  "improvement_over_parent": round(gain, 5), "improvement_frac": round(gain / med["parent"], 4),
                  "improvement_over_twice_the_spread": round(gain / (2 * se), 2),
                  "gain": bool(gain > 2 * se), "slower": bool(-gain > 2 * se),
                  "gain_if_the_spread_were_the_stdev_of_single_runs": bool(gain > 2 * sd)}}


def ab(parent, rounds, out):
    labels = [("this", None), ("parent", parent), ("control", parent)]
    runs = {name: [] for name, _ in labels}
    for k in range(rounds):
        for name, lib in labels:
            env = dict(os.environ)
            if lib:
                env.update(ARCTIC_HIP_LIBRARY=os.path.abspath(lib), ARCTIC_HIP_LIBRARY_OLDER="1")
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=240)
            if p.returncode != 0:   # nothing more is started on the device after a failed run
                sys.exit(f"bench.py failed for {name} (exit status {p.returncode})")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            runs[name].append({"ms_per_step": line["ms_per_step"]})
            print(f"[ab] round {k} {name}: {runs[name][-1]}", file=sys.stderr, flush=True)
    res = {"command": "bench.py --gpus 1 --steps 20 --warmup 5, one child process per run, labels alternating", "rounds": rounds, "runs": runs}
    res.update(judge(runs))
    store(out, "ab", res)


def shade(label, out):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    from arctic_renderer_amd import binding
    sc = pkg.scenes.config3(scale=1.0)
    r = sc.upload(pkg.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc); r.flush()
    has_option = hasattr(binding.lib(), "arctic_light_pair_table")
    res = {"library": os.environ.get("ARCTIC_HIP_LIBRARY", "this build"), "how": "arctic_time_shade, 5 warm-up + 40 launches per sample, median; 5 samples per setting, the settings alternating"}
    settings = [(n, runs) for n in (64, 16) for runs in ((1, 0) if has_option else (None,))]
    samples = {s: [] for s in settings}
    for _ in range(5):
        for n, runs in settings:
            if runs is not None:
                r.set_option("light_pair_runs", runs)
            r.update_lights(sc.lights[:n])
            samples[(n, runs)].append(float(statistics.median(r.time_shade(sc.desc, sc.settings, 5, 40))))
    for (n, runs), ms in samples.items():
        res[f"{n}_lights" + ("" if runs is None else f"_runs_{runs}")] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    # whole frames as bench.py --full times them: arctic_render_frame_device, static sun, 20 frames enqueued back to back behind 3
    r.update_lights(sc.lights)
    frames = {runs: [] for _, runs in settings[:len(settings) // 2]}
    for _ in range(5):
        for runs in frames:
            if runs is not None:
                r.set_option("light_pair_runs", runs)
            for k in range(3 + 20):
                if k == 3:
                    r.flush()
                    t0 = time.perf_counter()
                r.render_frame_device(sc.desc, sc.settings, None)
            r.flush()
            frames[runs].append((time.perf_counter() - t0) / 20 * 1e3)
    for runs, ms in frames.items():
        res["whole_frame_static_sun" + ("" if runs is None else f"_runs_{runs}")] = {"ms_median": round(statistics.median(ms), 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)]}
    r.close()
    store(out, f"shade_{label}", res)


def counters(label, root, out):
    acc = {}
    for path in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            if "k_material" in row["Kernel_Name"]:
                key = (path, row["Dispatch_Id"])
                acc.setdefault(row["Counter_Name"], {}).setdefault(key, 0.0)
                acc[row["Counter_Name"]][key] += float(row["Counter_Value"])
    store(out, f"counters_{label}", {"command": "rocprofv3 --pmc <set> --kernel-trace -- python3 tools/prof_shade.py full (tools/profile_round.sh, pass 3); per launch of k_material<2>",
                                     "per_launch": {c: sum(v.values()) / len(v) for c, v in sorted(acc.items())}, "launches": {c: len(v) for c, v in acc.items()}})


if __name__ == "__main__":
    args = sys.argv[1:]
    out = args[args.index("--out") + 1] if "--out" in args else None
    if args and args[0] == "ab":
        ab(args[args.index("--parent") + 1], int(args[args.index("--rounds") + 1]) if "--rounds" in args else 16, out)
    elif args and args[0] == "shade":
        shade(args[1], out)
    elif args and args[0] == "counters":
        counters(args[1], args[2], out)
    else:
        sys.exit(__doc__)
