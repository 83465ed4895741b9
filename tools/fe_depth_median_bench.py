#!/usr/bin/env python3
"""Cost of the front end's median stage (cvo_fe_set_depth_median): host-to-host time of one depth frame
(create_pointcloud) at 640 x 480 and at 1241 x 376 without the filter and with it at (radius, fill_min) = (1, 0), (2, 0),
(1, 5) and (2, 13), and the duration of the stage's launch (k_fe_median<R, FILL>) beside k_fe_depth_gate<0>, the kernel
of the same shape (a uint16 tile with a halo in, a plane and flags out).

    python tools/fe_depth_median_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_depth_median_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_depth_median.json

One generator per (size, case), all alternating in one process: a round times --frames frames of each in turn (host clock
around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest and
largest round beside it.  The depth frames are data.synthetic_rgbd_frame's with 5 % of the pixels at random depths and
5 % without one.  --root: the package of another checkout of the project (the parent commit's, built), which runs the
cases without the filter only; such a process counts as tree "parent".  --off-only: this tree the same way, two
generators and nothing else in the process, which is the process the parent's is compared with: a frame timed between
the frames of eight other generators is not the frame a process without the filter sees.
--trace-run: 30 frames of each case with the filter and of a frame under a gate (0.8 m / 4 m / jump_rel 0.05, grow 0), size by size, and nothing else, for a rocprofv3
--kernel-trace run of its own (no counters); --kernel-trace: the kernel_trace.csv of such a run: per size the durations
(median, smallest, largest) of every instance of k_fe_median and of k_fe_depth_gate<0>, and the ratio of the medians.
--merge: no GPU; the --out files of several processes of one session, in the order they ran, become one file: `runs`
lists every process, `medians_min_max_runs` the smallest and largest median per tree and case over them,
`median_cost_ms` what a case adds to `off` in the same process, `off_this_minus_parent_ms` the two trees' processes
that ran nothing but the cases without the filter beside the spread of each over its processes; --bench: result
lines of bench.py, "<tree>=<the JSON line>" each, in the order they ran.  Nothing here is asserted, and nothing here measures accuracy: no real frames are shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_FRAMES = 30
SIZES = (("vga", 640, 480), ("kitti", 1241, 376))
MEDIANS = (("m1_0", (1, 0)), ("m2_0", (2, 0)), ("m1_5", (1, 5)), ("m2_13", (2, 13)))
GATE = (0.8, 4.0, 0.05, 0)
GATE_KERNEL = "k_fe_depth_gate<0>"


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def _short(name):
    """"void (anonymous namespace)::k_fe_median<1, false>(FeMedianArgs)" -> "k_fe_median<1, false>" """
    s = name[name.index("k_fe_"):].split("(")[0].strip()
    return s.replace(",f", ", f").replace(",t", ", t")


def kernel_times(path):
    """The dispatches of a --trace-run's kernel trace in the order they started: every instance ran TRACE_FRAMES times
    per size, the first size first"""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_median" in name or "k_fe_depth_gate" in name:
                start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                by.setdefault(_short(name), []).append((start, (end - start) / 1e3))
    out = {}
    for k, v in sorted(by.items()):
        v.sort()
        if len(v) != len(SIZES) * TRACE_FRAMES:
            raise SystemExit("fe_depth_median_bench: %d dispatches of %s in the trace, expected %d"
                             % (len(v), k, len(SIZES) * TRACE_FRAMES))
        for j, (size, _, _) in enumerate(SIZES):
            out.setdefault(size, {})[k] = _stats([d for _, d in v[j * TRACE_FRAMES:(j + 1) * TRACE_FRAMES]])
    for o in out.values():
        if GATE_KERNEL in o:
            o["ratio_to_" + GATE_KERNEL] = {k: o[k]["median_us"] / o[GATE_KERNEL]["median_us"] for k in o if k.startswith("k_fe_median")}
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "sizes", "rounds", "frames_per_round", "timing", "gate") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: what the filter is worth in trajectory accuracy needs real frames, and none are shipped"
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread, cost = {}, {}
    for r in res["runs"]:
        alone = len(r["ms_per_frame"]) == len(SIZES)   # (a process that ran the cases without the filter and nothing else)
        for case, v in r["ms_per_frame"].items():
            size, _, what = case.partition("_")
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
            if r["tree"] == "this" and what != "off":
                cost.setdefault(case, []).append(v[0] - r["ms_per_frame"][size + "_off"][0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["median_cost_ms"] = {k: [statistics.median(v), min(v), max(v)] for k, v in sorted(cost.items())}
    res["off_this_minus_parent_ms"] = {}
    for size, _, _ in SIZES:
        p, t = spread.get("parent:%s_off_alone" % size), spread.get("this:%s_off_alone" % size)
        if p and t:
            res["off_this_minus_parent_ms"][size] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                                     "parent_spread_max_minus_min": max(p) - min(p),
                                                     "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        for k in ("points", "pixels"):
            if k in f and f["tree"] == "this":
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    if bench:
        res["bench_py"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 in each tree in turn, in this order", "runs": []}
        for item in bench:
            tree, _, line = item.partition("=")
            d = json.loads(line)
            res["bench_py"]["runs"].append({"tree": tree, "value": d.get("value"), "unit": d.get("unit"), "ms_per_step": d.get("ms_per_step")})
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    print(json.dumps(res["median_cost_ms"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def spoiled(dep, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    dep = dep.copy()
    salt = rng.random(dep.shape) < 0.05
    dep[salt] = rng.integers(1500, 40000, int(salt.sum())).astype(np.uint16)
    dep[rng.random(dep.shape) < 0.05] = 0
    return dep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_depth_median_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_depth_median_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_median = hasattr(F, "DepthMedian") and not args.off_only
    frames, gens = {}, {}
    for size, w, h in SIZES:
        frames[size] = []
        for k in range(8):
            bgr, dep = pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k), holes=0.0)
            frames[size].append((bgr, spoiled(dep, 170 + k)))
        if not args.trace_run:
            gens[size + "_off"] = F.PcdGenerator(w, h)
        for name, m in MEDIANS if has_median else ():
            gens[size + "_" + name] = F.PcdGenerator(w, h)
            gens[size + "_" + name].set_depth_median(F.DepthMedian(*m))
        if args.trace_run:
            gens[size + "_gate"] = F.PcdGenerator(w, h)
            gens[size + "_gate"].set_depth_gate(F.DepthGate(*GATE))

    def frame(name, k):
        bgr, dep = frames[name.split("_")[0]][k % 8]
        return gens[name].create_pointcloud(bgr, dep, 1, F.FEATURES_HSV)

    if args.trace_run:
        for name in gens:   # (size by size: the order kernel_times() relies on)
            for k in range(TRACE_FRAMES):
                frame(name, k)
        for gen in gens.values():
            gen.close()
        return
    clouds = {name: [frame(name, k) for k in range(12)][-1] for name in gens}   # warm-up: the graphs are captured here
    per_round = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name in gens:
            t0 = time.perf_counter()
            for k in range(args.frames):
                frame(name, k)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "tree": "this" if root == ROOT else "parent", "device": torch.cuda.get_device_name(0),
           "sizes": {size: [w, h] for size, w, h in SIZES}, "rounds": args.rounds, "frames_per_round": args.frames,
           "gate": "of the traced run: min_range %.1f, max_range %.1f, jump_rel %.2f, grow %d" % GATE,
           "timing": "host clock around create_pointcloud (synchronous), the cases (two sizes; without the filter and with it at "
                     "(radius, fill_min) = (1, 0), (2, 0), (1, 5), (2, 13)) alternating per round in one process; ms per frame: "
                     "median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "points": {name: int(len(c[0])) for name, c in clouds.items()}}
    if has_median:
        res["pixels"] = {}
        for name, gen in gens.items():
            if not name.endswith("_off"):
                flags = gen.read_stage(F.STAGE_MEDIAN)
                res["pixels"][name] = {"changed": int(np.count_nonzero(flags == F.MEDIAN_CHANGED)),
                                       "filled": int(np.count_nonzero(flags == F.MEDIAN_FILLED))}
    if args.kernel_trace:
        res["kernel_trace_us"] = kernel_times(args.kernel_trace)
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
