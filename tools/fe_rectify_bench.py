#!/usr/bin/env python3
"""Cost of a camera model in the front end: host-to-host time of one VGA frame (create_pointcloud: staging, upload,
every kernel, the cloud back on the host) without a model, with a zero-distortion model and with the TUM fr1 model
(the rectification pass k_fe_rectify in front of everything else).

    python tools/fe_rectify_bench.py [--out profiles/fe_rectify.json] [--rounds 9] [--frames 300] [--root DIR]
                                     [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>] [--label TEXT]
    python tools/fe_rectify_bench.py --merge A.json B.json ... --out profiles/fe_rectify.json [--bench parent.json this.json]

One generator per case, the cases alternating in one process: a round times --frames frames of each case in turn (host
clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest
and largest round beside it.  The frames are synthetic (data.synthetic_rgbd_frame, texture 1.0), eight of them in turn.
--root: measure the package of another checkout of the project (e.g. the parent commit's, built) the same way; a package
without camera models runs the first case only.  --trace-run: 50 fr1 frames and nothing else, for a rocprofv3
--kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of such a run, whose k_fe_rectify durations (median,
smallest, largest, count) are folded into the output.  --merge: no GPU; the --out files of several processes of one
session, in the order they ran (give each a --label; a --root other than the tool's own tree counts as tree "parent"),
become one file: `runs` lists every process, `medians_min_max_runs` the smallest and largest median per tree and case
over them with the number of processes, the kernel trace of the last file that has one is kept with the bytes per second
k_fe_rectify's median stands for, and --bench adds `value` / `ms_per_step` of two saved bench.py result lines (the
parent's, this tree's).  Nothing here is asserted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_times(path):
    """Durations (us) of the dispatches of a rocprofv3 kernel trace, by kernel name, k_fe_* only."""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_" not in name:
                continue
            short = name[name.index("k_fe_"):].split("(")[0]
            by.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}
            for k, v in sorted(by.items())}


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "image", "rounds", "frames_per_round", "timing") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["runs"] = [{"run": f.get("label", ""), "tree": "this" if f.get("root", ".") == "." else "parent",
                    "ms_per_frame": f["ms_per_frame"]} for f in files]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    for f in files:
        for k in ("points", "zero_distortion_cloud_equals_no_model", "rectify_bytes"):
            if k in f:
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    if "kernel_trace_us" in res and "k_fe_rectify" in res["kernel_trace_us"] and "rectify_bytes" in res:
        res["k_fe_rectify_bytes_per_s"] = (sum(res["rectify_bytes"].values()) /
                                           (res["kernel_trace_us"]["k_fe_rectify"]["median_us"] * 1e-6))
    if bench:
        rows = [json.loads(open(p).read().strip().split("\n")[-1]) for p in bench]
        res["bench_py"] = {name: {"value": r.get("value"), "ms_per_step": r.get("ms_per_step"), "unit": r.get("unit")}
                           for name, r in zip(("parent", "this"), rows)}
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench", nargs=2, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_rectify_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_rectify_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    w, h = 640, 480
    frames = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    cases = [("no_model", None)]
    if hasattr(F, "CameraModel"):
        row1 = F.camera(1)
        cases.append(("zero_distortion", F.CameraModel(row1["scaling_factor"], row1["fx"], row1["fy"], row1["cx"],
                                                       row1["cy"])))
        cases.append(("fr1", F.TUM_CAMERAS["fr1"]))
    if args.trace_run:
        gen = F.PcdGenerator(w, h)
        gen.set_camera(F.TUM_CAMERAS["fr1"])
        for k in range(50):
            gen.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
        gen.close()
        return
    gens = []
    for name, cam in cases:
        g = F.PcdGenerator(w, h)
        if cam is not None:
            g.set_camera(cam)
        gens.append(g)
    clouds = []
    for g in gens:   # warm-up: the graph of each context is captured here
        for k in range(16):
            c = g.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
        clouds.append(c)
    per_round = {name: [] for name, _ in cases}
    for _ in range(args.rounds):
        for (name, _), g in zip(cases, gens):
            t0 = time.perf_counter()
            for k in range(args.frames):
                g.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "root": os.path.relpath(root, ROOT), "device": torch.cuda.get_device_name(0),
           "image": [w, h], "rounds": args.rounds, "frames_per_round": args.frames,
           "timing": "host clock around create_pointcloud (synchronous), cases alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {}}
    for name, _ in cases:
        v = per_round[name]
        res["ms_per_frame"][name] = [statistics.median(v), min(v), max(v)]
    if len(cases) > 1:
        res["zero_distortion_cloud_equals_no_model"] = bool(np.array_equal(clouds[0][0], clouds[1][0]) and
                                                            np.array_equal(clouds[0][1], clouds[1][1]))
        res["points"] = {name: int(len(c[0])) for (name, _), c in zip(cases, clouds)}
        res["rectify_bytes"] = {"images_read": w * h * 5, "map_read": w * h * 8, "images_written": w * h * 5}
    if args.kernel_trace:
        res["kernel_trace_us"] = kernel_times(args.kernel_trace)
    for g in gens:
        g.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
