#!/usr/bin/env python3
"""Cost of motion compensation of a spinning scan (cvo_fe_set_lidar_sweep): host-to-host time of one LiDAR frame
(create_pointcloud_lidar) at 1241 x 376 with a sweep of each mode against the same frame without one, all alternating
in one process, and the durations of the instances of k_fe_lidar_project beside instance 0 and k_fe_lidar_cull in one
trace.  The scan is tools/fe_lidar_bench.py's: 120 000 points of KITTI's shape, whose fourth word carries a time here
(a float32 in seconds, or a uint32 in nanoseconds, by the azimuth); the twist changes with every frame.

    python tools/fe_lidar_sweep_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                         [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_lidar_sweep_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_lidar_sweep.json

One generator per case; a round times --frames frames of each in turn (host clock around synchronous calls); recorded
per case are the median over the rounds of the per-frame time and the smallest and largest round beside it.  --root: the
package of another checkout of the project (the parent commit's, built), which runs the cases without a sweep only;
such a process counts as tree "parent".  --off-only: this tree the same way, which is the process the parent's is
compared with.  --trace-run: 30 frames of each case and nothing else, for a rocprofv3 --kernel-trace run of its own (no
counters); --kernel-trace: the kernel_trace.csv of such a run.  --merge: no GPU; the --out files of several processes of
one session, in the order they ran, become one file; --bench: result lines of bench.py, "<tree>=<the JSON line>" each.
Nothing here is asserted, and nothing here measures accuracy: no real scans are shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fe_lidar_bench import H, LINES, STEPS, VELO_R, VELO_T, W, scan  # noqa: E402

TRACE_FRAMES = 30
SWEEP_S = 0.1                                   # a sweep of 0.1 s
INSTANCES = {"k_fe_lidar_project<0>": "project_0_no_sweep", "k_fe_lidar_project<1>": "project_1_time_f32",
             "k_fe_lidar_project<2>": "project_2_time_u32", "k_fe_lidar_project<3>": "project_3_azimuth",
             "k_fe_lidar_project(": "project_parent", "k_fe_lidar_cull": "cull", "k_fe_depth_final": "depth_final"}


def timed(points, as_u32):
    """the scan with its fourth word a time by the azimuth: seconds as float32, or nanoseconds as uint32"""
    out = points.copy()
    turn = np.arctan2(points[:, 1], points[:, 0]) / (2 * np.pi) + 0.5
    if as_u32:
        out[:, 3].view(np.uint32)[:] = (turn * SWEEP_S * 1e9).astype(np.uint32)
    else:
        out[:, 3] = (turn * SWEEP_S).astype(np.float32)
    return out


def kernel_times(path):
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            for key, label in INSTANCES.items():
                if key in name:
                    by.setdefault(label, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}
            for k, v in sorted(by.items())}


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    res = {k: files[-1][k] for k in ("device", "size", "rounds", "frames_per_round", "timing", "scan") if k in files[-1]}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: what motion compensation is worth in trajectory accuracy needs real scans, and none are shipped"
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = not any(k.startswith("sweep") for k in r["ms_per_frame"])
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    for f in files:
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
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


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
            raise SystemExit("fe_lidar_sweep_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_lidar_sweep_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_sweep = hasattr(F, "LidarSweep") and not args.off_only
    kitti = [pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    plain = [scan(k) for k in range(4)]
    scans = {"no_sweep": plain, "depth": None}
    lidar = F.Lidar(LINES * STEPS, 1, VELO_R, VELO_T, 0.0, 0.0, 0.25, 7, 1)
    gens = {"depth": F.PcdGenerator(W, H), "no_sweep": F.PcdGenerator(W, H)}
    gens["no_sweep"].set_lidar(lidar)
    if has_sweep:
        sweeps = {"sweep_time_f32": F.LidarSweep(F.SWEEP_TIME_F32, 12, 0.0, 1.0 / SWEEP_S, s_ref=0.5),
                  "sweep_time_u32": F.LidarSweep(F.SWEEP_TIME_U32, 12, 0.0, 1e-9 / SWEEP_S, s_ref=0.5),
                  "sweep_azimuth": F.LidarSweep(F.SWEEP_AZIMUTH, phase0=0.5, direction=1, s_ref=0.5)}
        scans.update({"sweep_time_f32": [timed(p, False) for p in plain], "sweep_time_u32": [timed(p, True) for p in plain],
                      "sweep_azimuth": plain})
        for name, sw in sweeps.items():
            gens[name] = F.PcdGenerator(W, H)
            gens[name].set_lidar(lidar)
            gens[name].set_lidar_sweep(sw)
    twists = [np.array([0.002 * k, -0.001 * k, 0.05 + 0.004 * k, 1.0 + 0.02 * k, 0.01 * k, 0.0], np.float32) for k in range(8)]

    def frame(name, k):
        if name == "depth":
            return gens[name].create_pointcloud(kitti[k % 8][0], kitti[k % 8][1], 4, F.FEATURES_HSV)
        if name != "no_sweep":
            gens[name].set_lidar_motion(twists[k % 8])
        return gens[name].create_pointcloud_lidar(kitti[k % 8][0], scans[name][k % 4], 4, F.FEATURES_HSV)

    if args.trace_run:
        for name in gens:
            for k in range(TRACE_FRAMES):
                frame(name, k)
        for gen in gens.values():
            gen.close()
        return
    for name in gens:   # warm-up: the graphs are captured here
        for k in range(12):
            frame(name, k)
    per_round = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name in gens:
            t0 = time.perf_counter()
            for k in range(args.frames):
                frame(name, k)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "tree": "this" if root == ROOT else "parent", "device": torch.cuda.get_device_name(0),
           "size": [W, H], "rounds": args.rounds, "frames_per_round": args.frames,
           "scan": "synthetic, %d lines x %d steps = %d points of 16 bytes, max_points the same; splat 1, occlusion window 7 x 1"
                   % (LINES, STEPS, LINES * STEPS),
           "timing": "host clock around create_pointcloud* (synchronous; under a sweep set_lidar_motion in front of it), the "
                     "cases alternating per round in one process; ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()}}
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
