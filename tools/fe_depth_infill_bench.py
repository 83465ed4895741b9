#!/usr/bin/env python3
"""Cost and reach of the infill stage on the depth plane (cvo_fe_set_depth_infill): host-to-host time of one LiDAR frame
(create_pointcloud_lidar) at 1241 x 376 with and without the stage in the same process, the duration of the stage's
launch (k_fe_infill) at (2, 8) and at (15, 31) beside k_fe_lidar_cull and k_fe_median in one trace, and what the plane
holds: its coverage and the size of the cloud under SELECT_DEPTH at splat 0 with the stage, beside splat 1..3 and the
median stage's fill.

    python tools/fe_depth_infill_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_depth_infill_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_depth_infill.json

The scan is tools/fe_lidar_bench.py's synthetic one, of KITTI's shape, on the same colour images.
One generator per case, all alternating in one process: a round times --frames frames of each in turn (host clock around
synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest and largest
round beside it.  --root: the package of another checkout of the project (the parent commit's, built), which runs the
depth frames only; such a process counts as tree "parent".  --off-only: this tree the same way, two generators and
nothing else in the process, which is the process the parent's is compared with.
--trace-run: 30 LiDAR frames each (splat 0, occlusion window 7 x 1, the median stage (1, 3) behind the stage) under the
stage at (2, 8, 0.25) and at (15, 31, 0.25), and nothing else, for a rocprofv3 --kernel-trace run of its own (no
counters); --kernel-trace: the kernel_trace.csv of such a run: the durations (median, smallest, largest) of k_fe_infill at
either setting (the first 30 dispatches and the last 30), of k_fe_lidar_cull and of k_fe_median, and k_fe_infill over
k_fe_lidar_cull.
--merge: no GPU; the --out files of several processes of one session, in the order they ran, become one file; --bench:
result lines of bench.py, "<tree>=<the JSON line>" each, in the order they ran.  Nothing here is asserted, and nothing
here measures accuracy: no real scans are shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

from fe_lidar_bench import H, LINES, STEPS, VELO_R, VELO_T, W, scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_FRAMES = 30
TRACE_SETTINGS = ((2, 8, 0.25), (15, 31, 0.25))
KERNELS = ("k_fe_infill", "k_fe_lidar_cull", "k_fe_median")


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path):
    """The durations of KERNELS in a --trace-run's kernel trace; k_fe_infill by setting, in the order of the run"""
    by = {}
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for row in rows:
        name = row.get("Kernel_Name", "")
        for k in KERNELS:
            if k + "(" in name or k + "<" in name:
                by.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {k: _stats(v) for k, v in sorted(by.items()) if k != "k_fe_infill"}
    v = by.get("k_fe_infill", [])
    if len(v) == len(TRACE_SETTINGS) * TRACE_FRAMES:
        for n, f in enumerate(TRACE_SETTINGS):
            out["k_fe_infill_%d_%d" % f[:2]] = _stats(v[n * TRACE_FRAMES:(n + 1) * TRACE_FRAMES])
            if "k_fe_lidar_cull" in out:
                out["k_fe_infill_%d_%d_over_k_fe_lidar_cull" % f[:2]] = \
                    out["k_fe_infill_%d_%d" % f[:2]]["median_us"] / out["k_fe_lidar_cull"]["median_us"]
    elif v:
        out["k_fe_infill"] = _stats(v)
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "size", "rounds", "frames_per_round", "timing", "scan") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: what the stage is worth in trajectory accuracy needs real scans, and none are shipped"
    res["kernel"] = {"k_fe_infill": {"vgprs": 50, "scratch_bytes": 0, "lds_bytes": 25608, "waves_per_simd": 6,
                                     "from": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"}}
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = set(r["ms_per_frame"]) == {"depth_vga", "depth_kitti"}
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["off_this_minus_parent_ms"] = {}
    for case in ("depth_vga", "depth_kitti"):
        p, t = spread.get("parent:%s_alone" % case), spread.get("this:%s_alone" % case)
        if p and t:
            res["off_this_minus_parent_ms"][case] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                                     "parent_spread_max_minus_min": max(p) - min(p),
                                                     "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        if "plane" in f and f["tree"] == "this":
            res["plane"] = f["plane"]
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
            raise SystemExit("fe_depth_infill_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_depth_infill_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_infill = hasattr(F, "DepthInfill") and not args.off_only
    kitti = [pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    gens, scans = {}, []

    def lidar(splat):
        return F.Lidar(LINES * STEPS, splat, VELO_R, VELO_T, 0.0, 0.0, 0.25, 7, 1)

    if has_infill:
        scans = [scan(k) for k in range(4)]
    if args.trace_run:
        gen = F.PcdGenerator(W, H)
        gen.set_lidar(lidar(0))
        gen.set_depth_median(F.DepthMedian(1, 3))
        for f in TRACE_SETTINGS:
            gen.set_depth_infill(F.DepthInfill(*f))
            for k in range(TRACE_FRAMES):
                gen.create_pointcloud_lidar(kitti[k % 8][0], scans[k % 4], 4, F.FEATURES_HSV)
        gen.close()
        return
    gens["depth_vga"] = F.PcdGenerator(640, 480)
    gens["depth_kitti"] = F.PcdGenerator(W, H)
    if has_infill:
        for name, f in (("lidar_s0", None), ("lidar_s0_infill_2_8", (2, 8, 0.25)), ("lidar_s0_infill_15_31", (15, 31, 0.25))):
            gens[name] = F.PcdGenerator(W, H)
            gens[name].set_lidar(lidar(0))
            gens[name].set_depth_infill(None if f is None else F.DepthInfill(*f))
        gens["depth_kitti_infill_2_8"] = F.PcdGenerator(W, H)
        gens["depth_kitti_infill_2_8"].set_depth_infill(F.DepthInfill(2, 8, 0.25))

    def frame(name, k):
        if name == "depth_vga":
            return gens[name].create_pointcloud(vga[k % 8][0], vga[k % 8][1], 1, F.FEATURES_HSV)
        if name.startswith("depth_kitti"):
            return gens[name].create_pointcloud(kitti[k % 8][0], kitti[k % 8][1], 4, F.FEATURES_HSV)
        return gens[name].create_pointcloud_lidar(kitti[k % 8][0], scans[k % 4], 4, F.FEATURES_HSV)

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
           "scan": "synthetic, %d lines x %d steps = %d points of 16 bytes, max_points the same" % (LINES, STEPS, LINES * STEPS),
           "timing": "host clock around create_pointcloud* (synchronous), the cases alternating per round in one process; ms per "
                     "frame: median [min, max] over the rounds.  lidar_s0: splat 0, occl_rel 0.25 in a window of 7 x 1; "
                     "infill_X_Y: the stage at (X, Y, 0.25)",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()}}
    if has_infill:
        # what the plane holds: coverage and the cloud under SELECT_DEPTH at splat 0 with the stage, beside splat 0..3
        # without it and the median stage's fill
        gen = F.PcdGenerator(W, H)
        gen.set_select_mode(F.SELECT_DEPTH)
        res["plane"] = {}
        cases = [("splat%d" % s, s, None, None) for s in range(4)] + [("splat1_median_fill", 1, None, F.DepthMedian(1, 3))] + \
                [("splat0_infill_%d_%d%s" % (f[0], f[1], "" if f[2] else "_no_jump_test"), 0, f, None) for f in ((2, 8, 0.25), (2, 8, 0.0), (15, 31, 0.25))] + \
                [("splat0_infill_2_8_median_fill", 0, (2, 8, 0.25), F.DepthMedian(1, 3))]
        for name, splat, f, fill in cases:
            gen.set_lidar(lidar(splat))
            gen.set_depth_infill(None if f is None else F.DepthInfill(*f))
            gen.set_depth_median(fill)
            cloud = gen.create_pointcloud_lidar(kitti[0][0], scans[0], 4, F.FEATURES_HSV)
            entry = {"coverage": float(np.mean(gen.read_stage(F.STAGE_RECT_DEPTH) != 0)), "num_points": int(len(cloud[0])),
                     "num_want": gen.num_want, **{k: v for k, v in gen.info().items() if k in ("num_selected", "canny_used")}}
            if f is not None:
                flags = gen.read_stage(F.STAGE_INFILL)
                entry.update({"settings": list(f), "sparse_coverage": float(np.mean(gen.read_stage(F.STAGE_SPARSE_DEPTH) != 0)),
                              "row_share": float(np.mean(flags == F.INFILL_ROW)), "col_share": float(np.mean(flags == F.INFILL_COL)),
                              "jump_share": float(np.mean(flags == F.INFILL_JUMP))})
            res["plane"][name] = entry
        gen.close()
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
