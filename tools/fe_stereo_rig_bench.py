#!/usr/bin/env python3
"""Cost of a stereo rig in the front end, by the method of tools/fe_stereo_bench.py (whose synthetic pair this uses):
host-to-host time of one 1241 x 376 stereo frame (create_pointcloud_stereo) with a rig set -- both images resampled on
the device in front of the matcher -- against the same frame without one, at max_disp 64 and 128, the four cases
alternating per round in one process.

    python tools/fe_stereo_rig_bench.py [--out FILE] [--rounds 7] [--frames 100] [--root DIR] [--label TEXT] [--tree NAME]
                                        [--only rig|stereo|depth] [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_stereo_rig_bench.py --merge A.json B.json ... [--bench-lines FILE] --out profiles/fe_stereo_rig.json

--only rig (the default): the four cases above.  --only stereo: the two cases without a rig and nothing else; --only depth:
a plain VGA depth frame and nothing else -- the unchanged paths, for processes of this tree and of the parent commit's
(--root, built) that alternate.  --trace-run: 30 rig frames at each max_disp and 30 VGA depth frames under a distorting
camera model (TUM fr1: k_fe_rectify, the yardstick) and nothing else, for a rocprofv3 --kernel-trace run of its own;
--kernel-trace: the kernel_trace.csv of such a run, whose k_fe_* durations are folded into the output with the time per
output pixel of k_fe_stereo_rectify (two images of 1241 x 376) beside k_fe_rectify's (one colour and one depth image of
640 x 480).  --merge: no GPU; the --out files of the processes of one session, in the order they ran, become one file:
`runs` lists every process, `medians_min_max_runs` the smallest and largest median per tree and case over them with the
number of processes, `rig_minus_no_rig_ms` the cost of a rig per max_disp (median over the processes of the difference
of the two cases' medians), `this_minus_parent_ms` the difference of the two trees' medians on the unchanged paths beside
each tree's own spread, the kernel trace of the last file that has one, and --bench-lines: a file of lines
"<tree>_<k> <the JSON line bench.py printed>" recorded in the same session.  Nothing here is asserted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fe_stereo_bench import H, W, _stats, pair   # noqa: E402  (the synthetic pair and the statistics of the stereo tool)

TRACE_FRAMES = 30
DISPS = (64, 128)
SETTINGS = dict(baseline=0.54, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1)
# a rig of KITTI raw's kind for W x H: wide lenses with a barrel distortion, the cameras half a degree apart
CALIB = dict(left=(984.2, 980.8, 690.0, 233.2, (-0.3728, 0.2037, 0.0022, 0.0014, -0.0723)),
             right=(989.5, 987.5, 702.0, 245.6, (-0.3644, 0.1790, 0.0011, -0.0006, -0.0532)),
             R=(0.99996, 0.0078, -0.0042, -0.0078, 0.99997, -0.0011, 0.0042, 0.0011, 0.99999), T=(-0.537, 0.0048, -0.0125))
PIXELS = {"k_fe_stereo_rectify": 2 * W * H, "k_fe_rectify": 640 * 480}


def kernel_times(path):
    """Durations (us) of the dispatches of a rocprofv3 kernel trace by kernel name, k_fe_* only, and the resampling
    kernels' time per output pixel"""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_" not in name:
                continue
            short = name[name.index("k_fe_"):].split("(")[0]
            by.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {k: _stats(v) for k, v in sorted(by.items())}
    per_pixel = {k: out[k]["median_us"] * 1e3 / n for k, n in PIXELS.items() if k in out}
    if len(per_pixel) == 2:
        per_pixel["ratio"] = per_pixel["k_fe_stereo_rectify"] / per_pixel["k_fe_rectify"]
    return out, {"ns_per_output_pixel": per_pixel, "output_pixels": PIXELS}


def merge(paths, bench_lines, out_path):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "stereo_image", "depth_image", "rounds", "frames_per_round", "timing", "settings",
                                "calibration") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["runs"] = [{"run": f.get("label", ""), "tree": f.get("tree") or ("this" if f.get("root", ".") == "." else "parent"),
                    "only": f.get("only", "rig"), "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread, cost = {}, {D: [] for D in DISPS}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault("%s:%s:%s" % (r["tree"], r["only"], case), []).append(v[0])
        for D in DISPS:
            a, b = r["ms_per_frame"].get("stereo_d%d_rig" % D), r["ms_per_frame"].get("stereo_d%d" % D)
            if a and b:
                cost[D].append(a[0] - b[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["rig_minus_no_rig_ms"] = {"d%d" % D: {"median_of_the_runs": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}
                                  for D, v in cost.items() if v}
    unchanged = {}
    for key, t in spread.items():
        tree, only, case = key.split(":")
        p = spread.get("parent:%s:%s" % (only, case))
        if tree == "this" and only != "rig" and p:
            unchanged[case] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                               "parent_spread_max_minus_min": max(p) - min(p), "this_spread_max_minus_min": max(t) - min(t)}
    res["this_minus_parent_ms"] = unchanged
    for f in files:
        for k in ("points", "pixels_kept"):
            if k in f:
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
            res["resampling"] = f["resampling"]
    if bench_lines:
        res["bench_py"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5 in each tree in turn, in the same session"}
        for line in open(bench_lines):
            name, _, text = line.strip().partition(" ")
            if text.startswith("{"):
                got = json.loads(text)
                res["bench_py"][name] = {k: got[k] for k in ("value", "ms_per_step") if k in got}
    print(json.dumps({k: res[k] for k in ("medians_min_max_runs", "rig_minus_no_rig_ms", "this_minus_parent_ms")}), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--only", choices=("rig", "stereo", "depth"), default="rig")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_stereo_rig_bench: --merge needs --out")
        merge(args.merge, args.bench_lines, args.out)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_stereo_rig_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    if (args.only == "rig" or args.trace_run) and not hasattr(F, "StereoRig"):
        raise SystemExit("fe_stereo_rig_bench: the package of --root has no stereo rig: --only stereo or --only depth")
    pairs = [pair(400 + k) for k in range(4)]
    depth_frames = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    gens = {}
    with_rig = args.only == "rig" or args.trace_run
    if args.only != "depth" or args.trace_run:
        rig = F.stereo_rectify(F.StereoCalib(**CALIB), W, H, 2000.0) if with_rig else None
        for D in DISPS:
            for name, r in (("stereo_d%d" % D, None), ("stereo_d%d_rig" % D, rig)):
                if (r is None) == (name.endswith("_rig") or args.trace_run):   # (no rig: no rig case; a trace run: rig cases only)
                    continue
                gens[name] = F.PcdGenerator(W, H)
                gens[name].set_stereo(F.Stereo(max_disp=D, **SETTINGS))
                if r is not None:
                    gens[name].set_stereo_rig(r)
    if args.only == "depth" or args.trace_run:
        gens["depth_vga"] = F.PcdGenerator(640, 480)
        if args.trace_run:
            gens["depth_vga"].set_camera(F.TUM_CAMERAS["fr1"])

    def frame(name, k):
        if name == "depth_vga":
            return gens[name].create_pointcloud(depth_frames[k % 8][0], depth_frames[k % 8][1], 1, F.FEATURES_HSV)
        return gens[name].create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)

    if args.trace_run:
        for name in gens:
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
    res = {"label": args.label, "tree": args.tree, "root": os.path.relpath(root, ROOT), "only": args.only,
           "device": torch.cuda.get_device_name(0), "stereo_image": [W, H], "depth_image": [640, 480], "rounds": args.rounds,
           "frames_per_round": args.frames, "settings": SETTINGS, "calibration": {k: list(v) for k, v in CALIB.items()},
           "timing": "host clock around create_pointcloud[_stereo] (synchronous), cases alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "points": {name: int(len(c[0])) for name, c in clouds.items()}}
    stereo_gens = [n for n in gens if n != "depth_vga"]
    if stereo_gens:
        res["pixels_kept"] = {n: int(np.count_nonzero(gens[n].read_stage(F.STAGE_STEREO) == 0)) for n in stereo_gens}
    if args.kernel_trace:
        res["kernel_trace_us"], res["resampling"] = kernel_times(args.kernel_trace)
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
