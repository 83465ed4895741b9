#!/usr/bin/env python3
"""Cost of the stereo matcher in the front end: host-to-host time of one 1241 x 376 stereo frame
(create_pointcloud_stereo: staging, upload of both images, every kernel, the cloud back on the host) at max_disp 64 and
128, beside the time of a plain VGA depth frame (create_pointcloud) on the same tree -- the unchanged path.

    python tools/fe_stereo_bench.py [--out FILE] [--rounds 7] [--frames 100] [--root DIR] [--label TEXT] [--tree NAME]
                                    [--depth-only] [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_stereo_bench.py --merge A.json B.json ... --out profiles/fe_stereo.json

One generator per case, the cases alternating in one process: a round times --frames frames of each case in turn (host
clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest
and largest round beside it.  The pairs are synthetic (one smoothed random texture, a background at 6 pixels, a box at
40 and a ramp from 4 to 9), four of them in turn; the depth frames are data.synthetic_rgbd_frame's.
--root: measure the package of another checkout of the project (e.g. the parent commit's, built) the same way; a package
without stereo runs the depth case only, and so does --depth-only on any tree: a depth frame timed between stereo frames
(each of which streams a cost volume of 60 or 119 MB through the caches) is not the frame a process without stereo sees, so
the comparison of the unchanged path with the parent is made between processes that run nothing else.  --trace-run: 30
frames of each stereo case in turn and nothing else, for a rocprofv3 --kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of such a run, whose k_fe_* durations
(median, smallest, largest, count) are folded into the output, the matcher's kernels per case as well (their dispatches in
the order they started).  --merge: no GPU; the --out files of several processes of one session, in the order they ran
(give each a --label; a --root other than the tool's own tree counts as tree "parent" unless --tree names it), become one
file: `runs` lists every process, `medians_min_max_runs` the smallest and largest median per tree and case over them with
the number of processes, `depth_frame_this_minus_parent_ms` the difference of the two trees' depth-frame medians beside
each tree's own spread over its processes, and the kernel trace of the last file that has one.  Nothing here is asserted."""
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
STEREO = (("stereo_d64", 64), ("stereo_d128", 128))
W, H = 1241, 376
MATCHER = ("k_fe_stereo_grey", "k_fe_census", "k_fe_sgm_path", "k_fe_sgm_winner", "k_fe_stereo_final")


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path):
    """Durations (us) of the dispatches of a rocprofv3 kernel trace, by kernel name, k_fe_* only; the matcher's also per
    case of a --trace-run (the first half of a kernel's dispatches belongs to the first case)."""
    by, when = {}, {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_" not in name:
                continue
            short = name[name.index("k_fe_"):].split("(")[0]
            start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
            by.setdefault(short, []).append((end - start) / 1e3)
            base = short.split("<")[0]
            if base in MATCHER:
                when.setdefault(base, []).append((start, (end - start) / 1e3))
    out = {k: _stats(v) for k, v in sorted(by.items())}
    for base, v in sorted(when.items()):
        v.sort()
        half = len(v) // 2
        if half and len(v) % (2 * TRACE_FRAMES) == 0:
            for (case, _), part in zip(STEREO, (v[:half], v[half:])):
                out[base + ":" + case] = _stats([d for _, d in part])
                out[base + ":" + case]["per_frame"] = len(part) // TRACE_FRAMES
    return out


def merge(paths, out_path):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "stereo_image", "depth_image", "rounds", "frames_per_round", "timing", "settings")
           if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["runs"] = [{"run": f.get("label", ""), "tree": f.get("tree") or ("this" if f.get("root", ".") == "." else "parent"),
                    "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = len(r["ms_per_frame"]) == 1   # (a process that ran the depth case and nothing else)
        for case, v in r["ms_per_frame"].items():
            name = "depth_vga_alone" if case == "depth_vga" and alone else case
            spread.setdefault(r["tree"] + ":" + name, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    if "parent:depth_vga_alone" in spread and "this:depth_vga_alone" in spread:
        p, t = spread["parent:depth_vga_alone"], spread["this:depth_vga_alone"]
        res["depth_frame_this_minus_parent_ms"] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                                   "parent_spread_max_minus_min": max(p) - min(p),
                                                   "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        for k in ("points", "pixels_kept"):
            if k in f:
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def pair(seed):
    """A synthetic rectified pair of W x H: the right image a window of a smoothed random texture, the left one resampled
    at x - disp (bilinear, rounded)"""
    pad = 48
    rng = np.random.Generator(np.random.PCG64(seed))
    t = rng.integers(0, 256, (H + 2, W + pad + 2, 3)).astype(np.float64)
    t = (t[:, :-2] + 2.0 * t[:, 1:-1] + t[:, 2:]) / 4.0
    t = (t[:-2] + 2.0 * t[1:-1] + t[2:]) / 4.0
    t = (t - t.min()) * (255.0 / (t.max() - t.min()))
    disp = np.full((H, W), 6.0)
    disp[H // 4:3 * H // 4, W // 3:2 * W // 3] = 40.0
    disp[:H // 6, :] = 4.0 + 5.0 * np.arange(W)[None, :] / (W - 1)
    xs = pad + np.arange(W)[None, :] - disp
    x0 = np.floor(xs).astype(np.int64)
    a = (xs - x0)[:, :, None]
    rows = np.arange(H)[:, None]
    left = (1.0 - a) * t[rows, x0] + a * t[rows, x0 + 1]
    as_bytes = lambda v: np.ascontiguousarray(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return as_bytes(left), as_bytes(t[:, pad:pad + W])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--depth-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_stereo_bench: --merge needs --out")
        merge(args.merge, args.out)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_stereo_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_stereo = hasattr(F, "Stereo") and not args.depth_only
    pairs = [pair(400 + k) for k in range(4)] if has_stereo else []
    depth_frames = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    settings = dict(baseline=0.54, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1)
    gens = {}
    if has_stereo:
        for name, D in STEREO:
            gens[name] = F.PcdGenerator(W, H)
            gens[name].set_stereo(F.Stereo(max_disp=D, **settings))
    if args.trace_run:
        for name, _ in STEREO:
            for k in range(TRACE_FRAMES):
                gens[name].create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)
        for gen in gens.values():
            gen.close()
        return
    gens["depth_vga"] = F.PcdGenerator(640, 480)

    def frame(name, k):
        if name == "depth_vga":
            return gens[name].create_pointcloud(depth_frames[k % 8][0], depth_frames[k % 8][1], 1, F.FEATURES_HSV)
        return gens[name].create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)

    clouds = {name: [frame(name, k) for k in range(12)][-1] for name in gens}   # warm-up: the graphs are captured here
    per_round = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name in gens:
            t0 = time.perf_counter()
            for k in range(args.frames):
                frame(name, k)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "tree": args.tree, "root": os.path.relpath(root, ROOT), "device": torch.cuda.get_device_name(0),
           "stereo_image": [W, H], "depth_image": [640, 480], "rounds": args.rounds, "frames_per_round": args.frames,
           "settings": settings,
           "timing": "host clock around create_pointcloud[_stereo] (synchronous), cases alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "points": {name: int(len(c[0])) for name, c in clouds.items()}}
    if has_stereo:
        res["pixels_kept"] = {name: int(np.count_nonzero(gens[name].read_stage(F.STAGE_STEREO) == 0)) for name, _ in STEREO}
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
