#!/usr/bin/env python3
"""Cost of a LiDAR scan in place of the depth image (cvo_fe_set_lidar): host-to-host time of one frame
(create_pointcloud_lidar) at 1241 x 376 beside a stereo frame and a plain depth frame in the same process, the
durations of the stage's launches (k_fe_lidar_project, k_fe_lidar_cull) beside k_fe_depth_warp / k_fe_depth_final and
k_fe_median in one trace, and what the plane holds: its coverage and the size of the cloud under SELECT_DEPTH at splat
0..3, with and without the median stage's fill.

    python tools/fe_lidar_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                   [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_lidar_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_lidar.json

The scan is synthetic, of KITTI's shape: 64 lines between +2 and -24.8 degrees, 1875 azimuth steps (120 000 points), a
ground plane 1.73 m below the scanner, a wall at 30 m and twelve poles and boxes nearer, seen from a scanner 0.27 m
behind and 0.08 m above the camera (Tr_velo_to_cam's shape); four scans in turn, the scene turned a little each.  Some
16 000 of its points are in the camera's view (`in_view` of the output).  The colour images are data.synthetic_rgbd_frame's.
One generator per case, all alternating in one process: a round times --frames frames of each in turn (host clock around
synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest and largest
round beside it.  --root: the package of another checkout of the project (the parent commit's, built), which runs the
depth frames only; such a process counts as tree "parent".  --off-only: this tree the same way, two generators and
nothing else in the process, which is the process the parent's is compared with.
--trace-run: 30 frames each of a LiDAR frame (splat 1, occlusion window 7 x 1, the median stage (1, 3) behind it) and of
a frame under a depth camera of the colour image's size, and nothing else, for a rocprofv3 --kernel-trace run of its own
(no counters); --kernel-trace: the kernel_trace.csv of such a run: the durations (median, smallest, largest) of the five
kernels.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_FRAMES = 30
W, H = 1241, 376
LINES, STEPS = 64, 1875
# velodyne (x forward, y left, z up) -> camera (x right, y down, z forward), and where the scanner sits
VELO_R = (0.0, -1.0, 0.0, 0.0, 0.0, -1.0, 1.0, 0.0, 0.0)
VELO_T = (0.0, -0.08, -0.27)
KERNELS = ("k_fe_lidar_project", "k_fe_lidar_cull", "k_fe_depth_warp", "k_fe_depth_final", "k_fe_median")


def scan(seed):
    """A synthetic scan of KITTI's shape: LINES * STEPS x 4 float32 (x y z reflectance) in the scanner's frame"""
    rng = np.random.Generator(np.random.PCG64(seed))
    el = np.deg2rad(np.linspace(2.0, -24.8, LINES))[:, None]
    az = (np.arange(STEPS) * (2.0 * np.pi / STEPS) + 0.01 * seed)[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1)
    with np.errstate(divide="ignore"):
        r = np.where(d[..., 2] < 0, -1.73 / d[..., 2], np.inf)                  # the ground
    r = np.minimum(r, 30.0 / np.hypot(d[..., 0], d[..., 1]))                      # a wall around
    for k in range(12):                                                           # poles and boxes: vertical cylinders
        a, dist, rad, top = rng.uniform(-0.7, 0.7), rng.uniform(5.0, 25.0), rng.uniform(0.15, 1.2), rng.uniform(-0.5, 1.0)
        cx, cy = dist * np.cos(a), dist * np.sin(a)
        b = d[..., 0] * cx + d[..., 1] * cy
        h2 = d[..., 0] ** 2 + d[..., 1] ** 2
        disc = b * b - h2 * (cx * cx + cy * cy - rad * rad)
        t = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / h2, np.inf)
        t = np.where((t > 0) & (t * d[..., 2] < top), t, np.inf)
        r = np.minimum(r, t)
    r = r * (1.0 + 0.002 * rng.standard_normal(r.shape))
    pts = (d * r[..., None]).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([pts, rng.random((len(pts), 1))], axis=1).astype(np.float32))


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path):
    """The durations of KERNELS in a --trace-run's kernel trace"""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            for k in KERNELS:
                if k + "(" in name or k + "<" in name:
                    by.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: _stats(v) for k, v in sorted(by.items())}


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "size", "rounds", "frames_per_round", "timing", "scan") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: what the stage is worth in trajectory accuracy needs real scans, and none are shipped"
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
        for k in ("plane", "in_view"):
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
            raise SystemExit("fe_lidar_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_lidar_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_lidar = hasattr(F, "Lidar") and not args.off_only
    kitti = [pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    gens, scans = {}, []

    def lidar(splat, occl=True):
        return F.Lidar(LINES * STEPS, splat, VELO_R, VELO_T, 0.0, 0.0, 0.25 if occl else 0.0, 7 if occl else 0, 1 if occl else 0)

    if has_lidar:
        scans = [scan(k) for k in range(4)]
    if args.trace_run:
        gens["lidar"] = F.PcdGenerator(W, H)
        gens["lidar"].set_lidar(lidar(1))
        gens["lidar"].set_depth_median(F.DepthMedian(1, 3))
        gens["rig"] = F.PcdGenerator(W, H)
        row = F.camera(4)
        gens["rig"].set_depth_camera(F.DepthCamera(width=W, height=H, depth_scale=row["scaling_factor"], fx=row["fx"], fy=row["fy"],
                                                   cx=row["cx"], cy=row["cy"], T=(0.05, 0.0, 0.0)))
        for k in range(TRACE_FRAMES):
            gens["lidar"].create_pointcloud_lidar(kitti[k % 8][0], scans[k % 4], 4, F.FEATURES_HSV)
        for k in range(TRACE_FRAMES):
            gens["rig"].create_pointcloud(kitti[k % 8][0], kitti[k % 8][1], 4, F.FEATURES_HSV)
        for gen in gens.values():
            gen.close()
        return
    gens["depth_vga"] = F.PcdGenerator(640, 480)
    gens["depth_kitti"] = F.PcdGenerator(W, H)
    if has_lidar:
        from fe_stereo_bench import pair
        pairs = [pair(400 + k) for k in range(4)]
        gens["stereo_64"] = F.PcdGenerator(W, H)
        gens["stereo_64"].set_stereo(F.Stereo(baseline=0.54, max_disp=64, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1))
        for splat in (0, 1, 3):
            gens["lidar_s%d" % splat] = F.PcdGenerator(W, H)
            gens["lidar_s%d" % splat].set_lidar(lidar(splat))
        gens["lidar_s1_noocc"] = F.PcdGenerator(W, H)
        gens["lidar_s1_noocc"].set_lidar(lidar(1, occl=False))
        gens["lidar_s1_median_select"] = F.PcdGenerator(W, H)
        gens["lidar_s1_median_select"].set_lidar(lidar(1))
        gens["lidar_s1_median_select"].set_depth_median(F.DepthMedian(1, 3))
        gens["lidar_s1_median_select"].set_select_mode(F.SELECT_DEPTH)

    def frame(name, k):
        if name == "depth_vga":
            return gens[name].create_pointcloud(vga[k % 8][0], vga[k % 8][1], 1, F.FEATURES_HSV)
        if name == "depth_kitti":
            return gens[name].create_pointcloud(kitti[k % 8][0], kitti[k % 8][1], 4, F.FEATURES_HSV)
        if name.startswith("stereo"):
            return gens[name].create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)
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
                     "frame: median [min, max] over the rounds.  lidar_sK: splat K, occl_rel 0.25 in a window of 7 x 1",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()}}
    if has_lidar:
        # what the plane holds: coverage and the cloud under SELECT_DEPTH, splat by splat, with and without the fill
        gen = F.PcdGenerator(W, H)
        gen.set_select_mode(F.SELECT_DEPTH)
        res["plane"] = {}
        for splat in range(4):
            for fill in (None, F.DepthMedian(1, 3)):
                gen.set_lidar(lidar(splat))
                gen.set_depth_median(fill)
                cloud = gen.create_pointcloud_lidar(kitti[0][0], scans[0], 4, F.FEATURES_HSV)
                flags = gen.read_stage(F.STAGE_LIDAR)
                res["plane"]["splat%d%s" % (splat, "_fill" if fill else "")] = {
                    "hit_share": float(np.mean(flags != 0)), "occluded_share": float(np.mean((flags & F.LIDAR_OCCLUDED) != 0)),
                    "coverage": float(np.mean(gen.read_stage(F.STAGE_RECT_DEPTH) != 0)), "num_points": int(len(cloud[0])),
                    "num_want": gen.num_want, **{k: v for k, v in gen.info().items() if k in ("num_selected", "canny_used")}}
        gen.set_lidar(lidar(0, occl=False))
        gen.set_depth_median(None)
        gen.create_pointcloud_lidar(kitti[0][0], scans[0], 4, F.FEATURES_HSV)
        # (at splat 0 several points share a pixel: the pixels hit bound the points in view from below)
        res["in_view"] = {"points": int(len(scans[0])), "pixels_hit_at_splat_0": int(np.count_nonzero(gen.read_stage(F.STAGE_LIDAR)))}
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
