#!/usr/bin/env python3
"""Cost of cvo_hip_pose_scan next to the loop of cvo_hip_pose_score calls it replaces, in one process on the same clouds.

    python tools/pose_scan_bench.py [--out profiles/pose_scan.json] [--reps 7] [--cases 3000,10000,desk]
                                    [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]

For the synthetic cvo pairs of 3 000 and 10 000 points and the first pair of the shipped fr1/desk clouds, at ell = 0.1, with
K = 256 and K = 4 096 candidate poses -- perturbations of the pose of the accuracy tests (rotation 2 .. 10 degrees about
random axes, translation 3 .. 15 cm, PCG64 seed 20261) -- and warm norm caches:
  (a) one cvo_hip_pose_scan of the K poses;
  (b) K = 256 only: a loop of K cvo_hip_pose_score calls.
The two are timed alternately, --reps times each after a warm-up of each; recorded are the medians, the smallest and the
largest time (host clock around synchronous calls), poses per second, and the segment pairs that survive the scan's
culling (counted on the host from the device clouds' bounding spheres with the kernel's test in float64).
--trace-run: only the scans, three times each (for a rocprofv3 --kernel-trace run of its own).  --kernel-trace: the
kernel_trace.csv of such a run; the median duration of k_pose_scan per case and K is folded into the output together with
the pair tests per second it stands for (surviving segment pairs x 4 096 / time).  Nothing here is asserted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ELL = 0.1
KS = (256, 4096)


def rot(axis, th):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def poses(n):
    rng = np.random.Generator(np.random.PCG64(20261))
    R0 = rot([0.3, -0.5, 0.8], 0.02)
    T0 = np.array([0.01, -0.02, 0.015])
    Rs, Ts = [], []
    for _ in range(n):
        d = rng.normal(size=3)
        Rs.append(R0 @ rot(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 10.0))))
        Ts.append(T0 + d / np.linalg.norm(d) * rng.uniform(0.03, 0.15))
    return np.asarray(Rs, np.float32), np.asarray(Ts, np.float32)


def surviving_segment_pairs(ctx, capi, Rs, Ts, ell):
    """Segment pairs (fixed segment, moving segment, pose) the scan's waves do not skip: |c_x - c_y'| - r_x - r_y <= sqrt(tau),
    in float64 without the kernel's rounding slack (1e-5 m: it moves the count by a handful of pairs in a million)."""
    p = ctx.params
    tau = -2.0 * ell * ell * np.log(np.float32(p.sp_thres) / (np.float32(p.sigma) * np.float32(p.sigma)))
    segs = []
    for which in (0, 1):
        d = ctx.device_cloud(which)
        segs.append(d["seg"][:(d["points"] + 63) // 64].astype(np.float64))
    sx, sy = segs
    reach = np.sqrt(tau) + sx[:, None, 3] + sy[None, :, 3]
    total = 0
    for R, T in zip(Rs.astype(np.float64), Ts.astype(np.float64)):
        cy = (sy[:, :3] - T) @ R   # R^T (c - T), row vectors
        dist = np.linalg.norm(sx[:, None, :3] - cy[None, :, :], axis=2)
        total += int(np.count_nonzero(dist <= reach))
    return total, len(sx), len(sy)


def kernel_times(path):
    """Median duration (us) of the k_pose_scan dispatches of a rocprofv3 kernel trace by (grid x, grid y)."""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_pose_scan" not in row.get("Kernel_Name", "") or "reduce" in row["Kernel_Name"]:
                continue
            key = (int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))
            by.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: (statistics.median(v), len(v)) for k, v in by.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="3000,10000,desk")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    ktimes = kernel_times(args.kernel_trace) if args.kernel_trace else {}
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pose_scan_bench: needs a GPU")
    pkg = ge.load_package()
    capi = pkg.capi
    stream = torch.cuda.current_stream().cuda_stream
    res = {"ell": ELL, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "timing": "host clock around synchronous calls, scan and score loop alternating; median [min, max] of reps",
           "rows": []}
    for case in args.cases.split(","):
        if case == "desk":
            desk = dict(np.load(os.path.join(ROOT, "tests", "golden", "desk_pcd_ds.npz")))
            xf, ff = desk["xyz0"], pkg.data.cvo_features(desk["rgb0"])
            xm, fm = desk["xyz1"], pkg.data.cvo_features(desk["rgb1"])
        else:
            n = int(case)
            xf, ff, xm, fm = pkg.data.synthetic_pair(n, n, seed=n % 97 + 3)
        c = capi.Context(mode=capi.MODE_CVO, device=0, stream=stream)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        for K in KS:
            Rs, Ts = poses(K)
            s = c.pose_scan(Rs, Ts, ELL)   # (warm-up; both norms cached from here on)
            if args.trace_run:
                for _ in range(3):
                    c.pose_scan_raw(Rs, Ts, ELL)
                continue
            row = {"case": case, "n_fixed": s.n_fixed, "n_moving": s.n_moving, "poses": K,
                   "members_per_pose_mean": float(np.mean(s.nnz)), "poses_with_members": int(np.count_nonzero(s.nnz))}
            score_loop = K == 256
            if score_loop:
                for k in range(K):
                    c.pose_score_raw(Rs[k], Ts[k], ELL)
            t_scan, t_loop = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                c.pose_scan_raw(Rs, Ts, ELL)
                t1 = time.perf_counter()
                if score_loop:
                    for k in range(K):
                        c.pose_score_raw(Rs[k], Ts[k], ELL)
                t2 = time.perf_counter()
                t_scan.append((t1 - t0) * 1e3)
                t_loop.append((t2 - t1) * 1e3)
            row["scan_ms"] = [statistics.median(t_scan), min(t_scan), max(t_scan)]
            row["scan_poses_per_s"] = K / (row["scan_ms"][0] * 1e-3)
            if score_loop:
                row["score_loop_ms"] = [statistics.median(t_loop), min(t_loop), max(t_loop)]
                row["score_loop_poses_per_s"] = K / (row["score_loop_ms"][0] * 1e-3)
                row["scan_over_score_loop"] = row["scan_ms"][0] / row["score_loop_ms"][0]
            pairs, na, nb = surviving_segment_pairs(c, capi, Rs, Ts, ELL)
            row["segments"] = [na, nb]
            row["surviving_segment_pairs"] = pairs
            row["surviving_fraction"] = pairs / float(na * nb * K)
            key = (((na + 3) // 4) * 256, K)
            if key in ktimes:
                row["k_pose_scan_us"] = ktimes[key][0]
                row["k_pose_scan_dispatches_traced"] = ktimes[key][1]
                row["pair_tests_per_s"] = pairs * 4096.0 / (ktimes[key][0] * 1e-6)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        c.close()
    if args.out and not args.trace_run:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
