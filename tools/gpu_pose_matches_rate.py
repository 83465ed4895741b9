#!/usr/bin/env python3
"""Cost of cvo_hip_pose_matches next to cvo_hip_pose_score, in one process on the same clouds.

    python tools/gpu_pose_matches_rate.py [--out profiles/pose_matches.json] [--quick] [--reps 30] [--cases 3000,10000,desk]
                                          [--stats-csv <rocprofv3 kernel_stats.csv>]

For synthetic cvo pairs of 3k and 10k points and the first pair of the shipped fr1/desk clouds, at R = I,
T = (0.02, -0.01, 0.015) and ell = 0.1: the median wall time of --reps synchronous calls of pose_matches with both
sides, one side and no arrays, in the wave-combined form (option matches_combine = 1, the default) and with plain atomics
(0), beside pose_score with warm norms.  --quick: both sides only, both forms (for rocprofv3 --kernel-trace --stats
runs; the two forms are two instantiations of k_pose_matches, so one trace holds both).  --stats-csv: the kernel
statistics of such a run, folded into the output as kernel_stats_us.  Nothing here is asserted."""
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


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def kernel_stats(path):
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if any(k in name for k in ("k_pose_matches", "k_pose_score", "k_process<0", "k_filter", "k_post_flow")):
                out[name] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                             "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="3000,10000,desk")
    ap.add_argument("--stats-csv", default=None)
    args = ap.parse_args()
    res = {"calls_median_ms": []}
    if args.stats_csv:
        res["kernel_stats_us"] = kernel_stats(args.stats_csv)
    import torch
    pkg = ge.load_package()
    capi = pkg.capi
    stream = torch.cuda.current_stream().cuda_stream
    R, T, ell = np.eye(3, dtype=np.float32), np.array([0.02, -0.01, 0.015], np.float32), 0.1
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
        m = c.pose_matches(R, T, ell)
        row = {"case": case, "n_fixed": m.n_fixed, "n_moving": m.n_moving, "nnz": m.nnz, "exact": bool(m.exact),
               "max_members_fixed": int(m.fixed.count.max()), "max_members_moving": int(m.moving.count.max())}
        for comb, tag in ((1, "combined"), (0, "plain")):
            c.set_option("matches_combine", comb)
            row["pose_matches_both_%s_ms" % tag] = median_ms(lambda: c.pose_matches(R, T, ell), args.reps)
            if not args.quick:
                row["pose_matches_fixed_only_%s_ms" % tag] = median_ms(lambda: c.pose_matches(R, T, ell, moving=False), args.reps)
                row["pose_matches_no_arrays_%s_ms" % tag] = median_ms(
                    lambda: c.pose_matches(R, T, ell, fixed=False, moving=False), args.reps)
        c.set_option("matches_combine", 1)
        c.pose_score(R, T, ell)   # (both norms cached from here on)
        row["pose_score_warm_ms"] = median_ms(lambda: c.pose_score(R, T, ell), args.reps)
        res["calls_median_ms"].append(row)
        print(json.dumps(row), flush=True)
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
