#!/usr/bin/env python3
"""Cost of cvo_hip_pose_hessian next to the passes it resembles, at the converged pose of a registration.

    python tools/gpu_pose_hessian_rate.py [--out profiles/pose_hessian.json] [--quick] [--reps 30] [--sizes 10000]

For synthetic cvo pairs of 3k, 10k and 200k points (--quick: 10k and 200k, no desk sequence) it aligns once, then times each of
cvo_hip_pose_hessian, cvo_hip_step_coeffs and cvo_hip_flow called alone at the final (R, T, ell) (median wall time of
--reps synchronous calls).  Then the per-frame cost of align(hessian=True) against align() over the five shipped
fr1/desk clouds (cvo and acvo), and the eigenvalues of -H at the converged poses (reported, not asserted).
Per-kernel durations come from rocprofv3 --kernel-trace --stats runs of --quick --sizes N."""
import argparse
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


def eig_neg_h(h):
    return [float(e) for e in np.linalg.eigvalsh(-h.H)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default=None, help="comma-separated pair sizes (default 3000,10000,200000; --quick 10000,200000)")
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi = pkg.capi
    res = {"calls": [], "desk_sequence": [], "eig_neg_H": {}}
    sizes = [10000, 200000] if args.quick else [3000, 10000, 200000]
    if args.sizes:
        sizes = [int(t) for t in args.sizes.split(",")]
    for n in sizes:
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, n, seed=pkg.data.SEED_CFG2)
        c = capi.Context(mode=capi.MODE_CVO, device=0, stream=torch.cuda.current_stream().cuda_stream)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        st = capi.init_state(c.params)
        iters, _ = c.align(st, trace_cap=0)
        R, T, ell = np.array(st.R, np.float32), np.array(st.T, np.float32), st.ell
        h = c.pose_hessian(R, T, ell)
        c.transform_pcd(R, T)
        fl = c.flow(ell)
        om, v = fl[0:3].astype(np.float32), fl[3:6].astype(np.float32)
        row = {"n": n, "iterations": iters, "ell": float(ell), "nnz": h.nnz,
               "pose_hessian_ms": median_ms(lambda: c.pose_hessian(R, T, ell), args.reps),
               "step_coeffs_ms": median_ms(lambda: c.step_coeffs(om, v, ell), args.reps),
               "flow_ms": median_ms(lambda: c.flow(ell), args.reps)}
        res["calls"].append(row)
        res["eig_neg_H"]["synthetic_%d" % n] = eig_neg_h(h)
        print(json.dumps(row), flush=True)
        c.close()
    if not args.quick:
        desk = dict(np.load(os.path.join(ROOT, "tests", "golden", "desk_pcd_ds.npz")))
        for name, Reg, feats in (("cvo", pkg.Cvo, pkg.data.cvo_features), ("acvo", pkg.Acvo, pkg.data.acvo_features)):
            frames = [(str(k), desk["xyz%d" % k], feats(desk["rgb%d" % k])) for k in range(5)]
            per = {}
            for hessian in (False, True, False, True):
                reg = Reg(device=0, stream=torch.cuda.current_stream().cuda_stream)
                reg.run_cvo(frames[0][1], frames[0][2])
                ts = []
                for k in range(1, 5):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    reg.run_cvo(frames[k][1], frames[k][2], hessian=hessian)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t) * 1e3)
                    if hessian:
                        res["eig_neg_H"]["desk_%s_%d_%d" % (name, k - 1, k)] = eig_neg_h(reg.hessian)
                reg.close()
                per[hessian] = ts   # (the second pass of each kind: warm)
            row = {"mode": name, "frame_ms_plain": per[False], "frame_ms_hessian": per[True],
                   "mean_extra_ms": float(np.mean(per[True]) - np.mean(per[False]))}
            res["desk_sequence"].append(row)
            print(json.dumps(row), flush=True)
    for k, e in res["eig_neg_H"].items():
        print("eig(-H) %s: %s  positive definite: %s" % (k, " ".join("%.4g" % x for x in e), all(x > 0 for x in e)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
