#!/usr/bin/env python3
"""Cost of cvo_hip_pose_score next to the passes it resembles, at the converged pose of a registration.

    python tools/gpu_pose_score_rate.py [--out profiles/pose_score.json] [--quick] [--reps 30] [--sizes 3000,10000]

For synthetic cvo and acvo pairs of 3k and 10k points it aligns once, then times cvo_hip_pose_score called alone at the
final (R, T) and params' ell_init with a cold cache (cvo_hip_set_params with the same parameters before every call, not
timed: both self passes run) and a warm one (both norms cached), next to cvo_hip_flow and cvo_hip_pose_hessian at the
same pose and ell (median wall time of --reps synchronous calls).  Then cvo_hip_pose_score_many over 64 contexts of
10k-point pairs against 64 lone calls, cold and warm, and the per-frame cost of run_sequence(score=True) against
run_sequence() over the five shipped fr1/desk clouds.  --quick: the single calls only (for rocprofv3 --kernel-trace
--stats runs).  Nothing here is asserted."""
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


def median_ms(fn, reps, before=None):
    if before:
        before()
    fn()
    ts = []
    for _ in range(reps):
        if before:
            before()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sizes", default="3000,10000")
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    import torch
    pkg = ge.load_package()
    capi = pkg.capi
    stream = torch.cuda.current_stream().cuda_stream
    res = {"calls_median_ms": [], "many_ms": None, "desk_sequence_frame_ms": []}
    for n in [int(t) for t in args.sizes.split(",")]:
        for mode_name, mode in (("cvo", capi.MODE_CVO), ("acvo", capi.MODE_ACVO)):
            xf, ff, xm, fm = pkg.data.synthetic_pair(n, n, seed=pkg.data.SEED_CFG2, acvo=mode == capi.MODE_ACVO)
            c = capi.Context(mode=mode, device=0, stream=stream)
            c.set_fixed(xf, ff)
            c.set_moving(xm, fm)
            st = capi.init_state(c.params)
            iters, _ = c.align(st, trace_cap=0)
            R, T = np.array(st.R, np.float32), np.array(st.T, np.float32)
            ell = float(c.params.ell_init)
            s = c.pose_score(R, T, ell)
            row = {"n": n, "mode": mode_name, "iterations": iters, "ell": ell, "nnz": s.nnz, "nnz_fixed": s.nnz_fixed,
                   "nnz_moving": s.nnz_moving, "cos_angle": s.cos_angle,
                   "pose_score_cold_ms": median_ms(lambda: c.pose_score(R, T, ell), args.reps,
                                                   before=lambda: c.set_params(c.params)),
                   "pose_score_warm_ms": median_ms(lambda: c.pose_score(R, T, ell), args.reps),
                   "pose_hessian_ms": median_ms(lambda: c.pose_hessian(R, T, ell), args.reps)}
            c.transform_pcd(R, T)
            row["flow_ms"] = median_ms(lambda: c.flow(ell), args.reps)
            res["calls_median_ms"].append(row)
            print(json.dumps(row), flush=True)
            c.close()
    if not args.quick:
        nb = args.batch
        ctxs, Rs, Ts = [], [], []
        for k in range(nb):
            xf, ff, xm, fm = pkg.data.synthetic_pair(10000, 10000, seed=1000 + k)
            c = capi.Context(mode=capi.MODE_CVO, device=0, stream=stream)
            c.set_fixed(xf, ff)
            c.set_moving(xm, fm)
            ctxs.append(c)
            Rs.append(np.eye(3, dtype=np.float32))
            Ts.append(np.zeros(3, np.float32))
        ells = [float(ctxs[0].params.ell_init)] * nb

        def cold():
            for c in ctxs:
                c.set_params(c.params)

        def lone():
            for c, R, T, e in zip(ctxs, Rs, Ts, ells):
                c.pose_score(R, T, e)

        reps = max(5, args.reps // 3)
        res["many_ms"] = {"contexts": nb, "n": 10000,
                          "many_cold": median_ms(lambda: capi.pose_score_many(ctxs, Rs, Ts, ells), reps, before=cold),
                          "lone_cold": median_ms(lone, reps, before=cold),
                          "many_warm": median_ms(lambda: capi.pose_score_many(ctxs, Rs, Ts, ells), reps),
                          "lone_warm": median_ms(lone, reps)}
        print(json.dumps(res["many_ms"]), flush=True)
        for c in ctxs:
            c.close()
        desk = dict(np.load(os.path.join(ROOT, "tests", "golden", "desk_pcd_ds.npz")))
        for name, Reg, feats in (("cvo", pkg.Cvo, pkg.data.cvo_features), ("acvo", pkg.Acvo, pkg.data.acvo_features)):
            frames = [(str(k), desk["xyz%d" % k], feats(desk["rgb%d" % k])) for k in range(5)]
            per = {}
            cos = None
            for score in (False, True, False, True):
                reg = Reg(device=0, stream=stream)
                reg.run_cvo(frames[0][1], frames[0][2])
                ts = []
                for k in range(1, 5):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    reg.run_cvo(frames[k][1], frames[k][2], score=score)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t) * 1e3)
                    if score:
                        cos = (cos or []) + [reg.score.cos_angle]
                reg.close()
                per[score] = ts   # (the second pass of each kind: warm)
            row = {"mode": name, "frame_ms_plain": per[False], "frame_ms_score": per[True],
                   "mean_extra_ms": float(np.mean(per[True]) - np.mean(per[False])), "cos_angle": cos[-4:]}
            res["desk_sequence_frame_ms"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
