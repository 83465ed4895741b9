#!/usr/bin/env python3
"""Cost of the depth gate in the front end: host-to-host time of one VGA frame (create_pointcloud: staging, upload,
every kernel, the cloud back on the host) without gate and mask, with the gate (0.8 m, 4 m, jump_rel 0.05) at grow 0
and at grow 3, with that gate and a mask, and with gate and mask under the TUM fr1 colour lens (k_fe_rectify in front,
the mask through its map) -- k_fe_depth_gate between the depth plane and level 0 in each gated case.

    python tools/fe_gate_bench.py [--out profiles/fe_depth_gate.json] [--rounds 9] [--frames 300] [--root DIR]
                                  [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>] [--label TEXT] [--tree NAME]
    python tools/fe_gate_bench.py --merge A.json B.json ... --out profiles/fe_depth_gate.json [--bench parent.json this.json ...]

One generator per case, the cases alternating in one process: a round times --frames frames of each case in turn (host
clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest
and largest round beside it.  The frames are synthetic (data.synthetic_rgbd_frame, texture 1.0), eight of them in turn,
each depth image with a near box, a far strip and a few dozen boxes of other depths, so that every rule of the gate has
pixels to drop.
--root: measure the package of another checkout of the project (e.g. the parent commit's, built) the same way; a package
without the gate runs the first case only.  --trace-run: 50 frames of each gated case in turn and nothing else, for a
rocprofv3 --kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of such a run, whose k_fe_* durations
(median, smallest, largest, count) are folded into the output, k_fe_depth_gate's per case as well (its dispatches in
the order they started, 50 per case).  --merge: no GPU; the --out files of several processes of one session, in the
order they ran (give each a --label; a --root other than the tool's own tree counts as tree "parent" unless --tree
names it), become one file: `runs` lists every process, `medians_min_max_runs` the smallest and largest median per tree
and case over them with the number of processes, `gate_cost_ms` what each case adds to `off` (difference of the medians,
per process), `off_this_minus_parent_ms` the difference of the two trees' `off` medians beside the parent's own spread
over its processes, the kernel trace of the last file that has one, and --bench adds `value` / `ms_per_step` of saved
bench.py result lines (the parent's and this tree's in turn, in the order they ran).  Nothing here is asserted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_FRAMES = 50
GATED = ("gate_grow0", "gate_grow3", "gate_grow3_mask", "gate_grow3_mask_fr1_lens")


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path):
    """Durations (us) of the dispatches of a rocprofv3 kernel trace, by kernel name, k_fe_* only; k_fe_depth_gate's
    also per case of a --trace-run."""
    by, gate = {}, []
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_" not in name:
                continue
            short = name[name.index("k_fe_"):].split("(")[0]
            start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
            by.setdefault(short, []).append((end - start) / 1e3)
            if short.split("<")[0] == "k_fe_depth_gate":   # (one instance per grow)
                gate.append((start, (end - start) / 1e3))
    out = {k: _stats(v) for k, v in sorted(by.items())}
    if len(gate) == TRACE_FRAMES * len(GATED):
        gate.sort()
        for k, case in enumerate(GATED):
            out["k_fe_depth_gate:" + case] = _stats([d for _, d in gate[k * TRACE_FRAMES:(k + 1) * TRACE_FRAMES]])
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "image", "rounds", "frames_per_round", "timing", "gate") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["runs"] = [{"run": f.get("label", ""), "tree": f.get("tree") or ("this" if f.get("root", ".") == "." else "parent"),
                    "ms_per_frame": f["ms_per_frame"]} for f in files]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["gate_cost_ms"] = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            if case != "off":
                res["gate_cost_ms"].setdefault(r["tree"], {}).setdefault(case, []).append(v[0] - r["ms_per_frame"]["off"][0])
    if "parent:off" in spread and "this:off" in spread:
        p, t = spread["parent:off"], spread["this:off"]
        res["off_this_minus_parent_ms"] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                           "parent_spread_max_minus_min": max(p) - min(p),
                                           "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        for k in ("points", "pixels", "kernel_bytes"):
            if k in f:
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    if bench:
        rows = [json.loads(open(p).read().strip().split("\n")[-1]) for p in bench]
        names = ["%s_%d" % (("parent", "this")[k % 2], k // 2 + 1) for k in range(len(rows))]
        res["bench_py"] = {name: {"value": r.get("value"), "ms_per_step": r.get("ms_per_step"), "unit": r.get("unit")}
                           for name, r in zip(names, rows)}
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def scene(pkg, k):
    """Frame k: the synthetic frame with steps and out-of-range surfaces in its depth image"""
    bgr, dep = pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k))
    dep = dep.astype(np.int64)
    h, w = dep.shape
    rng = np.random.Generator(np.random.PCG64(170 + k))
    for _ in range(40):
        bw, bh = rng.integers(8, 64, endpoint=True), rng.integers(8, 48, endpoint=True)
        x, y = rng.integers(0, w - bw, endpoint=True), rng.integers(0, h - bh, endpoint=True)
        hole = dep[y:y + bh, x:x + bw] == 0
        dep[y:y + bh, x:x + bw] = np.where(hole, 0, int(rng.integers(4500, 19000)))
    dep[0:h // 5, 0:w // 4][dep[0:h // 5, 0:w // 4] != 0] = 3500
    dep[h - h // 8:, w // 2:][dep[h - h // 8:, w // 2:] != 0] = 27500
    return bgr, np.ascontiguousarray(dep.astype(np.uint16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench", nargs="+", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_gate_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_gate_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    w, h = 640, 480
    frames = [scene(pkg, k) for k in range(8)]
    mask = np.zeros((h, w), np.uint8)
    mask[h // 2:h // 2 + 120, w // 8:w // 8 + 160] = 255
    gate = (0.8, 4.0, 0.05)
    cases = [("off", None, False, None)]
    if hasattr(F, "DepthGate"):
        cases += [(GATED[0], F.DepthGate(*gate, 0), False, None), (GATED[1], F.DepthGate(*gate, 3), False, None),
                  (GATED[2], F.DepthGate(*gate, 3), True, None), (GATED[3], F.DepthGate(*gate, 3), True, F.TUM_CAMERAS["fr1"])]
    gens = []
    for name, g, with_mask, cam in cases:
        gen = F.PcdGenerator(w, h)
        if cam is not None:
            gen.set_camera(cam)
        if g is not None:
            gen.set_depth_gate(g)
        if with_mask:
            gen.set_mask(mask)
        gens.append(gen)
    if args.trace_run:
        for gen in gens[1:]:
            for k in range(TRACE_FRAMES):
                gen.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
        for gen in gens:
            gen.close()
        return
    clouds = []
    for gen in gens:   # warm-up: the graph of each context is captured here
        for k in range(16):
            c = gen.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
        clouds.append(c)
    per_round = {c[0]: [] for c in cases}
    for _ in range(args.rounds):
        for (name, _, _, _), gen in zip(cases, gens):
            t0 = time.perf_counter()
            for k in range(args.frames):
                gen.create_pointcloud(frames[k % 8][0], frames[k % 8][1], 1, F.FEATURES_HSV)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "tree": args.tree, "root": os.path.relpath(root, ROOT), "device": torch.cuda.get_device_name(0),
           "image": [w, h], "rounds": args.rounds, "frames_per_round": args.frames, "gate": list(gate),
           "timing": "host clock around create_pointcloud (synchronous), cases alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {}}
    for c in cases:
        v = per_round[c[0]]
        res["ms_per_frame"][c[0]] = [statistics.median(v), min(v), max(v)]
    if len(cases) > 1:
        res["points"] = {c[0]: int(len(cl[0])) for c, cl in zip(cases, clouds)}
        res["pixels"] = {}
        for (name, _, _, _), gen in zip(cases[1:], gens[1:]):
            fl = gen.read_stage(F.STAGE_GATE)
            res["pixels"][name] = {"with_depth": int(np.count_nonzero(gen.read_stage(F.STAGE_UNGATED_DEPTH))),
                                   "masked": int(np.count_nonzero(fl & 1)), "out_of_range": int(np.count_nonzero(fl & 2)),
                                   "near_a_jump": int(np.count_nonzero(fl & 4)),
                                   "kept": int(np.count_nonzero(gen.read_stage(F.STAGE_RECT_DEPTH)))}
        # what k_fe_depth_gate moves per frame: the plane once (the halo re-reads of neighbouring tiles are served by
        # the caches), depth and flags out, the mask and under a lens the two planes of the map
        res["kernel_bytes"] = {"k_fe_depth_gate": {"depth_read": w * h * 2, "depth_written": w * h * 2, "flags_written": w * h,
                                                   "mask_read_if_set": w * h, "map_read_under_a_lens_with_a_mask": w * h * 8}}
    if args.kernel_trace:
        res["kernel_trace_us"] = kernel_times(args.kernel_trace)
    for gen in gens:
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
