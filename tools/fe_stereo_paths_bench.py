#!/usr/bin/env python3
"""Cost of the stereo matcher's paths (cvo_fe_set_stereo_paths): host-to-host time of one 1241 x 376 stereo frame
(create_pointcloud_stereo) under the default mask 0x0F and under 0xFF, at max_disp 64 and 128, and the duration of every
path launch of a frame under 0xFF -- the four diagonal launches beside the two vertical ones, which have the same waves,
the same steps and the same bytes of S.

    python tools/fe_stereo_paths_bench.py [--out FILE] [--rounds 7] [--frames 100] [--label TEXT]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_stereo_paths_bench.py --merge A.json B.json ... [--default-frames fe_stereo.json] [--bench-values FILE]
                                          --out profiles/fe_stereo_paths.json

One generator per (max_disp, mask), the four alternating in one process: a round times --frames frames of each in turn
(host clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the
smallest and largest round beside it.  The pairs are tools/fe_stereo_bench.py's.  --trace-run: 30 frames under 0xFF at
each max_disp and nothing else, for a rocprofv3 --kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of
such a run: the k_fe_sgm_path dispatches in the order they started are eight per frame, one per bit, and their durations
(median, smallest, largest) are recorded per max_disp and bit, with the ratio of every diagonal launch's median to the
slower vertical launch's.  --merge: no GPU; the --out files of several processes of one session become one file: `runs`
lists every process, `medians_min_max_runs` the smallest and largest median per case over them, `ms_per_path` what
the four additional launches cost per frame and path; --default-frames: the merged output of tools/fe_stereo_bench.py
run on this tree and on the parent commit's in alternation (frames of contexts that never set a mask, and plain VGA
depth frames), folded in as it is; --bench-values: a JSON file of bench.py's result lines on the two trees.  Nothing
here is asserted, and nothing here measures accuracy: what the diagonals are worth on real pairs is unmeasured."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_stereo_bench as B   # noqa: E402  (the pairs, the settings' image size, the statistics of a trace)

DISPS = (64, 128)
MASKS = (("paths4", 0x0F), ("paths8", 0xFF))
BITS = ("0 left to right", "1 right to left", "2 top to bottom", "3 bottom to top", "4 (+1,+1)", "5 (-1,-1)", "6 (-1,+1)",
        "7 (+1,-1)")
SETTINGS = dict(baseline=0.54, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1)


def path_times(path):
    """The k_fe_sgm_path dispatches of a --trace-run's kernel trace in the order they started: eight per frame, the
    first half of them at the first max_disp.  Per max_disp and bit the durations in us."""
    v = []
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_fe_sgm_path" in row.get("Kernel_Name", ""):
                start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                v.append((start, (end - start) / 1e3))
    v.sort()
    if len(v) != len(DISPS) * B.TRACE_FRAMES * 8:
        raise SystemExit("fe_stereo_paths_bench: %d path dispatches in the trace, expected %d" % (len(v), len(DISPS) * B.TRACE_FRAMES * 8))
    out = {}
    half = len(v) // len(DISPS)
    for k, D in enumerate(DISPS):
        part = [d for _, d in v[k * half:(k + 1) * half]]
        per_bit = {BITS[b]: B._stats(part[b::8]) for b in range(8)}
        slower_vertical = max(per_bit[BITS[2]]["median_us"], per_bit[BITS[3]]["median_us"])
        for b in range(4, 8):
            per_bit[BITS[b]]["median_over_slower_vertical_median"] = per_bit[BITS[b]]["median_us"] / slower_vertical
        out["d%d" % D] = per_bit
    return out


def merge(paths, out_path, default_frames, bench_values):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "stereo_image", "rounds", "frames_per_round", "timing", "settings") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: no real pairs are shipped, and on the synthetic pairs eight paths are neither more nor less accurate than four"
    res["runs"] = [{"run": f.get("label", ""), "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["ms_per_path"] = {}
    for D in DISPS:
        a, b = spread.get("d%d_paths4" % D), spread.get("d%d_paths8" % D)
        if a and b:
            res["ms_per_path"]["d%d" % D] = {"four_more_paths_ms": statistics.median(b) - statistics.median(a),
                                             "per_additional_path_ms": (statistics.median(b) - statistics.median(a)) / 4.0}
    for f in files:
        for k in ("points", "pixels_kept"):
            if k in f:
                res[k] = f[k]
        if "path_launches_us" in f:
            res["path_launches_from"] = f.get("label", "")
            res["path_launches_us"] = f["path_launches_us"]
    if default_frames:
        res["default_frames_this_and_parent"] = json.load(open(default_frames))
    if bench_values:
        res["bench_py"] = json.load(open(bench_values))
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    print(json.dumps(res["ms_per_path"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--default-frames", default=None)
    ap.add_argument("--bench-values", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--label", default="")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_stereo_paths_bench: --merge needs --out")
        merge(args.merge, args.out, args.default_frames, args.bench_values)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_stereo_paths_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    pairs = [B.pair(400 + k) for k in range(4)]
    gens = {}
    for D in DISPS:
        for name, mask in MASKS:
            if args.trace_run and mask != F.PATHS_8:
                continue
            gen = F.PcdGenerator(B.W, B.H)
            gen.set_stereo(F.Stereo(max_disp=D, **SETTINGS))
            gen.set_stereo_paths(mask)
            gens["d%d_%s" % (D, name)] = gen

    def frame(name, k):
        return gens[name].create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)

    if args.trace_run:
        for name in gens:
            for k in range(B.TRACE_FRAMES):
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
    res = {"label": args.label, "device": torch.cuda.get_device_name(0), "stereo_image": [B.W, B.H], "rounds": args.rounds,
           "frames_per_round": args.frames, "settings": SETTINGS,
           "timing": "host clock around create_pointcloud_stereo (synchronous), the four cases (max_disp 64 and 128, masks 0x0F "
                     "and 0xFF) alternating per round in one process; ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "points": {name: int(len(c[0])) for name, c in clouds.items()},
           "pixels_kept": {name: int(np.count_nonzero(gens[name].read_stage(F.STAGE_STEREO) == 0)) for name in gens}}
    if args.kernel_trace:
        res["path_launches_us"] = path_times(args.kernel_trace)
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
