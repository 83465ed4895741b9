#!/usr/bin/env python3
"""Cost of the stereo matcher's speckle filter (cvo_fe_set_stereo_speckle): host-to-host time of one 1241 x 376 stereo
frame (create_pointcloud_stereo) without the filter and with it, at max_disp 64 and 128, and the duration of the filter's
launches (k_fe_speckle_tiles, _seams, _count, _apply) beside the matcher's winner launch and its path launches.

    python tools/fe_stereo_speckle_bench.py [--out FILE] [--rounds 7] [--frames 100] [--label TEXT]
                                            [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_stereo_speckle_bench.py --merge A.json B.json ... [--default-frames FILE] [--bench-values FILE]
                                            --out profiles/fe_stereo_speckle.json

One generator per (max_disp, filter off / on), the four alternating in one process: a round times --frames frames of each
in turn (host clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and
the smallest and largest round beside it.  The pairs are tools/fe_stereo_bench.py's; the filter's settings are SPECKLE.
--trace-run: 30 frames with the filter at each max_disp and nothing else, for a rocprofv3 --kernel-trace run of its own;
--kernel-trace: the kernel_trace.csv of such a run: per max_disp the durations (median, smallest, largest) of each of the
filter's kernels, their sum per frame, and those of k_fe_sgm_winner and of the fastest k_fe_sgm_path launch as yardsticks.
--merge: no GPU; the --out files of several processes of one session become one file: `runs` lists every process,
`medians_min_max_runs` the smallest and largest median per case over them, `filter_ms_per_frame` what the filter costs
host to host; --default-frames: the merged output of tools/fe_stereo_bench.py run on this tree and on the parent commit's
in alternation (frames of contexts that never set a filter, and plain VGA depth frames), folded in as it is;
--bench-values: a JSON file of bench.py's result lines on the two trees.  Nothing here is asserted, and nothing here
measures accuracy: the synthetic pairs hold few speckles."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fe_stereo_bench as B   # noqa: E402  (the pairs, the image size, the statistics of a trace)

DISPS = (64, 128)
CASES = (("plain", None), ("speckle", (100, 16)))
SPECKLE = dict(max_size=100, max_diff=16)
SETTINGS = dict(baseline=0.54, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1)
KERNELS = ("k_fe_speckle_tiles", "k_fe_speckle_seams", "k_fe_speckle_count", "k_fe_speckle_apply")


def filter_times(path):
    """The dispatches of a --trace-run's kernel trace in the order they started, the first half of every kernel's at the
    first max_disp: per max_disp the filter's kernels, their sum, the winner launch and the path launches (four per frame)"""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            for k in KERNELS + ("k_fe_sgm_winner", "k_fe_sgm_path"):
                if k in name:
                    start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                    by.setdefault(k, []).append((start, (end - start) / 1e3))
    out = {}
    for k, v in by.items():
        v.sort()
        per_frame = 4 if k == "k_fe_sgm_path" else 1
        if len(v) != len(DISPS) * B.TRACE_FRAMES * per_frame:
            raise SystemExit("fe_stereo_speckle_bench: %d dispatches of %s in the trace, expected %d"
                             % (len(v), k, len(DISPS) * B.TRACE_FRAMES * per_frame))
        half = len(v) // len(DISPS)
        for j, D in enumerate(DISPS):
            part = [d for _, d in v[j * half:(j + 1) * half]]
            o = out.setdefault("d%d" % D, {})
            if k == "k_fe_sgm_path":
                o["k_fe_sgm_path, the fastest of the four launches"] = min((B._stats(part[b::4]) for b in range(4)),
                                                                            key=lambda s: s["median_us"])
            else:
                o[k] = B._stats(part)
    for o in out.values():
        o["filter_sum_of_medians_us"] = sum(o[k]["median_us"] for k in KERNELS if k in o)
    return out


def merge(paths, out_path, default_frames, bench_values):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "stereo_image", "rounds", "frames_per_round", "timing", "settings", "speckle") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: no real pairs are shipped, and the synthetic pairs hold few speckles"
    res["runs"] = [{"run": f.get("label", ""), "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["filter_ms_per_frame"] = {}
    for D in DISPS:
        a, b = spread.get("d%d_plain" % D), spread.get("d%d_speckle" % D)
        if a and b:
            res["filter_ms_per_frame"]["d%d" % D] = statistics.median(b) - statistics.median(a)
    for f in files:
        for k in ("points", "pixels_kept", "pixels_removed"):
            if k in f:
                res[k] = f[k]
        if "filter_launches_us" in f:
            res["filter_launches_from"] = f.get("label", "")
            res["filter_launches_us"] = f["filter_launches_us"]
    if default_frames:
        res["default_frames_this_and_parent"] = json.load(open(default_frames))
    if bench_values:
        res["bench_py"] = json.load(open(bench_values))
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    print(json.dumps(res["filter_ms_per_frame"]), flush=True)
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
            raise SystemExit("fe_stereo_speckle_bench: --merge needs --out")
        merge(args.merge, args.out, args.default_frames, args.bench_values)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_stereo_speckle_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    pairs = [B.pair(400 + k) for k in range(4)]
    gens = {}
    for D in DISPS:
        for name, on in CASES:
            if args.trace_run and not on:
                continue
            gen = F.PcdGenerator(B.W, B.H)
            gen.set_stereo(F.Stereo(max_disp=D, **SETTINGS))
            if on:
                gen.set_stereo_speckle(F.Speckle(**SPECKLE))
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
    flags = {name: gens[name].read_stage(F.STAGE_STEREO) for name in gens}
    res = {"label": args.label, "device": torch.cuda.get_device_name(0), "stereo_image": [B.W, B.H], "rounds": args.rounds,
           "frames_per_round": args.frames, "settings": SETTINGS, "speckle": SPECKLE,
           "timing": "host clock around create_pointcloud_stereo (synchronous), the four cases (max_disp 64 and 128, without and "
                     "with the filter) alternating per round in one process; ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "points": {name: int(len(c[0])) for name, c in clouds.items()},
           "pixels_kept": {name: int(np.count_nonzero(f == 0)) for name, f in flags.items()},
           "pixels_removed": {name: int(np.count_nonzero(f & F.STEREO_SPECKLE)) for name, f in flags.items()}}
    if args.kernel_trace:
        res["filter_launches_us"] = filter_times(args.kernel_trace)
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
