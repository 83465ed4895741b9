#!/usr/bin/env python3
"""Cost and effect of the selector's depth mode (cvo_fe_set_select_mode): host-to-host time of a frame with the mode off
and on in one process, the duration of k_fe_select in both instances, and what the mode does to num_selected and
num_points at num_want 3000.

    python tools/fe_select_depth_bench.py [--out FILE] [--rounds 5] [--frames 100] [--label TEXT]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_select_depth_bench.py --merge A.json B.json ... [--default-frames FILE] [--bench-values FILE]
                                          --out profiles/fe_select_depth.json

Timed cases, one generator each, alternating per round in one process (host clock around synchronous calls; per case the
median over the rounds of the per-frame time and the smallest and largest round): a VGA depth frame whose depth image
has holes (seeded blobs over about 30 % of it), and a 1241 x 376 stereo frame at max_disp 64 and 128
(tools/fe_stereo_bench.py's pairs), each with the mode off and on.
Counted, at num_want 3000, mode off and on: num_selected and num_points of the VGA frame under the blob holes and under
DepthGate(0.8, 4.0, 0.05, 1) on its own depth image, and of the stereo pair at both max_disp.
--trace-run: 30 frames of the VGA case and of the stereo case at 64 in each mode and nothing else, for a rocprofv3
--kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of such a run: the durations of k_fe_select<false>
and k_fe_select<true> per case and pass (two launches per frame; the first half of an instance's dispatches belongs to
the VGA case).
--merge: no GPU; the --out files of several processes of one session become one file: `runs` lists every process,
`medians_min_max_runs` the smallest and largest median per case over them, `mode_ms_per_frame` what the mode costs host
to host; --default-frames: the merged output of tools/fe_stereo_bench.py run on this tree and on the parent commit's in
alternation (frames of contexts that never set the mode), folded in as it is; --bench-values: a JSON file of bench.py's
result lines on the two trees.  Nothing here is asserted, and nothing here measures trajectory accuracy: no real frames
are shipped."""
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
SETTINGS = dict(baseline=0.54, min_disp=1, p1=8, p2=32, uniqueness=10, lr_max=1)
GATE = (0.8, 4.0, 0.05, 1)
NUM_WANT = 3000
HOLE_SHARE = 0.30
TRACED = ("depth_vga", "stereo_d64")


def blob_holes(np, w, h, seed, share):
    """a (h, w) bool plane, True = hole: seeded squares of 3 to 9 pixels, 64 at a time until `share` of it is covered"""
    rng = np.random.default_rng(seed)
    hole = np.zeros((h, w), bool)
    while hole.mean() < share:
        for _ in range(64):
            s = int(rng.integers(3, 10))
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            hole[y:y + s, x:x + s] = True
    return hole


def select_times(path):
    """The k_fe_select dispatches of a --trace-run's kernel trace, by instance, in the order they started: per traced
    case the first launch of a frame (potential 3) and the second (which returns at once unless the frame re-selects)"""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_select" in name:
                inst = "k_fe_select<true>" if "<true>" in name or "ILb1" in name else "k_fe_select<false>"
                start, end = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                by.setdefault(inst, []).append((start, (end - start) / 1e3))
    out = {}
    for inst, v in sorted(by.items()):
        v.sort()
        if len(v) != len(TRACED) * B.TRACE_FRAMES * 2:
            raise SystemExit("fe_select_depth_bench: %d dispatches of %s in the trace, expected %d"
                             % (len(v), inst, len(TRACED) * B.TRACE_FRAMES * 2))
        half = len(v) // len(TRACED)
        for j, case in enumerate(TRACED):
            part = [d for _, d in v[j * half:(j + 1) * half]]
            out["%s:%s:first_pass" % (inst, case)] = B._stats(part[0::2])
            out["%s:%s:second_pass" % (inst, case)] = B._stats(part[1::2])
    return out


def merge(paths, out_path, default_frames, bench_values):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "stereo_image", "depth_image", "rounds", "frames_per_round", "timing", "settings",
                                "num_want", "hole_share", "gate") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = "unmeasured: what the mode is worth in trajectory accuracy needs real frames, and none are shipped"
    res["runs"] = [{"run": f.get("label", ""), "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["mode_ms_per_frame"] = {}
    for case in sorted({k.rsplit("_", 1)[0] for k in spread}):
        a, b = spread.get(case + "_off"), spread.get(case + "_on")
        if a and b:
            res["mode_ms_per_frame"][case] = {"on_minus_off_per_run": [y - x for x, y in zip(a, b)],
                                              "median": statistics.median(y - x for x, y in zip(a, b))}
    for f in files:
        if "counts" in f:
            res["counts"] = f["counts"]
        if "select_launches_us" in f:
            res["select_launches_from"] = f.get("label", "")
            res["select_launches_us"] = f["select_launches_us"]
    if default_frames:
        res["default_frames_this_and_parent"] = json.load(open(default_frames))
    if bench_values:
        res["bench_py"] = json.load(open(bench_values))
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    print(json.dumps(res["mode_ms_per_frame"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--default-frames", default=None)
    ap.add_argument("--bench-values", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--label", default="")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_select_depth_bench: --merge needs --out")
        merge(args.merge, args.out, args.default_frames, args.bench_values)
        return
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_select_depth_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    pairs = [B.pair(400 + k) for k in range(4)]
    depth_frames = []
    for k in range(8):
        bgr, dep = pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k))
        holed = np.where(blob_holes(np, 640, 480, 900 + k, HOLE_SHARE), 0, dep).astype(np.uint16)
        depth_frames.append((bgr, np.ascontiguousarray(dep), np.ascontiguousarray(holed)))
    modes = (("off", F.SELECT_IMAGE), ("on", F.SELECT_DEPTH))

    def make(case, mode, gate=None):
        gen = F.PcdGenerator(640, 480) if case == "depth_vga" else F.PcdGenerator(B.W, B.H)
        if case != "depth_vga":
            gen.set_stereo(F.Stereo(max_disp=int(case[len("stereo_d"):]), **SETTINGS))
        if gate:
            gen.set_depth_gate(F.DepthGate(*gate))
        gen.set_select_mode(mode)
        return gen

    def frame(gen, case, k, which=2):
        if case == "depth_vga":
            return gen.create_pointcloud(depth_frames[k % 8][0], depth_frames[k % 8][which], 1, F.FEATURES_HSV)
        return gen.create_pointcloud_stereo(pairs[k % 4][0], pairs[k % 4][1], 4, F.FEATURES_HSV)

    if args.trace_run:
        for case in TRACED:
            for name, mode in modes:
                gen = make(case, mode)
                for k in range(B.TRACE_FRAMES):
                    frame(gen, case, k)
                gen.close()
        return
    cases = ("depth_vga",) + tuple("stereo_d%d" % D for D in DISPS)
    gens = {"%s_%s" % (case, name): (make(case, mode), case) for case in cases for name, mode in modes}
    for gen, case in gens.values():   # warm-up: the graphs are captured here
        for k in range(12):
            frame(gen, case, k)
    per_round = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name, (gen, case) in gens.items():
            t0 = time.perf_counter()
            for k in range(args.frames):
                frame(gen, case, k)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    # the counts: one frame each (the first of its kind), num_want 3000
    counts = {}

    def count(label, gen, case, which=2):
        frame(gen, case, 0, which)
        info = gen.info()
        depth = gen.read_stage(F.STAGE_RECT_DEPTH)
        counts[label] = {"num_selected": info["num_selected"], "num_points": info["num_points"], "pot_used": info["pot_used"],
                         "reselected": info["reselected"], "canny_used": info["canny_used"],
                         "pixels_without_depth_share": float((depth == 0).mean())}

    for name, (gen, case) in gens.items():
        count(("vga_blob_holes_" if case == "depth_vga" else case + "_") + name.rsplit("_", 1)[1], gen, case)
    for name, mode in modes:
        gen = make("depth_vga", mode, GATE)
        count("vga_gate_" + name, gen, "depth_vga", which=1)
        gen.close()
    res = {"label": args.label, "device": torch.cuda.get_device_name(0), "stereo_image": [B.W, B.H], "depth_image": [640, 480],
           "rounds": args.rounds, "frames_per_round": args.frames, "settings": SETTINGS, "num_want": NUM_WANT,
           "hole_share": HOLE_SHARE, "gate": list(GATE),
           "timing": "host clock around create_pointcloud[_stereo] (synchronous), the six cases (a VGA depth frame with blob "
                     "holes, a stereo frame at max_disp 64 and 128; mode off and on) alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "counts": counts}
    if args.kernel_trace:
        res["select_launches_us"] = select_times(args.kernel_trace)
    for gen, _ in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
