#!/usr/bin/env python3
"""Cost of input binning of the front end (cvo_fe_set_input_binning): the duration of k_fe_bin<F> at three sizes beside
k_fe_unpack and k_fe_depth_convert<F32> on planes of the same byte count in one trace; host-to-host time of a binned
frame beside a frame of a context at the input size (what the stage saves) and a frame of the working size (what the
larger upload costs), for depth frames and for a stereo pair at max_disp 128, and of a binned frame from device memory;
and frames without binning, for this library against the parent commit's.

    python tools/fe_binning_bench.py [--out FILE] [--rounds 5] [--frames 60] [--root DIR] [--label TEXT] [--off-only]
                                     [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_binning_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_binning.json

The pictures are the synthetic frames of the package; a stereo pair is a picture and the same picture sixteen columns to
the side.  One generator per case, all alternating in one process: a round times --frames frames of each in turn (host
clock around submit + collect, which is synchronous); recorded per case are the median over the rounds of the per-frame
time and the smallest and largest round beside it.  --root: the package of another checkout of the project (the parent
commit's, built), which runs the frames without binning only; such a process counts as tree "parent".  --off-only: this
tree the same way, one generator and nothing else in the process, which is the process the parent's is compared with.
--trace-run: per size 20 runs each of cvo_fe_bin_image, cvo_fe_bin_depth, cvo_fe_unpack_image (RGB8, the colour input's
bytes) and cvo_fe_convert_depth (F32, a plane of the colour input's bytes), then 10 conversions of a 4096 x 4096 float32
plane, and nothing else, for a rocprofv3 --kernel-trace run of its own (no counters); --kernel-trace: the
kernel_trace.csv of such a run.  --merge: no GPU; the --out files of several processes of one session, in the order they
ran, become one file; --bench: result lines of bench.py, "<tree>=<the JSON line>" each, in the order they ran.
Nothing here is asserted, and nothing here measures what binning is worth in accuracy on real recordings: none is shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((640, 360, 2), (640, 360, 3), (960, 540, 4))   # working width, height, factor: 1280x720, 1920x1080, 3840x2160 in
BIG = 4096
RUNS = 20
HBM_PEAK_TB_S = 8.0   # MI355X, the vendor's figure
# from hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (profiles/fe_binning_isa_resources.txt)
RESOURCES = {"k_fe_bin<2>": {"vgprs": 34, "sgprs": 30, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 8},
             "k_fe_bin<3>": {"vgprs": 46, "sgprs": 30, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 8},
             "k_fe_bin<4>": {"vgprs": 65, "sgprs": 30, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 7}}


def _stats(v, moved):
    med = statistics.median(v)
    return {"median_us": med, "min_us": min(v), "max_us": max(v), "dispatches": len(v), "bytes_moved": moved,
            "tb_per_s_at_the_median": moved / (med * 1e-6) / 1e12}


def kernel_times(path):
    """The durations of a --trace-run's kernels, in its order: per size RUNS of k_fe_bin (colour), RUNS of k_fe_bin
    (depth), RUNS of k_fe_unpack, RUNS of k_fe_depth_convert; then the 4096 x 4096 conversions"""
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    seq = {"k_fe_bin": [], "k_fe_unpack": [], "k_fe_depth_convert": []}
    for row in rows:
        name = row.get("Kernel_Name", "")
        for key in seq:
            if key in name:
                seq[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for k, (w, h, f) in enumerate(SIZES):
        fw, fh = f * w, f * h
        tag = "%dx%d -> %dx%d" % (fw, fh, w, h)
        bins = seq["k_fe_bin"][2 * RUNS * k:2 * RUNS * (k + 1)]
        if len(bins) == 2 * RUNS:
            out["k_fe_bin<%d> colour %s" % (f, tag)] = _stats(bins[:RUNS], fw * fh * 3 + w * h * 3)
            out["k_fe_bin<%d> depth %s" % (f, tag)] = _stats(bins[RUNS:], fw * fh * 2 + w * h * 2)
        un = seq["k_fe_unpack"][RUNS * k:RUNS * (k + 1)]
        if len(un) == RUNS:
            out["k_fe_unpack<RGB8> %dx%d" % (fw, fh)] = _stats(un, fw * fh * 6)
        cv = seq["k_fe_depth_convert"][RUNS * k:RUNS * (k + 1)]
        if len(cv) == RUNS:
            out["k_fe_depth_convert<F32> %dx%d" % (fw * 3 // 4, fh)] = _stats(cv, (fw * 3 // 4) * fh * 6)
    big = seq["k_fe_depth_convert"][RUNS * len(SIZES):]
    if big:
        out["k_fe_depth_convert<F32> 4096x4096"] = _stats(big, BIG * BIG * 6)
        ref = out["k_fe_depth_convert<F32> 4096x4096"]["tb_per_s_at_the_median"]
        out["fraction_of_hbm_peak_of_the_4096_conversion"] = ref / HBM_PEAK_TB_S
        for key in [k for k in out if k.startswith("k_fe_bin")]:
            out[key]["bytes_per_second_over_the_4096_conversion"] = out[key]["tb_per_s_at_the_median"] / ref
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "rounds", "frames_per_round", "timing", "pictures") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = ("unmeasured: what binning is worth in accuracy on real recordings needs frames in a sensor's own "
                       "resolution, and none are shipped")
    res["kernel"] = dict(RESOURCES, **{"from": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"})
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = set(r["ms_per_frame"]) == {"depth_vga_off"}
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["binned_minus_other_within_a_process_ms"] = [f["binned_minus_other_ms"] for f in files if "binned_minus_other_ms" in f]
    p, t = spread.get("parent:depth_vga_off_alone"), spread.get("this:depth_vga_off_alone")
    if p and t:
        res["default_this_minus_parent_ms"] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                               "parent_spread_max_minus_min": max(p) - min(p),
                                               "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    args = ap.parse_args()
    if args.merge:
        if not args.out:
            raise SystemExit("fe_binning_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    if args.kernel_trace and not args.trace_run:   # (a trace alone: no GPU)
        res = {"label": args.label, "tree": "this", "kernel_trace_us": kernel_times(args.kernel_trace)}
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_binning_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_binning = hasattr(F.PcdGenerator, "set_input_binning") and not args.off_only
    rng = np.random.default_rng(1)
    if args.trace_run:
        for w, h, f in SIZES:
            fw, fh = f * w, f * h
            img = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
            dep = rng.integers(0, 65536, (fh, fw), dtype=np.uint16)
            fl = rng.uniform(0.1, 12.0, (fh, fw * 3 // 4)).astype(np.float32)
            b = F.Binning(f, 1)
            for _ in range(RUNS):
                F.bin_image(img, f)
            for _ in range(RUNS):
                F.bin_depth(dep, b)
            for _ in range(RUNS):
                F.unpack_image(img.reshape(fh, fw * 3), F.PIXEL_RGB8, fw, fh)
            for _ in range(RUNS):
                F.convert_depth(fl, F.DEPTH_F32, fw * 3 // 4, fh, 1.0, 5000.0)
        big = rng.uniform(0.1, 12.0, (BIG, BIG)).astype(np.float32)
        for _ in range(10):
            F.convert_depth(big, F.DEPTH_F32, BIG, BIG, 1.0, 5000.0)
        return
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(4)]
    gens, frames, calls = {}, {}, {}

    def case(name, w, h, images, stereo=False, binning=None, device=False):
        g = F.PcdGenerator(w, h)
        if stereo:
            g.set_stereo(F.Stereo(0.54, 128))
        if binning is not None:
            g.set_input_binning(binning)
        gens[name] = g
        frames[name] = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in fr) for fr in images] if device else images
        calls[name] = ((g.submit_stereo_device if device else g.submit_stereo) if stereo else (g.submit_device if device else g.submit),
                       4 if stereo else 1)

    def frame(name, k):
        submit, seq = calls[name]
        a, b = frames[name][k % len(frames[name])]
        submit(a, b, seq, F.FEATURES_HSV)
        return gens[name].collect()

    case("depth_vga_off", 640, 480, vga)
    if has_binning:
        w, h, f = 640, 360, 2
        full = [pkg.data.synthetic_rgbd_frame(width=f * w, height=f * h, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(4)]
        small = [pkg.data.synthetic_rgbd_frame(width=w, height=h, seed=70 + k, texture=1.0, motion=(0.6 * k, 0.3 * k)) for k in range(4)]
        pairs = [(np.ascontiguousarray(img), np.ascontiguousarray(np.roll(img, -16, axis=1))) for img, _ in full]
        spairs = [(np.ascontiguousarray(img), np.ascontiguousarray(np.roll(img, -8, axis=1))) for img, _ in small]
        b = F.Binning(f, 2)
        case("depth_1280x720_binned_to_640x360", w, h, full, binning=b)
        case("depth_1280x720_at_the_input_size", f * w, f * h, full)
        case("depth_640x360_at_the_working_size", w, h, small)
        case("depth_1280x720_binned_from_the_device", w, h, full, binning=b, device=True)
        case("stereo_1280x720_binned_to_640x360", w, h, pairs, stereo=True, binning=b)
        case("stereo_1280x720_at_the_input_size", f * w, f * h, pairs, stereo=True)
        case("stereo_640x360_at_the_working_size", w, h, spairs, stereo=True)
    torch.cuda.synchronize()
    for name in gens:   # warm-up: the graphs are captured here
        for k in range(8):
            frame(name, k)
    per_round = {name: [] for name in gens}
    for _ in range(args.rounds):
        for name in gens:
            n = max(4, args.frames // 6) if "stereo_1280x720_at" in name else args.frames   # (tens of ms a frame)
            t0 = time.perf_counter()
            for k in range(n):
                frame(name, k)
            per_round[name].append((time.perf_counter() - t0) / n * 1e3)
    res = {"label": args.label, "tree": "this" if root == ROOT else "parent", "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "frames_per_round": args.frames,
           "pictures": "synthetic frames of the package; depth_vga_off: 640 x 480 without binning; the others: 1280 x 720 images "
                       "binned by 2 with depth_min 2, the same images in a context of 1280 x 720, and images of 640 x 360 in a "
                       "context of that size; stereo: Stereo(0.54, 128), a picture and itself 16 (8) columns to the side; "
                       "from_the_device: torch tensors made before the clock starts",
           "timing": "host clock around submit* + collect (synchronous), the cases alternating per round in one process; ms per "
                     "frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()}}
    if has_binning:
        diff = {}
        for kind in ("depth", "stereo"):
            a = "%s_1280x720_binned_to_640x360" % kind
            for other in ("%s_1280x720_at_the_input_size" % kind, "%s_640x360_at_the_working_size" % kind):
                d = [x - y for x, y in zip(per_round[a], per_round[other])]
                diff[a + " - " + other] = {"median_of_the_rounds": statistics.median(d), "min": min(d), "max": max(d)}
        d = [x - y for x, y in zip(per_round["depth_1280x720_binned_from_the_device"], per_round["depth_1280x720_binned_to_640x360"])]
        diff["depth binned from the device - from the host"] = {"median_of_the_rounds": statistics.median(d), "min": min(d), "max": max(d)}
        res["binned_minus_other_ms"] = diff
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
