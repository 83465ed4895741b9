#!/usr/bin/env python3
"""Cost of device input and of the float depth formats of the front end (cvo_fe_submit_device, cvo_fe_set_depth_format):
host-to-host time of one VGA depth frame and of one 1241 x 376 stereo frame handed over in device memory, beside the same
frames handed over from the host in the same process; and the duration of k_fe_depth_convert<F32> on a VGA plane beside
k_fe_rectify in one trace, and on a 4096 x 4096 plane against the HBM peak.

    python tools/fe_device_input_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_device_input_bench.py --merge A.json B.json ... [--bench LINE ...] [--second C.json ...]
                                          --out profiles/fe_device_input.json

The pictures are the synthetic frames of the package; a stereo pair is a picture and the same picture eight columns to
the side.  The device images are torch tensors made once, before the clock starts (a decoder's surfaces, a network's
output): a device frame's time holds no upload.
One generator per case, all alternating in one process: a round times --frames frames of each in turn (host clock around
submit + collect, which is synchronous); recorded per case are the median over the rounds of the per-frame time and the
smallest and largest round beside it.  --root: the package of another checkout of the project (the parent commit's,
built), which runs the host frames only; such a process counts as tree "parent".  --off-only: this tree the same way, two
generators and nothing else in the process, which is the process the parent's is compared with.
--trace-run: 30 VGA frames with float32 depth under a distorting camera model, then 10 conversions of a 4096 x 4096
float32 plane (cvo_fe_convert_depth), and nothing else, for a rocprofv3 --kernel-trace run of its own (no counters);
--kernel-trace: the kernel_trace.csv of such a run: the durations (median, smallest, largest) of k_fe_depth_convert per
VGA plane (its first 30 dispatches) and per 4096 x 4096 plane (the rest), and of k_fe_rectify.
--merge: no GPU; the --out files of several processes of one session, in the order they ran, become one file; --bench:
result lines of bench.py, "<tree>=<the JSON line>" each, in the order they ran; --second: the --out files of a later call
(host frames alone in the other order), recorded apart.  Nothing here is asserted, and nothing
here measures what device input is worth behind a real decoder or network: none is shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1241, 376
BIG = 4096
TRACE_FRAMES = 30
HBM_PEAK_TB_S = 8.0   # MI355X, the vendor's figure
DISTORTING = (5000.0, 517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
# from hipcc -Rpass-analysis=kernel-resource-usage, gfx950
RESOURCES = {"k_fe_depth_convert<F32>": {"vgprs": 14, "sgprs": 20, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 8},
             "k_fe_depth_convert<F16>": {"vgprs": 12, "sgprs": 20, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 8}}


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path):
    """The durations of k_fe_depth_convert by plane and of k_fe_rectify in a --trace-run's trace"""
    conv, rect = [], []
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for row in rows:
        name = row.get("Kernel_Name", "")
        us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        if "k_fe_depth_convert" in name:
            conv.append(us)
        elif "k_fe_rectify(" in name or "k_fe_rectify<" in name:
            rect.append(us)
    out = {}
    if conv[:TRACE_FRAMES]:
        out["k_fe_depth_convert<F32> vga"] = _stats(conv[:TRACE_FRAMES])
    if conv[TRACE_FRAMES:]:
        big = _stats(conv[TRACE_FRAMES:])
        moved = BIG * BIG * 6
        big["bytes_moved"] = moved
        big["tb_per_s_at_the_median"] = moved / (big["median_us"] * 1e-6) / 1e12
        big["fraction_of_hbm_peak"] = big["tb_per_s_at_the_median"] / HBM_PEAK_TB_S
        out["k_fe_depth_convert<F32> 4096x4096"] = big
    if rect:
        out["k_fe_rectify vga"] = _stats(rect)
    if conv[:TRACE_FRAMES] and rect:
        out["convert_median_over_rectify_median"] = out["k_fe_depth_convert<F32> vga"]["median_us"] / out["k_fe_rectify vga"]["median_us"]
        out["convert_max_over_rectify_max"] = out["k_fe_depth_convert<F32> vga"]["max_us"] / out["k_fe_rectify vga"]["max_us"]
    return out


def merge(paths, out_path, bench, second=None):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "rounds", "frames_per_round", "timing", "pictures") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["real_producers"] = ("unmeasured: what device input is worth behind a real decoder or network needs one, and none is "
                             "shipped")
    res["kernel"] = dict(RESOURCES, **{"from": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"})
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = set(r["ms_per_frame"]) == {"depth_vga_host", "stereo_kitti_host"}
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["device_minus_host_ms"] = {}
    for kind in ("depth_vga", "stereo_kitti"):
        base = spread.get("this:%s_host" % kind)
        for k, v in sorted(spread.items()):
            tree, _, case = k.partition(":")
            if tree == "this" and base and case.startswith(kind + "_") and case != kind + "_host" and not case.endswith("_alone"):
                res["device_minus_host_ms"][case] = {"difference_of_the_medians_of_the_runs": statistics.median(v) - statistics.median(base),
                                                     "host_spread_max_minus_min": max(base) - min(base)}
        # within each process: the round-by-round differences, which the drift of a machine between processes cancels in
    res["device_minus_host_within_a_process_ms"] = [f["device_minus_host_ms"] for f in files if "device_minus_host_ms" in f]
    res["default_this_minus_parent_ms"] = {}
    for case in ("depth_vga_host", "stereo_kitti_host"):
        p, t = spread.get("parent:%s_alone" % case), spread.get("this:%s_alone" % case)
        if p and t:
            res["default_this_minus_parent_ms"][case] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                                         "parent_spread_max_minus_min": max(p) - min(p),
                                                         "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        if "bytes_from_the_host" in f and f["tree"] == "this":
            res["bytes_from_the_host"] = f["bytes_from_the_host"]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    if bench:
        res["bench_py"] = {"command": "python bench.py --gpus 1 --steps 20 --warmup 3 in each tree in turn, in this order", "runs": []}
        for item in bench:
            tree, _, line = item.partition("=")
            d = json.loads(line)
            res["bench_py"]["runs"].append({"tree": tree, "value": d.get("value"), "unit": d.get("unit"), "ms_per_step": d.get("ms_per_step")})
    if second:   # (the host frames alone once more, in another call and the other order: kept apart, a machine of its own)
        res["second_session"] = {"what": "host frames alone, this library's process first, in a later call (another machine of the pool); "
                                         "in the order they ran",
                                 "runs": [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]}
                                          for f in (json.load(open(p)) for p in second)]}
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--bench", nargs="+", default=None)
    ap.add_argument("--second", nargs="+", default=None)
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
            raise SystemExit("fe_device_input_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench, args.second)
        return
    if args.kernel_trace and not args.trace_run and args.rounds == 0:   # (a trace alone: no GPU)
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
        raise SystemExit("fe_device_input_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_device = hasattr(F.PcdGenerator, "submit_device") and not args.off_only
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    if args.trace_run:
        gen = F.PcdGenerator(640, 480)
        gen.set_camera(F.CameraModel(*DISTORTING))
        gen.set_depth_format(F.DEPTH_F32)
        for k in range(TRACE_FRAMES):
            bgr, dep = vga[k % 8]
            gen.create_pointcloud(bgr, dep.astype(np.float32) / np.float32(5000.0), 1, F.FEATURES_HSV)
        gen.close()
        big = np.random.default_rng(1).uniform(0.1, 12.0, (BIG, BIG)).astype(np.float32)
        for _ in range(10):
            F.convert_depth(big, F.DEPTH_F32, BIG, BIG, 1.0, 5000.0)
        return
    kitti = [pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k))[0] for k in range(4)]
    pairs = [(np.ascontiguousarray(img), np.ascontiguousarray(np.roll(img, -8, axis=1))) for img in kitti]
    gens, images, kinds = {}, {}, {}

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

    def case(name, kind, frames, fmt=None):
        stereo = name.startswith("stereo")
        gens[name] = F.PcdGenerator(W, H) if stereo else F.PcdGenerator(640, 480)
        if stereo:
            gens[name].set_stereo(F.Stereo(0.54, 128))
        if fmt is not None:
            gens[name].set_depth_format(fmt)
        images[name] = [tuple(up(a) for a in fr) for fr in frames] if kind == "device" else frames
        kinds[name] = kind

    def frame(name, k):
        g = gens[name]
        a, b = images[name][k % len(images[name])]
        if name.startswith("depth"):
            (g.submit_device if kinds[name] == "device" else g.submit)(a, b, 1, F.FEATURES_HSV)
        else:
            (g.submit_stereo_device if kinds[name] == "device" else g.submit_stereo)(a, b, 4, F.FEATURES_HSV)
        return g.collect()

    case("depth_vga_host", "host", vga)
    case("stereo_kitti_host", "host", pairs)
    if has_device:
        metres = [(bgr, dep.astype(np.float32) / np.float32(5000.0)) for bgr, dep in vga]
        case("depth_vga_device", "device", vga)
        case("stereo_kitti_device", "device", pairs)
        case("depth_vga_host_f32", "host", metres, F.DEPTH_F32)
        case("depth_vga_device_f32", "device", metres, F.DEPTH_F32)
    torch.cuda.synchronize()
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
           "rounds": args.rounds, "frames_per_round": args.frames,
           "pictures": "synthetic frames of the package; depth_vga: 640 x 480 and a depth image (uint16, or _f32: float32 metres); "
                       "stereo_kitti: a pair of %d x %d, Stereo(0.54, 128); device: torch tensors made before the clock starts" % (W, H),
           "timing": "host clock around submit* + collect (synchronous), the cases alternating per round in one process; ms per "
                     "frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "bytes_from_the_host": {name: (0 if kinds[name] == "device" else int(sum(np.asarray(a).nbytes for a in images[name][0])))
                                   for name in gens}}
    if has_device:
        diff = {}
        for dev, host in (("depth_vga_device", "depth_vga_host"), ("stereo_kitti_device", "stereo_kitti_host"),
                          ("depth_vga_device_f32", "depth_vga_host_f32"), ("depth_vga_host_f32", "depth_vga_host")):
            d = [a - b for a, b in zip(per_round[dev], per_round[host])]
            diff[dev + " - " + host] = {"median_of_the_rounds": statistics.median(d), "min": min(d), "max": max(d),
                                        "host_rounds_max_minus_min": max(per_round[host]) - min(per_round[host])}
        res["device_minus_host_ms"] = diff
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
