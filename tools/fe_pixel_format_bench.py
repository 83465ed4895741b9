#!/usr/bin/env python3
"""Cost of the pixel formats of the front end (cvo_fe_set_pixel_format): host-to-host time of one VGA depth frame under
every format, and of one 1241 x 376 stereo frame under the formats an odd width takes, beside the same frames in BGR8
in the same process, with the bytes each uploads; and the duration of the launch (k_fe_unpack<FORMAT>) per VGA image
and per 1241 x 376 pair beside k_fe_rectify and k_fe_median in one trace.

    python tools/fe_pixel_format_bench.py [--out FILE] [--rounds 7] [--frames 200] [--root DIR] [--label TEXT] [--off-only]
                                          [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_pixel_format_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_pixel_format.json

The pictures are the synthetic frames of the package, packed by the test side's packers (tests/fe_unpack_ref.py); a
stereo pair is a picture and the same picture eight columns to the side.
One generator per case, all alternating in one process: a round times --frames frames of each in turn (host clock around
synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest and largest
round beside it.  --root: the package of another checkout of the project (the parent commit's, built), which runs the
BGR8 frames only; such a process counts as tree "parent".  --off-only: this tree the same way, two generators and
nothing else in the process, which is the process the parent's is compared with.
--trace-run: 30 VGA depth frames under every format, 30 stereo frames at 1241 x 376 under every format that size takes,
and 30 VGA frames in GREY8 under a distorting camera model and the median stage (1, 5), and nothing else, for a
rocprofv3 --kernel-trace run of its own (no counters); --kernel-trace: the kernel_trace.csv of such a run: the durations
(median, smallest, largest) of every instance of k_fe_unpack per VGA image (its first 30 dispatches) and per pair (the next 30), of
k_fe_rectify and of k_fe_median.
--merge: no GPU; the --out files of several processes of one session, in the order they ran, become one file; --bench:
result lines of bench.py, "<tree>=<the JSON line>" each, in the order they ran.  Nothing here is asserted, and nothing
here measures what the formats are worth on real recordings: no frames are shipped."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1241, 376
TRACE_FRAMES = 30
DISTORTING = (5000.0, 517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
# from hipcc -Rpass-analysis=kernel-resource-usage, gfx950: VGPRs, LDS bytes per workgroup; no instance uses scratch
RESOURCES = {"RGB8": (20, 0), "BGRA8": (20, 0), "RGBA8": (20, 0), "GREY8": (11, 0), "YUY2": (21, 0), "UYVY": (21, 0),
             "NV12": (22, 0), "BAYER_RGGB8": (30, 1296), "BAYER_BGGR8": (30, 1296), "BAYER_GRBG8": (30, 1296),
             "BAYER_GBRG8": (30, 1296)}


def _stats(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}


def kernel_times(path, names, pair_formats):
    """The durations of k_fe_unpack by instance and image, of k_fe_rectify and of k_fe_median in a --trace-run's trace"""
    by = {}
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for row in rows:
        name = row.get("Kernel_Name", "")
        us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        m = re.search(r"k_fe_unpack<(\d+)>", name)
        if m:
            by.setdefault("k_fe_unpack<%s>" % names[int(m.group(1))], []).append(us)
        for k in ("k_fe_rectify", "k_fe_median"):
            if k + "(" in name or k + "<" in name:
                by.setdefault(k, []).append(us)
    out = {}
    for k, v in sorted(by.items()):
        if not k.startswith("k_fe_unpack"):
            out[k] = _stats(v)
            continue
        out[k + " vga"] = _stats(v[:TRACE_FRAMES])
        if k[12:-1] in pair_formats and len(v) >= 2 * TRACE_FRAMES:
            out[k + " pair_1241x376"] = _stats(v[TRACE_FRAMES:2 * TRACE_FRAMES])
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "rounds", "frames_per_round", "timing", "pictures") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["recordings"] = "unmeasured: what the formats are worth on real recordings needs real frames, and none are shipped"
    res["kernel"] = {"k_fe_unpack<%s>" % k: {"vgprs": v[0], "lds_bytes": v[1], "scratch_bytes": 0} for k, v in RESOURCES.items()}
    res["kernel"]["from"] = "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = set(r["ms_per_frame"]) == {"depth_vga_BGR8", "stereo_kitti_BGR8"}
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["format_minus_bgr8_ms"] = {}
    for k, v in sorted(spread.items()):
        tree, _, case = k.partition(":")
        for kind in ("depth_vga", "stereo_kitti"):
            base = spread.get("this:%s_BGR8" % kind)
            if tree == "this" and case.startswith(kind + "_") and case != kind + "_BGR8" and not case.endswith("_alone") and base:
                res["format_minus_bgr8_ms"][case] = {"difference_of_the_medians_of_the_runs": statistics.median(v) - statistics.median(base),
                                                     "bgr8_spread_max_minus_min": max(base) - min(base)}
    res["default_this_minus_parent_ms"] = {}
    for case in ("depth_vga_BGR8", "stereo_kitti_BGR8"):
        p, t = spread.get("parent:%s_alone" % case), spread.get("this:%s_alone" % case)
        if p and t:
            res["default_this_minus_parent_ms"][case] = {"difference_of_the_medians_of_the_runs": statistics.median(t) - statistics.median(p),
                                                         "parent_spread_max_minus_min": max(p) - min(p),
                                                         "this_spread_max_minus_min": max(t) - min(t)}
    for f in files:
        if "bytes_uploaded" in f and f["tree"] == "this":
            res["bytes_uploaded"] = f["bytes_uploaded"]
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
            raise SystemExit("fe_pixel_format_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_pixel_format_bench: needs a GPU")
    import fe_unpack_ref as K
    pkg = ge.load_package()
    F = pkg.frontend
    has_formats = hasattr(F, "PIXEL_BGR8") and not args.off_only
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    kitti = [pkg.data.synthetic_rgbd_frame(width=W, height=H, seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k))[0] for k in range(4)]
    pairs = [(np.ascontiguousarray(img), np.ascontiguousarray(np.roll(img, -8, axis=1))) for img in kitti]
    vga_formats = [f for f in K.FORMATS if f != K.BGR8] if has_formats else []
    pair_formats = [f for f in vga_formats if K.fits(f, W, H)]
    gens, images = {}, {}

    def depth_case(fmt):
        name = "depth_vga_" + K.NAMES[fmt]
        gens[name] = F.PcdGenerator(640, 480)
        if fmt != K.BGR8:
            gens[name].set_pixel_format(fmt)
        images[name] = [(bgr if fmt == K.BGR8 else K.pack(bgr, fmt), dep) for bgr, dep in vga]
        return name

    def stereo_case(fmt):
        name = "stereo_kitti_" + K.NAMES[fmt]
        gens[name] = F.PcdGenerator(W, H)
        gens[name].set_stereo(F.Stereo(0.54, 128))
        if fmt != K.BGR8:
            gens[name].set_pixel_format(fmt)
        images[name] = [(a, b) if fmt == K.BGR8 else (K.pack(a, fmt), K.pack(b, fmt)) for a, b in pairs]
        return name

    def frame(name, k):
        a, b = images[name][k % len(images[name])]
        if name.startswith("depth"):
            return gens[name].create_pointcloud(a, b, 1, F.FEATURES_HSV)
        return gens[name].create_pointcloud_stereo(a, b, 4, F.FEATURES_HSV)

    if args.trace_run:
        for fmt in vga_formats:
            name = depth_case(fmt)
            for k in range(TRACE_FRAMES):
                frame(name, k)
            if fmt in pair_formats:
                name = stereo_case(fmt)
                for k in range(TRACE_FRAMES):
                    frame(name, k)
        gen = F.PcdGenerator(640, 480)
        gen.set_camera(F.CameraModel(*DISTORTING))
        gen.set_depth_median(F.DepthMedian(1, 5))
        gen.set_pixel_format(K.GREY8)
        for k in range(TRACE_FRAMES):
            gen.create_pointcloud(K.pack(vga[k % 8][0], K.GREY8), vga[k % 8][1], 1, F.FEATURES_HSV)
        for g in list(gens.values()) + [gen]:
            g.close()
        return
    depth_case(K.BGR8)
    stereo_case(K.BGR8)
    for fmt in vga_formats:
        depth_case(fmt)
    for fmt in pair_formats:
        stereo_case(fmt)
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
           "pictures": "synthetic frames of the package, packed by tests/fe_unpack_ref.py; depth_vga: 640 x 480 and a depth image; "
                       "stereo_kitti: a pair of %d x %d, Stereo(0.54, 128)" % (W, H),
           "timing": "host clock around create_pointcloud* (synchronous), the cases alternating per round in one process; ms per "
                     "frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()},
           "bytes_uploaded": {name: int(sum(np.asarray(a).nbytes for a in images[name][0])) for name in gens}}
    if args.kernel_trace:
        res["kernel_trace_us"] = kernel_times(args.kernel_trace, K.NAMES, [K.NAMES[f] for f in pair_formats])
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
