#!/usr/bin/env python3
"""Cost of the photometric stage of the front end (cvo_fe_set_photometric): the durations of k_fe_photo_apply and
k_fe_photo_stat at three sizes beside k_fe_unpack<RGB8> on the same images in one trace; host-to-host time of a VGA frame
with and without the stage; and frames without the stage, for this library against the parent commit's.

    python tools/fe_photometric_bench.py [--out FILE] [--rounds 5] [--frames 60] [--root DIR] [--label TEXT] [--off-only]
                                         [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>]
    python tools/fe_photometric_bench.py --merge A.json B.json ... [--bench LINE ...] --out profiles/fe_photometric.json

The pictures are the synthetic frames of the package.  One generator per case, all alternating in one process: a round
times --frames frames of each in turn (host clock around submit + collect, which is synchronous); recorded per case are
the median over the rounds of the per-frame time and the smallest and largest round beside it.  --root: the package of
another checkout of the project (the parent commit's, built), which runs the frames without the stage only; such a
process counts as tree "parent".  --off-only: this tree the same way, one generator and nothing else in the process,
which is the process the parent's is compared with.  --trace-run: per size 20 runs each of cvo_fe_photometric_image with
both tables and the caller's gains (k_fe_photo_apply<3>), of the same with AUTO and a target (k_fe_photo_stat<3>,
k_fe_photo_gain, k_fe_photo_apply<3>), of the first without the response table (k_fe_photo_apply<2>: no LDS) and of
cvo_fe_unpack_image (RGB8), and nothing else, for a rocprofv3
--kernel-trace run of its own (no counters); --kernel-trace: the kernel_trace.csv of such a run.  --merge: no GPU; the
--out files of several processes of one session, in the order they ran, become one file; --bench: result lines of
bench.py, "<tree>=<the JSON line>" each, in the order they ran.
Nothing here is asserted, and nothing here measures what the stage is worth in trajectory accuracy: no real frames are
shipped."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((640, 480), (1920, 1080), (3840, 2160))
RUNS = 20
# from hipcc -Rpass-analysis=kernel-resource-usage, gfx950 (profiles/fe_photometric_isa_resources.txt)
RESOURCES = {"k_fe_photo_apply<3>": {"vgprs": 26, "sgprs": 22, "lds_bytes": 1536, "scratch_bytes": 0, "occupancy_waves_per_simd": 8},
             "k_fe_photo_stat<3>": {"vgprs": 34, "sgprs": 34, "lds_bytes": 1664, "scratch_bytes": 0, "occupancy_waves_per_simd": 8},
             "k_fe_photo_gain": {"vgprs": 31, "sgprs": 32, "lds_bytes": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 8}}


def _stats(v, moved):
    med = statistics.median(v)
    return {"median_us": med, "min_us": min(v), "max_us": max(v), "dispatches": len(v), "bytes_moved": moved,
            "tb_per_s_at_the_median": moved / (med * 1e-6) / 1e12}


def kernel_times(path):
    """The durations of a --trace-run's kernels, in its order: per size RUNS of k_fe_photo_apply (the caller's gains), then
    RUNS of k_fe_photo_stat, k_fe_photo_gain and k_fe_photo_apply (AUTO), then RUNS of k_fe_photo_apply without a response
    table (no LDS), then RUNS of k_fe_unpack"""
    with open(path) as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    seq = {"k_fe_photo_apply": [], "k_fe_photo_stat": [], "k_fe_photo_gain": [], "k_fe_unpack": []}
    for row in rows:
        name = row.get("Kernel_Name", "")
        for key in seq:
            if key in name:
                seq[key].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for k, (w, h) in enumerate(SIZES):
        npix = w * h
        tag = "%dx%d" % (w, h)
        ap = seq["k_fe_photo_apply"][3 * RUNS * k:3 * RUNS * (k + 1)]
        if len(ap) == 3 * RUNS:
            out["k_fe_photo_apply<3> gains %s" % tag] = _stats(ap[:RUNS], npix * 8)
            out["k_fe_photo_apply<3> auto %s" % tag] = _stats(ap[RUNS:2 * RUNS], npix * 8)
            out["k_fe_photo_apply<2> gains, no response table %s" % tag] = _stats(ap[2 * RUNS:], npix * 8)
        for key, moved in (("k_fe_photo_stat", npix * 5), ("k_fe_photo_gain", 0), ("k_fe_unpack", npix * 6)):
            v = seq[key][RUNS * k:RUNS * (k + 1)]
            if len(v) == RUNS:
                out["%s %s" % ({"k_fe_photo_stat": "k_fe_photo_stat<3>", "k_fe_unpack": "k_fe_unpack<RGB8>"}.get(key, key), tag)] = _stats(v, moved)
        a, u = out.get("k_fe_photo_apply<3> gains %s" % tag), out.get("k_fe_unpack<RGB8> %s" % tag)
        if a and u:
            out["apply over unpack %s" % tag] = {"ratio_of_the_medians": a["median_us"] / u["median_us"], "bytes_ratio": 8.0 / 6.0,
                                                 "unpack_spread_us": u["max_us"] - u["min_us"],
                                                 "apply_spread_us": a["max_us"] - a["min_us"],
                                                 "apply_minus_unpack_us": a["median_us"] - u["median_us"],
                                                 "bound_8_over_6_plus_spread_us": u["median_us"] * 8.0 / 6.0 + (u["max_us"] - u["min_us"])}
    return out


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "rounds", "frames_per_round", "timing", "pictures") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["accuracy"] = ("unmeasured: what the stage is worth in trajectory accuracy needs a recording under auto exposure with a "
                       "calibration, and no real frames are shipped")
    res["kernel"] = dict(RESOURCES, **{"from": "hipcc -Rpass-analysis=kernel-resource-usage, gfx950"})
    res["runs"] = [{"run": f.get("label", ""), "tree": f["tree"], "ms_per_frame": f["ms_per_frame"]} for f in files if "ms_per_frame" in f]
    spread = {}
    for r in res["runs"]:
        alone = set(r["ms_per_frame"]) == {"depth_vga_off"}
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case + ("_alone" if alone else ""), []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["stage_minus_off_within_a_process_ms"] = [f["stage_minus_off_ms"] for f in files if "stage_minus_off_ms" in f]
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


def _tables(w, h):
    b = np.arange(256, dtype=np.int64)
    response = np.stack([np.clip(b * 256 + (c + 1) * ((b * (255 - b)) >> 1), 0, 65535) for c in range(3)]).astype(np.uint16)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    r2 = (xx - w // 2) ** 2 + (yy - h // 2) ** 2
    vignette = (4096 + (r2 * 2000) // ((w // 2) ** 2 + (h // 2) ** 2)).astype(np.uint16)
    return response, vignette


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
            raise SystemExit("fe_photometric_bench: --merge needs --out")
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
        raise SystemExit("fe_photometric_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    has_stage = hasattr(F.PcdGenerator, "set_photometric") and not args.off_only
    rng = np.random.default_rng(1)
    if args.trace_run:
        for w, h in SIZES:
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            response, vignette = _tables(w, h)
            gains = F.Photometric(F.PHOTO_GAIN | F.PHOTO_RESPONSE | F.PHOTO_VIGNETTE)
            auto = F.Photometric(F.PHOTO_AUTO | F.PHOTO_RESPONSE | F.PHOTO_VIGNETTE, per_channel=1, target=(33000, 33000, 33000))
            for _ in range(RUNS):
                F.photometric_image(img, gains, response, vignette, (5000, 4096, 3300))
            for _ in range(RUNS):
                F.photometric_image(img, auto, response, vignette)
            plain = F.Photometric(F.PHOTO_GAIN | F.PHOTO_VIGNETTE)
            for _ in range(RUNS):
                F.photometric_image(img, plain, None, vignette, (5000, 4096, 3300))
            for _ in range(RUNS):
                F.unpack_image(img.reshape(h, w * 3), F.PIXEL_RGB8, w, h)
        return
    vga = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(4)]
    gens = {}

    def case(name, photometric=None, tables=False):
        g = F.PcdGenerator(640, 480)
        if photometric is not None:
            g.set_photometric(photometric, *(_tables(640, 480) if tables else ()))
        gens[name] = g

    def frame(name, k):
        a, b = vga[k % len(vga)]
        gens[name].submit(a, b, 1, F.FEATURES_HSV)
        return gens[name].collect()

    case("depth_vga_off")
    if has_stage:
        case("depth_vga_gains_and_tables", F.Photometric(F.PHOTO_GAIN | F.PHOTO_RESPONSE | F.PHOTO_VIGNETTE), True)
        gens["depth_vga_gains_and_tables"].set_photometric_gain((1.2, 1.0, 0.8))
        case("depth_vga_gains_alone", F.Photometric(F.PHOTO_GAIN))
        case("depth_vga_auto_and_tables", F.Photometric(F.PHOTO_AUTO | F.PHOTO_RESPONSE | F.PHOTO_VIGNETTE, per_channel=1), True)
    torch.cuda.synchronize()
    for name in gens:   # warm-up: the graphs are captured here
        for k in range(8):
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
           "pictures": "synthetic frames of the package, 640 x 480; off: a context that never made the call; gains_and_tables: "
                       "a response table, a vignette and the caller's gains; gains_alone: no tables; auto_and_tables: the "
                       "tables and AUTO per channel with the lock",
           "timing": "host clock around submit + collect (synchronous), the cases alternating per round in one process; ms per "
                     "frame: median [min, max] over the rounds",
           "ms_per_frame": {name: [statistics.median(v), min(v), max(v)] for name, v in per_round.items()}}
    if has_stage:
        diff = {}
        for name in per_round:
            if name != "depth_vga_off":
                d = [x - y for x, y in zip(per_round[name], per_round["depth_vga_off"])]
                diff[name + " - depth_vga_off"] = {"median_of_the_rounds": statistics.median(d), "min": min(d), "max": max(d)}
        res["stage_minus_off_ms"] = diff
    for gen in gens.values():
        gen.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
