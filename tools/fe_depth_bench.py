#!/usr/bin/env python3
"""Cost of a depth camera of its own in the front end: host-to-host time of one VGA frame (create_pointcloud: staging,
upload, every kernel, the cloud back on the host) without a rig, with the identity rig, with a VGA Kinect-like rig
(k_fe_depth_warp and k_fe_depth_final in front of everything else) and with that rig beside the TUM fr1 colour lens
(k_fe_rectify for colour as well).

    python tools/fe_depth_bench.py [--out profiles/fe_depth_camera.json] [--rounds 9] [--frames 300] [--root DIR]
                                   [--trace-run] [--kernel-trace <rocprofv3 kernel_trace.csv>] [--label TEXT] [--tree NAME]
    python tools/fe_depth_bench.py --merge A.json B.json ... --out profiles/fe_depth_camera.json [--bench parent.json this.json ...]

One generator per case, the cases alternating in one process: a round times --frames frames of each case in turn (host
clock around synchronous calls); recorded per case are the median over the rounds of the per-frame time and the smallest
and largest round beside it.  The frames are synthetic (data.synthetic_rgbd_frame, texture 1.0), eight of them in turn;
the rig's depth images are those of the frames divided by 5 (1000 units per metre).
--root: measure the package of another checkout of the project (e.g. the parent commit's, built) the same way; a package
without depth cameras runs the first case only.  --trace-run: 50 frames of the Kinect-like rig and nothing else, for a
rocprofv3 --kernel-trace run of its own; --kernel-trace: the kernel_trace.csv of such a run, whose k_fe_* durations
(median, smallest, largest, count) are folded into the output.  --merge: no GPU; the --out files of several processes of
one session, in the order they ran (give each a --label; a --root other than the tool's own tree counts as tree
"parent" unless --tree names it, e.g. a build that clears the z-buffer another way), become one file: `runs` lists
every process, `medians_min_max_runs` the smallest and largest median per tree and case over them with the number of
processes, `rig_cost_ms` what each case adds to no_rig (difference of the medians, per tree and process), the kernel trace of the last file that has one is kept with the bytes per second
the two kernels' medians stand for, and --bench adds `value` / `ms_per_step` of saved bench.py result lines (the
parent's and this tree's in turn, in the order they ran).  Nothing here is asserted."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the VGA Kinect-like depth camera of tests/fe_depth_ref.py (VGA_RIG)
KINECT = dict(width=640, height=480, depth_scale=1000.0, fx=580.0, fy=580.0, cx=314.0, cy=252.0,
              dist=(-0.1, 0.3, 0.001, -0.001, -0.2), T=(0.025, -0.001, 0.002))


def _rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                     "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax], np.float64)


KINECT_R = _rot("z", 0.003) @ _rot("y", -0.007) @ _rot("x", 0.004)


def kernel_times(path):
    """Durations (us) of the dispatches of a rocprofv3 kernel trace, by kernel name, k_fe_* only."""
    by = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Kernel_Name", "")
            if "k_fe_" not in name:
                continue
            short = name[name.index("k_fe_"):].split("(")[0]
            by.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "dispatches": len(v)}
            for k, v in sorted(by.items())}


def merge(paths, out_path, bench):
    files = [json.load(open(p)) for p in paths]
    last = files[-1]
    res = {k: last[k] for k in ("device", "image", "rounds", "frames_per_round", "timing") if k in last}
    res["session"] = "the processes of one session on one machine, in the order they ran"
    res["runs"] = [{"run": f.get("label", ""), "tree": f.get("tree") or ("this" if f.get("root", ".") == "." else "parent"),
                    "ms_per_frame": f["ms_per_frame"]} for f in files]
    spread = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            spread.setdefault(r["tree"] + ":" + case, []).append(v[0])
    res["medians_min_max_runs"] = {k: [min(v), max(v), len(v)] for k, v in sorted(spread.items())}
    res["rig_cost_ms"] = {}
    for r in res["runs"]:
        for case, v in r["ms_per_frame"].items():
            if case != "no_rig":
                res["rig_cost_ms"].setdefault(r["tree"], {}).setdefault(case, []).append(v[0] - r["ms_per_frame"]["no_rig"][0])
    for f in files:
        for k in ("points", "identity_cloud_equals_no_rig", "kernel_bytes", "kinect_rig_pixels"):
            if k in f:
                res[k] = f[k]
        if "kernel_trace_us" in f:
            res["kernel_trace_from"] = f.get("label", "")
            res["kernel_trace_us"] = f["kernel_trace_us"]
    for name in ("k_fe_depth_warp", "k_fe_depth_final"):
        if name in res.get("kernel_trace_us", {}) and name in res.get("kernel_bytes", {}):
            res[name + "_bytes_per_s"] = (sum(res["kernel_bytes"][name].values()) /
                                          (res["kernel_trace_us"][name]["median_us"] * 1e-6))
    if bench:
        rows = [json.loads(open(p).read().strip().split("\n")[-1]) for p in bench]
        names = ["%s_%d" % (("parent", "this")[k % 2], k // 2 + 1) for k in range(len(rows))]
        res["bench_py"] = {name: {"value": r.get("value"), "ms_per_step": r.get("ms_per_step"), "unit": r.get("unit")}
                           for name, r in zip(names, rows)}
    print(json.dumps(res["medians_min_max_runs"]), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


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
            raise SystemExit("fe_depth_bench: --merge needs --out")
        merge(args.merge, args.out, args.bench)
        return
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fe_depth_bench: needs a GPU")
    pkg = ge.load_package()
    F = pkg.frontend
    w, h = 640, 480
    frames = [pkg.data.synthetic_rgbd_frame(seed=70 + k, texture=1.0, motion=(1.2 * k, 0.6 * k)) for k in range(8)]
    raw = [np.ascontiguousarray(f[1] // 5) for f in frames]
    cases = [("no_rig", None, None, False)]
    if hasattr(F, "DepthCamera"):
        row1 = F.camera(1)
        ident = F.DepthCamera(width=w, height=h, depth_scale=row1["scaling_factor"], fx=row1["fx"], fy=row1["fy"],
                              cx=row1["cx"], cy=row1["cy"])
        kinect = F.DepthCamera(R=KINECT_R, **KINECT)
        cases += [("identity_rig", ident, None, False), ("kinect_rig", kinect, None, True),
                  ("kinect_rig_fr1_lens", kinect, F.TUM_CAMERAS["fr1"], True)]
    if args.trace_run:
        gen = F.PcdGenerator(w, h)
        gen.set_depth_camera(cases[2][1])
        for k in range(50):
            gen.create_pointcloud(frames[k % 8][0], raw[k % 8], 1, F.FEATURES_HSV)
        gen.close()
        return
    gens = []
    for name, rig, cam, _ in cases:
        g = F.PcdGenerator(w, h)
        if cam is not None:
            g.set_camera(cam)
        if rig is not None:
            g.set_depth_camera(rig)
        gens.append(g)
    clouds = []
    for (_, _, _, use_raw), g in zip(cases, gens):   # warm-up: the graph of each context is captured here
        for k in range(16):
            c = g.create_pointcloud(frames[k % 8][0], raw[k % 8] if use_raw else frames[k % 8][1], 1, F.FEATURES_HSV)
        clouds.append(c)
    written = None
    if len(cases) > 1:
        written = int(np.count_nonzero(gens[2].read_stage(F.STAGE_RECT_DEPTH)))
        live = int(np.count_nonzero(raw[15 % 8]))
    per_round = {c[0]: [] for c in cases}
    for _ in range(args.rounds):
        for (name, _, _, use_raw), g in zip(cases, gens):
            t0 = time.perf_counter()
            for k in range(args.frames):
                g.create_pointcloud(frames[k % 8][0], raw[k % 8] if use_raw else frames[k % 8][1], 1, F.FEATURES_HSV)
            per_round[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    res = {"label": args.label, "tree": args.tree, "root": os.path.relpath(root, ROOT), "device": torch.cuda.get_device_name(0),
           "image": [w, h], "rounds": args.rounds, "frames_per_round": args.frames,
           "timing": "host clock around create_pointcloud (synchronous), cases alternating per round in one process; "
                     "ms per frame: median [min, max] over the rounds",
           "ms_per_frame": {}}
    for c in cases:
        v = per_round[c[0]]
        res["ms_per_frame"][c[0]] = [statistics.median(v), min(v), max(v)]
    if len(cases) > 1:
        res["identity_cloud_equals_no_rig"] = bool(np.array_equal(clouds[0][0], clouds[1][0]) and
                                                   np.array_equal(clouds[0][1], clouds[1][1]))
        res["points"] = {c[0]: int(len(cl[0])) for c, cl in zip(cases, clouds)}
        # what the two kernels move per frame of the Kinect-like rig: the atomics count 4 bytes each, one per colour
        # pixel of a footprint -- at least the pixels that ended up written, about one per live depth pixel here
        res["kernel_bytes"] = {
            "k_fe_depth_warp": {"depth_read": w * h * 2, "rays_read": (w + 1) * (h + 1) * 8,
                                "z_buffer_atomics_at_least": written * 4},
            "k_fe_depth_final": {"z_buffer_read": w * h * 4, "z_buffer_rearmed": w * h * 4, "depth_written": w * h * 2}}
        res["kinect_rig_pixels"] = {"live_depth_pixels": live, "colour_pixels_written": written}
    if args.kernel_trace:
        res["kernel_trace_us"] = kernel_times(args.kernel_trace)
    for g in gens:
        g.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
