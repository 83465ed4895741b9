#!/usr/bin/env python3
"""bench.py -- frame-pair registrations/s of the CVO inner loop on MI355X.

A "step" is one pass of the hot path over one BATCH of synthetic input: `--batch`
(default 64) independent, DISTINCT frame pairs of the BASELINE.json configs[1] shape --
synthetic 10k x 10k RGB-D clouds; pair 0 is the configs[1] pair itself (seed 20190402),
pair i >= 1 has seed 1000 + i -- each run through a full align()
(ref src/cvo.cpp:361-420: 43-102 gradient-flow iterations, each = transform + all-pairs
neighbour filter + flow pass + step-size pass) from the reference object's initial state,
all clouds already resident in HBM, all registrations of the batch handed to ONE
cvo_hip_align_many call (three engines of up to 32 slots each share the GPU; a slot's registration
is one blockIdx.z slice of every kernel launch of its engine; a slot that falls free takes
the next pair of the batch -- continuous batching).  `value` = registrations completed per second.  A plain run
sets up, warms up, times `--steps` steps, writes the results of the last one under `--dump-outputs DIR` if given,
and prints the line.  With `--full`, side legs of the same run
(rank 0, N = 1; none of them inside the timed region): the same batch size with copies of
ONE pair (`identical_pairs`), one registration at a time (`single_stream`), kernel
durations by HIP events for the roofline objects, BASELINE configs[4] per GPU
(`config4`: 8 concurrent 20k x 20k), the RGB-D front end, and the CPU oracle timed on
this box (`cpu_baseline`) -- whose result for pair 0 is compared with the GPU's
(`parity_vs_oracle`).

One process per GPU; for N > 1 every rank runs its own batches (independent frame pairs:
weak scaling, no data-path collective), and -- with `--full`, as a separately reported leg -- all ranks
also run the target-sharded mode of BASELINE configs[3] (200k x 200k, rows split over the
ranks, partial sums exchanged through peer mailboxes over xGMI, RCCL as the fall-back).

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

FLOP_PER_PAIR = 8.0            # 3 sub + 3 mul + 2 add per pair test
FLOP_PER_MEMBER = 45.0         # flow sweep, per surviving pair (+ 2 exp)
F64_OPS_PER_EXP = 14.0         # the device exp (cvo_kernels.hip exp_neg)
BYTES_PER_POINT = 32.0         # xyz 12 B + 5 features 20 B
PEAK_F32_TFLOPS = 157.3        # MI355X_MICROARCH.md: FP32 vector = FP32 MFMA peak
PEAK_HBM_GBS = 8000.0
FETCH_CALIBRATION = "profiles/r05_fetch_calibration.txt"   # what TCC FETCH_SIZE counts on a 16-byte gather of known footprint
def _profile_tag():
    """The newest round whose rocprofv3 summaries are committed under profiles/ (tools/gpu_profile_r6.sh)."""
    for tag in ("r06", "r05"):
        if os.path.exists(os.path.join(ROOT, "profiles", "%s_pmc_summary.json" % tag)):
            return tag
    return "r05"


PROFILE_TAG = _profile_tag()


COMPACT_LIMIT = 6000   # bytes: the driver keeps an 8 KB tail of stdout; the headline line must sit inside it whole


def _num(x, digits=6):
    """A finite number rounded to `digits` significant figures (strict JSON: no NaN / Infinity), else None."""
    try:
        x = float(x)
    except (TypeError, ValueError):
        return None
    if x != x or x in (float("inf"), float("-inf")):
        return None
    if x == 0.0:
        return 0.0
    if x == int(x) and abs(x) < 1e15:
        return int(x)
    return float("%.*g" % (digits, x))


def _get(obj, *path):
    for key in path:
        if not isinstance(obj, dict) or key not in obj:
            return None
        obj = obj[key]
    return obj


def compact_line(out, detail_file="bench_detail.json"):
    """The headline object of the run: the contract's keys, `config`, `roofline`, `cpu_baseline` and
    `parity_vs_oracle` as numbers and short names only.  Everything else the run measured (per-phase
    tables, the side legs, the prose) is `detail_file`.  Pure function of the full object, so a CPU test
    holds it to COMPACT_LIMIT on canned legs (tests/test_bench_line.py)."""
    cfg = out.get("config", {}) or {}
    one = cfg.get("one_registration_at_a_time") or {}
    rl = out.get("roofline") or {}
    line = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                    "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    for k in ("value", "ms_per_step"):
        line[k] = _num(line[k], 7)
    if out.get("ranks_on_device0"):
        line["ranks_on_device0"] = True
    mode = cfg.get("mode", "cvo")
    n, m, batch = cfg.get("points_fixed"), cfg.get("points_moving"), cfg.get("batch")
    c = {"workload": "BASELINE configs[1] shape: %s distinct synthetic %sx%s RGB-D cloud pairs (xyz + 5-dim colour) per "
                     "align_many call, %s align() to convergence, clouds resident in HBM"
                     % (batch, n, m, mode) if cfg.get("distinct_pairs", True) else
                     "BASELINE configs[1]: %s copies of the synthetic %sx%s pair per align_many call, %s align() to convergence"
                     % (batch, n, m, mode),
         "points_fixed": n, "points_moving": m, "mode": mode, "batch": batch,
         "iterations_per_registration": _num(out.get("iterations_per_registration"), 5),
         "ms_per_iteration": _num(out.get("ms_per_iteration"), 5)}
    if one:
        o = {"registrations_per_s": _num(one.get("registrations_per_s")),
             "ms_per_iteration": _num(one.get("ms_per_iteration"), 5),
             "iterations": _num(one.get("iterations"), 5)}
        rr = _get(out, "single_stream", "resident_runs")
        if rr:
            o["iterations_inside_resident_runs"] = _num(rr.get("iterations_inside"))
        run = out.get("roofline_run") or {}
        if run:
            o["kt_run_valu_active_frac"] = _num(run.get("frac"), 4)
            o["kt_run_us_per_iteration"] = _num(run.get("us_per_iteration"), 4)
        ac = _get(out, "acvo", "single_stream")
        if ac:
            o["acvo_registrations_per_s"] = _num(ac.get("registrations_per_s"))
            o["acvo_ms_per_iteration"] = _num(ac.get("ms_per_iteration"), 5)
        c["one_registration_at_a_time"] = o
    for k in ("value_including_set_pcd", "config4_registrations_per_s"):
        if cfg.get(k) is not None:
            c[k] = _num(cfg[k])
    for name, path in (("acvo_batched_registrations_per_s", ("acvo", "registrations_per_s")),
                       ("saturation_256_per_call_registrations_per_s", ("saturation", "registrations_per_s")),
                       ("config3_200k_single_gpu_ms_per_registration", ("config3_single_gpu", "ms_per_registration")),
                       ("config3_list_pass_hbm_frac", ("config3_single_gpu", "roofline", "frac")),
                       ("frontend_frames_per_s", ("frontend", "frames_per_s")),
                       ("driver_loop_cvo_frames_per_s", ("frontend", "stream", "cvo", "frames_per_s")),
                       ("driver_loop_acvo_frames_per_s", ("frontend", "stream", "acvo", "frames_per_s"))):
        v = _num(_get(out, *path))
        if v is not None:
            c[name] = v
    sc = _get(out, "small_calls", "fresh_process") or _get(out, "small_calls", "per_call")
    if isinstance(sc, dict):
        c["small_calls_3k_registrations_per_s"] = {k: _num(_get(v, "registrations_per_s") if isinstance(v, dict) else v, 5)
                                                   for k, v in sc.items()}
    line["config"] = c
    if rl:
        r = {"kernel": "cvo_dev::kt_process<PROC_FLOW>", "bound": rl.get("bound"),
             "achieved": _num(rl.get("achieved")), "peak": _num(rl.get("peak")), "unit": rl.get("unit"),
             "frac": _num(rl.get("frac"), 4), "traffic": _num(rl.get("traffic")),
             "algorithmic_bytes_per_launch": _num(rl.get("algorithmic_bytes_per_launch")),
             "registrations_per_launch": _num(rl.get("registrations_per_launch"), 4),
             "avg_launch_us": _num(rl.get("avg_launch_us"), 5), "launches": _num(rl.get("launches")),
             "source": "hip-events, one engine of the timed region's shape",
             "rocprofv3_avg_launch_us": _num(_get(rl, "rocprofv3", "avg_launch_us"), 5),
             "rocprofv3_source": (_get(rl, "rocprofv3", "source") or "").replace("committed ", "") or None,
             "frac_at_rocprofv3_duration": _num(rl.get("frac_at_rocprofv3_duration"), 4),
             "traffic_source": (rl.get("traffic_source") or "").replace("committed ", "") or None,
             "valu_issue_frac": _num(rl.get("valu_issue_frac"), 4)}
        ph = rl.get("by_phase") or {}
        if isinstance(_get(ph, "light", "chain_us"), (int, float)):
            r["narrow_chain_us"] = _num(ph["light"]["chain_us"], 4)
        line["roofline"] = r
        rf = out.get("roofline_filter") or {}
        if rf:
            line["roofline_filter"] = {"kernel": "cvo_dev::kt_filter", "bound": rf.get("bound"),
                                       "achieved": _num(rf.get("achieved")), "peak": _num(rf.get("peak")),
                                       "unit": rf.get("unit"), "frac": _num(rf.get("frac"), 4),
                                       "avg_launch_us": _num(rf.get("avg_launch_us"), 5)}
        run = out.get("roofline_run") or {}
        if run:
            line["roofline_run"] = {k: (_num(v, 5) if isinstance(v, (int, float)) else v) for k, v in run.items()
                                    if isinstance(v, (int, float)) or k in ("kernel", "bound", "unit", "source")}
    cpu = out.get("cpu_baseline") or {}
    if cpu:
        line["cpu_baseline"] = {"value": _num(cpu.get("value")), "unit": cpu.get("unit"), "cores": cpu.get("cores"),
                                "kind": cpu.get("kind"), "ms_per_iteration": _num(cpu.get("ms_per_iteration"), 5),
                                "sample": (cpu.get("sample") or "")[:120],
                                "one_thread_value": _num(_get(cpu, "one_thread", "value"))}
    par = out.get("parity_vs_oracle") or {}
    if par:
        b = par.get("batched") or {}
        line["parity_vs_oracle"] = {"iterations_gpu": par.get("iterations_gpu"), "iterations_oracle": par.get("iterations_oracle"),
                                    "R_T_bit_identical": par.get("R_T_bit_identical"), "rot": _num(par.get("rot")),
                                    "trans": _num(par.get("trans")), "tolerance": par.get("tolerance"),
                                    "batched_registrations": b.get("registrations"),
                                    "batched_bit_identical_to_lone_align": b.get("bit_identical_to_lone_cvo_hip_align"),
                                    "batched_vs_oracle_checked": b.get("vs_oracle_checked"),
                                    "batched_vs_oracle_bit_identical": b.get("vs_oracle_bit_identical"),
                                    "oracle": "oracle/cvo_oracle.c (parity with the reference binary unpinned)"}
    sh = out.get("sharded_allreduce")
    if isinstance(sh, dict):
        line["sharded_allreduce"] = {k: (_num(v) if isinstance(v, float) else v) for k, v in sh.items()
                                     if isinstance(v, (int, float, bool)) or k in ("error", "exchange")}
        if "error" in sh:
            line["sharded_allreduce"]["error"] = str(sh["error"])[:160]
    errs = sorted(k for k, v in out.items() if isinstance(v, dict) and "error" in v and k != "sharded_allreduce")
    if errs:
        line["leg_errors"] = errs
    line["detail"] = detail_file
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    if len(text) > COMPACT_LIMIT:   # cannot happen with the keys above; never let a leg push the headline out
        for k in ("sharded_allreduce", "roofline_filter", "roofline_run", "leg_errors"):
            line.pop(k, None)
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    return text


def _strict(o):
    """The full object as strict JSON (NaN / Infinity -> null)."""
    if isinstance(o, dict):
        return {str(k): _strict(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_strict(v) for v in o]
    if isinstance(o, (float, np.floating)):
        o = float(o)
        return o if o == o and o not in (float("inf"), float("-inf")) else None
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.bool_):
        return bool(o)
    return o


def emit(out):
    """Rank 0's output: the full object to bench_detail.json (repo root, and gpurun_out/ where that exists) and to
    stderr; the compact headline as the ONE JSON line of stdout, last."""
    full = json.dumps(_strict(out), allow_nan=False)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_detail.json"), "w") as fh:
                    fh.write(full + "\n")
            except OSError:
                pass
    sys.stderr.write("bench detail: " + full + "\n")
    sys.stderr.flush()
    print(compact_line(out), flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, run every side leg as well (one-at-a-time rate, roofline, CPU "
                         "baseline and parity, other modes and sizes, the sharded leg under N ranks)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the results of the last timed step (iteration counts, final states) as DIR/<name>.npy")
    ap.add_argument("--points", type=int, default=10000, help="N = M of the synthetic pairs")
    ap.add_argument("--batch", type=int, default=64, help="frame pairs handed to one align_many call per step")
    ap.add_argument("--identical", action="store_true",
                    help="the timed batch is `--batch` copies of the configs[1] pair (round-1 behaviour)")
    ap.add_argument("--mode", default="cvo", choices=["cvo", "acvo"])
    ap.add_argument("--cpu-seconds", type=float, default=12.0,
                    help="budget of the main cpu_baseline sample (rank 0, N=1 only)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-frontend", action="store_true", help="skip the RGB-D front end side leg")
    ap.add_argument("--no-side-legs", action="store_true", help="with --full: timed region + roofline only (profiling runs)")
    ap.add_argument("--saturation-batch", type=int, default=256,
                    help="side leg: distinct pairs per call with the tail of a call amortised (0 = skip)")
    ap.add_argument("--config4-points", type=int, default=20000, help="N = M of the BASELINE configs[4] leg")
    ap.add_argument("--config4-count", type=int, default=8, help="concurrent registrations per GPU of that leg")
    ap.add_argument("--sharded-points", type=int, default=200000)
    ap.add_argument("--sharded-steps", type=int, default=2)
    ap.add_argument("--sharded-timeout", type=int, default=240, help="watchdog of the sharded leg, seconds")
    ap.add_argument("--sharded-exchange", default="mailbox", choices=["mailbox", "rccl"])
    ap.add_argument("--roofline-only", action="store_true",
                    help="run the roofline leg alone (one engine of --roofline-pairs registrations) and print its "
                         "object: the command rocprofv3 is run on for profiles/*_kernel_stats_roofline.csv")
    ap.add_argument("--roofline-pairs", type=int, default=22,
                    help="registrations in the single engine of the roofline leg (an engine of the timed region holds 21-22)")
    ap.add_argument("--force-sharded-leg", action="store_true",
                    help="run the sharded leg even on one GPU (world size 1): exercises the "
                         "multi-rank code path where only one GPU is available")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def respawn_under_torchrun(gpus, torch):
    """`python bench.py --gpus N` without a launcher: run
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same arguments>`
    (the driver's command for N > 1) as a child and exit with its status, so that both launch conventions
    run the same ranks.  A child, not exec: this process has initialised the GPU already, and replacing
    such a process's program can take the GPU driver down."""
    on_dev0 = os.environ.get("CVO_BENCH_RANKS_ON_DEVICE0", "") not in ("", "0")
    have = torch.cuda.device_count()
    if have < gpus and not on_dev0:
        raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s) "
                         "(CVO_BENCH_RANKS_ON_DEVICE0=1 rehearses N ranks on device 0)" % (gpus, have))
    import socket
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            port = str(s.getsockname()[1])
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL and the mailbox handles need it
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    sys.stderr.flush()
    import subprocess
    rc = subprocess.call(cmd)
    raise SystemExit(rc if rc >= 0 else 128 - rc)   # (a launcher killed by a signal: the shell's 128 + signal)


def pair_seed(pkg, i):
    return pkg.data.SEED_CFG2 if i == 0 else pkg.data.SEED_CFG5_BASE + i


def dump_outputs(path, pkg, its, states):
    """What a caller of align_many received from the last timed step, registrations in batch order: the
    iteration counts (`iterations.npy`) and every field of the final states (`<field>.npy`: R as B x 3 x 3,
    the transforms as B x 4 x 4).  The inputs are seeded, so two builds can be compared file for file."""
    import ctypes
    os.makedirs(path, exist_ok=True)
    arrays = {"iterations": np.array(its, np.float64)}
    shapes = {"R": (3, 3), "transform": (4, 4), "prev_transform": (4, 4), "accum_transform": (4, 4)}
    for name, ctype in pkg.capi.State._fields_:
        if name == "pad_":
            continue
        dtype = np.float64 if ctype is ctypes.c_int32 else np.float32
        a = np.array([np.array(getattr(s, name), dtype) for s in states])
        arrays[name] = a.reshape((len(states),) + shapes.get(name, a.shape[1:]))
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # A bare `python bench.py --gpus N`: become the launcher the driver's other convention uses --
        # one process per GPU under torch.distributed.run on this node, rendezvous on 127.0.0.1.
        respawn_under_torchrun(args.gpus, torch)
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: they must agree" % (args.gpus, world))
    # Rehearsal of the multi-GPU run where only one GPU is to be had (CVO_BENCH_RANKS_ON_DEVICE0=1): every
    # rank works on device 0, torch's collectives go through gloo (RCCL refuses two ranks on one device) --
    # the weak-scaling leg, the all_gather of the IPC handles, the mailbox leg with its RCCL fall-back
    # decision, the watchdog and the assembly of the line all run as they will on 8 GPUs.
    on_dev0 = os.environ.get("CVO_BENCH_RANKS_ON_DEVICE0", "") not in ("", "0")
    if on_dev0:
        local_rank = 0
    backend = "gloo" if on_dev0 else "nccl"
    red_dev = "cpu" if on_dev0 else "cuda"
    torch.cuda.set_device(local_rank)
    if world == 1 and args.force_sharded_leg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if on_dev0:
            dist.init_process_group(backend, rank=0, world_size=1)
        else:
            dist.init_process_group(backend, rank=0, world_size=1, device_id=torch.device("cuda", local_rank))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if on_dev0:
            dist.init_process_group(backend, rank=rank, world_size=world)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))

    pkg = ge.load_package()
    capi = pkg.capi
    acvo = args.mode == "acvo"
    mode = capi.MODE_ACVO if acvo else capi.MODE_CVO
    n = m = args.points
    B = max(1, args.batch)
    if args.roofline_only:
        print(json.dumps(roofline_engine_leg(args, pkg, torch, mode, acvo, n, m)), flush=True)
        return None
    # every rank registers its own frame pairs: `batch` contexts, one stream each.  This process
    # issues HIP work from this one thread only, so the contexts may capture their batches of
    # iterations into hipGraphs although the streams are torch's (cvo_hip_set_graph_capture).
    pairs = [pkg.data.synthetic_pair(n, m, seed=pair_seed(pkg, 0 if args.identical else i), acvo=acvo)
             for i in range(B)]
    streams = [torch.cuda.Stream() for _ in range(B)]
    ctxs = []
    for b in range(B):
        c = capi.Context(mode=mode, device=local_rank, stream=streams[b].cuda_stream, graph_capture=True)
        c.set_fixed(pairs[b][0], pairs[b][1])
        c.set_moving(pairs[b][2], pairs[b][3])
        ctxs.append(c)
    ctx = ctxs[0]

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def one_step(cs):
        states = [capi.init_state(c.params) for c in cs]
        its = capi.align_many(cs, states)
        return its, states

    for _ in range(args.warmup):
        one_step(ctxs)
    # The interpreter's cyclic collector walks every object torch has created (35 ms when a full
    # pass falls into a step: a pause of this harness, not of the path measured): collect now,
    # keep it off while the steps are timed.
    import gc
    gc.collect()
    gc.disable()
    barrier()
    t0 = time.perf_counter()
    iters = 0
    last_states, last_its = None, None
    for _ in range(args.steps):
        its, states = one_step(ctxs)
        iters += sum(its)
        last_states, last_its = states, its
    barrier()
    elapsed = time.perf_counter() - t0
    # (left off for the side legs below as well; the process ends after them)

    t_max = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
    it_sum = torch.tensor([float(iters)], dtype=torch.float64, device=red_dev)
    if world > 1:
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        dist.all_reduce(it_sum, op=dist.ReduceOp.SUM)
    elapsed = float(t_max.item())
    total_regs = args.steps * world * B
    value = total_regs / elapsed
    iters_per_reg = float(it_sum.item()) / total_regs

    out = None
    if rank == 0:
        xf, ff, xm, fm = pairs[0]
        out = {
            "metric": "frame-pair registrations/sec",
            "value": value,
            "unit": "registrations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed * 1e3 / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "ranks_on_device0": True if on_dev0 else None,
            "config": {
                "workload": "synthetic %dk x %dk RGB-D cloud pairs (xyz + 5-dim colour), %s align() to convergence; "
                            "a step = a batch of %d %s pairs in flight (pair 0 = BASELINE configs[1], seed %d%s)"
                            % (n // 1000, m // 1000, args.mode, B, "identical" if args.identical else "distinct",
                               pkg.data.SEED_CFG2, "" if args.identical else "; pair i = seed 1000 + i"),
                "points_fixed": n, "points_moving": m, "mode": args.mode,
                "pairs_per_sweep": float(n) * m,
                "batch": B, "distinct_pairs": not args.identical,
                "iterations_per_registration_min_max": [int(min(last_its)), int(max(last_its))],
                "parallelism": "%d registrations per align_many call per GPU: 3 engines x 21-22 of 32 slots share their "
                               "kernel launches (blockIdx.z = slot), slots refilled from the batch as registrations stop" % B,
                "graph_capture": "opted in (single-threaded process; default is eager on a caller's stream)",
            },
            "iterations_per_registration": iters_per_reg,
            "ms_per_iteration": elapsed * 1e3 * world / max(float(it_sum.item()), 1.0),
        }
        # two all-pairs sweeps (flow, step size) per iteration, 8 flop per
        # pair test.  The path culls tile pairs, re-uses its neighbour lists across
        # iterations and evaluates the step-size sweep on the members of A only, so this
        # is an EQUIVALENT rate (work the reference's dense formulation would do / time).
        sweep_flop_per_iter = 2.0 * FLOP_PER_PAIR * float(n) * m
        out["equivalent_sweep_rate"] = {
            "definition": "2 sweeps x 8 flop x N x M per iteration / time (SURVEY 8d b); may exceed the f32 peak: "
                          "most pair tests are proven unnecessary, not executed",
            "batched_TFLOPs": sweep_flop_per_iter * float(it_sum.item()) / elapsed / 1e12,
            "peak_TFLOPs": PEAK_F32_TFLOPS}
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, pkg, last_its, last_states)

    if rank == 0 and args.full:
        # ---- one registration at a time (latency view): the configs[1] pair on context 0, through
        # cvo_hip_align -- the call a sequential VO loop makes (ref src/cvo.cpp:361-420), BASELINE configs[1] read
        # literally.  Under N ranks: rank 0's GPU, the others wait at the next barrier.  The figures also go into
        # `config` (the part of the line the driver keeps whole).
        def lone():
            st = capi.init_state(ctx.params)
            k, _ = ctx.align(st, trace_cap=0)
            return [k], [st]
        for _ in range(2):
            lone()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        it1 = 0
        n1 = max(5, args.steps)
        for _ in range(n1):
            its, st1 = lone()
            it1 += its[0]
        torch.cuda.synchronize()
        el1 = time.perf_counter() - t1
        out["single_stream"] = {"registrations_per_s": n1 / el1, "ms_per_registration": el1 * 1e3 / n1,
                                "ms_per_iteration": el1 * 1e3 / max(it1, 1), "iterations": it1 / n1,
                                "pair": "BASELINE configs[1] (seed %d)" % pkg.data.SEED_CFG2,
                                "resident_runs": dict(zip(("runs", "declined", "iterations_inside", "candidates_of_last_record"), ctx.run_stats()))}
        out["config"]["one_registration_at_a_time"] = {
            "what": "BASELINE configs[1] literally: one %dk x %dk pair, cvo_hip_align to convergence, nothing else on the GPU "
                    "(`value` is %d distinct pairs in flight per GPU)" % (n // 1000, m // 1000, B),
            "registrations_per_s": out["single_stream"]["registrations_per_s"],
            "ms_per_iteration": out["single_stream"]["ms_per_iteration"],
            "iterations": out["single_stream"]["iterations"]}
        out["equivalent_sweep_rate"]["single_stream_TFLOPs"] = \
            sweep_flop_per_iter / (out["single_stream"]["ms_per_iteration"] * 1e-3) / 1e12
        gpu_state0, gpu_iters0 = st1[0], its[0]
    if rank == 0 and world == 1 and args.full:
        # ---- the path that produced `value`, checked in this run: every registration of the last timed
        # step (engines, 32-slot tables, candidate lists) against the same pair registered on its own
        # (cvo_hip_align), bit for bit; four of them against the oracle in the cpu leg below
        lone_equal, lone_diff = 0, []
        for b, c in enumerate(ctxs):
            st_l = capi.init_state(c.params)
            n_l, _ = c.align(st_l, trace_cap=0)
            if bytes(st_l) == bytes(last_states[b]) and n_l == last_its[b]:
                lone_equal += 1
            else:
                lone_diff.append(b)
        batched_parity = {"registrations": B, "bit_identical_to_lone_cvo_hip_align": lone_equal,
                          "differing": lone_diff[:8],
                          "what": "the %d final states (R, T, ell, transforms, iter) and iteration counts of the last timed "
                                  "align_many step vs cvo_hip_align of the same pair on the same context" % B}
        out.update(roofline_legs(args, pkg, ctx, ctxs, one_step, n, m))
        if not args.no_side_legs:
            try:
                ho = handover_leg(args, pkg, ctxs, pairs, one_step, torch)
                out["value_including_set_pcd"] = ho["registrations_per_s"]
                out["value_including_set_pcd_over_value"] = ho["registrations_per_s"] / value
                out["config"]["value_including_set_pcd"] = ho["registrations_per_s"]
                out["hand_over"] = ho
            except Exception as e:
                out["value_including_set_pcd"] = None
                out["hand_over"] = {"error": repr(e)}
        if not args.no_side_legs:
            try:
                out["identical_pairs"] = identical_leg(args, pkg, ctxs, pairs[0], one_step, torch)
            except Exception as e:
                out["identical_pairs"] = {"error": repr(e)}
        for c in ctxs:   # (dozens of idle streams slow every other stream's submissions down)
            c.close()
        ctxs = []
        if not args.no_side_legs:
            try:
                out["small_calls"] = small_calls_leg(args, pkg, torch, mode, acvo)
            except Exception as e:
                out["small_calls"] = {"error": repr(e)}
        if not args.no_side_legs and args.saturation_batch > B:
            try:
                out["saturation"] = saturation_leg(args, pkg, torch, mode, acvo, n, m)
            except Exception as e:
                out["saturation"] = {"error": repr(e)}
        if not args.no_side_legs:
            try:
                out["roofline"].update(roofline_engine_leg(args, pkg, torch, mode, acvo, n, m))
            except Exception as e:
                out["roofline"]["engine_leg_error"] = repr(e)
            if not acvo:
                try:   # the mode of BASELINE configs[2] (ref src/adaptive_cvo.cpp:490-555), same batch shape
                    out["acvo"] = mode_leg(args, pkg, torch, capi.MODE_ACVO, True, n, m, B)
                except Exception as e:
                    out["acvo"] = {"error": repr(e)}
            try:
                out["config4"] = config4_leg(args, pkg, torch, mode, acvo)
                out["config"]["config4_registrations_per_s"] = out["config4"]["registrations_per_s"]
            except Exception as e:
                out["config4"] = {"error": repr(e)}
            try:   # the N = 1 point of the strong-scaling curve of BASELINE configs[3]
                out["config3_single_gpu"] = config3_leg(args, pkg, torch, mode, acvo)
            except Exception as e:
                out["config3_single_gpu"] = {"error": repr(e)}
            try:   # ... and what one of eight GPUs would hold
                out["config3_shard_of_8"] = shard_leg(args, pkg, torch, mode, acvo)
                out["config3_projection_8gpu"] = strong_scaling_projection(out["config3_single_gpu"], out["config3_shard_of_8"])
            except Exception as e:
                out["config3_shard_of_8"] = {"error": repr(e)}
            if not args.no_frontend:
                try:
                    out["frontend"] = frontend_leg(args, pkg)
                except Exception as e:   # the headline line must survive a side leg
                    out["frontend"] = {"error": repr(e)}
        try:
            out["roofline_run"] = roofline_run_leg(out.get("single_stream"), (out.get("acvo") or {}).get("single_stream"))
        except Exception as e:
            out["roofline_run"] = {"error": repr(e)}
        # (last: the OpenMP team of the CPU leg keeps spinning for a while after its last
        # parallel region and would slow the host side of everything timed after it)
        if not args.no_cpu:
            cpu, parity = cpu_baseline(args, pkg, xf, ff, xm, fm, acvo, gpu_state0, gpu_iters0)
            out["cpu_baseline"] = cpu
            out["parity_vs_oracle"] = parity
            batched_parity.update(batched_vs_oracle(pkg, pairs, last_states, last_its, acvo, cpu["cores"]))
        out.setdefault("parity_vs_oracle", {})["batched"] = batched_parity
    if world > 1 and args.full and not args.no_side_legs:
        # BASELINE configs[4] IS "64 concurrent 20k x 20k across 8 GPUs": under N ranks every rank runs the leg on its own
        # registrations (collective: all ranks, or none -- an exception on one rank is agreed on before anybody waits)
        import threading
        for c in ctxs:
            c.close()
        ctxs = []

        def give_up4():   # (a rank that fails leaves the others at a barrier: the headline line must still go out)
            if rank == 0:
                out["config4"] = {"error": "timed out after %d s" % args.sharded_timeout}
                emit(out)
            os._exit(0)
        dog4 = threading.Timer(args.sharded_timeout, give_up4)
        dog4.daemon = True
        dog4.start()
        try:
            c4 = config4_leg(args, pkg, torch, mode, acvo, world=world, rank=rank, barrier=barrier, dist=dist, red_dev=red_dev)
        except Exception as e:
            c4 = {"error": repr(e)}
        dog4.cancel()
        if rank == 0:
            out["config4"] = c4
            if "registrations_per_s" in c4:
                out["config"]["config4_registrations_per_s"] = c4["registrations_per_s"]
    # The target-sharded leg runs last and under a watchdog: the headline line above it must
    # not depend on it, not even if an exchange hangs.
    if ((world > 1 and args.full) or args.force_sharded_leg) and args.sharded_steps > 0:
        import threading

        def give_up():
            if rank == 0:
                out["sharded_allreduce"] = {"error": "timed out after %d s" % args.sharded_timeout}
                emit(out)
            os._exit(0)

        for c in ctxs:
            c.close()
        ctxs = []
        if world > 1:
            dist.barrier()
        dog = threading.Timer(args.sharded_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            sharded = sharded_leg(args, pkg, dist, torch, rank, world, local_rank, barrier, red_dev)
        except Exception as exc:
            sharded = {"error": repr(exc)}
        dog.cancel()
        if rank == 0:
            out["sharded_allreduce"] = sharded
    if rank == 0:
        emit(out)
    for c in ctxs:
        c.close()
    if world > 1 or args.force_sharded_leg:
        if world > 1:
            dist.barrier()
        dist.destroy_process_group()
    return out


def committed(name):
    """A summary committed under profiles/ (rocprofv3 cannot run inside this process): the
    value is a constant of the repository, tagged as such in the line."""
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None, None
    try:
        with open(path) as fh:
            return json.load(fh), "committed profiles/" + name
    except Exception:
        return None, None


def roofline_legs(args, pkg, ctx, ctxs, one_step, n, m):
    """Kernel durations measured live: profiling mode = one registration in flight (a launch has
    the device to itself), eager launches, a HIP event pair attached to every dispatch of
    k_filter, k_process<PROC_FLOW> and k_step_twist on the context's own stream."""
    import torch
    # members of A per iteration of this pair (trace of one registration)
    st = pkg.capi.init_state(ctx.params)
    n_it, tr = ctx.align(st, trace_cap=2000)
    members = float(np.mean([t["nnz"] for t in tr])) if tr else 0.0
    ctx.set_profiling(True)
    ctx.get_profile(reset=True)
    regs = max(3, args.steps // 4)
    for _ in range(regs):
        one_step([ctx])
    torch.cuda.synchronize()
    prof = ctx.get_profile(reset=True)
    ctx.set_profiling(False)
    algo_bytes = BYTES_PER_POINT * (n + m)
    pairs = float(n) * m
    pmc, pmc_src = committed("%s_pmc_summary.json" % PROFILE_TAG)
    live, live_src = committed("%s_kernel_live.json" % PROFILE_TAG)
    shares = None
    # (rounds 1-2 named the file ..._batch32.csv; round 4 looked for that name and found nothing)
    sname = "%s_kernel_stats_batch.csv" % PROFILE_TAG
    if not os.path.exists(os.path.join(ROOT, "profiles", sname)):
        sname = "%s_kernel_stats_batch32.csv" % PROFILE_TAG
    spath = os.path.join(ROOT, "profiles", sname)
    if os.path.exists(spath):
        try:
            import csv
            rows = [r for r in csv.DictReader(open(spath)) if "cvo_dev::" in r["Name"]]
            tot = sum(float(r["TotalDurationNs"]) for r in rows)
            top = sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:6]
            shares = {"source": "committed profiles/" + sname}
            shares.update({r["Name"].replace("void ", "").replace("cvo_dev::", "").split("(")[0]:
                           round(float(r["TotalDurationNs"]) / tot, 3) for r in top})
        except Exception:
            shares = None

    def traffic_of(kernel):
        """HBM bytes per launch from the committed PMC passes (FETCH_SIZE in KB, doubled as
        MI355X_MICROARCH.md prescribes for gfx950, + WRITE_SIZE in KB)."""
        if not pmc or kernel not in pmc or "FETCH_SIZE" not in pmc[kernel]:
            return None
        k = pmc[kernel]
        return {"bytes_per_launch": 2.0 * k["FETCH_SIZE"]["avg"] * 1024.0 + k.get("WRITE_SIZE", {}).get("avg", 0.0) * 1024.0,
                "source": pmc_src}

    def rocprof_us(kernel):
        if not live or kernel not in live:
            return None
        return {"avg_launch_us": live[kernel].get("live_avg_us"), "source": live_src}

    rocprof_batch = None   # rocprofv3's average of the same kernel over the same command (committed summary)
    if os.path.exists(spath):
        try:
            import csv
            for r in csv.DictReader(open(spath)):
                if "kt_process<0, 0>" in r["Name"]:
                    rocprof_batch = {"avg_launch_us": float(r["AverageNs"]) / 1e3, "launches": int(r["Calls"]),
                                     "source": "committed profiles/" + sname,
                                     "note": "under the kernel trace a step takes ~1.4x as long and the engines' launches overlap "
                                             "less: a launch has more of the GPU to itself and is shorter than in the timed run"}
        except Exception:
            rocprof_batch = None
    res = {"kernel_time_shares_batched": shares}
    # ---- the kernel that dominates the timed region: the flow pass.  In the timed region one launch of it
    # (kt_process<PROC_FLOW>) serves the up to 32 registrations of an engine: measured on exactly those
    # launches -- the batch once more with engine profiling on (eager launches, a HIP event pair attached
    # to every flow-pass dispatch of the engines' own streams).
    capi = pkg.capi
    capi.engine_profiling(True)
    capi.engine_profile(reset=True)
    if len(ctxs) > 1:
        one_step(ctxs)
    torch.cuda.synchronize()
    e_ms, e_n, e_regs = capi.engine_profile(reset=True)
    capi.engine_profiling(False)
    pf_n = prof["proc_flow_launches"]
    pf_us = prof["proc_flow_ms"] * 1e3 / max(pf_n, 1)
    single_gbs = algo_bytes / (pf_us * 1e-6) / 1e9 if pf_us > 0 else 0.0
    flow_flop = members * (FLOP_PER_MEMBER + 2.0 * 2.0 * F64_OPS_PER_EXP)   # an f64 op priced as 2 flop
    tr_flow = traffic_of("k_process<0, 0>")
    pmc_b, pmc_b_src = committed("%s_pmc_batch.json" % PROFILE_TAG)
    tr_batch = None
    if pmc_b and "kt_process<0, 0>" in pmc_b and "FETCH_SIZE" in pmc_b["kt_process<0, 0>"]:
        kb = pmc_b["kt_process<0, 0>"]
        tr_batch = {"bytes_per_launch": 2.0 * kb["FETCH_SIZE"]["avg"] * 1024.0 + kb.get("WRITE_SIZE", {}).get("avg", 0.0) * 1024.0,
                    "source": pmc_b_src}
    if e_n > 0 and e_ms > 0:
        regs_per_launch = e_regs / e_n
        b_us = e_ms * 1e3 / e_n
        b_bytes = algo_bytes * regs_per_launch
        gbs = b_bytes / (b_us * 1e-6) / 1e9
        how = ("HIP events attached to every flow-pass dispatch of the engines (one more step of the timed batch, "
               "eager launches): %d launches, %.1f registrations per launch on average" % (e_n, regs_per_launch))
    else:   # a batch of one has no engines: the single-stream figure is all there is
        regs_per_launch, b_us, b_bytes, gbs, how = 1.0, pf_us, algo_bytes, single_gbs, "see single_stream_launch"
    res["roofline"] = {
        "kernel": "cvo_dev::kt_process<PROC_FLOW> (exact membership test + kernel weights + flow sums over the candidate "
                  "lists of the registrations of an engine; the largest share of the GPU time of the timed region)",
        "bound": "hbm",
        "bound_note": "the roof `frac` is quoted against (the contract's algorithmic bytes over 8 TB/s).  It is NOT what limits the "
                      "kernel: see limited_by and by_phase",
        "limited_by": "dependent latency while the kernel is wide (one gather round trip per 64 candidates and wave; vector issue ~0.5, "
                      "4 of 6 waves per SIMD resident, each waiting ~3/4 of its cycles, L2 hit rate 0.66: profiles/r04_ab.txt 8, 14), "
                      "the chain of dependent launches while it is narrow",
        "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
        "algorithmic_bytes_per_launch": b_bytes,
        "bytes_definition": "32 B x (N + M) points read once per sweep (SURVEY 8d) x the registrations the launch serves",
        "registrations_per_launch": regs_per_launch,
        "avg_launch_us": b_us, "launches": e_n if e_n > 0 else pf_n,
        "measured": how,
        "rocprofv3": rocprof_batch,
        "frac_at_rocprofv3_duration": (b_bytes / (rocprof_batch["avg_launch_us"] * 1e-6) / 1e9 / PEAK_HBM_GBS)
                                      if rocprof_batch and rocprof_batch["avg_launch_us"] > 0 else None,
        "traffic": tr_batch["bytes_per_launch"] if tr_batch else None,
        "traffic_source": tr_batch["source"] if tr_batch else None,
        "traffic_note": "PMC FETCH_SIZE x 2 + WRITE_SIZE per launch of the batched run (launches of every occupancy averaged)",
        "single_stream_launch": {
            "kernel": "cvo_dev::k_process<PROC_FLOW>, one registration per launch",
            "avg_launch_us": pf_us, "launches": pf_n, "achieved_GBs": single_gbs, "frac": single_gbs / PEAK_HBM_GBS,
            "algorithmic_bytes_per_launch": algo_bytes,
            "measured": "HIP events attached to every dispatch of %d single-stream registrations of the configs[1] pair" % regs,
            "rocprofv3": rocprof_us("k_process<0, 0>"),
            "traffic": tr_flow["bytes_per_launch"] if tr_flow else None,
            "traffic_source": tr_flow["source"] if tr_flow else None,
            "members_of_A_per_launch": members},
        "valu_view": {"flop_per_launch": flow_flop * regs_per_launch,
                      "definition": "members of A x (45 flop + 2 exp x 14 float64 ops x 2), SURVEY 8d per surviving pair, "
                                    "members counted on the configs[1] pair",
                      "achieved_TFLOPs": flow_flop * regs_per_launch / (b_us * 1e-6) / 1e12 if b_us > 0 else 0.0,
                      "peak_TFLOPs": PEAK_F32_TFLOPS,
                      "frac": (flow_flop * regs_per_launch / (b_us * 1e-6) / 1e12 / PEAK_F32_TFLOPS) if b_us > 0 else 0.0},
        "reading": "the algorithmic bytes are the two clouds; what the pass does is evaluate ~1e5-1e6 candidate pairs per "
                   "registration at ~85 vector instructions per 64 of them (float32 geometry, a float64 exp, six float64 sums) "
                   "and write the members of A out for the step pass. It is at neither roof: in the wide iterations vector "
                   "issue is ~0.5 busy and the counter traffic ~0.5 of what HBM delivers (by_phase); a round of 64 candidates is "
                   "one dependent chain (record, two gathers, arithmetic, store) and a wave waits ~3/4 of its life for it. "
                   "Round 4 arranged the loop so that the chain holds only data dependences and the next record is in flight "
                   "during the arithmetic (+5...+9 % batched); deeper pipelines, more waves, staged stores all lose "
                   "(profiles/r04_ab.txt 15-20, DESIGN 4.2)",
    }
    # ---- the all-pairs test: k_filter (f32 MFMA), launches that build a list
    kf_n = prof["flow_launches"]
    kf_us = prof["flow_ms"] * 1e3 / max(kf_n, 1)
    kf_tf = FLOP_PER_PAIR * pairs / (kf_us * 1e-6) / 1e12 if kf_us > 0 else 0.0
    tr_f = traffic_of("k_filter")
    res["roofline_filter"] = {
        "kernel": "cvo_dev::k_filter (all target x source pair tests, v_mfma_f32_16x16x4_f32)",
        "bound": "mfma", "pipe": "f32 MFMA issue (f32 MFMA peak == f32 vector peak on gfx950)",
        "achieved": kf_tf, "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": kf_tf / PEAK_F32_TFLOPS,
        "flop_per_launch": FLOP_PER_PAIR * pairs,
        "flop_definition": "8 flop x N x M pair tests (SURVEY 8d; N x M = %.3g, padding not counted); an EQUIVALENT "
                           "rate: tile pairs whose bounding spheres are out of reach are never tested" % pairs,
        "avg_launch_us": kf_us, "launches": kf_n,
        "launches_note": "k_filter works only in the iterations that rebuild the tile list (%.1f per registration "
                         "here); the other launches return at once and are not counted" % (kf_n / float(regs)),
        "measured": "HIP events attached to the dispatches, same registrations as above",
        "rocprofv3": rocprof_us("k_filter"),
        "traffic": tr_f["bytes_per_launch"] if tr_f else None,
        "traffic_source": tr_f["source"] if tr_f else None,
        "algorithmic_bytes_per_launch": algo_bytes,
    }
    st_n = prof["step_launches"]
    res["step_kernel"] = {"kernel": "cvo_dev::k_step_twist (twist from the flow partials + step-size sums over A)",
                          "avg_launch_us": prof["step_ms"] * 1e3 / max(st_n, 1), "launches": st_n,
                          "algorithmic_bytes_per_launch": 12.0 * members + algo_bytes,
                          "rocprofv3": rocprof_us("k_step_twist")}
    return res


def roofline_engine_leg(args, pkg, torch, mode, acvo, n, m):
    """The roofline object's own measurement: ONE engine holding `--roofline-pairs` (22) distinct pairs --
    what each of the three engines of the timed region holds -- with a HIP event pair attached to every
    flow-pass dispatch (kt_process<PROC_FLOW>) on the engine's stream.  With one engine no other stream
    contends for the GPU, so the dispatch durations are the kernel's own and agree with rocprofv3's of the
    same command (`bench.py --roofline-only`, committed as profiles/<tag>_kernel_stats_roofline.csv); in the
    timed region three such launch sequences overlap and a launch takes about twice as long (`in_timed_region`).
    Units per launch = registrations that execute in it = (sum of the iterations of the call) / launches."""
    import csv
    capi = pkg.capi
    count = max(2, args.roofline_pairs)
    ctxs, streams = [], []
    for i in range(count):
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pair_seed(pkg, i), acvo=acvo)
        st = torch.cuda.Stream()
        c = capi.Context(mode=mode, device=torch.cuda.current_device(), stream=st.cuda_stream, graph_capture=True)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c)
        streams.append(st)
    ctxs[0].set_option("engines", 1)   # (a call goes by its first context's switches)
    try:
        def step():
            states = [capi.init_state(c.params) for c in ctxs]
            return capi.align_many(ctxs, states)
        step()
        torch.cuda.synchronize()
        capi.engine_profiling(True)
        capi.engine_profile(reset=True)
        reps, its = max(3, args.steps // 4), 0
        # per phase of the loop (cvo: the length scale is a function of the iteration, ref src/cvo.cpp:408-410 --
        # ell = 0.15 in iterations 0-3, 0.10 in 4-10, 0.06 in 11-20, 0.03 from 21 on; every registration of a call
        # starts at iteration 0 together, so the i-th flow launch of a call IS iteration i)
        phases = {}
        for _ in range(reps):
            capi.engine_flow_trace(reset=True)
            its_call = step()
            its += sum(its_call)
            torch.cuda.synchronize()
            dur, per, _sl = capi.engine_flow_trace(reset=True)
            for i in range(len(dur)):
                running = sum(1 for k in its_call if k > i)
                if running == 0:
                    continue
                name = "all" if acvo else ("ell_0.15" if i < 4 else "ell_0.10" if i < 11 else "ell_0.06" if i < 21 else "ell_0.03")
                ph = phases.setdefault(name, {"launches": 0, "us": 0.0, "registrations": 0, "period_us": 0.0, "periods": 0})
                ph["launches"] += 1
                ph["us"] += float(dur[i])
                ph["registrations"] += running
                if per[i] > 0.0 and i + 1 < len(dur):
                    ph["period_us"] += float(per[i])
                    ph["periods"] += 1
        e_ms, e_n, e_slots = capi.engine_profile(reset=True)
        capi.engine_profiling(False)
    finally:
        for c in ctxs:
            c.close()
    algo_bytes = BYTES_PER_POINT * (n + m)
    regs_per_launch = its / float(max(e_n, 1))
    us = e_ms * 1e3 / max(e_n, 1)
    b_bytes = algo_bytes * regs_per_launch
    gbs = b_bytes / (us * 1e-6) / 1e9 if us > 0 else 0.0
    res = {"achieved": gbs, "frac": gbs / PEAK_HBM_GBS, "algorithmic_bytes_per_launch": b_bytes,
           "registrations_per_launch": regs_per_launch, "slots_per_launch": e_slots / float(max(e_n, 1)),
           "avg_launch_us": us, "launches": int(e_n),
           "measured": "HIP events attached to every flow-pass dispatch of ONE engine holding %d distinct pairs (%d align_many "
                       "calls, eager launches): %d launches; units per launch = iterations executed / launches = %.2f registrations"
                       % (count, reps, e_n, regs_per_launch)}
    spath = os.path.join(ROOT, "profiles", "%s_kernel_stats_roofline.csv" % PROFILE_TAG)
    if os.path.exists(spath):
        try:
            for r in csv.DictReader(open(spath)):
                if "kt_process<0, 0>" in r["Name"]:
                    ru = float(r["AverageNs"]) / 1e3
                    res["rocprofv3"] = {"avg_launch_us": ru, "launches": int(r["Calls"]),
                                        "source": "committed profiles/%s_kernel_stats_roofline.csv" % PROFILE_TAG,
                                        "command": "rocprofv3 --kernel-trace --stats -- python bench.py --roofline-only"}
                    res["frac_at_rocprofv3_duration"] = b_bytes / (ru * 1e-6) / 1e9 / PEAK_HBM_GBS if ru > 0 else None
        except Exception:
            pass
    valu, valu_src = committed("%s_valu.json" % PROFILE_TAG)
    if valu:
        res["valu_issue_frac"] = valu.get("valu_issue_frac")
        res["valu_issue"] = dict(valu, source=valu_src)
    ph, ph_src = committed("%s_pmc_phases.json" % PROFILE_TAG)
    pmc = ph.get("kt_process<0, 0>") if ph else None
    if pmc:
        res["traffic"] = pmc.get("all", {}).get("hbm_bytes_per_launch")
        res["traffic_source"] = ph_src
        res["traffic_note"] = ("PMC FETCH_SIZE x 2 + WRITE_SIZE per launch, the SAME launches in both passes and in the kernel "
                               "trace (one engine of %d pairs: the k-th dispatch of a pass is the k-th of the others)" % count)
        res["traffic_by_length_scale"] = {kk: vv for kk, vv in pmc.items() if kk != "all"}
    # ---- one bound with one number per phase: the heavy iterations (ell >= 0.06) are
    # throughput-bound -- counter bytes of the SAME launches (committed PMC passes of this command) over the
    # duration measured live here, against what HBM delivers; the light ones (ell = 0.03) are bound by the
    # engine's chain of dependent launches -- the live period from one flow launch to the next.
    ACHIEVABLE_HBM_GBS = 6300.0   # MI355X_MICROARCH.md: what a streaming kernel reaches of the 8 TB/s

    def phase_obj(names):
        sel = [phases[k] for k in names if k in phases]
        if not sel:
            return None
        ln = sum(p["launches"] for p in sel)
        us = sum(p["us"] for p in sel) / max(ln, 1)
        regs = sum(p["registrations"] for p in sel) / float(max(ln, 1))
        prd = sum(p["period_us"] for p in sel) / max(sum(p["periods"] for p in sel), 1)
        o = {"launches": ln, "avg_launch_us": us, "registrations_per_launch": regs, "iteration_period_us": prd,
             "algorithmic_GBs": algo_bytes * regs / (us * 1e-6) / 1e9 if us > 0 else None}
        if pmc:   # counter bytes per launch of the same phases, weighted by their launches in the committed passes
            tot_b = tot_l = 0.0
            for k in names:
                if k in pmc and isinstance(pmc[k], dict) and pmc[k].get("launches"):
                    tot_b += pmc[k]["hbm_bytes_per_launch"] * pmc[k]["launches"]
                    tot_l += pmc[k]["launches"]
            if tot_l:
                o["counter_bytes_per_launch"] = tot_b / tot_l
                o["counter_GBs"] = tot_b / tot_l / (us * 1e-6) / 1e9 if us > 0 else None
                o["frac_of_achievable_hbm"] = o["counter_GBs"] / ACHIEVABLE_HBM_GBS if o["counter_GBs"] else None
        return o
    if acvo:
        res["by_phase"] = {"all": phase_obj(["all"])}
    else:
        heavy = phase_obj(["ell_0.15", "ell_0.10", "ell_0.06"])
        light = phase_obj(["ell_0.03"])
        sq, sq_src = committed("%s_sq_phases.json" % PROFILE_TAG)   # (per-phase SQ counters of the same command, where collected)
        if heavy:
            heavy["bound"] = "dependent-latency"
            heavy["what"] = ("iterations 0-20 (ell >= 0.06): the streaming flow pass waits for one gather round trip per round of 64 "
                             "candidates and wave -- vector instructions issue 44-52 %% of the time, 3.8-4.4 of 6 waves per SIMD are "
                             "resident and each waits 73-79 %% of its cycles, L2 hit rate 0.66, texture addresser 4-6 %% busy "
                             "(profiles/r04_ab.txt 8, 14).  counter_GBs = FETCH_SIZE x 2 + WRITE_SIZE of the same launches (committed %s) "
                             "over the live duration: FETCH_SIZE counts Infinity-Cache hits too and one engine's working set fits that "
                             "cache, so this is a traffic figure at the L2's far side, not an HBM roof (calibration: %s)"
                             % (ph_src or "profiles/%s_pmc_phases.json" % PROFILE_TAG, FETCH_CALIBRATION))
            heavy["step_pass"] = {"bound": "valu-issue", "issue_frac_by_length_scale": {"ell_0.15": 0.86, "ell_0.10": 0.81, "ell_0.06": 0.71},
                                  "source": (sq_src or "profiles/r04_ab.txt 8")}
        if light:
            light["bound"] = "launch-chain"
            light["launches_per_iteration"] = 5
            light["chain_us"] = light["iteration_period_us"]
            light["what"] = ("iterations 21+ (ell = 0.03): an iteration of the engine = its chain of five dependent launches (filter, "
                             "flow, post-flow, step, post-step); chain_us = live time from one flow launch's begin to the next one's")
        res["by_phase"] = {"heavy": heavy, "light": light,
                           "per_length_scale": {k: phase_obj([k]) for k in sorted(phases)}}
    res["bound_note"] = ("per phase: see by_phase (wide flow pass: dependent-latency, wide step pass: valu-issue, narrow: launch-chain); "
                         "`frac` is the contract's algorithmic-bytes figure against the HBM roof")
    return res


def roofline_run_leg(single_stream, acvo_single):
    """The resident runs (csrc/cvo_kernels.hip kt_run / kt_run_acvo: 57 % of the kernel time of one registration at a time): no HBM roof
    and no MFMA roof applies -- an iteration inside a run touches no memory at all --, so the entry says what fraction of the GPU's
    vector issue the kernel uses while it runs (committed SQ_ACTIVE_INST_VALU x 4 cycles / (1024 SIMDs x the kernel's cycles)) and where
    an iteration's time goes (committed ticks of a -DCVO_RUN_CLOCKS build): the two exchanges and the head's chain, not arithmetic."""
    pmc, pmc_src = committed("%s_pmc_summary.json" % PROFILE_TAG)
    clk, clk_src = committed("%s_run_clocks.json" % PROFILE_TAG)
    out = {"kernel": "cvo_dev::kt_run", "bound": "latency", "unit": "fraction of vector issue", "peak": 1.0,
           "what": "vector-issue fraction while the kernel runs; per-iteration microseconds by phase from a clocked build"}
    k = (pmc or {}).get("single_stream", {}).get("kt_run") if pmc else None
    if k and "SQ_ACTIVE_INST_VALU" in k and "GRBM_GUI_ACTIVE" in k:
        cyc = k["GRBM_GUI_ACTIVE"]["avg"] / 8.0
        out["achieved"] = out["frac"] = k.get("valu_active_frac", k["SQ_ACTIVE_INST_VALU"]["avg"] * 4.0 / (1024.0 * cyc))
        out["avg_launch_us"] = cyc / 2400.0
        out["launches"] = k["SQ_ACTIVE_INST_VALU"]["executed"]
        out["source"] = pmc_src
    ka = (pmc or {}).get("single_stream_acvo", {}).get("kt_run_acvo") if pmc else None
    if ka and "SQ_ACTIVE_INST_VALU" in ka and "GRBM_GUI_ACTIVE" in ka:
        out["acvo_frac"] = ka.get("valu_active_frac", ka["SQ_ACTIVE_INST_VALU"]["avg"] * 4.0 / (1024.0 * ka["GRBM_GUI_ACTIVE"]["avg"] / 8.0))
    if clk:
        c = clk.get("clocks", {})
        for mode in ("cvo", "acvo"):
            for n in ("n_3000", "n_10000"):
                e = c.get(mode, {}).get(n)
                if not e or "ticks_by_phase" not in e:
                    continue
                ph = e["ticks_by_phase"]
                t = lambda *names: sum(ph.get(x, 0) for x in names) / 2400.0
                key = "%s_%s" % (mode, n[2:])
                out["us_per_iteration_" + key] = e.get("us_per_run_iteration")
                out["by_phase_us_" + key] = {"passes": t("flow rounds", "step rounds"), "sums_and_barriers": t("wave sums", "barrier+block sum", "step sums"),
                                             "exchanges": t("exch A", "exch B"), "twist_constants": t("twist", "consts"),
                                             "head_chain": t("pre-head", "head_post", "inverse+sync", "tail"),
                                             "entry_per_run": ph.get("entry", 0) / 2400.0}
        out["clocks_source"] = clk_src
        if "us_per_iteration_cvo_10000" in out:
            out["us_per_iteration"] = out["us_per_iteration_cvo_10000"]
    if single_stream:
        out["measured_ms_per_iteration_one_at_a_time"] = single_stream.get("ms_per_iteration")
    return out


def handover_leg(args, pkg, ctxs, pairs, one_step, torch):
    """`value` with row a1's work inside the timed region: every step first hands both clouds of every pair over
    again from host memory (the tail of set_pcd(), ref src/cvo.cpp:344-356: PCIe, bounding box, Morton keys, sort,
    packed rows, bounding spheres), then registers the batch.  Two ways: the whole batch in one call
    (cvo_hip_set_pcd_many: staged by the library in pieces, one transfer and one launch per piece) -- the
    headline --, and one cvo_hip_set_fixed / _set_moving call per cloud (one launch each)."""
    capi = pkg.capi
    steps = max(3, args.steps // 4)
    fixed = [(np.ascontiguousarray(p[0], np.float32), np.ascontiguousarray(p[1], np.float32)) for p in pairs]
    moving = [(np.ascontiguousarray(p[2], np.float32), np.ascontiguousarray(p[3], np.float32)) for p in pairs]

    def per_call():
        for c, pr in zip(ctxs, pairs):
            c.set_fixed(pr[0], pr[1])
            c.set_moving(pr[2], pr[3])

    def timed(hand_over):
        hand_over()
        one_step(ctxs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t_ho = 0.0
        for _ in range(steps):
            t1 = time.perf_counter()
            hand_over()
            t_ho += time.perf_counter() - t1
            one_step(ctxs)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return {"registrations_per_s": steps * len(ctxs) / el, "ms_per_step": el * 1e3 / steps,
                "host_ms_in_the_hand_over_calls": t_ho * 1e3 / steps}
    out = {"steps": steps,
           "includes": "both clouds of every pair handed over from host memory in every step, then the batch registered",
           "batched": timed(lambda: capi.set_pcd_many(ctxs, fixed, moving)),
           "one_call_per_cloud": timed(per_call)}
    out["registrations_per_s"] = out["batched"]["registrations_per_s"]
    out["ms_per_step"] = out["batched"]["ms_per_step"]
    return out


def mode_leg(args, pkg, torch, mode, acvo, n, m, count):
    """The timed region's batch shape in the other mode (acvo: the mode of BASELINE configs[2])."""
    capi = pkg.capi
    ctxs, streams = [], []
    for i in range(count):
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pair_seed(pkg, i), acvo=acvo)
        st = torch.cuda.Stream()
        c = capi.Context(mode=mode, device=torch.cuda.current_device(), stream=st.cuda_stream, graph_capture=True)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c)
        streams.append(st)

    def step():
        states = [capi.init_state(c.params) for c in ctxs]
        return capi.align_many(ctxs, states)
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.4:
        step()
    torch.cuda.synchronize()
    steps, it = max(3, args.steps // 4), 0
    t0 = time.perf_counter()
    for _ in range(steps):
        it += sum(step())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # one at a time (the reference's use: a sequential VO loop)
    c0 = ctxs[0]
    for _ in range(2):
        c0.align(capi.init_state(c0.params), trace_cap=0)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n1, it1 = 8, 0
    for _ in range(n1):
        k, _ = c0.align(capi.init_state(c0.params), trace_cap=0)
        it1 += k
    torch.cuda.synchronize()
    el1 = time.perf_counter() - t1
    for c in ctxs:
        c.close()
    return {"workload": "%d distinct %dk x %dk pairs per align_many call, %s" % (count, n // 1000, m // 1000, "acvo" if acvo else "cvo"),
            "registrations_per_s": steps * count / el, "ms_per_step": el * 1e3 / steps,
            "iterations_per_registration": it / float(steps * count), "steps": steps,
            "single_stream": {"registrations_per_s": n1 / el1, "ms_per_registration": el1 * 1e3 / n1,
                              "ms_per_iteration": el1 * 1e3 / max(it1, 1), "iterations": it1 / float(n1)}}


def per_length_scale_ms(c, capi, torch, caps=(4, 11, 21, 40)):
    """ms per iteration of context c's registration in each phase of the cvo length-scale schedule (ell changes at the END of
    iterations 3, 10, 20, ref src/cvo.cpp:408-410): the registration stopped after 4 / 11 / 21 / 40 iterations (max_iter),
    differences of the times.  The first window carries the call's fixed cost."""
    import copy
    base = copy.copy(c.params)
    names = ("ell_0.15", "ell_0.10", "ell_0.06", "ell_0.03")
    res, prev_it, prev_ms = {}, 0, 0.0
    for cap, name in zip(caps, names):
        p = copy.copy(base)
        p.max_iter = cap
        c.set_params(p)
        c.align(capi.init_state(c.params), trace_cap=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k, _ = c.align(capi.init_state(c.params), trace_cap=0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if k > prev_it:
            res[name] = {"iterations": [prev_it, k - 1], "ms_per_iteration": (ms - prev_ms) / (k - prev_it)}
        prev_it, prev_ms = k, ms
    c.set_params(base)
    return res


def config3_leg(args, pkg, torch, mode, acvo):
    """BASELINE configs[3] on ONE GPU: a single 200k x 200k registration (the N = 1 point of the strong-scaling
    curve of the sharded leg)."""
    capi = pkg.capi
    n = m = args.sharded_points
    xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pkg.data.SEED_CFG4, acvo=acvo)
    c = capi.Context(mode=mode, device=torch.cuda.current_device(), graph_capture=True)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    c.align(capi.init_state(c.params), trace_cap=0)
    torch.cuda.synchronize()
    reps, it = 2, 0
    t0 = time.perf_counter()
    for _ in range(reps):
        k, _ = c.align(capi.init_state(c.params), trace_cap=0)
        it += k
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"workload": "one synthetic %dk x %dk registration (BASELINE configs[3], seed %d), unsharded" % (n // 1000, m // 1000, pkg.data.SEED_CFG4),
           "registrations_per_s": reps / el, "ms_per_registration": el * 1e3 / reps,
           "ms_per_iteration": el * 1e3 / max(it, 1), "iterations": it / float(reps),
           "pairs_per_sweep": float(n) * m}
    if not acvo:
        try:   # the same iteration windows as config3_shard_of_8 (like against like)
            out["per_length_scale"] = per_length_scale_ms(c, capi, torch)
        except Exception as e:
            out["per_length_scale"] = {"error": repr(e)}
    # ---- the roofline of this size: the heavy iterations (0-20, ell >= 0.06) are the kept list -- every member of A
    # written by the flow pass (8 B) and read back by the step pass (8 B) -- on top of the tile list the flow pass
    # expands (16 B per entry) and the gathers; durations by HIP events on every dispatch (profiling mode: the
    # by-value launches of the same kernel bodies), members per iteration from the trace of the same run
    try:
        import copy
        prm = copy.copy(c.params)
        heavy_iters = 21
        prm.max_iter = heavy_iters
        c.set_params(prm)
        c.set_profiling(True)
        c.get_profile(reset=True)
        k_h, tr = c.align(capi.init_state(c.params), trace_cap=heavy_iters)
        torch.cuda.synchronize()
        pr = c.get_profile(reset=True)
        c.set_profiling(False)
        members = [t["nnz"] for t in tr[:k_h]]
        kept_bytes = 16.0 * float(sum(members))   # 8 B written + 8 B read per member and iteration
        list_ms = pr["proc_flow_ms"] + pr["step_ms"]
        algo = BYTES_PER_POINT * (n + m) * 2.0 * k_h   # two sweeps per iteration
        gbs = kept_bytes / (list_ms * 1e-3) / 1e9 if list_ms > 0 else None
        out["roofline"] = {
            "bound": "hbm", "kernel": "k_process<PROC_FLOW> + k_process<PROC_STEP> (the list passes) of iterations 0-%d" % (k_h - 1),
            "iterations": k_h, "members_of_A_per_iteration_min_max": [int(min(members)), int(max(members))] if members else None,
            "kept_list_bytes_written_and_read": kept_bytes, "list_pass_ms": list_ms,
            "flow_pass_ms": pr["proc_flow_ms"], "step_pass_ms": pr["step_ms"], "filter_ms": pr["flow_ms"],
            "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS if gbs else None,
            "achieved_algorithmic": algo / (list_ms * 1e-3) / 1e9 if list_ms > 0 else None,
            "frac_algorithmic": algo / (list_ms * 1e-3) / 1e9 / PEAK_HBM_GBS if list_ms > 0 else None,
            "what": "achieved = the kept list's own bytes (16 B per member and iteration: written by the flow pass, read back by the "
                    "step pass) over the list passes' kernel time; the contract's algorithmic figure (32 B x (N + M) x 2 sweeps) beside it; "
                    "traffic by counters: profiles/%s_pmc_big.json where committed" % PROFILE_TAG}
        big, big_src = committed("%s_pmc_big.json" % PROFILE_TAG)
        if big:
            out["roofline"]["traffic"] = big
            out["roofline"]["traffic_source"] = big_src
    except Exception as e:
        out["roofline"] = {"error": repr(e)}
    c.close()
    return out


def shard_leg(args, pkg, torch, mode, acvo, world=8):
    """The per-GPU problem of BASELINE configs[3] on 8 GPUs, on ONE GPU: rank 0's share of the target rows
    (25k of 200k) against the whole source cloud, as a world of one (the mailbox exchange runs -- in local memory --
    and the sharded launch scheme with it).  What the 8-GPU run adds per iteration is two exchanges across xGMI;
    their latency is measured by the sharded leg of a multi-GPU run (`sharded_allreduce.allreduce_latency_us`) and
    not available here: `projected_8gpu_ms_per_iteration` = shard time + 2 x that latency where this line
    holds one (`--gpus N` runs), else + 2 x 10 us (SURVEY 8e's estimate), labelled as such."""
    capi = pkg.capi
    n = m = args.sharded_points
    xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pkg.data.SEED_CFG4, acvo=acvo)
    c = capi.Context(mode=mode, device=torch.cuda.current_device(), graph_capture=True)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    lo, hi = capi.shard_range(n, 0, world)
    slo, shi = capi.shard_range(m, 0, world)
    c.set_shard(lo, hi, slo, shi)
    c.mailbox_create(0, 1)
    c.mailbox_connect(ptrs=[None])
    prm = c.params
    import copy
    p2 = copy.copy(prm)
    p2.max_iter = 40   # (a shard alone does not converge to the full registration's pose: time a fixed number of iterations)
    c.set_params(p2)
    c.align(capi.init_state(c.params), trace_cap=0)
    torch.cuda.synchronize()
    reps, it = 3, 0
    t0 = time.perf_counter()
    for _ in range(reps):
        k, _ = c.align(capi.init_state(c.params), trace_cap=0)
        it += k
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ms_it = el * 1e3 / max(it, 1)
    out = {"workload": "rows [%d, %d) of a %dk x %dk registration (one eighth of BASELINE configs[3]) on one GPU, world of one, %d iterations"
                       % (lo, hi, n // 1000, m // 1000, it // reps),
           "launches_per_iteration": "filter, flow pass, step pass with the twist and the flow-side exchange in front (every block reads its "
                                     "rank's mailbox), post-step with the step-side exchange: 4 (5 until round 5)",
           "ms_per_iteration": ms_it, "iterations": it / float(reps),
           "projected_8gpu_ms_per_iteration": ms_it + 2 * 0.010,
           "projection": "shard time + 2 exchanges x 10 us (SURVEY 8e's estimate of one small all-reduce over xGMI; a multi-GPU run "
                         "of this bench measures it: sharded_allreduce.allreduce_latency_us) -- a PROJECTION, not a measurement"}
    if not acvo:
        try:
            c.set_params(prm)
            out["per_length_scale"] = per_length_scale_ms(c, capi, torch)
        except Exception as e:
            out["per_length_scale"] = {"error": repr(e)}
    c.close()
    return out


def strong_scaling_projection(single, shard, exchange_us=10.0, world=8):
    """BASELINE configs[3] on 8 GPUs from what ONE GPU can measure, like against like: per length scale, an 8-GPU iteration = the
    slowest shard's iteration (rank 0's share, measured as a world of one over the SAME iteration window as the unsharded
    registration) + two exchanges; a registration = the unsharded run's iterations per length scale at that pace.  The exchange
    latency is an ASSUMPTION named in the result (a multi-GPU run of this bench measures it)."""
    a, b = single.get("per_length_scale") or {}, shard.get("per_length_scale") or {}
    if "error" in a or "error" in b or not a or not b:
        return None
    total_it = int(round(single["iterations"]))
    table, ms_single, ms_proj, seen = {}, 0.0, 0.0, 0
    for name in ("ell_0.15", "ell_0.10", "ell_0.06", "ell_0.03"):
        if name not in a or name not in b:
            continue
        lo = a[name]["iterations"][0]
        its = (total_it - lo) if name == "ell_0.03" else (a[name]["iterations"][1] - lo + 1)
        its = max(its, 0)
        one = b[name]["ms_per_iteration"] + 2.0 * exchange_us * 1e-3
        table[name] = {"iterations_of_the_registration": its, "single_gpu_ms_per_iteration": a[name]["ms_per_iteration"],
                       "shard_ms_per_iteration": b[name]["ms_per_iteration"], "projected_8gpu_ms_per_iteration": one,
                       "speedup": a[name]["ms_per_iteration"] / one if one > 0 else None}
        ms_single += its * a[name]["ms_per_iteration"]
        ms_proj += its * one
        seen += its
    if not seen or ms_proj <= 0:
        return None
    return {"per_length_scale": table,
            "single_gpu_registrations_per_s_from_the_same_table": 1e3 / ms_single,
            "projected_8gpu_registrations_per_s": 1e3 / ms_proj,
            "projected_speedup_on_%d_gpus" % world: ms_single / ms_proj,
            "assumed_exchange_us": exchange_us,
            "assumption": "one mailbox exchange across xGMI = %.0f us (SURVEY 8e's estimate; never measured on this pool: SCALE runs have been "
                          "skipped) -- two per iteration; every rank's shard as slow as rank 0's; the first window carries a call's fixed cost on "
                          "both sides.  A PROJECTION." % exchange_us}


def batched_vs_oracle(pkg, pairs, last_states, last_its, acvo, cores, count=4):
    """Four registrations of the last timed step (pairs 0-3) against the oracle's of the same pairs."""
    from oracle import pyoracle as po
    p = po.default_params(po.MODE_ACVO if acvo else po.MODE_CVO)
    po.set_threads(max(1, cores))
    same, rows = 0, []
    for b in range(min(count, len(pairs))):
        xf, ff, xm, fm = pairs[b]
        st = po.init_state(p)
        n_it, _ = po.align(p, st, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=1)
        g = last_states[b]
        ok = bool(int(n_it) == int(last_its[b]) and np.array_equal(np.array(g.R), np.array(st.R)) and
                  np.array_equal(np.array(g.T), np.array(st.T)))
        same += ok
        rows.append({"pair": b, "iterations_gpu": int(last_its[b]), "iterations_oracle": int(n_it), "R_T_bit_identical": ok})
    return {"vs_oracle": rows, "vs_oracle_bit_identical": same, "vs_oracle_checked": len(rows)}



def identical_leg(args, pkg, ctxs, pair0, one_step, torch):
    """The round-1 headline: `--batch` copies of the configs[1] pair (every member stops at the
    same iteration: no tail, the best case of the fused groups)."""
    if args.identical:
        return {"note": "the timed region already is this"}
    for c in ctxs:
        c.set_fixed(pair0[0], pair0[1])
        c.set_moving(pair0[2], pair0[3])
    one_step(ctxs)
    torch.cuda.synchronize()
    steps = max(3, args.steps // 4)
    t0 = time.perf_counter()
    it = 0
    for _ in range(steps):
        its, _ = one_step(ctxs)
        it += sum(its)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"registrations_per_s": steps * len(ctxs) / el, "ms_per_step": el * 1e3 / steps,
            "iterations_per_registration": it / float(steps * len(ctxs)), "steps": steps}


def small_calls_leg(args, pkg, torch, mode, acvo):
    """cvo_hip_align_many with a FEW registrations per call on front-end-sized clouds (3k x 3k): the call leaves them to the
    streams of their contexts -- each runs most of its iterations inside resident runs, several side by side (csrc/cvo_engine.cpp
    better_alone) -- against the same calls through the engines' shared launches (option "small_calls_alone" = 0)."""
    capi = pkg.capi
    n = 3000
    out = {"workload": "distinct %d x %d pairs, 2 / 4 / 8 per align_many call" % (n, n), "per_call": {}}
    for count in (2, 4, 8):
        ctxs, streams = [], []
        for i in range(count):
            xf, ff, xm, fm = pkg.data.synthetic_pair(n, n, seed=pair_seed(pkg, 100 + i), acvo=acvo)
            s = torch.cuda.Stream()
            c = capi.Context(mode=mode, device=torch.cuda.current_device(), stream=s.cuda_stream, graph_capture=True)
            c.set_fixed(xf, ff)
            c.set_moving(xm, fm)
            ctxs.append(c)
            streams.append(s)

        def rate():
            for _ in range(3):
                capi.align_many(ctxs, [capi.init_state(c.params) for c in ctxs])
            torch.cuda.synchronize()
            reps = 12
            t0 = time.perf_counter()
            for _ in range(reps):
                capi.align_many(ctxs, [capi.init_state(c.params) for c in ctxs])
            torch.cuda.synchronize()
            return reps * count / (time.perf_counter() - t0)

        on_their_own = rate()
        ctxs[0].set_option("small_calls_alone", 0)   # (a call goes by its first context's switches)
        through_engines = rate()
        for c in ctxs:
            c.close()
        out["per_call"][str(count)] = {"registrations_per_s": on_their_own, "through_the_engines": through_engines}
    # The same calls in a process of their own (tools/gpu_small_calls.py): what a host program with a few cameras sees.  This process has
    # created > 70 streams by now and the runtime deals streams to its 4 hardware queues in turn: two of a call's four streams then share
    # a queue and their resident runs -- persistent kernels -- run one after the other (4 per call 3 138 /s fresh, 2 004 /s here:
    # profiles/r06_ab.txt 9).  `per_call` keeps this process's figures; `fresh_process` is the one quoted in the compact line.
    try:
        import re
        import subprocess
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_small_calls.py"), str(n), "2", "4", "8"],
                           capture_output=True, text=True, timeout=300, env=dict(os.environ, ACVO="1") if acvo else dict(os.environ))
        fresh = {}
        for m in re.finditer(r"(\d+) per call: on their own +([0-9.]+) /s \(entries given up (\d+)\), through the engines +([0-9.]+) /s", r.stdout):
            fresh[m.group(1)] = {"registrations_per_s": float(m.group(2)), "through_the_engines": float(m.group(4)), "entries_given_up": int(m.group(3))}
        if fresh:
            out["fresh_process"] = fresh
    except Exception as e:
        out["fresh_process_error"] = repr(e)
    return out


def saturation_leg(args, pkg, torch, mode, acvo, n, m):
    """The same workload with `--saturation-batch` distinct pairs per align_many call (four engines of 32
    slots, the others waiting in the queue): a step of 64 pairs ends with the few longest
    registrations running almost alone; this is the rate with that tail amortised."""
    capi = pkg.capi
    count = args.saturation_batch
    ctxs, streams = [], []
    for i in range(count):
        xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pair_seed(pkg, i), acvo=acvo)
        s = torch.cuda.Stream()
        c = capi.Context(mode=mode, device=torch.cuda.current_device(), stream=s.cuda_stream, graph_capture=True)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c)
        streams.append(s)

    def step():
        states = [capi.init_state(c.params) for c in ctxs]
        return capi.align_many(ctxs, states)

    # (making the pairs kept the GPU idle for seconds: warm up by wall time, not by a step count)
    t_w = time.perf_counter()
    while time.perf_counter() - t_w < 0.6:
        step()
    torch.cuda.synchronize()
    steps, it = 4, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        it += sum(step())
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    for c in ctxs:
        c.close()
    return {"workload": "%d distinct pairs per align_many call (pair i as in the timed region)" % count,
            "registrations_per_s": steps * count / el, "ms_per_step": el * 1e3 / steps,
            "iterations_per_registration": it / float(steps * count), "steps": steps}


def config4_leg(args, pkg, torch, mode, acvo, count=None, points=None, world=1, rank=0, barrier=None, dist=None, red_dev="cuda"):
    """BASELINE configs[4] per GPU: 8 concurrent 20k x 20k registrations (seeds 1000 + i; under N ranks rank r takes seeds
    1000 + 8 r + i: "64 concurrent 20k x 20k across 8 GPUs"), one align_many call per step; with ranks: every rank its own
    registrations, no data-path collective, barrier + max-over-ranks clock as the headline."""
    capi = pkg.capi
    count = count or args.config4_count
    points = points or args.config4_points
    streams = [torch.cuda.Stream() for _ in range(count)]
    ctxs = []
    for i in range(count):
        xf, ff, xm, fm = pkg.data.synthetic_pair(points, points, seed=pkg.data.SEED_CFG5_BASE + rank * count + i, acvo=acvo)
        c = capi.Context(mode=mode, device=torch.cuda.current_device(), stream=streams[i].cuda_stream,
                         graph_capture=True)
        c.set_fixed(xf, ff)
        c.set_moving(xm, fm)
        ctxs.append(c)

    def step():
        states = [capi.init_state(c.params) for c in ctxs]
        return capi.align_many(ctxs, states)
    step()
    sync = barrier if barrier else torch.cuda.synchronize
    sync()
    steps = 5
    t0 = time.perf_counter()
    it = 0
    for _ in range(steps):
        it += sum(step())
    sync()
    el = time.perf_counter() - t0
    for c in ctxs:
        c.close()
    if world > 1:
        t_max = torch.tensor([el], dtype=torch.float64, device=red_dev)
        it_sum = torch.tensor([float(it)], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t_max, op=dist.ReduceOp.MAX)
        dist.all_reduce(it_sum, op=dist.ReduceOp.SUM)
        el, it = float(t_max.item()), float(it_sum.item())
    return {"workload": "%d concurrent %dk x %dk registrations per GPU x %d GPU(s) (BASELINE configs[4], seeds 1000 + i), "
                        "one align_many call per step and rank" % (count, points // 1000, points // 1000, world),
            "registrations_per_s": steps * count * world / el, "ms_per_step": el * 1e3 / steps, "n_gpus": world,
            "iterations_per_registration": it / float(steps * count * world), "steps": steps}


def frontend_leg(args, pkg, frames=100):
    """Side leg (not part of `value`): the RGB-D front end on synthetic VGA
    frames, host images in / host cloud out (PCIe inclusive), and its CPU restatement
    (oracle, one thread) on the same frames."""
    imgs = [pkg.data.synthetic_rgbd_frame(seed=100 + k, texture=1.0) for k in range(4)]
    gen = pkg.frontend.PcdGenerator(640, 480)
    # (warm-up by wall time: the legs before this one end with seconds of host-only work, and the first
    # tens of milliseconds after such a pause run at idle clocks -- 0.56 instead of 0.18 ms per frame)
    t_w = time.perf_counter()
    k = 0
    while time.perf_counter() - t_w < 0.25:
        gen.create_pointcloud(*imgs[k % 4])
        k += 1
    t0 = time.perf_counter()
    for k in range(frames):
        xyz, _ = gen.create_pointcloud(*imgs[k % 4])
    dt = (time.perf_counter() - t0) / frames
    out = {"frames_per_s": 1.0 / dt, "ms_per_frame": dt * 1e3, "image": "640x480 synthetic, texture 1.0",
           "points": int(len(xyz)), "includes": "staging + PCIe in, kernels, cloud out"}
    # the reference's driver loop end to end (ref src/cvo_main.cpp:36-66) on a synthetic
    # sequence: image pair -> front end -> run_cvo -> pose
    seq = [("%d" % k,) + pkg.data.synthetic_rgbd_frame(seed=77, texture=1.0, motion=(1.5 * k, 0.7 * k))
           for k in range(12)]
    stream = {}
    for name, cls in (("cvo", pkg.Cvo), ("acvo", pkg.Acvo)):
        passes = []
        for _ in range(3):   # three passes on fresh objects, the median one is reported
            reg = cls()
            pkg.frontend.run_frames(reg, seq[:3], 1, generator=gen)   # warm-up
            reg.close()
            reg = cls()
            t0 = time.perf_counter()
            pkg.frontend.run_frames(reg, seq * 3, 1, generator=gen)
            passes.append((time.perf_counter() - t0) / (3 * len(seq)))
            reg.close()
        dt = sorted(passes)[1]
        stream[name] = {"frames_per_s": 1.0 / dt, "ms_per_frame": dt * 1e3,
                        "passes_ms_per_frame": [round(v * 1e3, 3) for v in passes]}
    out["stream"] = stream
    # the MATLAB driver's cloud preparation (range filter + grid average) on the device against
    # its numpy oracle, on a shipped fr1/desk cloud (~50k points -> ~700)
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "desk_pcd_ds.npz"))
        xyz0, rgb0 = z["xyz0"], z["rgb0"]
        pkg.data.prepare_matlab_cloud(xyz0, rgb0)
        t0 = time.perf_counter()
        for _ in range(20):
            g = pkg.data.prepare_matlab_cloud(xyz0, rgb0)
        dt = (time.perf_counter() - t0) / 20
        prep = {"ms_per_cloud": dt * 1e3, "points_in": int(len(xyz0)), "points_out": int(len(g[0])),
                "what": "pcRangeFilter(4.0, 0.8) + gridAverage(0.05), host arrays in and out"}
        if not args.no_cpu:
            from oracle import matlab_prep as mp
            t0 = time.perf_counter()
            for _ in range(5):
                go = mp.grid_average(*mp.pc_range_filter(xyz0, rgb0))
            prep["cpu_ms_per_cloud"] = (time.perf_counter() - t0) / 5 * 1e3
            prep["cpu_kind"] = "port (numpy), 1 thread"
            prep["bit_identical_to_oracle"] = bool(np.array_equal(g[0].view(np.uint32), go[0].view(np.uint32)) and np.array_equal(g[1], go[1]))
        out["matlab_prep"] = prep
    except Exception as e:
        out["matlab_prep"] = {"error": repr(e)}
    # the shape of BASELINE configs[2] (the PNGs of fr1/desk are not in the reference's tree): a synthetic VGA
    # sequence through the front end and ONE acvo object, clouds handed over in device memory, the state carried
    # from pair to pair as the reference's driver does (ref src/adaptive_cvo_main.cpp:36-66); the same chain is
    # held against the oracle chain in tests/test_gpu_frontend.py
    try:
        nfr = 60
        frames = [pkg.data.synthetic_rgbd_frame(seed=55, texture=1.0 + 0.5 * np.sin(k / 5.0),
                                                motion=(1.2 * k, 0.6 * np.sin(k / 3.0) * 4)) for k in range(nfr)]
        chain = {}
        for name, cls, ftype in (("acvo", pkg.Acvo, 0), ("cvo", pkg.Cvo, 1)):
            for rep in range(2):   # (the first pass warms up; a fresh object per pass, as a driver has one per sequence)
                reg = cls()
                its = 0
                t0 = time.perf_counter()
                for bgr, dep in frames:
                    gen.submit(bgr, dep, 1, ftype)
                    d_xyz, d_feat, npts = gen.collect_device()
                    reg.run_cvo_device(d_xyz, d_feat, npts)
                    its += reg.num_iterations
                dt = (time.perf_counter() - t0) / nfr
                reg.close()
            chain[name] = {"frames_per_s": 1.0 / dt, "ms_per_frame": dt * 1e3, "frames": nfr,
                           "iterations_per_pair": its / float(nfr - 1)}
        out["chain"] = chain
    except Exception as e:
        out["chain"] = {"error": repr(e)}
    out["stream_note"] = "36 synthetic VGA frames (12, three times over), ~3k points each, decoded images in host memory, one frame at a time; median of 3 passes"
    gen.close()
    if not args.no_cpu:
        from oracle import pyoracle_fe as fo
        t0 = time.perf_counter()
        for k in range(4):
            fo.create_pointcloud(*imgs[k])
        out["cpu_ms_per_frame"] = (time.perf_counter() - t0) / 4 * 1e3
        out["cpu_kind"] = "port, 1 thread"
    return out


def sharded_leg(args, pkg, dist, torch, rank, world, local_rank, barrier, red_dev="cuda"):
    """BASELINE configs[3]: target rows sharded over the ranks; the 13 + 4 float64 partial sums of
    every iteration are summed over the ranks through peer mailboxes (stores over xGMI inside the
    post kernels) -- or, as the fall-back, with RCCL between the kernels."""
    capi = pkg.capi
    acvo = args.mode == "acvo"
    n = m = args.sharded_points
    xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=pkg.data.SEED_CFG4, acvo=acvo)

    def make_ctx(exchange):
        ctx = capi.Context(mode=capi.MODE_ACVO if acvo else capi.MODE_CVO, device=local_rank, graph_capture=True)
        ctx.set_fixed(xf, ff)
        ctx.set_moving(xm, fm)
        lo, hi = capi.shard_range(n, rank, world)
        slo, shi = capi.shard_range(m, rank, world)
        ctx.set_shard(lo, hi, slo, shi)
        if exchange == "mailbox":
            handle, _ = ctx.mailbox_create(rank, world)
            handles = [None] * world
            if world > 1:
                dist.all_gather_object(handles, handle)
            else:
                handles = [handle]
            ctx.mailbox_connect(handles=handles)
        else:
            uid = [capi.comm_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(uid, src=0)
            ctx.comm_init(uid[0], rank, world)
        return ctx

    def agree(ok):
        # every rank must take the same branch: the minimum of the ranks' verdicts
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=red_dev)
        if world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return int(flag.item()) == 1

    def run(exchange):
        ctx, err = None, None
        try:
            ctx = make_ctx(exchange)
        except Exception as exc:   # noqa: BLE001
            err = exc
        if not agree(err is None):   # (before anybody waits in an exchange for a rank that is not coming)
            if ctx is not None:
                ctx.close()
            raise RuntimeError("setting up the %s exchange failed on a rank: %r" % (exchange, err))
        try:
            st = capi.init_state(ctx.params)
            ctx.align(st, trace_cap=0)   # warm-up (RCCL: also sets up the channels)
            barrier()
            t0 = time.perf_counter()
            iters = 0
            for _ in range(args.sharded_steps):
                st = capi.init_state(ctx.params)
                n_it, _ = ctx.align(st, trace_cap=0)
                iters += n_it
            barrier()
            el = time.perf_counter() - t0
        finally:
            barrier()
            ctx.close()
        t = torch.tensor([el], dtype=torch.float64, device=red_dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
        return {"registrations_per_s": args.sharded_steps / el, "ms_per_registration": el * 1e3 / args.sharded_steps,
                "ms_per_iteration": el * 1e3 / max(iters, 1), "iterations": iters / args.sharded_steps}

    res = {"workload": "synthetic %dk x %dk (BASELINE configs[3], seed %d), target rows sharded %d ways, "
                       "13 + 4 float64 summed over the ranks per iteration" % (n // 1000, m // 1000, pkg.data.SEED_CFG4, world),
           "scaling": "strong"}
    order = ["mailbox", "rccl"] if args.sharded_exchange == "mailbox" else ["rccl"]
    for ex in order:
        try:
            ok = True
            try:
                r = run(ex)
            except Exception as exc:   # noqa: BLE001
                ok, r = False, {"error": repr(exc)}
            res[ex] = r
            if agree(ok):
                res["exchange"] = ex
                res.update(r)
                if ex == "mailbox" and world > 1 and "rccl" in order:
                    try:   # the comparison SURVEY 8e asks for
                        res["rccl"] = run("rccl")
                    except Exception as exc:   # noqa: BLE001
                        res["rccl"] = {"error": repr(exc)}
                break
        except Exception as exc:   # noqa: BLE001
            res[ex] = {"error": repr(exc)}
    return res


def cpu_baseline(args, pkg, xf, ff, xm, fm, acvo, gpu_state, gpu_iters):
    """The oracle (kind "port": the reference cannot be built here) timed on the host cores of
    this box on a bounded sample of the same workload -- the configs[1] pair -- in the three forms
    SURVEY 8d lists: the reference-faithful one (uniform-grid radius search + CSR Gram matrix +
    two row sweeps, OpenMP) at its best thread count, the same on ONE thread, and the
    dense-threshold variant (every pair tested, the GPU's formulation)."""
    from oracle import pyoracle as po
    p = po.default_params(po.MODE_ACVO if acvo else po.MODE_CVO)
    # the restatement's OpenMP regions are short: more threads than it can feed
    # make it slower, so calibrate the thread count on one registration each
    po.set_threads(0)
    ncpu = po.get_threads()
    best, cores = None, 1
    t_one = None
    st_or, it_or = None, None
    for nt in sorted({1, 8, 16, 32, 64, ncpu}):
        if nt > ncpu:
            continue
        po.set_threads(nt)
        t0 = time.perf_counter()
        st = po.init_state(p)
        n_it, _ = po.align(p, st, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=1)
        dt = time.perf_counter() - t0
        if nt == 1:
            t_one = (dt, n_it)
        if st_or is None:
            st_or, it_or = st, n_it
        if best is None or dt < best:
            best, cores = dt, nt
        if dt > 4 * best:
            break
    po.set_threads(cores)
    done, iters = 0, 0
    t0 = time.perf_counter()
    while True:
        st = po.init_state(p)
        n_it, _ = po.align(p, st, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=1)
        done += 1
        iters += n_it
        el = time.perf_counter() - t0
        if el >= args.cpu_seconds or done >= 50:
            break
    t0 = time.perf_counter()
    st = po.init_state(p)
    n_d, _ = po.align(p, st, xf, ff, xm, fm, search=po.SEARCH_DENSE, trace_cap=1)
    t_dense = time.perf_counter() - t0
    cpu = {"value": done / el, "unit": "registrations/s", "cores": cores, "kind": "port",
           "ms_per_iteration": el * 1e3 / iters,
           "sample": "%d full registration(s) of the configs[1] %dk x %dk pair (%d iterations), "
                     "uniform-grid radius search + CSR Gram matrix as the reference, OpenMP on %d "
                     "threads, %.1f s" % (done, xf.shape[0] // 1000, xm.shape[0] // 1000, iters, cores, el),
           "note": "the oracle is this repository's restatement of the reference (oracle/cvo_oracle.c): the "
                   "reference itself (Eigen/TBB/ICC) cannot be built in this image",
           "one_thread": {"value": 1.0 / t_one[0], "ms_per_iteration": t_one[0] * 1e3 / max(t_one[1], 1),
                          "cores": 1, "sample": "1 registration"} if t_one else None,
           "dense_variant": {"value": 1.0 / t_dense, "ms_per_iteration": t_dense * 1e3 / max(n_d, 1), "cores": cores,
                             "pair_tests_per_s": float(xf.shape[0]) * xm.shape[0] * n_d / t_dense,
                             "sample": "1 registration, every pair tested (no spatial search)"}}
    # parity of the GPU registration of the SAME pair with the oracle's (north_star: <= 1e-4)
    T_gpu = np.array(gpu_state.transform, np.float32).reshape(4, 4)
    T_or = po.state_matrices(st_or)[0]
    rot, tr = pkg.data.rel_pose_error(T_gpu, T_or)
    parity = {"pair": "BASELINE configs[1] (seed %d)" % pkg.data.SEED_CFG2,
              "iterations_gpu": int(gpu_iters), "iterations_oracle": int(it_or),
              "iters_equal": bool(int(gpu_iters) == int(it_or)), "rot": rot, "trans": tr,
              "R_T_bit_identical": bool(np.array_equal(np.array(gpu_state.R), np.array(st_or.R)) and
                                        np.array_equal(np.array(gpu_state.T), np.array(st_or.T))),
              "tolerance": 1e-4,
              "oracle": "oracle/cvo_oracle.c (port of ref src/cvo.cpp:99-420; parity with the reference binary unpinned)"}
    gt_rot, gt_tr = pkg.data.rel_pose_error(np.linalg.inv(T_gpu.astype(np.float64)), np.linalg.inv(pkg.data.gt_motion()))
    parity["vs_synthetic_ground_truth_motion"] = {"rot": gt_rot, "trans": gt_tr,
                                                  "note": "registration accuracy on this surface, not parity"}
    return cpu, parity


if __name__ == "__main__":
    main()
