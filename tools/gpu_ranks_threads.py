#!/usr/bin/env python3
"""`world` ranks on ONE GPU, one host thread and one library-owned stream each, through mailboxes in device memory
(tests/helpers.py align_two_ranks) against the unsharded registration: lock step bit for bit, the same iteration count, transform
within 1e-6.  A process of its own (tests/test_gpu_paths.py runs it as a subprocess): the ranks' streams are then the first streams of
the process and get hardware queues of their own -- inside a long-lived process the runtime hands a new stream the least-used
hardware queue, two ranks can end up on one, and a rank that spins in a kernel for its peer keeps that peer's kernels from starting
(both time out).  Ranks that share a GPU exist in tests only.
usage: gpu_ranks_threads.py cvo|acvo n m world [in_launch] [seed] [--cuts c0,c1,...] [--mcuts c0,c1,...] [--trace CAP]
                             [--mailbox-timeout S] [--prefixes J]
--cuts / --mcuts: explicit cut lists of the fixed / the moving rows (tests/shard_cases.py; world is then their length - 1) in
place of the even split; --trace: records kept per rank.  With either, the clouds are iteration_ref_cases.clouds (unless a seed is given) and the tool
runs the judges of tests/shard_cases.py itself behind the in-kernel exchange: lock step (states and traces), the replay of
rank 0's trace (loop_ref_cases.judge_run) and record 0 against the dense reference on the device's rows.  --prefixes J: the
ranks then run the same registration with max_iter = 0 ... J on the same contexts and mailboxes (shard_cases.judge_chain):
lock step of every run, each a bit-identical prefix of the next, record j held at the state of run j against the dense
reference, and the census of the judged records from list_stats, printed: how many followed a narrowing of the candidate record
and how many streamed a re-used list -- the recorded synchronous plan of the sharded loop is what these ranks run.
--mailbox-timeout S: cvo_hip_set_option "mailbox_timeout_s" on every rank."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import __graft_entry__ as ge
from helpers import align_two_ranks

argv, named = [], {}
it_args = iter(sys.argv[1:])
for a in it_args:   # (the named arguments out of the way: the positional ones are where they always were)
    if a.startswith("--"):
        named[a[2:]] = next(it_args)
    else:
        argv.append(a)
sys.argv = sys.argv[:1] + argv
mode_name, n, m, world = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
cuts = tuple(int(v) for v in named["cuts"].split(",")) if "cuts" in named else None
mcuts = tuple(int(v) for v in named["mcuts"].split(",")) if "mcuts" in named else None
trace_cap = int(named.get("trace", 0))
judged = cuts is not None or mcuts is not None or trace_cap > 0
if cuts is None and mcuts is not None:
    cuts = tuple(n * r // (len(mcuts) - 1) for r in range(len(mcuts)))
if cuts is not None:
    world = len(cuts) - 1
if len(sys.argv) > 5 and sys.argv[5] == "in_launch":
    os.environ["CVO_HIP_TWIST_ON_SHARED_GPU"] = "1"
pkg = ge.load_package(); capi = pkg.capi
acvo = mode_name == "acvo"
mode = capi.MODE_ACVO if acvo else capi.MODE_CVO
seed = int(sys.argv[6]) if len(sys.argv) > 6 else 61
xf, ff, xm, fm = pkg.data.synthetic_pair(n, m, seed=seed, acvo=acvo)
params, options = None, {}
if judged:
    import iteration_ref_cases as ic, loop_ref_cases as lc, shard_cases as sc
    name = "acvo_default" if acvo else "cvo_default"
    if len(sys.argv) <= 6:   # (a seed on the command line: data.synthetic_pair with it, above -- a case of another seed)
        xf, ff, xm, fm = lc.clouds(pkg, mode_name, n, m, lc.setting(name)[3])
    params = lc.params(capi, mode_name, lc.setting(name)[2])
    trace_cap = trace_cap or 2000
if "mailbox-timeout" in named:
    options["mailbox_timeout_s"] = float(named["mailbox-timeout"])
# (the present command line makes the call it always made: the optional arguments alone reach for what tests/helpers.py gained with them)
chain_ps = []
if judged and "prefixes" in named:
    chain_ps = [lc.params(capi, mode_name, dict(lc.setting(name)[2], max_iter=j)) for j in range(int(named["prefixes"]) + 1)]
extra = dict(chain=chain_ps, cuts=cuts, mcuts=mcuts, params=params, trace_cap=trace_cap, barrier_timeout=60.0, options=options) if judged or options else {}
out = align_two_ranks(pkg, mode, xf, ff, xm, fm, exchange="mailbox", world=world, timeout=120, **extra)
ref = capi.Context(params=params, mode=mode, device=0) if judged else capi.Context(mode=mode, device=0)
ref.set_fixed(xf, ff); ref.set_moving(xm, fm)
dev = (sc.device_order(ref.device_cloud(0), xf, ff), sc.device_order(ref.device_cloud(1), xm, fm)) if judged else None
st_ref = capi.init_state(ref.params)
it_ref, _ = ref.align(st_ref, trace_cap=0)
ref.close()
T_ref = np.array(st_ref.transform, np.float32).reshape(4, 4)
for r in range(world):
    assert out[r][0] == it_ref, (r, out[r][0], it_ref)
    assert out[r][1] == out[0][1], "rank %d left lock step" % r
rot, tra = pkg.data.rel_pose_error(out[0][2], T_ref)
assert rot <= 1e-6 and tra <= 1e-6, (rot, tra)
if judged:
    from oracle import pyoracle as po
    ranks = [dict(n_it=o[0], raw=o[1], calls=o[3], trace=o[4], state0=o[5], state1=o[6], stats=o[7]) for o in (out[r] for r in range(world))]
    whole = dict(n_it=it_ref, state1=lc.snap(st_ref))
    worst, stats = lc.Worst(), sc.PassStats()
    sc.judge_lock_step(pkg, ranks, whole)
    sc.judge_replay(params, ranks[0], worst=worst)
    sc.judge_record(params, mode_name, ranks[0]["trace"][0], ranks[0]["state0"], dev, po.transform, worst, stats, with_dl=acvo)
    print("judges: lock step, replay, record 0: passed; worst (error / tolerance, error):",
          {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())}, dict(stats))
    if chain_ps:
        as_run = lambda o: dict(n_it=o[0], raw=o[1], calls=o[3], trace=o[4], state0=o[5], state1=o[6], stats=o[7])   # noqa: E731
        ref = capi.Context(params=params, mode=mode, device=0)
        ref.set_fixed(xf, ff); ref.set_moving(xm, fm)
        chain = []
        for j, pj in enumerate(chain_ps):
            rk = [as_run(out[r][8][j]) for r in range(world)]
            ref.set_params(pj)
            st_j = capi.init_state(pj)
            it_j, _ = ref.align(st_j, trace_cap=0)
            sc.judge_lock_step(pkg, rk, dict(n_it=it_j, state1=lc.snap(st_j)))
            sc.hold("prefix", rk[0]["n_it"] == min(j, ranks[0]["n_it"]), "max_iter %d ran %d iterations" % (j, rk[0]["n_it"]))
            chain.append(rk[0])
        ref.close()
        stats = sc.PassStats()
        print("list_stats of the runs with max_iter = 0 ...:", [tuple(c["stats"]) for c in chain])
        sc.judge_chain(params, mode_name, ranks[0], chain, dev, po.transform, worst, stats)
        print("prefixes: records judged %d, after a narrowing %d, on a re-used list %d; worst (error / tolerance, error):"
              % (stats["records"], stats["after_narrowing"], stats["on_reused_list"]),
              {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())})
        assert stats["records"] == len(chain_ps), dict(stats)   # (the census is the caller's to assert: it knows its case)
    print("census of rank 0 (list_stats): builds %d narrowings %d re-expansions %d" % tuple(ranks[0]["stats"]))
print("ranks on one gpu, world %d, %s %d x %d: OK (%d iterations, rot %.2g, trans %.2g)" % (world, mode_name, n, m, it_ref, rot, tra))
