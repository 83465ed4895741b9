"""-m gpu: the row-sharded passes and loop of the library (cvo_hip_set_shard) under the float64 references -- the judges,
cuts and cases of tests/shard_cases.py with the library in the oracle's place (tests/test_shard_ref_cpu.py proves them on
the oracle, mutants included).

    part A  one context per shard, no exchange: cvo_hip_flow, cvo_hip_step_coeffs and cvo_hip_function_inner_product of
            every shard of every cut list against the reference's members of those DEVICE rows, and the partition;
    part B  whole registrations of several ranks through the host all-reduce hook (host threads, a barrier with a
            time-out: no kernel waits for a peer): lock step, the replay of the head behind the exchange, and every
            record of max_iter = 0 ... J against the dense reference at its exact pose;
    part C  cvo_hip_align on a shard with no exchange attached, through every form of the loop;
    part D  the same judges behind the in-kernel exchange of the device mailboxes (tools/gpu_ranks_threads.py, a process
            of its own).
Nothing here reads the reference tree; the oracle is read through po.transform alone (and by the tool of part D).
Every test prints its worst error as a fraction of the tolerance and its census (pytest -s); DESIGN.md section 2
records them.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402
import iteration_ref_cases as ic  # noqa: E402
import loop_ref_cases as lc  # noqa: E402
import shard_cases as sc  # noqa: E402
from helpers import align_two_ranks  # noqa: E402
from test_gpu_loop_ref import FORMS  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _show(worst, stats=None):
    print("worst (error / tolerance, error):", {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())},
          dict(stats or {}))


def _params(pkg, mode):
    return pkg.capi.default_params(ic.mode_id(pkg.capi, mode))


def _context(pkg, p, clouds, shard=None, options=None, graph=None):
    import torch
    c = pkg.capi.Context(params=p, device=0, stream=torch.cuda.current_stream().cuda_stream, graph_capture=graph)
    for key, value in (options or {}).items():
        c.set_option(key, value)
    c.set_fixed(clouds[0], clouds[1])
    c.set_moving(clouds[2], clouds[3])
    if shard is not None:
        c.set_shard(*shard)
    return c


def _opener(pkg, p, clouds):
    return lambda shard: _context(pkg, p, clouds, shard)


def _device(pkg, p, clouds):
    c = _context(pkg, p, clouds)
    try:
        return sc.device_order(c.device_cloud(0), clouds[0], clouds[1]), sc.device_order(c.device_cloud(1), clouds[2], clouds[3])
    finally:
        c.close()


# ---- part A

@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("cut", sc.CUT_NAMES)
def test_every_shard_of_a_cut_list_matches_the_reference(pkg, po, mode, cut):
    """transform_pcd, then flow(ell), step_coeffs (the WHOLE cloud's float32 twist and iteration_ref_cases.twists) and for
    acvo function_inner_product(ell) on one context per shard, at the five sizes (the MATLAB weight: the flow at two), four
    length scales and three poses.  Per shard: out[8] inside count_ok of the reference's members of those device rows,
    out[0:8] within flow_tol, bcde within step_tol, out[9..12] against the Axx sum over [lo, hi) and the Ayy sum over the
    rows of [slo, shi) whose caller's index is >= n_fixed, with their counts; an empty shard exactly zero with CVO_HIP_OK
    (function_inner_product: NaN).  The partition: the three counts add up exactly, every float64 sum within
    2 N 2^-53 S of the unsharded context's."""
    worst, stats = lc.Worst(), sc.PassStats()
    for n, m in (sc.SIZES if mode != "matlab" else sc.MATLAB_SIZES):
        clouds = ic.clouds(pkg, mode, n, m)
        p = _params(pkg, mode)
        shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
        sc.judge_passes(pkg, _opener(pkg, p, clouds), po.transform, p, mode, clouds, shards, ic.ELLS, ic.poses, worst, stats,
                        steps=(mode != "matlab"), twist_seed=n * 1000 + m)
    _show(worst, stats)
    assert stats["borderline"] == 0 and stats["members"] > 1000
    # (the condition on the cases, as tests/test_shard_ref_cpu.py has it: the device's rows are others than the caller's)
    assert stats.get("least_members", 1) > 0 and stats.get("members_of_small_shards", 1) > 0, stats


@pytest.mark.parametrize("mcut", sorted(sc.moving_cut_lists(*sc.ACVO_TAIL_SIZE)))
def test_moving_row_cuts_around_n_fixed(pkg, po, mcut):
    """acvo 260 x 300: the moving rows cut at n_fixed - 1, n_fixed, n_fixed + 1, at 64 and evenly, apart from the fixed
    rows' even split: the Ayy count of a shard is of all its rows, its sum of those the caller's row rule counts."""
    n, m = sc.ACVO_TAIL_SIZE
    worst, stats = lc.Worst(), sc.PassStats()
    clouds = ic.clouds(pkg, "acvo", n, m)
    p = _params(pkg, "acvo")
    shards = sc.shards_of(sc.even(n, 2), sc.moving_cut_lists(n, m)[mcut])
    sc.judge_passes(pkg, _opener(pkg, p, clouds), po.transform, p, "acvo", clouds, shards, ic.ELLS, ic.poses, worst, stats,
                    twist_seed=n * 1000 + m)
    _show(worst, stats)
    assert stats["borderline"] == 0


@pytest.mark.parametrize("name,mode,ell,pose", sc.HOSTILE)
def test_shards_of_hostile_clouds(pkg, po, name, mode, ell, pose):
    """far600 (a straddling wave's two spheres meet cull_slack far from the origin) and dup (equal Morton keys on both
    sides of a cut) at their own 1 500 x 1 300, cut at (0, 65, 130, n): the per-shard counts against the float64 all-pairs
    members of those rows."""
    clouds = hc.clouds(pkg.data, name, acvo=(mode == "acvo"))
    n, m = len(clouds[0]), len(clouds[2])
    p = _params(pkg, mode)
    worst, stats = lc.Worst(), sc.PassStats()
    shards = sc.shards_of(sc.cut_lists(n)[sc.HOSTILE_CUT], sc.cut_lists(m)[sc.HOSTILE_CUT])
    sc.judge_passes(pkg, _opener(pkg, p, clouds), po.transform, p, mode, clouds, shards, [ell],
                    lambda _: [hc.poses(clouds[0])[pose]], worst, stats, twist_seed=7)
    _show(worst, stats)
    # (a borderline pair widens its shard's count window by one and its tolerances by its whole term: capped, so that no wide
    # window can hide a lost member of the straddling wave)
    assert stats["members"] > 1000 and stats["borderline"] <= sc.BORDER_CAP * stats["members"], stats


# ---- part B

def _drivers(pkg, mode, clouds, options=None):
    """(run_ranks, run_whole) of shard_cases over the library: ranks through the host all-reduce hook."""
    capi = pkg.capi

    def as_run(o):
        return dict(n_it=o[0], raw=o[1], calls=o[3], trace=o[4], state0=o[5], state1=o[6], stats=o[7])

    def run_ranks(p, shards, trace_cap=2000):
        out = align_two_ranks(pkg, p.mode, *clouds, exchange="hook", timeout=120, cuts=(0,) + tuple(s[1] for s in shards),
                              mcuts=(0,) + tuple(s[3] for s in shards), params=p, trace_cap=trace_cap, barrier_timeout=20.0)
        return [as_run(out[r]) for r in range(len(shards))]

    def run_whole(p, shard=None, trace_cap=2000, graph=None, stats_out=None):
        c = _context(pkg, p, clouds, shard, options, graph)
        try:
            st = capi.init_state(p)
            s0 = lc.snap(st)
            n_it, tr = c.align(st, trace_cap=trace_cap)
            if stats_out is not None:
                stats_out.append(c.run_stats())
            return dict(n_it=n_it, raw=bytes(st), calls=0, trace=tr, state0=s0, state1=lc.snap(st), stats=c.list_stats())
        finally:
            c.close()
    return run_ranks, run_whole


def _loop(pkg, case):
    _, mode, name, (n, m) = case
    clouds = lc.clouds(pkg, mode, n, m, lc.setting(name)[3])
    p = lc.params(pkg.capi, mode, lc.setting(name)[2])
    return mode, name, n, m, clouds, _device(pkg, p, clouds)


@pytest.mark.parametrize("cut", sc.LOOP_CUT_NAMES)
@pytest.mark.parametrize("case", sc.LOOP_CASES, ids=[c[0] for c in sc.LOOP_CASES])
def test_a_sharded_registration_through_the_hook(pkg, po, case, cut):
    """Ranks on host threads, the 13 + 4 partial sums added in rank order through host memory.  Lock step: every rank's
    state and trace bit-identical, the same number of hook calls on every rank (an empty one included), the unsharded
    registration's iteration count and its transform within 1e-6.  The head behind the exchange: rank 0's trace and state
    through the replay judge (loop_ref_cases.judge_run).  Every iteration: the runs with max_iter = 0 ... J are
    bit-identical prefixes of one another, and record j is held at the pose of run j against the dense reference -- nnz
    inside count_ok, omega_d, v_d, sum_a within flow_tol, bcde within step_tol at the record's own twist, for acvo nnz_xx,
    nnz_yy and at j = 0 dl; no record with more than one borderline pair per 1 000 members."""
    mode, name, n, m, clouds, dev = _loop(pkg, case)
    worst, stats = lc.Worst(), sc.PassStats()
    run_ranks, run_whole = _drivers(pkg, mode, clouds)
    shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
    sc.judge_sharded_registration(pkg, pkg.capi, run_ranks, run_whole, dev, po.transform, mode, name, shards, worst, stats)
    _show(worst, stats)
    # (the census, from Context.list_stats() of the runs one iteration apart.  Ranks behind the hook are issued launch by launch
    # (cvo_job.cpp job_begin: no table plan under host_reduce), keep no candidate record and so have none to narrow: their
    # branch is the re-used tile list; the narrowing is reached behind the mailboxes, part D.  acvo's ell moves in every one of
    # its first iterations)
    assert stats["records"] == lc.PREFIX_J[mode] + 1, stats
    assert stats["on_reused_list"] > 0 or mode == "acvo", stats


def test_eight_ranks_and_the_moving_row_cuts_through_the_hook(pkg, po):
    """The world-8 even split once (cvo 300 x 260), and acvo 260 x 300 with the moving rows cut at n_fixed - 1, n_fixed,
    n_fixed + 1, 64 and evenly."""
    worst, stats = lc.Worst(), sc.PassStats()
    mode, name, n, m, clouds, dev = _loop(pkg, sc.LOOP_CASES[0])
    run_ranks, run_whole = _drivers(pkg, mode, clouds)
    sc.judge_sharded_registration(pkg, pkg.capi, run_ranks, run_whole, dev, po.transform, mode, name,
                                  sc.shards_of(sc.even(n, 8), sc.even(m, 8)), worst, stats)
    mode, name, n, m, clouds, dev = _loop(pkg, sc.LOOP_CASES[1])
    run_ranks, run_whole = _drivers(pkg, mode, clouds)
    for mcuts in sc.moving_cut_lists(n, m).values():
        sc.judge_sharded_registration(pkg, pkg.capi, run_ranks, run_whole, dev, po.transform, mode, name,
                                      sc.shards_of(sc.even(n, 2), mcuts), worst, stats)
    _show(worst, stats)
    assert stats["on_reused_list"] > 0, stats


# ---- part C

@pytest.mark.parametrize("mode", ["cvo", "acvo"])
def test_a_shard_without_an_exchange_in_every_form_of_the_loop(pkg, po, mode):
    """cvo_hip_align on a context with set_shard(65, 257, 0 | 64, m) and no hook, communicator or mailbox: rows [65, 257) of
    the fixed cloud against the whole moving cloud (acvo: the Ayy rows [64, m)), what include/cvo_hip.h says of it.  Through
    the classic loop, head mode with and without captured batches, without resident runs, the default with runs (a run is
    entered) and as one of 16 contexts of an align_many call: the same iteration count and state bytes in every form;
    record 0 of max_iter = 1 has the reference's member count of those rows and its sums, step coefficients, and for acvo
    nnz_xx, nnz_yy and dl of the three restricted member sets; the full run passes the replay judge."""
    case = sc.LOOP_CASES[0] if mode == "cvo" else sc.LOOP_CASES[1]
    mode, name, n, m, clouds, dev = _loop(pkg, case)
    rows = tuple(m if v is None else v for v in sc.NO_EXCHANGE_SHARD[mode])
    worst, stats = lc.Worst(), sc.PassStats()
    full = {}
    for form, (options, graph) in sorted(FORMS.items()):
        run_stats = []
        _, run_whole = _drivers(pkg, mode, clouds, options)
        full[form] = sc.judge_no_exchange(pkg, pkg.capi, lambda p, shard=None: run_whole(p, shard, graph=graph, stats_out=run_stats),
                                          dev, po.transform, mode, name, rows, worst, stats)
        if form == "head" and mode == "cvo":
            assert run_stats[-1][0] >= 1, ("no resident run was entered", run_stats)
        print(form, "iterations", full[form]["n_it"], "run_stats", run_stats[-1])
    for form, run in full.items():
        assert run["n_it"] == full["classic"]["n_it"] > 4 and run["raw"] == full["classic"]["raw"], form
        # (everything the head wrote, bit for bit, as tests/test_gpu_loop_ref.py compares the forms' traces: the float64 sums of
        # a record are added in the order of the form's launches and are held to the references above, form by form)
        assert lc.same_records(run["trace"], full["classic"]["trace"]), form
    # one of 16 contexts of an align_many call: the shard on context 5, the others unsharded
    import torch
    capi = pkg.capi
    p = lc.params(capi, mode, lc.setting(name)[2])
    streams, ctxs = [], []
    try:
        for k in range(16):
            streams.append(torch.cuda.Stream())
            c = capi.Context(params=p, device=0, stream=streams[-1].cuda_stream)
            ctxs.append(c)
            c.set_fixed(clouds[0], clouds[1])
            c.set_moving(clouds[2], clouds[3])
        ctxs[5].set_shard(*rows)
        states = [capi.init_state(p) for _ in ctxs]
        its = capi.align_many(ctxs, states)
    finally:
        for c in ctxs:
            c.close()
    assert its[5] == full["classic"]["n_it"] and bytes(states[5]) == full["classic"]["raw"]
    assert bytes(states[4]) == bytes(states[6]) != bytes(states[5])
    _show(worst, stats)


# ---- part D

def _ranks_tool(args, timeout=240):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    env.pop("CVO_HIP_TWIST_ON_SHARED_GPU", None)
    return subprocess.run(["timeout", "-k", "10", str(timeout - 20), sys.executable, os.path.join(ROOT, "tools", "gpu_ranks_threads.py")] + args,
                          capture_output=True, text=True, timeout=timeout, env=env)


# (arguments of the tool, J of its prefix chain, whether a narrowing lies among the judged records)
MAILBOX_CASES = {
    "cvo_65": (["cvo", "300", "260", "2", "--cuts", "0,65,300"], lc.PREFIX_J["cvo"], True),
    "cvo_1_257": (["cvo", "300", "260", "3", "--cuts", "0,1,257,300"], lc.PREFIX_J["cvo"], True),
    # acvo narrows late (the first time at record 16 of this pair, where the pair has one borderline pair among 112 members, over the cap
    # of 1 per 1 000): the case as set is held up to J = 4, and the same cut on the pair of ANOTHER SEED (17: no borderline pair
    # over the cap in 25 records) up to J = 24, past both of its narrowings
    "acvo_moving_at_n_fixed": (["acvo", "260", "300", "2", "--mcuts", "0,260,300"], lc.PREFIX_J["acvo"], False),
    "acvo_moving_at_n_fixed_seed17": (["acvo", "260", "300", "2", "classic", "17", "--mcuts", "0,260,300"], 24, True),
    "cvo_65_in_launch": (["cvo", "300", "260", "2", "in_launch", "--cuts", "0,65,300"], lc.PREFIX_J["cvo"], True),
}


@pytest.mark.parametrize("case", sorted(MAILBOX_CASES))
def test_the_judges_behind_the_device_mailboxes(case):
    """tools/gpu_ranks_threads.py with explicit cuts and a trace, in a process of its own: the ranks exchange inside the
    kernels through mailboxes in device memory and run the recorded synchronous plan of the sharded loop (the moving cloud
    pre-transformed by the xy filter, the candidate record narrowed when ell drops).  The tool holds lock step, the replay
    judge and record 0 against the dense reference, then the runs with max_iter = 0 ... J on the same contexts: bit-identical
    prefixes and record j at the state of run j against the dense reference, no record over the cap of borderline pairs.
    The census, from list_stats of runs one iteration apart: among the judged records at least one streamed a re-used list
    and (where MAILBOX_CASES says a narrowing lies inside J) at least one followed a narrowing."""
    import re
    args, J, narrows = MAILBOX_CASES[case]
    r = _ranks_tool(args + ["--trace", "2000", "--prefixes", str(J)])
    print(r.stdout[-2500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert ": OK" in r.stdout and "judges: lock step, replay, record 0" in r.stdout
    builds, narrowings, _ = (int(v) for v in re.search(r"builds (\d+) narrowings (\d+) re-expansions (\d+)", r.stdout).groups())
    assert builds >= 1 and narrowings >= 1, r.stdout[-600:]
    judged, narrowed, reused = (int(v) for v in re.search(r"records judged (\d+), after a narrowing (\d+), on a re-used list (\d+)", r.stdout).groups())
    assert judged == J + 1 and reused >= 1 and (narrowed >= 1 or not narrows), r.stdout[-600:]


def test_an_empty_rank_behind_the_device_mailboxes():
    """cvo 300 x 260, world 2, cuts (0, 0, n): rank 0 has no rows and must still send and poll in every exchange; with
    mailbox_timeout_s = 5 a rank that did not take part would end its peer as CVO_HIP_ERR_COMM after seconds.

    What the code says of a rank whose lists are empty (cvo_plan.cpp): enqueue_flow calls enqueue_filter, which returns
    CVO_HIP_OK before it launches or records anything when row_hi - row_lo <= 0 (:150-151), and then enqueue_process, which
    does not look at the row range: it makes sure an (empty) list object exists (:262), so the flow pass streams a list
    whose counters zero_counters / the plan's prepare step left at zero; emit_post_flow (:592-593) and enqueue_step's
    enqueue_process and emit_post_step (:603, :664-665) are issued for every rank alike, and the exchange sits in those
    post kernels (pa.comm = ctx->comm_table, :581, :619) or in k_step_twist (a.comm, :377): an empty rank sends zeros."""
    r = _ranks_tool(["cvo", "300", "260", "2", "--cuts", "0,0,300", "--trace", "2000", "--mailbox-timeout", "5"])
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert ": OK" in r.stdout and "judges: lock step, replay, record 0" in r.stdout
