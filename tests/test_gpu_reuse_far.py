"""-m gpu: the device held to the oracle WHILE IT RE-USES LISTS far from the origin.

From the identity the far* registrations of tests/hostile_cases.py stop after 1 - 7 iterations on the algorithm's own break
tests, before any list is re-used, so tests/test_gpu_hostile.py says nothing about the travel bounds that keep a tile list or
a candidate record alive (csrc/cvo_device.h plan_lists, plan_xy_async, plan_self_async_one, reuse_slack).  Here the break tests
are off (eps = eps_2 = 0) and every registration runs 40 iterations (hostile_cases.long_params): cvo walks its whole
length-scale schedule 0.15 -> 0.03, acvo runs from 0.10 down to ell_min, 150 m to 3.7 km from the origin (far150, far600,
far1500 and far3700), and every iteration's members, twist and step and the final state must be the oracle's by bits -- under
the synchronous and the asynchronous list plans (test switch "async_builds"), with the record narrowed or rebuilt
("record_narrow") and with resident runs allowed or denied ("resident_runs").

Every lone run must SHOW that lists were re-used, else it has shown nothing.  Under the synchronous plan cvo_hip_get_list_stats
counts the xy list's all-pairs builds and narrowings: at least one build, fewer builds than iterations and, with narrowing on, at
least one narrowing for cvo.  It does not see the asynchronous plan (the library's default), whose builds and stall slots the
device counts in words of their own, read-only options "async_builds_named" and "async_stalls": under the asynchronous plan at
least one build named, builds and stalls each fewer than iterations, and -- where resident runs are allowed -- at least one run
entered that carried more iterations than there were runs (a run holds one record's candidates for all its iterations).  A device
that stalled or rebuilt in every slot would fail these, whatever its results.

There is no extremal stream on the GPU here as the cull has one: only a registration re-uses lists, and it chooses its own
poses.  The extremal search of the re-use bounds is the host driver's (tests/cpp/reuse_host.cpp through
tests/test_reuse_cpu.py), which runs the device's own source.

On an MI355X the nine tests take 2.4 s together, 0.02 - 0.21 s each."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("cvo", "acvo")
# (asynchronous plans, record_narrow, resident_runs)
SETTINGS = tuple((a, n, r) for a in (1, 0) for n in (1, 0) for r in (1, 0))


def _context(pkg, acvo, name):
    import torch
    capi = pkg.capi
    s = torch.cuda.Stream()
    p = hc.long_params(capi.default_params(capi.MODE_ACVO if acvo else capi.MODE_CVO))
    c = capi.Context(params=p, device=0, stream=s.cuda_stream, graph_capture=True)
    xf, ff, xm, fm = hc.clouds(pkg.data, name, acvo)
    c.set_fixed(xf, ff)
    c.set_moving(xm, fm)
    return c, s


def _set(c, setting):
    c.set_option("async_builds", setting[0])
    c.set_option("record_narrow", setting[1])
    c.set_option("resident_runs", setting[2])


@pytest.mark.parametrize("mode_name", MODES)
@pytest.mark.parametrize("name", hc.REUSE_NAMES)
def test_align_matches_oracle_while_lists_are_reused(pkg, po, name, mode_name):
    """tests/test_gpu_hostile.py test_align_matches_oracle on registrations that keep running: the iteration count, every
    iteration's nnz, ell, omega, v and step and the whole final state equal the oracle's, under every setting."""
    acvo = mode_name == "acvo"
    capi = pkg.capi
    n_or, tr_or, st_or = hc.oracle_long_align(po, pkg.data, name, acvo)
    assert n_or == hc.REUSE_ITERATIONS
    c, s = _context(pkg, acvo, name)
    try:
        for setting in SETTINGS:
            _set(c, setting)
            st = capi.init_state(c.params)
            n_it, tr = c.align(st, trace_cap=2000)
            builds, narrowings, reexpansions = c.list_stats()
            named, stalls = int(c.get_option("async_builds_named")), int(c.get_option("async_stalls"))
            runs = c.run_stats()
            tag = (name, mode_name) + setting
            print(tag, "iterations", n_it, "list_stats", (builds, narrowings, reexpansions), "async builds / stalls", (named, stalls),
                  "run_stats", runs)
            assert n_it == n_or, (tag, n_it, n_or)
            assert len(tr) == len(tr_or)
            for k, (a, b) in enumerate(zip(tr, tr_or)):
                assert a["nnz"] == b["nnz"] and a["ell"] == b["ell"], (tag, k, a["nnz"], b["nnz"])
                assert a["omega"] == b["omega"] and a["v"] == b["v"] and a["step"] == b["step"], (tag, k)
            assert bytes(st) == st_or, tag
            # ---- proof of re-use
            if setting[0]:   # the asynchronous plan: its own counters; the synchronous list's stay at zero
                assert builds == 0 and narrowings == 0, (tag, builds, narrowings)
                assert 1 <= named < n_it, (tag, named)
                assert 1 <= stalls < n_it, (tag, stalls)   # (the first slot only builds)
                if setting[2]:
                    assert runs[0] > 0 and runs[2] > runs[0], (tag, runs)
            else:
                assert named == 0, (tag, named)
                assert 1 <= builds < n_it, (tag, builds)
                if setting[1] and not acvo:
                    assert narrowings >= 1, (tag, narrowings)
                if not setting[1]:
                    assert narrowings == 0, (tag, narrowings)
    finally:
        c.close()


def test_align_many_of_all_far_registrations_matches_oracle(pkg, po):
    """The same registrations, cvo and acvo, in ONE cvo_hip_align_many call: iteration counts and whole states equal the
    oracle's, with the record narrowed or rebuilt and resident runs allowed or denied; every registration built a list at
    least once and in fewer slots than it ran iterations, under whichever plan its engine gave it."""
    capi = pkg.capi
    keys = [(name, acvo) for name in hc.REUSE_NAMES for acvo in (False, True)]
    made = [_context(pkg, acvo, name) for name, acvo in keys]
    ctxs = [m[0] for m in made]
    want = [hc.oracle_long_align(po, pkg.data, name, acvo) for name, acvo in keys]
    try:
        for narrow, runs in ((1, 1), (0, 1), (1, 0), (0, 0)):
            for c in ctxs:
                c.set_option("record_narrow", narrow)
                c.set_option("resident_runs", runs)
            states = [capi.init_state(c.params) for c in ctxs]
            its = capi.align_many(ctxs, states)
            # (builds of the synchronous list, narrowings, re-expansions, builds the asynchronous plan named: a slot of an engine
            # runs whichever plan the engine picks)
            stats = [c.list_stats() + (int(c.get_option("async_builds_named")),) for c in ctxs]
            print("narrow %d runs %d: list_stats + async builds %s" % (narrow, runs, dict(zip(keys, stats))))
            for k, it, st, w, ls in zip(keys, its, states, want, stats):
                assert it == w[0] == hc.REUSE_ITERATIONS, (k, narrow, runs, it, w[0])
                assert bytes(st) == w[2], (k, narrow, runs)
                assert 1 <= ls[0] + ls[3] < it, (k, narrow, runs, ls)   # some plan built, and not in every iteration
    finally:
        for c in ctxs:
            c.close()
