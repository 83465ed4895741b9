"""GPU: every form of the library's head -- the classic post-step launch (k_post_step), the head of the next flow launch
(head mode, with and without captured batches), the head block of the resident runs (kt_run, kt_run_acvo) and the
engines of cvo_hip_align_many -- against the float64 replay of its own trace in tests/cvo_loop_ref.py: the judge, the
settings and the tolerances of tests/loop_ref_cases.py with the library in the oracle's place (tests/test_loop_ref_cpu.py
proves them on the oracle, mutants included).  Nothing here reads the oracle.  Every test prints its worst error as a
fraction of the tolerance (pytest -s); DESIGN.md section 2 records them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvo_loop_ref as lr  # noqa: E402
import loop_ref_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

# (options, graph_capture).  With the defaults most iterations of these small registrations run inside resident runs, whose
# head block is kt_run's; "head_no_runs" leaves every iteration to the head of the next flow launch.
FORMS = {"classic": (dict(head_mode=0), False), "head": (dict(), False), "head_graphs": (dict(), True),
         "head_no_runs": (dict(resident_runs=0), False)}
# The smallest clouds of iteration_ref_cases.clouds at which a resident run is entered and carries ten iterations: a run
# starts once the candidate record in use is narrow enough for the run's registers (cvo_job.cpp job_pump: the hint against
# run_nnz_max), which needs no minimum size; the plan must be a head-mode plan with candidate records (cvo_plan.cpp plan_lone).
RUN_SIZE = (300, 260)


def make_driver(options=None, graph=False, trace_cap=2000, stats=None):
    """loop_ref_cases' driver over one capi.Context: frames[i + 1] registered to frames[i] with ps[i], all on one state."""
    def driver(capi, ps, mode, frames):
        import torch
        stream = torch.cuda.Stream()
        c = capi.Context(params=ps[0], device=0, stream=stream.cuda_stream, graph_capture=graph)
        try:
            for key, value in (options or {}).items():
                c.set_option(key, value)
            st = capi.init_state(ps[0])
            c.set_fixed(*frames[0])
            out = []
            for i, p in enumerate(ps):
                if i:
                    c.swap_moving_to_fixed()
                    c.set_params(p)
                c.set_moving(*frames[i + 1])
                s0 = lc.snap(st)
                n, tr = c.align(st, trace_cap=trace_cap)
                out.append((n, tr, s0, lc.snap(st)))
                if stats is not None:
                    stats.append(c.run_stats())
        finally:
            c.close()
        return out
    return driver


def _show(worst):
    print("worst (error / tolerance, error):", {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())})


@pytest.mark.parametrize("form", sorted(FORMS))
def test_settings_pass_the_replay(pkg, form):
    """Every setting of loop_ref_cases on both cloud orders through this form of the head: the exact parts exact, step,
    dist, pose and the three matrices within the derived bounds, no borderline record, no skipped step; and the library's
    own traces reach every branch of the census."""
    stats = []
    driver = make_driver(*FORMS[form], stats=stats)
    worst, census, bad = lc.Worst(), {}, {}
    for s in lc.SETTINGS:
        for size in lc.SIZES:
            run = lc.run_setting(pkg.capi, driver, pkg, s[0], size)
            fails = lc.judge_run(run, worst=worst, census=census)
            if fails:
                bad[(s[0], size)] = fails[:4]
    _show(worst)
    print("census:", census, " iterations inside resident runs:", sum(s[2] for s in stats))
    assert not bad, bad
    assert (sum(s[2] for s in stats) > 100) == (form in ("head", "head_graphs")), form   # (the form is the one its name says)
    for k in lr.CENSUS_KEYS:
        assert census[k] > 0, (k, census)
    for k in lr.CONDITION_KEYS:
        assert census[k] == 0, (k, census)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_one_update_at_a_time(pkg, form):
    """The same registration with max_iter = 0, 1 ... J (6 for cvo: the change of ell at k = 3 is inside; 4 for acvo): each run
    extends the one before bit for bit, its state differs from it by exactly one update, held to the single-update bound, and
    its prev_transform is the shorter run's transform bit for bit.

    (The regression test of kt_run_acvo's first Axx, with test_engines_leave_the_lone_runs_states: DESIGN.md section 2.)"""
    driver = make_driver(*FORMS[form])
    worst, bad = lc.Worst(), {}
    for name in lc.PREFIX_SETTINGS:
        for size in lc.SIZES:
            chain = lc.run_prefixes(pkg.capi, driver, pkg, name, size)
            for j in range(len(chain)):
                assert chain[j]["n_it"] == j
                fails = lc.judge_run(chain[j], shorter=chain[j - 1] if j else None, worst=worst)
                if fails:
                    bad[(name, size, j)] = fails[:4]
    _show(worst)
    assert not bad, bad
    assert "update_R" in worst and "update_T" in worst


@pytest.mark.parametrize("form", sorted(FORMS))
def test_carry_over(pkg, form):
    """Two align() calls on one state with swap_moving_to_fixed between them, then one with max_iter = 0: each replay starts
    from the carried state, both products of accum_transform are held, and with max_iter = 0 nothing moves while
    accum_transform is multiplied by the carried transform once more."""
    driver = make_driver(*FORMS[form])
    worst, bad = lc.Worst(), {}
    for mode in ("cvo", "acvo"):
        for size in lc.SIZES:
            a, b, c = lc.run_carry_over(pkg.capi, driver, pkg, mode, size)
            assert lc.same_state(a["state1"], b["state0"]) and b["n_it"] > 4 and c["n_it"] == 0
            if mode == "cvo":
                assert [t["ell"] for t in b["trace"][:5]] == [np.float32(0.03)] * 4 + [np.float32(0.10)]
            assert np.array_equal(c["state1"]["transform"], b["state1"]["transform"])
            assert np.array_equal(c["state1"]["prev_transform"], b["state1"]["transform"])
            for j, run in enumerate((a, b, c)):
                fails = lc.judge_run(run, worst=worst)
                if fails:
                    bad[(mode, size, j)] = fails[:4]
    _show(worst)
    assert not bad, bad


@pytest.mark.parametrize("name, max_iter", [("cvo_default", None), ("acvo_default", None), ("acvo_shrink", 37)])
def test_resident_runs_pass_the_replay(pkg, name, max_iter):
    """The head block of the resident runs (kt_run, kt_run_acvo: head_math on a twist stage formed ahead of time): a run is
    entered and carries at least ten iterations (run_stats), and the trace and state pass the judge."""
    worst = lc.Worst()
    for graph in (False, True):
        stats = []
        run = lc.run_setting(pkg.capi, make_driver(None, graph, stats=stats), pkg, name, RUN_SIZE, max_iter=max_iter)
        entered, _, iterations, _ = stats[0]
        assert entered >= 1 and iterations >= 10, (name, graph, stats[0])   # (otherwise this test checks nothing new)
        fails = lc.judge_run(run, worst=worst)
        assert not fails, (name, graph, fails[:4])
    _show(worst)


@pytest.mark.parametrize("name", lc.PREFIX_SETTINGS)
def test_engines_leave_the_lone_runs_states(pkg, name):
    """The registrations with max_iter = 0, 1 ... J and the full one through ONE cvo_hip_align_many call: it returns no trace,
    so its states must equal the lone runs' bit for bit; the per-update pose check is then applied to them with the lone
    full run's records."""
    import torch
    capi = pkg.capi
    _, mode, over, shift = lc.setting(name)
    size = lc.SIZES[0]
    lone = lc.run_prefixes(capi, make_driver(), pkg, name, size) + [lc.run_setting(capi, make_driver(), pkg, name, size)]
    xf, ff, xm, fm = lc.clouds(pkg, mode, size[0], size[1], shift)
    streams, ctxs = [], []
    try:
        for run in lone:
            streams.append(torch.cuda.Stream())
            c = capi.Context(params=run["p"], device=0, stream=streams[-1].cuda_stream)
            ctxs.append(c)
            c.set_fixed(xf, ff)
            c.set_moving(xm, fm)
        assert len(ctxs) <= 8
        states = [capi.init_state(c.params) for c in ctxs]
        its = capi.align_many(ctxs, states)
    finally:
        for c in ctxs:
            c.close()
    worst = lc.Worst()
    many = []
    for run, n, st in zip(lone, its, states):
        assert n == run["n_it"], (name, run["p"].max_iter)
        assert lc.same_state(lc.snap(st), run["state1"]), (name, run["p"].max_iter)
        many.append(dict(run, n_it=n, state1=lc.snap(st), trace=lone[-1]["trace"][:n]))
    for j in range(1, len(many) - 1):
        fails = lc.judge_run(many[j], shorter=many[j - 1], worst=worst)
        assert not fails, (name, j, fails[:4])
    fails = lc.judge_run(many[-1], worst=worst)
    assert not fails, (name, fails[:4])
    _show(worst)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_runs_without_a_trace_leave_the_same_state(pkg, form):
    """trace_cap = 0 and trace_cap = 3 on the 40 iterations of cvo_default: the state equals the full-trace run's bit for
    bit, and the three records are the full trace's first three."""
    options, graph = FORMS[form]
    full = lc.run_setting(pkg.capi, make_driver(options, graph), pkg, "cvo_default", lc.SIZES[0])
    assert full["n_it"] == 40 == len(full["trace"])
    for cap in (0, 3):
        run = lc.run_setting(pkg.capi, make_driver(options, graph, trace_cap=cap), pkg, "cvo_default", lc.SIZES[0])
        assert run["n_it"] == 40 and len(run["trace"]) == cap
        assert lc.same_state(run["state1"], full["state1"]), (form, cap)
        assert lc.same_records(run["trace"], full["trace"][:cap]), (form, cap)
