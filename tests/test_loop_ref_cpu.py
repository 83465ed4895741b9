"""CPU: the head of the oracle's loop (oracle/cvo_oracle.c cvo_oracle_align: the step from the cubic, both stop tests,
Exp_SEK3 and the update of R and T, the length-scale rules of cvo and acvo, iter, and what align() leaves in transform,
prev_transform and accum_transform) against the float64 replay of its own trace in tests/cvo_loop_ref.py.

The settings, the tolerances with their derivation, the judge and the mutants are in tests/loop_ref_cases.py; no figure
there comes from an observed error.  This file proves the replay and the cases where no GPU is needed:
tests/test_gpu_loop_ref.py runs the same judge over the library's heads.  Every test prints its worst error as a fraction
of the tolerance (pytest -s); DESIGN.md section 2 records them.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvo_loop_ref as lr  # noqa: E402
import loop_ref_cases as lc  # noqa: E402


def oracle_driver(po, ps, mode, frames):
    st = po.init_state(ps[0])
    out = []
    for i, p in enumerate(ps):
        s0 = lc.snap(st)
        n, tr = po.align(p, st, frames[i][0], frames[i][1], frames[i + 1][0], frames[i + 1][1],
                         search=po.SEARCH_DENSE if mode == "matlab" else po.SEARCH_GRID)
        out.append((n, tr, s0, lc.snap(st)))
    return out


@pytest.fixture(scope="module")
def runs(pkg, po):
    """Every run of the cases through the oracle, once: full[(name, size)], prefixes[(name, size)] = [max_iter 0 ... J],
    carry[(mode, size)] = [first, second, max_iter 0]."""
    full = {(s[0], size): lc.run_setting(po, oracle_driver, pkg, s[0], size) for s in lc.SETTINGS for size in lc.SIZES}
    prefixes = {(name, size): lc.run_prefixes(po, oracle_driver, pkg, name, size) for name in lc.PREFIX_SETTINGS for size in lc.SIZES}
    carry = {(mode, size): lc.run_carry_over(po, oracle_driver, pkg, mode, size) for mode in ("cvo", "acvo") for size in lc.SIZES}
    return dict(full=full, prefixes=prefixes, carry=carry)


def _judge_each(runs, rules=None, worst=None, census=None):
    """(run, its first failure) for every run of the cases that fails under `rules`, lazily: the one-update runs first."""
    for key, chain in runs["prefixes"].items():
        for j in range(len(chain)):
            bad = lc.judge_run(chain[j], rules, shorter=chain[j - 1] if j else None, worst=worst, census=census)
            if bad:
                yield ("prefix", j) + key, bad[0]
    for key, chain in runs["carry"].items():
        for j, run in enumerate(chain):
            bad = lc.judge_run(run, rules, worst=worst, census=census)
            if bad:
                yield ("carry", j) + key, bad[0]
    for key, run in runs["full"].items():
        bad = lc.judge_run(run, rules, worst=worst, census=census)
        if bad:
            yield ("full",) + key, bad[0]


def _judge_all(runs, rules=None, worst=None, census=None):
    return dict(_judge_each(runs, rules, worst, census))


def test_the_oracle_passes_the_replay(runs):
    """Every setting on both cloud orders, the runs of max_iter = 1 ... J one update at a time, and the carry-over: k,
    exit_code, ell, ell_max, iter and the twist's cast exact; the step within 1e-5 of numpy.roots; dist within 2e-5 + 1e-7
    of logm; one update of R, T within the derived bound; the pose after a whole registration within the walk's bound;
    transform, prev_transform, accum_transform as cvo.cpp:413-415 has them.  No record is borderline for break A or for the
    small-angle branch, and no cubic has a nearly double root."""
    worst, census = lc.Worst(), {}
    bad = _judge_all(runs, worst=worst, census=census)
    print("worst (error / tolerance, error):", {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())})
    assert not bad, bad
    for k in lr.CONDITION_KEYS:
        assert census[k] == 0, (k, census[k])
    for k in ("update_R", "update_T", "walk_R", "walk_T", "step", "dist", "accum_transform"):
        assert k in worst


def test_every_branch_is_taken(runs):
    """The census of the replay over the full runs: clamped, unclamped and min_step steps, the small-angle branch, break A,
    break B, the max_iter stop, acvo's shrink and floor, and each change of cvo's schedule are all reached."""
    census = {}
    for run in runs["full"].values():
        lc.judge_run(run, census=census)
    print("census:", census)
    for k in lr.CENSUS_KEYS:
        assert census[k] > 0, (k, census)


def test_the_settings_reach_what_they_are_there_for(runs):
    """What each setting is in the list for, on (300, 260)."""
    f = {name: runs["full"][(name, (300, 260))] for name, _, _, _ in lc.SETTINGS}

    def codes(name):
        return [t["exit_code"] for t in f[name]["trace"]]
    assert f["cvo_default"]["n_it"] == 40 and set(codes("cvo_default")) == {0} and f["cvo_default"]["state1"]["iter"] == 0
    assert codes("acvo_default")[-1] == 1 and f["acvo_default"]["state1"]["iter"] == f["acvo_default"]["n_it"] - 1 > 4
    assert codes("matlab")[-1] == 1 and f["matlab"]["n_it"] > 4
    steps = [t["step"] for t in f["cvo_cd_small"]["trace"]]
    assert max(steps[:8]) < 0.01 and max(steps) < 0.4   # (roots far below the clamp)
    assert codes("cvo_cd_large")[-1] == 1 and f["cvo_cd_large"]["n_it"] > 1
    assert codes("cvo_break_b") == [2] and not np.array_equal(f["cvo_break_b"]["state1"]["R"], np.eye(3, dtype=np.float32))
    assert codes("cvo_break_b_at_3") == [0, 0, 0, 2] and codes("acvo_eps_on_a_norm")[-1] == 1 and 5 < f["acvo_eps_on_a_norm"]["n_it"] < f["acvo_default"]["n_it"]
    assert f["acvo_ell_meets_ell_max"]["trace"][1]["ell"] == np.float32(float(np.float32(0.1)) * 0.7)
    assert codes("cvo_break_a_at_0") == [1] and f["cvo_break_a_at_0"]["trace"][0]["nnz"] > 100
    assert lc.same_state({k: v for k, v in f["cvo_break_a_at_0"]["state1"].items() if k in ("R", "T")},
                         {k: v for k, v in f["cvo_break_a_at_0"]["state0"].items() if k in ("R", "T")})
    for name, want in (("cvo_far_min_step_0.2", 0.2), ("cvo_far_min_step_0.05", 0.05), ("cvo_far_min_step_1.5", 0.8)):
        assert all(t["nnz"] == 0 and t["step"] == np.float32(want) for t in f[name]["trace"]), name
    late = f["cvo_empties_at_21"]["trace"]
    assert late[0]["nnz"] > 100 and late[20]["nnz"] > 0 and all(t["nnz"] == 0 and t["step"] == np.float32(0.2) for t in late[21:])
    for name in ("cvo_small_angle", "acvo_small_angle"):
        assert all(lr.small_angle(t["omega"]) for t in f[name]["trace"]) and f[name]["n_it"] > 1, name
        t = f[name]["trace"][0]
        assert abs(t["dist"] - np.linalg.norm(np.array(t["v"], np.float64))) <= 1e-6 * t["dist"]
    assert f["cvo_long_walk"]["n_it"] == 150 and f["cvo_long_walk"]["trace"][-1]["nnz"] < f["cvo_long_walk"]["trace"][0]["nnz"] / 4


def test_runs_one_iteration_apart_are_prefixes(runs):
    """The run with max_iter = j is, bit for bit, the first j records of the run with max_iter = j + 1 and of the full run:
    what lets two consecutive states differ by exactly one update."""
    for key, chain in runs["prefixes"].items():
        full = runs["full"][key]
        for j, run in enumerate(chain):
            assert run["n_it"] == j == len(run["trace"]), (key, j)
            assert lc.same_records(run["trace"], full["trace"][:j]), (key, j)


def test_carry_over(runs):
    """Two align() calls on one state and a third with max_iter = 0: the second replay starts from the carried R, T, ell (cvo:
    0.03, back to 0.10 after k = 3; acvo: reset to ell_init) and multiplies accum_transform once more; with max_iter = 0
    nothing moves and accum_transform is multiplied by the carried transform again."""
    for (mode, size), (a, b, c) in runs["carry"].items():
        assert lc.same_state(a["state1"], b["state0"]) and lc.same_state(b["state1"], c["state0"])
        assert b["n_it"] > 4 and c["n_it"] == 0
        if mode == "cvo":
            assert [t["ell"] for t in b["trace"][:5]] == [np.float32(0.03)] * 4 + [np.float32(0.10)]
        assert not np.array_equal(b["state1"]["accum_transform"], a["state1"]["accum_transform"])
        assert np.array_equal(c["state1"]["transform"], b["state1"]["transform"])
        assert np.array_equal(c["state1"]["prev_transform"], b["state1"]["transform"])
        for k in ("R", "T", "ell", "iter"):
            assert np.array_equal(c["state1"][k], b["state1"][k]) or (mode == "acvo" and k == "ell")


@pytest.mark.parametrize("name", sorted(lc.MUTANTS))
def test_the_cases_reject_every_mutant(runs, name):
    """A head with this error would fail the judge on some run of the cases, under the same tolerances (Python only)."""
    first = next((f for f in _judge_each(runs, lc.MUTANTS[name]) if not f[1].startswith("condition:")), None)
    print(name, "-> first told apart by", first)
    assert first is not None, name


@pytest.mark.parametrize("name", sorted(lc.UNREACHABLE_MUTANTS))
def test_the_unreachable_mutant_survives(runs, name):
    """Double norms in cvo's break A: no case without a borderline record can tell them from float norms (loop_ref_cases'
    docstring) -- held here, so that the list of mutants does not claim more than is shown."""
    assert not _judge_all(runs, rules=lc.UNREACHABLE_MUTANTS[name])
