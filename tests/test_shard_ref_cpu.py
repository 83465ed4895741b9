"""CPU: the proof that the judges of the row-sharded passes and loop judge (tests/shard_cases.py), with the oracle in the
library's place behind the same calls -- tests/test_gpu_shard_ref.py runs them over the library.

    the cut lists hold the boundaries they are named for (a wave, a tile, n_fixed, empty ranks, the clamps);
    the row-restricted reference summed over every cut list is the unrestricted one: counts exactly, sums to the
      partition bound;
    the conditions on the cases: no borderline pair at the poses of the passes, at most one per 1 000 members along the
      oracle's registrations, members in every shard of more than two rows of (300, 260) at ell >= 0.06;
    the judges pass on the oracle: the passes of every shard of every cut list, whole registrations of host-thread ranks
      around a barrier with a time-out (the empty rank included), a shard without an exchange;
    every mutant of the DRIVER fails a named judge by a value.
Every test prints its worst error as a fraction of its tolerance (pytest -s); DESIGN.md section 2 records them.
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostile_cases as hc  # noqa: E402
import iteration_ref_cases as ic  # noqa: E402
import loop_ref_cases as lc  # noqa: E402
import shard_cases as sc  # noqa: E402
from iteration_ref_judge import Ref  # noqa: E402


def _show(worst, stats=None):
    print("worst (error / tolerance, error):", {k: (round(v[0], 4), float("%.3g" % v[1])) for k, v in sorted(worst.items())},
          dict(stats or {}))


def _params(po, mode):
    return po.default_params(ic.mode_id(po, mode))


def _opener(po, p, mode, clouds, shards=None, mutate=None, ayy_first=None):
    """open_ctx of shard_cases.judge_passes over the oracle; mutate: a MUTANT_SHARDS entry (what the driver hands on)."""
    n, m = len(clouds[0]), len(clouds[2])

    def open_ctx(shard):
        if shard is not None and mutate is not None:
            shard = mutate(shards, shards.index(shard), n, m)
        return sc.OracleContext(po, p, mode, clouds, shard, ayy_first=ayy_first if shard is not None else None)
    return open_ctx


def test_the_cut_lists(pkg):
    """The cut lists: non-decreasing from 0, the even ones cvo_hip_shard_range's own, and over 300 rows the boundaries
    named: 1 row, 63 / 64 / 65, 255 / 256 / 257, two empty ranks, a clamped end, a range past the cloud."""
    for n in (300, 260, 257, 64, 1):
        for name, cuts in sc.cut_lists(n).items():
            assert cuts[0] == 0 and all(a <= b for a, b in zip(cuts, cuts[1:])), (n, name, cuts)
            cl = [sc.clamp(lo, hi, n) for lo, hi in sc.ranges(cuts)]
            assert sorted(r for lo, hi in cl for r in range(lo, hi)) == list(range(n)), (n, name)
        for world in (2, 3, 4, 8):
            assert sc.ranges(sc.even(n, world)) == [pkg.capi.shard_range(n, r, world) for r in range(world)]
    c = sc.cut_lists(300)
    assert c["first_row"] == (0, 1, 300) and c["last_row"] == (0, 299, 300) and c["wave"] == (0, 63, 64, 65, 300)
    assert c["tile"] == (0, 255, 256, 257, 300) and c["straddle"] == (0, 65, 130, 300)
    assert c["empty_first"] == (0, 0, 300) and c["empty_last"] == (0, 300, 300)
    assert c["hi_clamped"] == (0, 150, 400) and c["lo_past_n"] == (0, 305, 309)
    assert sc.clamp(305, 309, 300) == (300, 300)
    assert sc.ranges(sc.cut_lists(1)["even2"])[0] == (0, 0) == pkg.capi.shard_range(1, 0, 2)
    mv = sc.moving_cut_lists(*sc.ACVO_TAIL_SIZE)
    assert [v[1] for v in mv.values()] == [259, 260, 261, 64, 150]


def test_the_restricted_reference_adds_up_to_the_whole(pkg, po):
    """Ref.shard over every cut list against the unrestricted Ref: the members of the shards are the whole's exactly
    (counts, sure-in counts and borderline pairs add up, no member twice), the sums within the partition bound, the Ayy sum
    under the row rule included; and a shard of the cloud in another order (row_ids) counts the caller's rows."""
    worst = lc.Worst()
    for mode in sc.MODES:
        for n, m in (sc.SIZES if mode != "matlab" else sc.MATLAB_SIZES):
            xf, ff, xm, fm = ic.clouds(pkg, mode, n, m)
            p = _params(po, mode)
            for ell in ic.ELLS:
                for _, R, T in ic.poses(ell)[1:]:
                    y = po.transform(R, T, xm)
                    W = Ref(p, ell, xf, ff, y, fm)
                    fl = W.flow()[0]
                    Sy = Ref(p, ell, y, fm, y, fm) if mode == "acvo" else None
                    for name, cuts in sc.cut_lists(n).items():
                        parts = [W.shard(*sc.clamp(lo, hi, n)) for lo, hi in sc.ranges(cuts)]
                        assert sum(len(s.rows) for s in parts) == len(W.rows) and sum(s.sure_in for s in parts) == W.sure_in
                        assert sum(len(s.brows) for s in parts) == len(W.brows)
                        assert np.array_equal(np.concatenate([s.rows for s in parts]), W.rows)   # (cut lists ascend: CSR order)
                        fls = [s.flow()[0] for s in parts]
                        for key, scale in (("omega_d", "s_omega"), ("v_d", "s_v"), ("sum_a", "s_a"), ("sum_a_d2", "s_a_d2")):
                            err = np.abs(sum(np.asarray(f[key]) for f in fls) - fl[key])
                            worst.see("partition", err, 2.0 * len(W.rows) * sc.U53 * np.asarray(fl[scale]))
                            assert np.all(err <= 2.0 * len(W.rows) * sc.U53 * np.asarray(fl[scale])), (mode, n, m, ell, name, key)
                        if Sy is not None:
                            mparts = [Sy.shard(*sc.clamp(lo, hi, m)) for lo, hi in sc.ranges(sc.cut_lists(m)[name])]
                            want = Sy.self_flow(n)
                            got = sum(s.self_flow(n)["sum_a_d2"] for s in mparts)
                            assert abs(got - want["sum_a_d2"]) <= 2.0 * len(Sy.rows) * sc.U53 * want["s_a_d2"]
                            assert (want["sum_a_d2"] > 0) == (m > n and len(Sy.rows) > m)
    # another order of the rows: the Ayy rule follows the caller's index
    xf, ff, xm, fm = ic.clouds(pkg, "acvo", *sc.ACVO_TAIL_SIZE)
    n, m = sc.ACVO_TAIL_SIZE
    p = _params(po, "acvo")
    ids = np.random.default_rng(5).permutation(m)
    A, B = Ref(p, 0.1, xm, fm, xm, fm), Ref(p, 0.1, xm[ids], fm[ids], xm[ids], fm[ids], row_ids=ids)
    assert abs(A.self_sum(n)[0] - B.self_sum(n)[0]) <= 2.0 * len(A.rows) * sc.U53 * A.self_flow(n)["s_a_d2"]
    assert A.self_sum(n)[0] > 0 and len(A.rows) == len(B.rows)
    _show(worst)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("cut", sc.CUT_NAMES)
def test_the_oracle_passes_the_judges_of_the_passes(pkg, po, mode, cut):
    """Part A with the oracle's passes over the rows of every shard: per shard the count, the flow sums, the step
    coefficients (the whole cloud's float32 twist and the three samples), for acvo the Axx and Ayy sums and counts and
    function_inner_product; an empty shard exactly zero (NaN); the partition's counts exactly and sums to the bound.  The
    conditions on the cases: no borderline pair; every shard of (300, 260) with more than two rows has members at every
    pose at ell >= 0.06 (the least is printed), the shards of one or two rows at one pose at least -- a single point need
    not have a member at every pose."""
    worst, stats = lc.Worst(), sc.PassStats()
    for n, m in (sc.SIZES if mode != "matlab" else sc.MATLAB_SIZES):
        clouds = ic.clouds(pkg, mode, n, m)
        p = _params(po, mode)
        shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
        sc.judge_passes(pkg, _opener(po, p, mode, clouds), po.transform, p, mode, clouds, shards, ic.ELLS, ic.poses, worst, stats,
                        steps=(mode != "matlab"), twist_seed=n * 1000 + m)
    _show(worst, stats)
    assert stats["borderline"] == 0 and stats["members"] > 1000
    assert stats.get("least_members", 1) > 0 and stats.get("members_of_small_shards", 1) > 0, stats


@pytest.mark.parametrize("mcut", sorted(sc.moving_cut_lists(*sc.ACVO_TAIL_SIZE)))
def test_the_oracle_passes_the_judges_at_the_moving_row_cuts(pkg, po, mcut):
    """acvo 260 x 300: the moving rows cut at n_fixed - 1, n_fixed, n_fixed + 1, at 64 and evenly, the fixed rows evenly."""
    n, m = sc.ACVO_TAIL_SIZE
    worst, stats = lc.Worst(), sc.PassStats()
    clouds = ic.clouds(pkg, "acvo", n, m)
    p = _params(po, "acvo")
    shards = sc.shards_of(sc.even(n, 2), sc.moving_cut_lists(n, m)[mcut])
    sc.judge_passes(pkg, _opener(po, p, "acvo", clouds), po.transform, p, "acvo", clouds, shards, ic.ELLS, ic.poses, worst, stats,
                    twist_seed=n * 1000 + m)
    _show(worst, stats)
    assert stats["borderline"] == 0


@pytest.mark.parametrize("name,mode,ell,pose", sc.HOSTILE)
def test_the_oracle_passes_the_judges_on_hostile_clouds(pkg, po, name, mode, ell, pose):
    """far600 and dup of tests/hostile_cases.py at their own size, cut at (0, 65, 130, n), one length scale and one pose."""
    clouds = hc.clouds(pkg.data, name, acvo=(mode == "acvo"))
    n, m = len(clouds[0]), len(clouds[2])
    p = _params(po, mode)
    worst, stats = lc.Worst(), sc.PassStats()
    shards = sc.shards_of(sc.cut_lists(n)[sc.HOSTILE_CUT], sc.cut_lists(m)[sc.HOSTILE_CUT])
    sc.judge_passes(pkg, _opener(po, p, mode, clouds), po.transform, p, mode, clouds, shards, [ell],
                    lambda _: [hc.poses(clouds[0])[pose]], worst, stats, twist_seed=7)
    _show(worst, stats)
    assert stats["members"] > 1000 and stats["borderline"] <= sc.BORDER_CAP * stats["members"], stats


def _loop(pkg, po, case):
    _, mode, name, (n, m) = case
    clouds = lc.clouds(pkg, mode, n, m, lc.setting(name)[3])
    ident = np.arange(n), np.arange(m)
    dev = ((clouds[0], clouds[1], ident[0]), (clouds[2], clouds[3], ident[1]))
    return mode, name, n, m, clouds, dev


@pytest.mark.parametrize("cut", sc.LOOP_CUT_NAMES)
@pytest.mark.parametrize("case", sc.LOOP_CASES, ids=[c[0] for c in sc.LOOP_CASES])
def test_the_oracle_passes_the_judges_of_a_sharded_registration(pkg, po, case, cut):
    """Part B over the oracle's sharded loop, ranks as host threads around a barrier with a time-out: lock step bit for bit
    and equal exchange counts (the empty rank included), the unsharded iterations and transform, the replay of rank 0, and
    every record of max_iter = 0 ... J against the dense reference at its exact pose; at most one borderline pair per 1 000
    members along the way."""
    mode, name, n, m, clouds, dev = _loop(pkg, po, case)
    worst, stats = lc.Worst(), sc.PassStats()
    run_ranks, run_whole = sc.oracle_ranks(po, mode, clouds)
    shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
    sc.judge_sharded_registration(pkg, po, run_ranks, run_whole, dev, po.transform, mode, name, shards, worst, stats)
    _show(worst, stats)
    # (acvo's ell moves in every one of its first iterations: none of its judged records streams an unchanged list)
    assert stats["records"] == lc.PREFIX_J[mode] + 1 and stats["after_narrowing"] > 0, stats
    assert stats["on_reused_list"] > 0 or mode == "acvo", stats


def test_the_oracle_passes_the_judges_of_eight_ranks_and_of_the_moving_row_cuts(pkg, po):
    """The world-8 even split once (cvo 300 x 260), and acvo 260 x 300 with the moving rows cut apart from the fixed rows."""
    worst, stats = lc.Worst(), sc.PassStats()
    mode, name, n, m, clouds, dev = _loop(pkg, po, sc.LOOP_CASES[0])
    run_ranks, run_whole = sc.oracle_ranks(po, mode, clouds)
    sc.judge_sharded_registration(pkg, po, run_ranks, run_whole, dev, po.transform, mode, name,
                                  sc.shards_of(sc.even(n, 8), sc.even(m, 8)), worst, stats)
    mode, name, n, m, clouds, dev = _loop(pkg, po, sc.LOOP_CASES[1])
    run_ranks, run_whole = sc.oracle_ranks(po, mode, clouds)
    for mcut, mcuts in sc.moving_cut_lists(n, m).items():
        sc.judge_sharded_registration(pkg, po, run_ranks, run_whole, dev, po.transform, mode, name,
                                      sc.shards_of(sc.even(n, 2), mcuts), worst, stats)
    _show(worst, stats)


@pytest.mark.parametrize("mode", ["cvo", "acvo"])
def test_the_oracle_passes_the_judges_of_a_shard_without_an_exchange(pkg, po, mode):
    """allreduce = None and a shard: record 0 holds the reference's members of those rows, the run passes the replay."""
    case = sc.LOOP_CASES[0] if mode == "cvo" else sc.LOOP_CASES[1]
    mode, name, n, m, clouds, dev = _loop(pkg, po, case)
    rows = tuple(m if v is None else v for v in sc.NO_EXCHANGE_SHARD[mode])
    worst, stats = lc.Worst(), sc.PassStats()
    _, run_whole = sc.oracle_ranks(po, mode, clouds)
    full = sc.judge_no_exchange(pkg, po, run_whole, dev, po.transform, mode, name, rows, worst, stats)
    _show(worst, stats)
    assert full["n_it"] > 4


def _fails(judges, fn):
    try:
        fn()
    except sc.JudgeFailure as e:
        assert e.judge in judges, (e.judge, str(e))
        return e
    return None


def test_every_mutant_of_the_driver_fails_a_named_judge(pkg, po):
    """One plausible error of a driver each (shard_cases.MUTANT_SHARDS, MUTANT_AYY and oracle_ranks' mutants): every one fails
    a named judge by a value on at least one cut list, and the empty rank that skips its exchanges ends as the barrier's
    time-out turned into a failure in under 5 s."""
    killed, survivors = {}, {}
    ells, poses_of = [0.1], lambda ell: ic.poses(ell)[1:2]
    # part A's mutants.  The four errors in a shard's rows in cvo mode, 300 x 260, where the per-shard flow judge -- the count of
    # the members of those rows first -- is the only one that guards the rows: each must fail IT ("shard"), and by the count
    row_mutants = [k for k in sc.MUTANT_SHARDS if k != "the moving-row cut taken from the fixed-row cut"]
    mode, (n, m) = "cvo", sc.SIZES[0]
    clouds = ic.clouds(pkg, mode, n, m)
    p = _params(po, mode)
    for name in row_mutants:
        for cut in ("even2", "wave"):
            shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
            e = _fails(("shard",), lambda: sc.judge_passes(pkg, _opener(po, p, mode, clouds, shards, sc.MUTANT_SHARDS[name]), po.transform, p,
                                                           mode, clouds, shards, ells, poses_of, lc.Worst(), sc.PassStats(), twist_seed=3))
            if e is not None:
                assert "sure_in" not in str(e) and str(e).startswith("shard: ("), str(e)   # (check_flow's count assertion: its tuple)
                killed[name] = str(e)[:160]
                break
        else:
            survivors[name] = "no cut list of the candidates tells it apart"
    # acvo 260 x 300, where the Ayy rule and the moving-row cut matter
    mode, (n, m) = "acvo", sc.ACVO_TAIL_SIZE
    clouds = ic.clouds(pkg, mode, n, m)
    p = _params(po, mode)
    candidates = [sc.shards_of(sc.even(n, 2), sc.moving_cut_lists(n, m)["nf"]), sc.shards_of(sc.cut_lists(n)["wave"], sc.cut_lists(m)["wave"])]
    name = "the moving-row cut taken from the fixed-row cut"
    for shards in candidates:
        e = _fails(("shard_yy",), lambda: sc.judge_passes(pkg, _opener(po, p, mode, clouds, shards, sc.MUTANT_SHARDS[name]), po.transform, p, mode,
                                                          clouds, shards, ells, poses_of, lc.Worst(), sc.PassStats(), twist_seed=3))
        if e is not None:
            killed[name] = str(e)[:160]
            break
    else:
        survivors[name] = "no cut list of the candidates tells it apart"
    e = _fails(("shard_yy",), lambda: sc.judge_passes(pkg, _opener(po, p, mode, clouds, ayy_first=0), po.transform, p, mode, clouds,
                                                      candidates[0], ells, poses_of, lc.Worst(), sc.PassStats(), twist_seed=3))
    (killed if e is not None else survivors)[sc.MUTANT_AYY] = str(e)[:160] if e is not None else "not told apart"
    # part B's mutants: cvo 300 x 260, two ranks and an empty one
    mode, name, n, m, clouds, dev = _loop(pkg, po, sc.LOOP_CASES[0])
    for mutant, cut, judges, label in (("twice", "even2", ("iterations", "transform", "replay", "record_count"), "one rank's partials added twice"),
                                       ("skip_step", "even2", ("iterations", "transform", "replay", "record_step"),
                                        "one rank's step partials left out of the second exchange"),
                                       ("empty_skips", "empty_first", ("barrier",), "an empty rank that skips its exchanges")):
        run_ranks, run_whole = sc.oracle_ranks(po, mode, clouds, timeout=1.0, mutant=mutant)
        shards = sc.shards_of(sc.cut_lists(n)[cut], sc.cut_lists(m)[cut])
        t0 = time.monotonic()
        e = _fails(judges, lambda: sc.judge_sharded_registration(pkg, po, run_ranks, run_whole, dev, po.transform, mode, name, shards,
                                                                 lc.Worst(), sc.PassStats()))
        took = time.monotonic() - t0
        (killed if e is not None else survivors)[label] = str(e)[:160] if e is not None else "not told apart"
        if mutant == "empty_skips":
            assert took < 5.0, took
    for k, v in killed.items():
        print("killed:", k, "--", v)
    print("survivors:", survivors)
    assert not survivors, survivors
    assert len(killed) == 9
