"""CPU: the oracle's pair weight (oracle/cvo_oracle.c pair_weight: members and float32 weights) against the float64
reference of tests/cvo_iteration_ref.py at the parameter sets of tests/pair_weight_cases.py -- thresholds down to 1e-38,
exponents up to 83, each of the three cuts deciding, thresholds at and above sigma^2 -- on the star of isolated pairs and
on dense pairs.  The bound is iteration_ref_cases.weight_bound, derived there and unchanged; nothing is fitted.  The float64
reference's own exp is held to mpmath at 60 digits, so that the reference is high precision in fact.  Every test prints its
worst error as a fraction of the bound (pytest -s); DESIGN.md section 2 records them.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvo_iteration_ref as ref  # noqa: E402
import iteration_ref_cases as ic  # noqa: E402
import pair_weight_cases as pw  # noqa: E402


def _judge(p, ell, rows, cols, val, a, d2, d2c, sure_in, border, sure_out, tag):
    """Members between surely-in and surely-out; weights within weight_bound.  a, d2, d2c and the classes are indexed by
    (rows, cols) -- or, for a star, by rows alone.  Returns (worst error / bound, members, borderline pairs)."""
    idx = (rows,) if a.ndim == 1 else (rows, cols)
    mask = np.zeros(a.shape, bool)
    mask[idx] = True
    assert not (sure_in & ~mask).any(), (tag, "missing", int((sure_in & ~mask).sum()))
    assert not (sure_out & mask).any(), (tag, "extra", int((sure_out & mask).sum()))
    assert np.array_equal(sure_in, mask & ~border), tag   # (outside the borderline pairs the member set IS the reference's)
    if not len(rows):
        return 0.0, 0, int(border.sum())
    am = a[idx]
    bound = ic.weight_bound(p, ell, am, d2[idx], d2c[idx])
    frac = float(np.max(np.abs(val.astype(np.float64) - am) / bound))
    assert frac <= 1.0, (tag, frac)
    return frac, len(rows), int(border.sum())


@pytest.fixture(scope="module")
def stars(po):
    return [pw.star(po, name, ell, ps) for name, ell, ps in pw.star_cases()]


def test_star_members_and_weights_within_the_bound(stars):
    """Every star: the oracle's members are the reference's outside the borderline pairs, and every kept float32 weight is
    within u (5 + 5 E1 + 7 E2) a (MATLAB: u (7 + 5 E1) a) of the float64 one."""
    worst, count, border = {}, {}, {}
    for st in stars:
        s = st["set"]
        tag = (s.name, st["ell"], st["pose"])
        f, n, b = _judge(st["p"], st["ell"], st["rows"], st["rows"], st["val"], st["a"], st["d2"], st["d2c"], st["sure_in"],
                         st["border"], st["sure_out"], tag)
        assert (n > 200) == s.members and (s.members or n == 0), (tag, n)
        worst[s.name] = max(worst.get(s.name, 0.0), f)
        count[s.name] = count.get(s.name, 0) + n
        border[s.name] = border.get(s.name, 0) + b
    for name in worst:
        print("star %-18s members %6d  borderline %d  worst error / bound %.3f" % (name, count[name], border[name], worst[name]))
    print("star: borderline pairs left out of the float64 comparison, all sets:", sum(border.values()))


def test_dense_members_and_weights_within_the_bound(pkg, po):
    """The dense pairs (300, 260) and (257, 63) at the three poses of iteration_ref_cases.poses: the same two statements."""
    total_border = 0
    for s in pw.SETS:
        ell = pw.dense_ell(s)
        worst = members = border = 0
        for n, m in pw.DENSE_SIZES:
            for ps in ic.poses(ell):
                d = pw.dense_case(pkg, po, s.name, n, m, ell, ps)
                f, k, b = _judge(d["p"], ell, d["rows"], d["cols"], d["val"], d["a"], d["d2"], d["d2c"], d["sure_in"], d["border"],
                                 d["sure_out"], (s.name, n, m, ps[0]))
                worst, members, border = max(worst, f), members + k, border + b
        assert (members > 500) == s.members and (s.members or members == 0), (s.name, members)
        total_border += border
        print("dense %-18s members %7d  borderline %d  worst error / bound %.3f" % (s.name, members, border, worst))
    print("dense: borderline pairs left out of the float64 comparison, all sets:", total_border)


def test_each_set_reaches_the_exponents_it_is_meant_to(stars):
    """Kept pairs of every star of a set past the magnitudes of pair_weight_cases.REACH, so that a later change of a case
    cannot pull it back into [-6, 0]; the subnormal set keeps weights below FLT_MIN; in cvo_colour_cut and cvo_radius_cut
    the named cut alone removes pairs."""
    for st in stars:
        s, p = st["set"], st["p"]
        E1, E2 = pw.exponents(p, st["ell"], st["d2"], st["d2c"])
        keep = np.zeros(len(E1), bool)
        keep[st["rows"]] = True
        for which, mag, least in pw.REACH.get(s.name, []):
            n = int((keep & ((E1 if which == "E1" else E2) > mag)).sum())
            print("%s ell %g %s: %d kept pairs with %s > %g (largest %.1f)"
                  % (s.name, st["ell"], st["pose"], n, which, mag, float((E1 if which == "E1" else E2)[keep].max())))
            assert n >= least, (s.name, st["ell"], st["pose"], which, n)
        if s.name == "cvo_sp1e-6":
            assert int((keep & (E2 > 6.0)).sum()) >= 200
        if s.name == "cvo_subnormal":
            n = int((st["val"] < pw.FLT_MIN).sum())
            print("%s ell %g %s: %d of %d kept weights are subnormal, largest exponent %.1f"
                  % (s.name, st["ell"], st["pose"], n, len(st["val"]), float(E1[keep].max())))
            assert n >= 1 and E1[keep].max() > 80.0
        if s.name in ("cvo_colour_cut", "cvo_radius_cut", "cvo_wide"):
            tau, tau_c = ref.cuts(p, st["ell"], ic.c_sp_of(p))
            sp = float(np.float32(p.sp_thres))
            alone = dict(d2=int(((st["d2"] >= tau) & (st["d2c"] < tau_c) & (st["a"] > sp)).sum()),
                         d2c=int(((st["d2"] < tau) & (st["d2c"] >= tau_c) & (st["a"] > sp)).sum()))
            print("%s ell %g %s: pairs removed by one cut alone %s" % (s.name, st["ell"], st["pose"], alone))
            assert s.name != "cvo_colour_cut" or alone["d2c"] >= 20
            assert s.name == "cvo_colour_cut" or alone["d2"] >= 20
        if s.name == "cvo_tight":
            assert E1[keep].max() < 0.11


def test_float64_exp_is_within_an_ulp_of_the_true_value(stars):
    """numpy's float64 exp -- the reference's -- against mpmath at 60 digits at the exponents the sets reach, 300 samples
    of either exponent per set: within one ulp of the true value, so a float32 weight's error against the reference is the
    float32 side's."""
    import mpmath
    mpmath.mp.dps = 60
    for s in pw.SETS:
        if not s.members:
            continue
        args = []
        for st in stars:
            if st["set"] is s:
                ell, c_ell = float(np.float32(st["ell"])), float(np.float32(st["p"].c_ell))
                args += [-st["d2"][st["rows"]] / (2.0 * ell * ell), -st["d2c"][st["rows"]] / (2.0 * c_ell * c_ell)]
        x = np.concatenate(args)
        x = x[np.linspace(0, len(x) - 1, 600).astype(int)]
        x = np.concatenate([x, [x.min()]])
        got = np.exp(x)
        worst = 0.0
        for xv, gv in zip(x.tolist(), got.tolist()):
            true = mpmath.exp(mpmath.mpf(xv))
            worst = max(worst, float(abs(mpmath.mpf(gv) - true) / mpmath.mpf(math.ulp(float(true)))))
        print("%-18s exp at %d arguments down to %.1f: worst distance %.3f ulp" % (s.name, len(x), float(x.min()), worst))
        assert worst <= 1.0, (s.name, worst)


@pytest.mark.parametrize("name", [s.name for s in pw.SETS if not s.members])
def test_no_member_sets_keep_nothing_and_align_breaks_at_once(pkg, po, name):
    """tau <= 0 or tau_c <= 0: the oracle keeps no pair, on the star and on the dense pairs, and its align ends as
    tests/test_gpu_parity.py test_empty_gram_matrix_breaks_at_once describes: one iteration, break A at k = 0 with
    step = min_step, the pose untouched."""
    s = pw.BY_NAME[name]
    p = s.params(po)
    tau, tau_c = po.thresholds(p, 0.1)
    assert tau <= 0.0 or tau_c <= 0.0, (tau, tau_c)
    for ps in pw.POSES:
        assert len(pw.star(po, name, s.ells[0], ps)["rows"]) == 0
    xf, ff, xm, fm = ic.clouds(pkg, s.mode, 300, 260)
    p.max_iter = 30
    st = po.init_state(p)
    n_it, tr = po.align(p, st, xf, ff, xm, fm, search=po.SEARCH_GRID, trace_cap=30)
    assert n_it == 1 and tr[0]["exit_code"] == 1 and tr[0]["nnz"] == 0 and tr[0]["step"] == np.float32(p.min_step)
    assert np.array_equal(po.state_matrices(st)[0], np.eye(4, dtype=np.float32))
