"""CPU: the two statements of the selector's depth mode (tests/selector_depth_ref.py: the reference's walk and the
vectorised closed form, both with a validity plane) held to each other and to the existing restatement of the
reference (tests/selector_ref.py); every mutant told apart by a named case; the census of what the hole patterns of
tests/selector_depth_cases.py reach."""
import json

import numpy as np
import pytest

import selector_depth_cases as dc
import selector_depth_ref as dr
import selector_ref as sr
import selector_ref_cases as sc
from oracle import pyoracle_fe as fo

PY_CASES = [c for c in sc.CASES if sc.runs_in_python(c)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("map", "ths_smoothed")) and \
        all(a[k] == b[k] for k in ("count", "pot_used", "reselected", "num_have", "char_th"))


@pytest.fixture(scope="module")
def pattern():
    return sc.libc_pattern(sc.PY_MAX_PIXELS)


@pytest.fixture(scope="module")
def frames(pkg):
    """per frame of the depth cases: planes, smoothed thresholds, Canny edges, and the validity plane of each pattern"""
    out = {}
    for c in dc.FRAMES:
        bgr, _ = sc.frame(pkg, c)
        gray = fo.gray(bgr)
        planes = tuple(fo.pyramid(gray)[3])
        sm = dr.make_hists(planes[0])[1]
        valid = {p: dc.hole_pattern(p, *planes, sm, seed=c.seed) for p in dc.PATTERNS}
        out[c.name] = {"case": c, "planes": planes, "sm": sm, "edges": fo.canny(fo.blur3(gray)), "valid": valid}
    return out


@pytest.fixture(scope="module")
def runs(frames, pattern):
    """{(frame, pattern, budget): (closed form's make_maps, the walk's)}"""
    out = {}
    for name, f in frames.items():
        c = f["case"]
        for p in dc.PATTERNS:
            memo_c, memo_w = {}, {}
            for b in dc.budgets(c.w, c.h):
                out[name, p, b] = (dr.make_maps(*f["planes"], b, pattern, f["valid"][p], dr.select_closed, memo=memo_c),
                                   dr.make_maps(*f["planes"], b, pattern, f["valid"][p], dr.select_walk, memo=memo_w))
    return out


def test_the_cases_are_the_issues(frames):
    assert {(f["case"].w, f["case"].h) for f in frames.values()} == set(dc.SIZES)
    assert len(frames) == len(dc.FRAMES) == 9
    assert all(sc.reads_unwritten(w, h) for w, h in ((65, 70), (127, 193)))
    for f in frames.values():
        c = f["case"]
        assert dc.budgets(c.w, c.h) == (1, 50, c.w * c.h // 8, 10 ** 6)
        share = {p: 1.0 - f["valid"][p].mean() for p in dc.PATTERNS}
        assert share["none"] == 0.0 and share["all"] == 1.0
        assert 0.28 < share["blobs30"] < 0.40 and 0.88 < share["blobs90"] < 0.95, share
        assert 24 <= f["valid"]["few"].sum() <= 48
        assert share["checkerboard"] == pytest.approx(0.5, abs=0.01) and share["half"] == pytest.approx(0.5, abs=0.01)
        assert (~f["valid"]["columns"]).sum(axis=1).max() <= (c.w + 2) // 3


@pytest.mark.parametrize("case", PY_CASES, ids=lambda c: c.name)
def test_all_valid_is_the_reference(pkg, case, pattern):
    """with Z != 0 everywhere both forms are selector_ref.py's select and make_maps, thresholds included, bit for bit"""
    bgr, _ = sc.frame(pkg, case)
    planes = tuple(fo.pyramid(fo.gray(bgr))[3])
    full = np.ones((case.h, case.w), bool)
    ths, sm = sr.make_hists(planes[0])
    got = dr.make_hists(planes[0], full)
    assert np.array_equal(_bits(got[0]), _bits(ths)) and np.array_equal(_bits(got[1]), _bits(sm))
    for pot in (1, 2, 3, 5, 40):
        want = sr.select(*planes, sm, pot)
        for form in (dr.select_closed, dr.select_walk):
            mp, n = form(*planes, sm, pot, full)
            assert np.array_equal(_bits(mp), _bits(want[0])) and n == want[1], (form.__name__, pot)
    memo, memo_c = {}, {}
    for b in case.budgets:
        want = sr.make_maps(*planes, b, pattern, memo=memo)
        assert _same(dr.make_maps(*planes, b, pattern, full, memo=memo_c), want), b


def test_the_two_forms_agree(runs):
    for key, (closed, walk) in runs.items():
        assert _same(closed, walk), key


def test_consequences_of_the_contract(frames, runs):
    """every chosen pixel is valid; thresholds do not move with the holes; "none" is the unmasked selector"""
    for (name, p, b), (res, _) in runs.items():
        f = frames[name]
        assert not (res["map"] != 0)[~f["valid"][p]].any(), (name, p, b)
        assert np.array_equal(_bits(res["ths_smoothed"]), _bits(f["sm"]))
        assert res["count"] == np.count_nonzero(res["map"])


# what tells each mutant from the contract: (frame, hole pattern, budget)
MUTANT_CASE = {
    "valid_level0_only": ("tex1_s2_96x64", "level0_gone", 50),
    "valid_after_select": ("tex1_s2_96x64", "winner", 50),
    "invalid_sets_marks": ("tex1_s2_96x64", "level0_gone", 50),
    "valid_at_level_pixel": ("tex1_s2_96x64", "columns", 768),
    "ths_valid_only": ("tex1_s9_127x193", "level0_gone", 50),
    "topup_ignores_depth": ("tex1_s2_96x64", "few", 10 ** 6),
}


def _with_topup(res, f, valid, b, mutant=None):
    if not dr.topup_due(res["count"], b):
        return res["map"], 0
    mp, added, _ = dr.topup(res["map"], f["edges"], valid, mutant)
    return mp, added


@pytest.mark.parametrize("mutant", dr.MUTANTS)
def test_mutant_is_told_apart(mutant, frames, runs, pattern):
    assert sorted(MUTANT_CASE) == sorted(dr.MUTANTS)
    name, p, b = MUTANT_CASE[mutant]
    f = frames[name]
    valid = f["valid"][p]
    true = runs[name, p, b][0]
    mut = dr.make_maps(*f["planes"], b, pattern, valid, mutant=mutant)
    a, b_ = _with_topup(true, f, valid, b), _with_topup(mut, f, valid, b, mutant)
    differs = not np.array_equal(a[0], b_[0]) or any(true[k] != mut[k] for k in ("count", "pot_used", "reselected"))
    assert differs, "mutant %s survives %s" % (mutant, (name, p, b))
    # ... and on a frame without holes no mutant shows: they are misreadings of the validity alone
    full = f["valid"]["none"]
    same = dr.make_maps(*f["planes"], b, pattern, full, mutant=mutant)
    assert _same(same, runs[name, "none", b][0])


def _blocks(h, w, side):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // side) * ((w + side - 1) // side) + xs // side


def test_census(frames, runs):
    census = dict.fromkeys(("b2_moved_to_second", "b3_fell_to_level_1", "b4_fell_to_level_2", "reselected_differs",
                            "pot_used_differs", "topup_passed_a_hole", "no_valid_pixel"), 0)
    for name, f in frames.items():
        c, planes, sm = f["case"], f["planes"], f["sm"]
        h, w = c.h, c.w
        th0, _, _ = dr._cell_thresholds(sm, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        cand0 = (xs >= 4) & (xs < w - 5) & (ys >= 4) & (ys <= h - 4) & (planes[0] > th0)
        plain = dr.select_walk(*planes, sm, 3, f["valid"]["none"])[0]
        b2, b3, b4 = _blocks(h, w, 3), _blocks(h, w, 6), _blocks(h, w, 12)
        for p in dc.PATTERNS:
            valid = f["valid"][p]
            got = dr.select_walk(*planes, sm, 3, valid)[0]
            if p == "winner":
                for q in np.flatnonzero((got == 1).ravel()):
                    inside = (b2.ravel() == b2.ravel()[q]) & cand0.ravel()
                    vals = np.sort(planes[0].ravel()[inside])[::-1]
                    was = np.flatnonzero(inside & (plain.ravel() == 1))
                    if len(vals) >= 2 and len(was) == 1 and not valid.ravel()[was[0]] and \
                            vals[0] > vals[1] == planes[0].ravel()[q]:
                        census["b2_moved_to_second"] += 1
            for q in np.flatnonzero((got == 2).ravel()):
                inside = b3.ravel() == b3.ravel()[q]
                if (plain.ravel()[inside] == 1).any() and not valid.ravel()[inside & cand0.ravel()].any():
                    census["b3_fell_to_level_1"] += 1
            for q in np.flatnonzero((got == 4).ravel()):
                inside = b4.ravel() == b4.ravel()[q]
                if ((plain.ravel()[inside] == 1) | (plain.ravel()[inside] == 2)).any():
                    census["b4_fell_to_level_2"] += 1
            for b in dc.budgets(w, h):
                res, base = runs[name, p, b][0], runs[name, "none", b][0]
                census["reselected_differs"] += res["reselected"] != base["reselected"]
                census["pot_used_differs"] += res["pot_used"] != base["pot_used"]
                if dr.topup_due(res["count"], b):
                    mp, added, passed = dr.topup(res["map"], f["edges"], valid)
                    census["topup_passed_a_hole"] += passed > 0
                    assert not (mp != 0)[~valid].any() and np.count_nonzero(mp) == res["count"] + added
                if p == "all":
                    # numHave 0: quotia = +inf, the ideal potential 1, a second pass at potential 1, nothing kept
                    assert (res["first_have"], res["num_have"], res["count"]) == (0, 0, 0)
                    assert (res["pot_used"], res["reselected"], res["char_th"]) == (1, 1, None)
                    assert dr.topup_due(0, b) == (b >= 3) and dr.topup(res["map"], f["edges"], valid)[1] == 0
                    census["no_valid_pixel"] += 1
    print("census: %s" % json.dumps({k: int(v) for k, v in census.items()}))
    assert all(v > 0 for v in census.values()), census
