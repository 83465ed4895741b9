"""CPU: the pixel selector's three statements held to each other bit for bit on the cases of selector_ref_cases.py --
the REFERENCE'S OWN code (oracle/_ref/libselector_ref.so, compiled from thirdparty/PixelSelector2.cpp where it lies),
the C oracle (fe_cell_thresholds + fe_make_maps, what the HIP kernels are held to) and the plain restatement
(selector_ref.py).  Where oracle/_ref is not built the reference's results come from tests/golden/selector_ref.json
(its digests, recorded by tools/make_golden.py).  Then: the census of what the cases reach, and every mutant of the
restatement rejected."""
import hashlib
import json
import os

import numpy as np
import pytest

import selector_ref as sr
import selector_ref_cases as sc
from oracle import pyoracle_fe as fo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selector_ref.json")
FIELDS = ("count", "pot_used", "reselected", "num_have")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(res):
    """What the fixture keeps of one run"""
    out = {k: int(res[k]) for k in FIELDS}
    out.update(sha_ths=sha(res["ths"]), sha_ths_smoothed=sha(res["ths_smoothed"]), sha_map=sha(res["map"]))
    return out


def planes_of(pkg, case):
    bgr, _ = sc.frame(pkg, case)
    return tuple(fo.pyramid(fo.gray(bgr))[3])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["runs"]


@pytest.fixture(scope="module")
def planes(pkg):
    return {c.name: planes_of(pkg, c) for c in sc.CASES}


@pytest.fixture(scope="module")
def pattern():
    return sc.libc_pattern(PY_PIXELS)


PY_PIXELS = max(c.w * c.h for c in sc.CASES if sc.runs_in_python(c))


@pytest.fixture(scope="module")
def py_runs(planes, pattern):
    """selector_ref.py on every case it takes, every budget: {(case name, budget): result}"""
    out = {}
    for c in sc.CASES:
        if sc.runs_in_python(c):
            memo = {}
            for b in c.budgets:
                out[c.name, b] = sr.make_maps(*planes[c.name], b, pattern, memo=memo)
    return out


def test_groups_are_what_the_sizes_say():
    for c in sc.CASES:
        if c.group == "raw":
            assert not sc.reads_unwritten(c.w, c.h), c.name
        if c.group == "defined":
            assert sc.reads_unwritten(c.w, c.h) and (c.w, c.h) in sc.DEFINED_SIZES, c.name
        assert c.budgets == (1, 7, 50, 400, c.w * c.h // 8, c.w * c.h, 10 ** 6)
    assert {(c.w, c.h) for c in sc.CASES if c.group == "raw"} == {(96, 64), (128, 192), (65, 67), (644, 483)}
    assert {(c.w, c.h) for c in sc.CASES if c.group == "defined"} == set(sc.DEFINED_SIZES)
    assert sorted((c.w, c.h) for c in sc.CASES if c.group == "large") == [(640, 480), (1280, 720), (1280, 720)]
    assert sc.reads_unwritten(1280, 720) and not sc.reads_unwritten(640, 480)
    assert set(sr.OUT_OF_REACH) <= set(sr.MUTANTS)


def test_pattern_is_the_oracles(pattern):
    assert np.array_equal(np.frombuffer(pattern, np.uint8), fo.random_pattern(len(pattern)))


def test_fixture_lists_every_run(golden):
    assert sorted(golden) == sorted("%s/%d" % (c.name, b) for c in sc.CASES for b in c.budgets)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_reference_oracle_and_restatement_agree(case, planes, golden, py_runs):
    """ths, thsSmoothed, the map, the count, the potential used and the re-selection flag, bit for bit.  Raw group: the
    reference as it stands; the others: its unwritten cells defined as the last cell.  (On the sizes of the defined
    group with the cells left undefined the reference's map is indeterminate: nothing is asserted about it.)"""
    for b in case.budgets:
        want = golden["%s/%d" % (case.name, b)]
        if fo.ref_selector_lib() is not None:
            ref = fo.ref_make_maps(*planes[case.name], b, sc.define_unwritten(case))
            assert record(ref) == want, "the compiled reference left its recorded result at %s/%d" % (case.name, b)
            if case.group == "raw":   # ... and defining the cells changes nothing where none is read
                assert record(fo.ref_make_maps(*planes[case.name], b, True)) == want
        assert record(fo.make_maps(*planes[case.name], b)) == want, "oracle != reference at %s/%d" % (case.name, b)
        if sc.runs_in_python(case):
            assert record(py_runs[case.name, b]) == want, "selector_ref.py != reference at %s/%d" % (case.name, b)


def test_census_is_complete(planes, py_runs, golden):
    """Every condition the issue of this file names is met by the cases.  Potentials, re-selections and sub-sampling over
    all runs, from the recorded reference (which the test above holds); the picks (levels, cut blocks, ties, cells past
    the end) from the final selection pass of the runs selector_ref.py takes -- the compiled reference's pass where
    oracle/_ref is built, else the restatement's."""
    census = {}
    have_ref = fo.ref_selector_lib() is not None
    for c in sc.CASES:
        for b in c.budgets:
            rec = golden["%s/%d" % (c.name, b)]
            pre = sm = None
            if sc.runs_in_python(c):
                if have_ref:
                    pre, n = fo.ref_select(*planes[c.name], rec["pot_used"], sc.define_unwritten(c))
                    sm = fo.ref_make_maps(*planes[c.name], b, sc.define_unwritten(c))["ths_smoothed"]
                else:
                    sm = py_runs[c.name, b]["ths_smoothed"]
                    pre, n = sr.select(*planes[c.name], sm, rec["pot_used"])
                assert sum(n) == rec["num_have"]
            sc.census_add(census, c, b, rec, rec["num_have"], planes[c.name], sm, pre)
    print("census: %s" % json.dumps(census))
    assert sorted(census) == sorted(sc.CENSUS_KEYS)
    assert all(v > 0 for v in census.values()), census


def test_strict_greater_on_the_built_steps(planes, py_runs):
    """Built frame A: every threshold is exactly 49; the step of 14 gives ag0 == 49 exactly and is not selected at level
    0, the step of 15 gives 56.25 and is"""
    for c in sc.CASES:
        if c.kind != "steps":
            continue
        a0 = planes[c.name][0]
        assert (a0[4:-4, sc.STEP14_X:sc.STEP14_X + 2] == 49.0).all() and (a0[4:-4, sc.STEP15_X:sc.STEP15_X + 2] == 56.25).all()
        for b in c.budgets:
            res = py_runs[c.name, b]
            assert (res["ths_smoothed"] == 49.0).all()
        _, sm = sr.make_hists(a0)
        for pot in (1, 3):
            mp, n = sr.select(*planes[c.name], sm, pot)
            ys, xs = np.nonzero(mp == 1)
            assert n[0] > 0 and set(xs.tolist()) <= {sc.STEP15_X, sc.STEP15_X + 1}


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_mutant_is_rejected(mutant, planes, pattern, py_runs, golden):
    if mutant in sr.OUT_OF_REACH:
        # out of reach by arithmetic, not for want of a case: the restatement says why, and no case may differ
        hits = [(c.name, b) for c in sc.CASES if c.w * c.h < 7000 for b in c.budgets[:4]
                if record(sr.make_maps(*planes[c.name], b, pattern, mutant=mutant)) != golden["%s/%d" % (c.name, b)]]
        assert not hits and sr.OUT_OF_REACH[mutant]
        return
    order = sorted((c for c in sc.CASES if c.w * c.h <= sc.PY_MAX_PIXELS), key=lambda c: c.w * c.h)
    for c in order:
        memo = {}
        for b in c.budgets:
            if record(sr.make_maps(*planes[c.name], b, pattern, mutant=mutant, memo=memo)) != golden["%s/%d" % (c.name, b)]:
                print("mutant %s rejected by %s/%d" % (mutant, c.name, b))
                return
    pytest.fail("mutant %s survives every case" % mutant)
