"""GPU: the selector kernels (k_fe_hist, k_fe_smooth, k_fe_select, k_fe_decide, k_fe_count<0>, k_fe_subsample) held bit
for bit to the REFERENCE'S OWN selector on the cases of selector_ref_cases.py -- budgets from 1 to 10^6, so second-pass
potentials from 1 (one wave per 4x4 block on a busy image) to several hundred (one wave sweeping a block larger than
the image), re-selections both ways and none, sub-sampling down to a threshold of 0.

Nothing here reads the C oracle.  The truth, fed the squared-gradient planes as read back from the device:
  * oracle/_ref/libselector_ref.so (thirdparty/PixelSelector2.cpp compiled where it lies) where it is built;
  * else tests/selector_ref.py, the plain restatement, on the cases it takes (<= 25 000 pixels);
  * else (larger cases) what that library gave when tests/golden/selector_ref.json was recorded -- usable because the
    device's planes are first shown to be the recorded run's planes, digest for digest.
One context per image size lives through all its cases and budgets (cvo_fe_set_num_want between frames): counts or a
second-pass potential left over from the frame before would show."""
import hashlib
import json
import os

import numpy as np
import pytest

import selector_ref as sr
import selector_ref_cases as sc
from oracle import pyoracle_fe as fo   # (for ref_selector_lib / ref_make_maps: the reference's library, not the oracle)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selector_ref.json")
GPU_CASES = [c for c in sc.CASES if sc.on_gpu(c)]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def pattern():
    return sc.libc_pattern(sc.PY_MAX_PIXELS)


@pytest.fixture(scope="module")
def contexts(pkg):
    """One generator per image size, made when its first case runs and kept for the later ones"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[w, h] = pkg.frontend.PcdGenerator(w, h)
        return made[w, h]
    yield get
    for gen in made.values():
        gen.close()


def _set_num_want(pkg, gen, n):
    gen._chk(pkg.frontend.lib().cvo_fe_set_num_want(gen._h, int(n)), "set_num_want")
    gen.num_want = int(n)


def test_the_cases_this_file_is_about_are_here(golden):
    """Neither the large potentials nor potential 1 nor the threshold 0 may drop out of the GPU's list"""
    runs = [(c, golden["runs"]["%s/%d" % (c.name, b)]) for c in GPU_CASES for b in c.budgets]
    assert any(4 * r["pot_used"] > max(c.w, c.h) for c, r in runs)                 # one wave sweeps the whole image
    assert any(r["pot_used"] == 1 and r["num_have"] > c.w * c.h // 4 for c, r in runs)   # potential 1, busy image
    assert any(r["num_have"] > 255 and r["count"] < 8 for c, r in runs if c.kind == "quads")   # charTH == 0
    assert {1, 2, 3} <= {r["pot_used"] for c, r in runs}
    assert {(c.w, c.h) for c in GPU_CASES} == {(96, 64), (128, 192), (65, 67), (127, 193), (333, 251), (352, 300),
                                                (65, 70), (640, 480), (1280, 720)}
    assert all(c.budgets[0] == 1 and c.budgets[-1] == 10 ** 6 for c in GPU_CASES)
    assert any(c.kind == "quads" for c in GPU_CASES)


@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.name)
def test_selector_equals_the_reference(pkg, case, contexts, golden, pattern):
    F = pkg.frontend
    gen = contexts(case.w, case.h)
    bgr, dep = sc.frame(pkg, case)
    have_ref = fo.ref_selector_lib() is not None
    memo = {}
    for b in case.budgets:
        _set_num_want(pkg, gen, b)
        gen.create_pointcloud(bgr, dep, dataset_seq=1, feature_type=F.FEATURES_RGB)
        planes = [gen.read_stage(s) for s in (F.STAGE_AG0, F.STAGE_AG1, F.STAGE_AG2)]
        ths, mp, info = gen.read_stage(F.STAGE_THS), gen.read_stage(F.STAGE_MAP), gen.info()
        got = {"count": info["num_selected"], "pot_used": info["pot_used"], "reselected": info["reselected"]}
        if have_ref:
            t = fo.ref_make_maps(*planes, b, sc.define_unwritten(case))
        elif sc.runs_in_python(case):
            t = sr.make_maps(*planes, b, pattern, memo=memo)
        else:
            t = None
        where = "%s, num_want %d" % (case.name, b)
        print("%s: selected %d, potential %d, reselected %d, canny %d" % (where, got["count"], got["pot_used"],
                                                                            got["reselected"], info["canny_used"]))
        no_top_up = got["count"] >= b // 3   # (ref src/pcd_generator.cpp:141-144; with a top-up the map holds more)
        assert bool(info["canny_used"]) == (not no_top_up), where
        if t is not None:
            want = {k: int(t[k]) for k in got}
            assert np.array_equal(ths.view(np.uint32), t["ths_smoothed"].view(np.uint32)), where
            assert got == want, where
            if no_top_up:
                assert np.array_equal(mp.view(np.uint32), t["map"].view(np.uint32)), where
            else:   # the top-up only adds pixels (ref src/pcd_generator.cpp:160-170)
                kept = t["map"] != 0
                assert np.array_equal(mp[kept], t["map"][kept]), where
        else:
            rec = golden["runs"]["%s/%d" % (case.name, b)]
            assert sha(*planes) == golden["planes"][case.name], "%s: not the planes the recorded reference ran on" % where
            assert sha(ths) == rec["sha_ths_smoothed"], where
            assert got == {k: rec[k] for k in got}, where
            if no_top_up:
                assert sha(mp) == rec["sha_map"], where
