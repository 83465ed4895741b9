"""No GPU: the input bin of the front end (the binning contract of include/cvo_frontend.h, at cvo_fe_binning).  The
host-only entries -- cvo_fe_check_binning, cvo_fe_bin_camera, cvo_fe_bin_stereo_rig -- against the restatement
tests/fe_binning_ref.py, the working camera's geometry in float64, the constants, and, for every wrong version of
tests/fe_binning_mutants.py, an input of fe_binning_ref.cases() -- what tests/test_gpu_fe_binning.py runs the kernel
on -- that tells it from the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_binning_mutants as M
import fe_binning_ref as B
import fe_rectify_ref as R
import fe_stereo_rig_ref as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def _bits(values):
    return np.array(values, np.float32).view(np.uint32).tolist()


def _models(F):
    """the table's six rows as models of an input image, and a distorting one"""
    rows = [tuple(F.camera(seq).values()) + (ZERO,) for seq in range(6)]
    return rows + [R.FR1, R.SMALL["C"][2]]


def test_the_constants_and_the_symbols(pkg):
    F = pkg.frontend
    header = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for name, value in (("FULL_BGR", 32), ("FULL_RIGHT_BGR", 33), ("FULL_DEPTH", 34)):
        assert re.search(r"CVO_FE_STAGE_%s = %d\b" % (name, value), header), name
        assert getattr(F, "STAGE_" + name) == value
    assert "THE BINNING CONTRACT" in header and C.sizeof(F.Binning) == 12
    for sym in ("check_binning", "set_input_binning", "get_input_binning", "bin_camera", "bin_stereo_rig", "bin_image",
                "bin_depth"):
        assert "cvo_fe_" + sym in F.SYMBOLS and hasattr(F.lib(), "cvo_fe_" + sym)
    assert F.Binning(3, 4).astuple() == (3, 4) and F.Binning(2, 1) == F.Binning(2, 1) != F.Binning(2, 2)


def test_check_binning_against_the_restatement(pkg):
    F = pkg.frontend
    sizes = ((64, 64), (1, 1), (0, 8), (8, 0), (-1, 8), (2048, 2048), (2049, 8), (8, 2049), (2730, 2730), (2731, 8),
             (4096, 4096), (4097, 8), (8, 4097))
    seen = set()
    for f in (-1, 0, 1, 2, 3, 4, 5, 8):
        for dmin in (-1, 0, 1, 2, 4, 5, 8, 9, 10, 15, 16, 17):
            for pad in (0, 1):
                for w, h in sizes:
                    want = B.check((f, dmin, pad), w, h)
                    assert F.check_binning(F.Binning(f, dmin, pad), w, h) == want, (f, dmin, pad, w, h)
                    seen.add(want)
    assert seen == {True, False}
    assert not F.check_binning(None, 64, 64) and not B.check(None, 64, 64)


@pytest.mark.parametrize("f", B.FACTORS)
def test_bin_camera_by_bits(pkg, f):
    F = pkg.frontend
    for model in _models(F):
        got = F.bin_camera(F.CameraModel(*model), f)
        scale, fx, fy, cx, cy, dist = B.bin_camera(model, f)
        assert _bits([got.depth_scale, got.fx, got.fy, got.cx, got.cy] + list(got.dist)) == _bits([scale, fx, fy, cx, cy] + list(dist)), model
        assert got.depth_scale == np.float32(model[0]) and tuple(got.dist) == tuple(np.float32(d) for d in model[5])
        # ... and not cx / f
        wrong = M.camera_cx_over_f(model[1], model[2], model[3], model[4], f)
        assert (got.fx, got.fy) == wrong[:2] and got.cx != wrong[2] and got.cy != wrong[3]


@pytest.mark.parametrize("f", B.FACTORS)
def test_bin_stereo_rig_by_bits(pkg, f):
    F = pkg.frontend
    for name in ("A", "B"):
        w, h, _, calib = RG.CALIBS[name]
        rig = RG.to_struct(F, RG.rectify(calib, w, h, RG.DEPTH_SCALE))
        got = F.bin_stereo_rig(rig, f)
        left, right, rl, rr, fx, fy, cx, cy, baseline, scale = B.bin_stereo_rig(rig.astuple(), f)
        for lens, want in ((got.left, left), (got.right, right)):
            assert _bits([lens.fx, lens.fy, lens.cx, lens.cy] + list(lens.dist)) == _bits(list(want[:4]) + list(want[4]))
        assert _bits(list(got.R_left) + list(got.R_right)) == _bits(list(rl) + list(rr))
        assert _bits([got.fx, got.fy, got.cx, got.cy, got.baseline, got.depth_scale]) == _bits([fx, fy, cx, cy, baseline, scale])
        assert (got.baseline, got.depth_scale) == (rig.baseline, rig.depth_scale) and got.fx != rig.fx


def test_the_helpers_refuse(pkg):
    F = pkg.frontend
    L = F.lib()
    model, out = F.CameraModel(*R.FR1), F.CameraModel()
    for bad in (-1, 0, 1, 5, 8):
        with pytest.raises(pkg.capi.CvoHipError):
            F.bin_camera(model, bad)
        with pytest.raises(pkg.capi.CvoHipError):
            F.bin_stereo_rig(RG.to_struct(F, RG.RIG_I), bad)
    assert L.cvo_fe_bin_camera(None, 2, C.byref(out)) == -1 and L.cvo_fe_bin_camera(C.byref(model), 2, None) == -1
    with pytest.raises(pkg.capi.CvoHipError):
        F.bin_camera(F.CameraModel(5000.0, -1.0, 1.0, 0.0, 0.0), 2)      # what set_camera refuses
    with pytest.raises(pkg.capi.CvoHipError):
        F.bin_stereo_rig(RG.to_struct(F, dict(RG.RIG_I, baseline=-0.2)), 2)   # what check_stereo_rig refuses
    assert L.cvo_fe_bin_camera(C.byref(model), 2, C.byref(model)) == 0   # `out` may be `in`
    assert model == F.bin_camera(F.CameraModel(*R.FR1), 2)


@pytest.mark.parametrize("f", B.FACTORS)
def test_the_geometry_of_the_working_camera(pkg, f):
    """A point projected through the input camera to u and through the binned camera to u' satisfies
    u = f u' + (f - 1) / 2, in float64 on the float32 members.  The formula rounds THREE times per axis: once in
    fx' = fx / f (relative 2^-24 of fx x), and twice in cx' = (cx - c) / f, the subtraction and the division (each
    relative 2^-24 of cx - c; c = 0.5 (f - 1) and the conversions of f are exact).  So
    |u - (f u' + c)| <= (|fx x| + 2 |cx - c|) 2^-24 (1 + 2^-24), x the normalised coordinate behind the lens."""
    F = pkg.frontend
    eps = 2.0 ** -24
    rng = np.random.RandomState(3 + f)
    c = 0.5 * (f - 1)
    for model in _models(F):
        m, b = F.CameraModel(*model), F.bin_camera(F.CameraModel(*model), f)
        pts = rng.uniform(-1.0, 1.0, (200, 3)) * (2.0, 1.5, 1.0) + (0.0, 0.0, 3.0)
        x, y = pts[:, 0] / pts[:, 2], pts[:, 1] / pts[:, 2]
        k1, k2, p1, p2, k3 = (float(d) for d in m.dist)                 # (the same on both sides: dist is unchanged)
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
        yd = y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
        for nd, fin, cin, fout, cout in ((xd, m.fx, m.cx, b.fx, b.cx), (yd, m.fy, m.cy, b.fy, b.cy)):
            u = float(fin) * nd + float(cin)
            ub = float(fout) * nd + float(cout)
            bound = (np.abs(float(fin) * nd) + 2.0 * abs(float(cin) - c)) * eps * (1.0 + eps)
            assert (np.abs(u - (f * ub + c)) <= bound).all(), model
            # the mistake the helper exists for is far outside: cx / f puts the image (f - 1) / 2 input pixels off
            wrong = float(fout) * nd + float(np.float32(cin) / np.float32(f))
            assert (np.abs(u - (f * wrong + c)) > 0.4).all()


def test_the_restatement_on_inputs_known_by_hand():
    flat = np.full((8, 12, 3), 77, np.uint8)
    for f in (2, 4):
        assert (B.bin_colour(flat, f) == 77).all()                       # a flat block comes back exactly
    assert (B.bin_colour(np.full((6, 6, 3), 200, np.uint8), 3) == 200).all()
    half = np.zeros((2, 2, 3), np.uint8)
    half[0, :, 0] = 1                                                    # S = 2 of n = 4: a half, rounded up
    half[0, 0, 1] = 1                                                    # S = 1: below
    assert B.bin_colour(half, 2).tolist() == [[[1, 0, 0]]]
    d = np.array([[0, 9], [65535, 3]], np.uint16)
    assert [int(B.bin_depth(d, 2, k)[0, 0]) for k in (1, 2, 3, 4)] == [9, 9, 9, 0]   # 3 9 65535: the lower median
    d = np.array([[0, 9], [0, 3]], np.uint16)
    assert [int(B.bin_depth(d, 2, k)[0, 0]) for k in (1, 2, 3)] == [3, 3, 0]         # an even count: the lower one
    assert int(B.bin_depth(np.zeros((2, 2), np.uint16), 2, 1)[0, 0]) == 0
    assert int(B.bin_depth(np.full((3, 3), 65535, np.uint16), 3, 9)[0, 0]) == 65535  # 65535 is a depth like any other


def test_the_sizes_and_the_inputs_of_the_gpu_test():
    cases = B.cases()
    for f in B.FACTORS:
        mine = [c for c in cases if c[1] == f]
        assert {(w, h) for _, _, w, h, _, _ in mine} == set(B.sizes(f))
        assert (8192 // f, 1) in B.sizes(f) and B.check((f, 1, 0), 8192 // f, 1) and not B.check((f, 1, 0), 8192 // f + 1, 1)
        assert {k for p, _, _, _, k, _ in mine if p == "colour"} == set(B.COLOUR_KINDS)
        assert {k for p, _, _, _, k, _ in mine if p == "depth"} == set(B.DEPTH_KINDS)
        assert {d for p, _, _, _, _, d in mine if p == "depth"} == {1, f * f // 2, f * f}
        assert len(B.colour_input(f, 13, 7, "phases")) == f * f
        for dmin in B.depth_mins(f):                                     # "edge": exactly depth_min - 1 and depth_min valid
            k = (B.blocks(B.depth_input(f, 13, 7, "edge", dmin), f) != 0).sum(axis=2)
            assert set(np.unique(k)) == {dmin - 1, dmin}
        k = (B.blocks(B.depth_input(f, 13, 7, "one", 1), f) != 0).sum(axis=2)
        assert (k == 1).all()
        ext = B.depth_input(f, 13, 7, "extremes", 1)
        assert set(np.unique(ext)) == {0, 1, 65535}
        assert ((B.blocks(B.depth_input(f, 13, 7, "even", 1), f) != 0).sum(axis=2) % 2 == 0).all()


def _told_apart(mutant, plane):
    """an input of cases() on which the mutant and the restatement differ"""
    for case in B.cases():
        _, f, w, h, kind, dmin = case
        if case[0] != plane or max(w, h) > 200:
            continue
        for src in B.case_inputs(case):
            want = B.bin_colour(src, f) if plane == "colour" else B.bin_depth(src, f, dmin)
            got = mutant(src, f) if plane == "colour" else mutant(src, f, dmin)
            if got.shape != want.shape or not np.array_equal(got, want):
                return case
    return None


@pytest.mark.parametrize("mutant", M.COLOUR, ids=[m.__name__ for m in M.COLOUR])
def test_an_input_of_the_gpu_test_tells_the_colour_mutant_from_the_restatement(mutant):
    assert _told_apart(mutant, "colour") is not None
    for f in B.FACTORS:                                                  # ... at every factor where the mistake exists
        if mutant is M.colour_half_to_even and f == 3:
            src = B.colour_input(3, 13, 7, "random")                    # (f = 3: a half cannot occur)
            assert np.array_equal(mutant(src, 3), B.bin_colour(src, 3))
            continue
        found = any(not np.array_equal(mutant(src, f), B.bin_colour(src, f))
                    for case in B.cases() if case[0] == "colour" and case[1] == f and max(case[2], case[3]) <= 200
                    for src in B.case_inputs(case))
        assert found, f


@pytest.mark.parametrize("mutant", M.DEPTH, ids=[m.__name__ for m in M.DEPTH])
def test_an_input_of_the_gpu_test_tells_the_depth_mutant_from_the_restatement(mutant):
    assert _told_apart(mutant, "depth") is not None
    for f in B.FACTORS:
        found = any(not np.array_equal(mutant(src, f, case[5]), B.bin_depth(src, f, case[5]))
                    for case in B.cases() if case[0] == "depth" and case[1] == f and max(case[2], case[3]) <= 200
                    for src in B.case_inputs(case))
        assert found, f


def test_the_pair_of_the_gpu_test_tells_the_right_image_binned_from_the_left():
    import fe_stereo_ref as S
    for f in B.FACTORS:
        left, right, _ = S.pair(64 * f, 64 * f, 82)
        got = M.pair_right_from_left(left, right, f)
        assert np.array_equal(got[0], B.bin_colour(left, f)) and not np.array_equal(got[1], B.bin_colour(right, f))
