"""CPU: step 4 of the stereo contract under a path mask (include/cvo_frontend.h, cvo_fe_set_stereo_paths).  The numpy
restatement (tests/fe_stereo_paths_ref.py) in its two forms, against the four-path restatement it extends
(tests/fe_stereo_ref.py), against itself turned by 180 degrees, and against mutants of the diagonal scan
(tests/fe_stereo_paths_mutants.py) that the cases must tell from it, so that the GPU tests cannot pass on nothing; the
bounds the contract states; the library's host-only cvo_fe_check_stereo_paths and the enum against the binding.  No
accuracy is claimed or tested: what the diagonals are worth on real pairs is unmeasured."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_stereo_paths_mutants as M
import fe_stereo_paths_ref as P
import fe_stereo_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_bit(name):
    """the eight L_r of a case, int64"""
    _, Cv, st = P.case_volume(name)
    return [P.direction(Cv, st["p1"], st["p2"], *P.DIRS[b]) for b in range(8)]


# ---- the restatement checks itself -----------------------------------------------------------------

@pytest.mark.parametrize("h,w,D", [(7, 9, 8), (9, 7, 8), (1, 12, 8), (12, 1, 8)])
def test_the_two_forms_agree(h, w, D):
    """row by row with the previous row shifted, and pixel by pixel with p - r looked up: every one-bit mask, on random
    volumes wider than high, higher than wide, of one row and of one column"""
    rng = np.random.Generator(np.random.PCG64(5000 + 16 * h + w))
    for p1, p2 in ((8, 32), (1, 1), (255, 255)):
        Cv = rng.integers(0, 65, (h, w, D)).astype(np.int64)
        for b in range(8):
            a, l = P.path_sums(Cv, p1, p2, 1 << b), P.path_sums_loops(Cv, p1, p2, 1 << b)
            assert a.dtype == np.uint16 and np.array_equal(a, l), (b, p1, p2)
        assert np.array_equal(P.path_sums(Cv, p1, p2, 0x35), P.path_sums_loops(Cv, p1, p2, 0x35))
    # the first pixel of a path: one row has no p - r for any direction with ry != 0, one column none with rx != 0
    if h == 1 or w == 1:
        for b in range(8):
            rx, ry = P.DIRS[b]
            if (h == 1 and ry != 0) or (w == 1 and rx != 0):
                assert np.array_equal(P.direction(Cv, p1, p2, rx, ry), Cv)


@pytest.mark.parametrize("name", list(S.CASES))
def test_mask_0f_is_the_four_path_restatement(name):
    pre, Cv, st = P.case_volume(name)
    assert np.array_equal(P.path_sums(Cv, st["p1"], st["p2"], P.PATHS_4), S.case_planes(name)["sum"])
    assert np.array_equal(P.case_planes(name, P.PATHS_4)["depth"], S.case_planes(name)["depth"])


def test_a_direction_is_its_opposite_on_the_volume_turned_round():
    """bit 4 on C = bit 5 on C turned by 180 degrees, turned back; likewise 6 and 7, and (the existing forms) 0 and 1, 2
    and 3"""
    _, Cv, st = P.case_volume("default-127x193-83")
    turned = np.ascontiguousarray(Cv[::-1, ::-1])
    for a, b in ((4, 5), (6, 7), (0, 1), (2, 3)):
        La = P.direction(Cv, st["p1"], st["p2"], *P.DIRS[a])
        Lb = P.direction(turned, st["p1"], st["p2"], *P.DIRS[b])[::-1, ::-1]
        assert np.array_equal(La, Lb), (a, b)
    # ... and mirrored left to right bit 4 is bit 6, bit 5 is bit 7
    mirrored = np.ascontiguousarray(Cv[:, ::-1])
    for a, b in ((4, 6), (5, 7)):
        La = P.direction(Cv, st["p1"], st["p2"], *P.DIRS[a])
        assert np.array_equal(La, P.direction(mirrored, st["p1"], st["p2"], *P.DIRS[b])[:, ::-1]), (a, b)


def test_the_eight_directions_tell_apart():
    """on default-96x64-82 the eight one-bit sums are pairwise different (and so are the planes behind them for the
    diagonals): a kernel that runs the wrong direction cannot pass"""
    L = _one_bit("default-96x64-82")
    for a in range(8):
        for b in range(a + 1, 8):
            assert np.count_nonzero(L[a] != L[b]) > 1000, (a, b)
    assert sorted(P.DIRS) == sorted((rx, ry) for rx in (-1, 0, 1) for ry in (-1, 0, 1) if (rx, ry) != (0, 0))
    assert P.DIRS[:4] == ((1, 0), (-1, 0), (0, 1), (0, -1))          # bits 0 to 3: the four launches of before, in order
    flags = [P.case_planes("default-96x64-82", 1 << b)["disparity"] for b in range(4, 8)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(flags[a], flags[b])
    for name in ("default-96x64-82", "default-127x193-83"):
        assert not np.array_equal(P.case_planes(name, P.PATHS_8)["disparity"], P.case_planes(name, P.PATHS_4)["disparity"])


# ---- the bounds of the contract -------------------------------------------------------------------

@pytest.mark.parametrize("name,top", [("p255", 2552), ("p255-noise", 2552), ("noise", 768), ("saturated", 768), ("narrow", 768)])
def test_the_sums_reach_their_bound(name, top):
    """S under 0xFF reaches 8 * (64 + p2) exactly, and a one-bit sum 64 + p2; `off` stays in [-8, 8]"""
    _, Cv, st = P.case_volume(name)
    assert top == 8 * (64 + st["p2"])
    Sv = P.path_sums(Cv, st["p1"], st["p2"], P.PATHS_8)
    assert int(Sv.max()) == top < 1 << 12
    for b in (4, 7):
        assert int(P.direction(Cv, st["p1"], st["p2"], *P.DIRS[b]).max()) == 64 + st["p2"]
    ds, S1 = S.winners(Sv)
    off = S.subpixel(Sv, ds, S1) - 16 * ds
    assert off.min() >= -8 and off.max() <= 8
    # the key and the uniqueness test of the winner kernel keep their room
    assert (int(Sv.max()) << 8 | 127) < 1 << 20 and int(Sv.max()) * 100 < 1 << 19


# ---- the mutants ----------------------------------------------------------------------------------

def test_the_mutants_form_without_an_error_is_the_restatement():
    for name in ("tall", "default-96x64-82"):
        _, Cv, st = P.case_volume(name)
        for b in range(4, 8):
            assert np.array_equal(M.restated(Cv, st["p1"], st["p2"], *P.DIRS[b]), P.direction(Cv, st["p1"], st["p2"], *P.DIRS[b]))


@pytest.mark.parametrize("mutant,names", [("no-restart", ("tall", "wide", "default-96x64-82", "default-127x193-83")),
                                          ("ry-negated", ("tall", "default-96x64-82", "default-127x193-83")),
                                          ("wrong-border", ("tall", "wide", "default-96x64-82", "default-127x193-83")),
                                          ("next-cost", ("tall", "wide", "default-96x64-82", "default-127x193-83"))])
def test_the_cases_tell_every_mutant_of_the_diagonal_scan(mutant, names):
    """for every diagonal bit alone -- the sums, and a plane behind them -- and under a mask of several.  `tall` is where
    a wrapped line wraps five times, `wide` where a true diagonal is cut short by the other border.  (Negating ry turns
    bit 4 into bit 7 and bit 5 into bit 6: under 0xFF that mutant is no error, and 0x35 takes its place.)"""
    for name in names:
        _, Cv, st = P.case_volume(name)
        for mask in (0x10, 0x20, 0x40, 0x80, 0x35 if mutant == "ry-negated" else P.PATHS_8):
            got = M.sums(Cv, st, mask, mutant)
            if name == "wide":                              # (the sums suffice there: the planes behind take the longest)
                assert np.count_nonzero(got != P.path_sums(Cv, st["p1"], st["p2"], mask)) >= 16, (name, mask)
                continue
            want = P.case_planes(name, mask)
            assert np.count_nonzero(got != want["sum"]) >= 16, (name, mask)
            assert not np.array_equal(S.decide(got, st, S.FX, S.SCALE)["disparity"], want["disparity"]), (name, mask)
        # rows and columns are none of a diagonal mutant's business
        if name != "wide":
            assert np.array_equal(M.sums(Cv, st, P.PATHS_4, mutant), P.case_planes(name, P.PATHS_4)["sum"])


def test_tall_is_what_it_is_for():
    w, h, st, left, right = P.inputs("tall")
    assert (w, h, st["max_disp"]) == (64, 321, 32) and h // w == 5 and h % 8 == 1 and left.shape == (h, w, 3)
    Pl = P.case_planes("tall", P.PATHS_8)
    assert np.count_nonzero(Pl["depth"]) > 3000


# ---- the library's host side ----------------------------------------------------------------------

def test_check_set_and_get_on_the_host(pkg):
    F = pkg.frontend
    for good in (1, 0x0F, 0x10, 0x35, 0xFF):
        assert F.check_stereo_paths(good)
    for bad in (0, 0x100, 0xFFFFFFFF, -1, 1 << 32):
        assert not F.check_stereo_paths(bad)
    L = F.lib()
    assert L.cvo_fe_check_stereo_paths(0xFFFFFFFF) != 0 and L.cvo_fe_check_stereo_paths(0) != 0
    out = C.c_uint32(7)
    assert L.cvo_fe_set_stereo_paths(None, 0xFF) != 0 and L.cvo_fe_get_stereo_paths(None, C.byref(out)) != 0
    assert out.value == 7
    assert (F.PATHS_4, F.PATHS_8) == (P.PATHS_4, P.PATHS_8) == (0x0F, 0xFF)
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    assert re.search(r"enum \{ CVO_FE_PATHS_4 = 0x0F, CVO_FE_PATHS_8 = 0xFF \};", text)
    for name in ("cvo_fe_check_stereo_paths", "cvo_fe_set_stereo_paths", "cvo_fe_get_stereo_paths"):
        assert name in F.SYMBOLS
    # cvo_fe_stereo itself is what it was
    assert C.sizeof(F.Stereo) == 32 and "paths" not in [n for n, _ in F.Stereo._fields_]
