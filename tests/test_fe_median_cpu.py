"""No GPU: the restatement of the median contract (tests/fe_median_ref.py) against itself -- the vectorised form against
the per-pixel loop on every small plane made on purpose -- what the planes are for (each mutant of
tests/fe_median_mutants.py is told from the restatement by a plane and settings named here), that no case of
tests/test_gpu_fe_median.py is empty, and cvo_fe_check_depth_median with the other host-only refusals of the library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import fe_median_mutants as M
import fe_median_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and tuple(got[2:]) == tuple(want[2:])


# ---- 1. two statements of the contract ---------------------------------------------------------------

SMALL = [n for n in K.MADE_NAMES if K.plane(n).size <= 40 * 33]


@pytest.mark.parametrize("name", SMALL)
def test_the_vectorised_form_equals_the_loop(name):
    A = K.plane(name)
    for m in K.SETTINGS:
        got = K.made(name, m)
        assert got[1].dtype == np.uint16 and got[2].dtype == np.uint8 and got[1].shape == got[2].shape == A.shape
        assert _same(got[1:], K.median_loop(A, m)), (name, m)


def test_a_window_by_hand():
    """3 x 3 around a hole: four values, the lower median is the second; 65535 is a depth; a corner has four pixels"""
    A = np.array([[10, 0, 65535], [0, 0, 30], [20, 0, 0]], np.uint16)
    B, flags, changed, filled = K.median(A, (1, 4))
    assert B[1, 1] == 20 and flags[1, 1] == K.FILLED                  # {10, 20, 30, 65535}: v_1
    assert B[0, 2] == 30 and flags[0, 2] == K.CHANGED                 # {30, 65535}: v_0
    assert B[0, 0] == 10 and flags[0, 0] == 0 and B[2, 2] == 0        # {10} itself; {30}: one value, fewer than four
    assert K.median(A, (1, 0))[0][1, 1] == 0 and K.median(A, (1, 5))[0][1, 1] == 0
    assert (changed, filled) == (int(np.count_nonzero(flags == 1)), int(np.count_nonzero(flags == 2)))


def test_the_made_planes_are_what_they_are_made_for():
    assert [K.plane("noise-holes-%dx%d" % s).shape for s in K.DEGENERATE] == [(1, 1), (9, 1), (1, 9), (2, 2), (5, 3)]
    for name in ("noise-holes", "noise-full", "noise-sparse"):
        assert K.plane(name).shape == (35, 67)
    holes = {n: float(np.mean(K.plane(n) == 0)) for n in ("noise-holes", "noise-full", "noise-sparse", "ties")}
    assert 0.35 < holes["noise-holes"] < 0.45 and holes["noise-full"] == 0 and 0.8 < holes["noise-sparse"] < 0.9
    assert 0.25 < holes["ties"] < 0.35 and set(np.unique(K.plane("ties"))) == {0, 100, 101, 102}
    assert set(np.unique(K.plane("extremes"))) == {0, 1, 65534, 65535} and K.plane("extremes").shape == (33, 40)
    assert K.plane("noise-full").max() > 65000 and K.plane("noise-full").min() >= 1
    assert K.plane("ramp").shape == (17, 33) and K.plane("ramp").all()
    assert np.count_nonzero(K.plane("single")) == 1 and not K.plane("empty").any()
    s = K.plane("surface")
    assert s.shape == (70, 130) and 0.03 < np.mean(s == 0) < 0.07
    # every tile shape of the mutants, the kernel's among them, has a seam in both directions inside the noise planes
    for tw, th in M.TILES:
        assert tw < 67 and th < 35
    assert K.TILE in M.TILES
    for w, h in ((8192, 3), (3, 8192)):
        A = K.long_plane(w, h)
        for m in K.LONG_SETTINGS:      # (three rows: a 5 x 5 window holds fifteen pixels at the most)
            assert A.shape == (h, w) and K.median(A, m)[2] >= 20 and K.median(A, m)[3] >= 20


# ---- 2. the mutants ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant, name, m", [
    (M.upper_median, "ties", (1, 0)),                # an even number of values, the two middle ones apart
    (M.upper_median, "noise-holes", (2, 13)),
    (M.zeros_counted, "noise-sparse", (1, 0)),       # most of a window is holes: the middle of the padded lot is 0
    (M.zeros_counted, "single", (1, 1)),             # one value and eight zeros beside it
    (M.replicated_border, "ramp", (1, 0)),           # the border column counted twice moves the middle
    (M.replicated_border, "noise-full", (2, 0)),
    (M.in_place, "noise-full", (1, 0)),              # every window holds results of the rows above
    (M.in_place, "single", (1, 1)),                  # a filled pixel fills the next: the one value spreads over the plane
    (M.max_is_none, "extremes", (1, 0)),             # the only plane that holds 65535
    (M.max_is_none, "extremes", (2, 13)),
    (M.fill_strict, "single", (1, 1)),               # n == fill_min == 1 at the eight pixels around the one value
    (M.fill_strict, "noise-holes", (1, 5)),
    (M.fill_strict, "noise-holes", (2, 13)),
    (M.fill_strict, "surface", (2, 24)),             # pinholes whose other twenty-four pixels all have a depth
    (M.fill_strict, "surface", (1, 8)),
    (M.fixed_middle, "noise-holes", (1, 0)),         # n < 9 almost everywhere
    (M.fixed_middle, "single", (1, 0)),              # n == 1: the middle of the padded sort is "none"
    (M.fixed_middle, "noise-full", (2, 0)),          # n < 25 only at the border: the partial windows there
    (M.short_window, "noise-full", (1, 0)),
    (M.short_window, "ramp", (2, 0)),
    (M.short_window, "single", (1, 1)),              # the pixels to the left of the value see it no more
])
def test_a_plane_tells_the_mutant(mutant, name, m):
    A, B, flags, changed, filled = K.made(name, m)
    assert not _same(mutant(A, m), (B, flags, changed, filled))


@pytest.mark.parametrize("tile", M.TILES, ids=["%dx%d" % t for t in M.TILES])
def test_the_noise_tells_a_lost_halo(tile):
    """tiles of 32 x 8, 64 x 4, 16 x 16 and the kernel's 64 x 16: 67 x 35 has a seam of each inside, both ways, and
    both radii reach across it"""
    for name, m in (("noise-full", (1, 0)), ("noise-holes", (2, 0)), ("noise-holes", (1, 5)), ("noise-sparse", (2, 13))):
        A, B, flags, changed, filled = K.made(name, m)
        got = M.tile_cut(A, m, *tile)
        assert not _same(got, (B, flags, changed, filled))
        # ... and it is the seams that tell: away from them the mutant is the restatement
        ys, xs = np.nonzero(got[0] != B)
        r = m[0]
        near_x = (xs % tile[0] < r) | (xs % tile[0] >= tile[0] - r)
        near_y = (ys % tile[1] < r) | (ys % tile[1] >= tile[1] - r)
        assert len(ys) > 0 and (near_x | near_y).all()


def test_only_the_extremes_show_65535_taken_for_none():
    for name in K.MADE_NAMES:
        told = [m for m in K.SETTINGS if not _same(M.max_is_none(K.plane(name), m), K.made(name, m)[1:])]
        assert told == (K.SETTINGS if name == "extremes" else []), name


def test_every_mutant_is_told_at_every_radius():
    """beside the named cases above: each mutant differs from the restatement somewhere at radius 1 and at radius 2"""
    mutants = M.PLAIN + [lambda A, m, t=t: M.tile_cut(A, m, *t) for t in M.TILES]
    for mutant in mutants:
        for radius in (1, 2):
            assert any(not _same(mutant(K.plane(name), m), K.made(name, m)[1:])
                       for name in ("noise-holes", "extremes", "surface") for m in K.SETTINGS if m[0] == radius and m[1] > 0)


# ---- 3. no GPU case is empty -------------------------------------------------------------------------

def test_the_made_cases_change_and_fill():
    """every made plane that can has two CHANGED pixels at every setting and, at some setting that fills, two FILLED
    ones (a plane without holes has nothing to fill, and 2 x 2 cannot have two of each: fe_median_ref.py at the seeds)"""
    for name in K.MADE_NAMES:
        if name in K.NOTHING_TO_SHOW:
            continue
        counts = {m: K.made(name, m)[3:] for m in K.SETTINGS}
        assert all(c[0] >= 2 for c in counts.values()), (name, counts)
        most = max(c[1] for m, c in counts.items() if m[1] >= 1)
        assert most >= (0 if name in K.WITHOUT_HOLES else 1 if name in K.ONE_HOLE else 2), (name, counts)
        assert all(c[1] == 0 for m, c in counts.items() if m[1] == 0)
    assert K.made("noise-full", (1, 1))[4] == 0 and not (K.plane("noise-full") == 0).any()
    assert K.made("single", (1, 1))[3:] == (0, 8) and K.made("single", (2, 1))[3:] == (0, 24)
    assert all(K.made("empty", m)[3:] == (0, 0) for m in K.SETTINGS)
    # the plane the filter is for: most of the salt goes, most of the pinholes are filled, and the surface stays smooth
    A, B, flags, changed, filled = K.made("surface", (1, 5))
    assert filled > 0.9 * np.count_nonzero(A == 0) and changed > 0.04 * A.size
    clean = K.surface(130, 70, 6, pinholes=0.0, salt=0.0).astype(np.int64)
    assert np.mean(np.abs(B.astype(np.int64) - clean)[B != 0] > 200) < 0.01 < np.mean(np.abs(A.astype(np.int64) - clean)[A != 0] > 200)


def test_the_settings_differ_on_the_frames_plane():
    """the settings alternating on one context in tests/test_gpu_fe_median.py: a stale graph of another would show"""
    A = K.surface(160, 120, 31)
    outs = [K.median(A, m) for m in K.FRAME_SETTINGS]
    for i in range(len(outs)):
        assert outs[i][2] >= 20 and (K.FRAME_SETTINGS[i][1] == 0 or outs[i][3] >= 20)
        for j in range(i):
            assert outs[i][0].tobytes() != outs[j][0].tobytes()


# ---- 4. what is accepted, and the layers above -------------------------------------------------------

def _in_range(s):
    radius, fill_min, pad = s
    return radius in (1, 2) and 0 <= fill_min <= (2 * radius + 1) ** 2 - 1 and pad == 0


def test_the_struct_and_the_constants(pkg):
    F = pkg.frontend
    assert C.sizeof(F.DepthMedian) == 12 and bytes(F.DepthMedian(2, 13)) == np.array([2, 13, 0], np.int32).tobytes()
    assert bytes(F.DepthMedian()) == np.array([1, 0, 0], np.int32).tobytes()
    assert bytes(F.DepthMedian(1, 5, 7)) == np.array([1, 5, 7], np.int32).tobytes()
    assert F.DepthMedian(2, 13) == F.DepthMedian(radius=2, fill_min=13) != F.DepthMedian(2, 12)
    assert repr(F.DepthMedian(2, 13)) == "DepthMedian(radius=2, fill_min=13)"
    assert (F.STAGE_UNFILTERED_DEPTH, F.STAGE_MEDIAN, F.MEDIAN_CHANGED, F.MEDIAN_FILLED) == (24, 25, K.CHANGED, K.FILLED) == (24, 25, 1, 2)
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    for pattern in (r"CVO_FE_STAGE_UNFILTERED_DEPTH = 24\b", r"CVO_FE_STAGE_MEDIAN = 25\b", r"CVO_FE_MEDIAN_CHANGED = 1\b",
                    r"CVO_FE_MEDIAN_FILLED = 2\b", r"THE MEDIAN CONTRACT"):
        assert re.search(pattern, text), pattern
    for name in ("cvo_fe_check_depth_median", "cvo_fe_set_depth_median", "cvo_fe_get_depth_median", "cvo_fe_median_plane"):
        assert name in F.SYMBOLS
    hip = open(os.path.join(ROOT, "include", "cvo_hip.h")).read()
    assert "median" not in hip


def test_check_depth_median(pkg):
    """host only, through the library: the one statement of what is accepted"""
    F = pkg.frontend
    assert all(_in_range(s) for s in K.good_medians()) and not any(_in_range(s) for s in K.bad_medians())
    for s in K.good_medians() + [m + (0,) for m in K.SETTINGS]:
        assert F.check_depth_median(F.DepthMedian(*s)), s
    for s in K.bad_medians():
        assert not F.check_depth_median(F.DepthMedian(*s)), s
    assert not F.check_depth_median(None)
    L = F.lib()
    out, isset = F.DepthMedian(2, 3), C.c_int(7)
    assert L.cvo_fe_set_depth_median(None, C.byref(out)) != 0
    assert L.cvo_fe_get_depth_median(None, C.byref(out), C.byref(isset)) != 0 and (out.radius, out.fill_min, isset.value) == (2, 3, 7)
    # host-only refusals of the context-free entry: they come before any device is touched
    plane, changed, filled = np.ones((4, 4), np.uint16), C.c_int(-5), C.c_int(-6)
    u16p = C.POINTER(C.c_uint16)
    good = F.DepthMedian(1, 0)
    for w, h, stride, m in ((0, 4, 8, good), (4, 0, 8, good), (8193, 4, 16386, good), (4, 8193, 8, good), (4, 4, 7, good),
                            (4, 4, 8, F.DepthMedian(3, 0)), (4, 4, 8, F.DepthMedian(1, 9)), (4, 4, 8, F.DepthMedian(1, 0, 1))):
        assert L.cvo_fe_median_plane(0, plane.ctypes.data_as(u16p), stride, w, h, C.byref(m), None, C.byref(changed),
                                     C.byref(filled)) != 0
    assert L.cvo_fe_median_plane(0, plane.ctypes.data_as(u16p), 8, 4, 4, None, None, C.byref(changed), C.byref(filled)) != 0
    assert L.cvo_fe_median_plane(0, None, 8, 4, 4, C.byref(good), None, C.byref(changed), C.byref(filled)) != 0
    assert L.cvo_fe_median_plane(0, plane.ctypes.data_as(u16p), 8, 4, 4, C.byref(good), None, None, C.byref(filled)) != 0
    assert L.cvo_fe_median_plane(0, plane.ctypes.data_as(u16p), 8, 4, 4, C.byref(good), None, C.byref(changed), None) != 0
    assert (changed.value, filled.value) == (-5, -6) and plane.all()


def test_the_drivers_have_the_parameter(pkg):
    F = pkg.frontend
    for fn in (F.run_frames, F.run_directory, F.run_stereo_directory):
        p = inspect.signature(fn).parameters
        assert "depth_median" in p and p["depth_median"].default is None, fn.__name__
    assert callable(F.PcdGenerator.set_depth_median) and callable(F.PcdGenerator.depth_median)
    assert callable(F.median_plane) and callable(F.check_depth_median)
    hpp = open(os.path.join(ROOT, "include", "cvo.hpp")).read()
    assert "void set_depth_median(const cvo_fe_depth_median &" in hpp and "void clear_depth_median();" in hpp
