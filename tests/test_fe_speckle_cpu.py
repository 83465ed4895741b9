"""No GPU: the restatement of the speckle contract (tests/fe_speckle_ref.py) against itself -- the union-find against the
flood fill on every plane made on purpose and on disparity planes of the stereo cases -- what the planes are for (each
mutant of tests/fe_speckle_mutants.py is told from the restatement by a plane named here), that no case of
tests/test_gpu_fe_speckle.py is empty, and cvo_fe_check_speckle with the other host-only refusals of the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_speckle_mutants as M
import fe_speckle_ref as K
import fe_stereo_paths_ref as P
import fe_stereo_rig_ref as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


# ---- 1. two statements of the components -------------------------------------------------------------

@pytest.mark.parametrize("name", K.MADE_NAMES)
def test_union_find_equals_flood_fill_on_the_made_planes(name):
    q, sp, out, sizes, removed = K.made(name)
    assert sizes.dtype == np.uint32 and sizes.shape == q.shape
    assert np.array_equal(K.flood(q, sp[1]), sizes)
    assert removed == np.count_nonzero(q) - np.count_nonzero(out) and np.array_equal(out != 0, (q != 0) & (sizes > sp[0]))


@pytest.mark.parametrize("name", ["default-127x193-83", "d128", "noise"])
def test_union_find_equals_flood_fill_on_disparity_planes(name):
    q = P.case_planes(name, 0x0F)["disparity"]
    for max_diff in (16, 0):
        assert np.array_equal(K.flood(q, max_diff), K.components(q, max_diff))


def test_the_made_planes_are_what_they_are_made_for():
    for w, h in K.SHAPES:
        q, n = K.serpentine(w, h)
        assert K.census_of_sizes(K.components(q, 0)) == [n] == [np.count_nonzero(q)]      # the closed form
        assert (K.made("serpentine-%dx%d-all" % (w, h))[4], K.made("serpentine-%dx%d-none" % (w, h))[4]) == (n, 0)
        q, sp, out, sizes, removed = K.made("blobs-%dx%d" % (w, h))
        have = set(K.census_of_sizes(sizes))
        assert sp[0] in have and sp[0] + 1 in have and removed > 0 and out.any()
    assert K.census_of_sizes(K.made("ramp-one")[3]) == [127 * 193]
    assert K.census_of_sizes(K.made("ramp-columns")[3]) == [193] * 127
    assert (K.made("ramp-one")[4], K.made("ramp-columns")[4], K.made("ramp-columns-kept")[4]) == (0, 127 * 193, 0)
    assert set(K.census_of_sizes(K.made("checker")[3])) == {1}
    assert K.census_of_sizes(K.made("extremes-joined")[3]) == [32] and K.census_of_sizes(K.made("extremes-apart")[3]) == [16, 16]
    assert K.census_of_sizes(K.made("equal")[3]) == [33667] and (K.made("equal")[4], K.made("equal-all")[4]) == (0, 33667)
    assert [K.made(n)[0].shape for n in ("1x1", "1x300", "300x1")] == [(1, 1), (300, 1), (1, 300)]
    assert not K.made("zero")[3].any() and K.made("zero")[4] == 0


# ---- 2. the mutants ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant, name", [
    (M.eight_connected, "checker"),                  # one pixel each; with diagonals one component
    (M.eight_connected, "barred-checker"),
    (M.size_strict, "serpentine-64x64-all"),         # max_size is the component's size exactly
    (M.size_strict, "blobs-127x193"),                # components of max_size and of max_size + 1 pixels
    (M.diff_strict, "ramp-one"),                     # every step is max_diff exactly
    (M.against_first_pixel, "ramp-one"),             # a chain of small steps, its ends 378 apart
    (M.uint16_wrap, "extremes-apart"),               # 1 - 65535 in uint16 is 2
])
def test_a_plane_tells_the_mutant(mutant, name):
    q, sp, out, sizes, removed = K.made(name)
    assert not _same(mutant(q, sp), (out, sizes, removed))


@pytest.mark.parametrize("period, vertical", M.SEAMS)
def test_the_serpentine_tells_a_lost_seam(period, vertical):
    """borders 16, 32 and 64 pixels apart, between columns and between rows: 127 x 193 has each of them inside"""
    for name in ("serpentine-127x193-none", "serpentine-1241x64-all") if vertical or period < 64 else ("serpentine-127x193-none",):
        q, sp, out, sizes, removed = K.made(name)
        assert not _same(M.seam_cut(q, sp, period, vertical), (out, sizes, removed))
    q, sp, out, sizes, removed = K.made("equal")
    assert not _same(M.seam_cut(q, sp, period, vertical), (out, sizes, removed))


# ---- 3. no GPU case is empty -------------------------------------------------------------------------

def _changes_and_keeps(f, before):
    gone = (f["flags"] & K.SPECKLE) != 0
    assert np.array_equal(gone, (before != 0) & (f["disparity"] == 0))
    return int(np.count_nonzero(gone)), int(np.count_nonzero(f["disparity"]))


def test_the_made_cases_change_and_keep():
    for name in K.MADE_NAMES:
        q, sp, out, sizes, removed = K.made(name)
        if name.startswith(K.ALL_OR_NOTHING):
            assert removed in (0, np.count_nonzero(q)), name
        else:
            assert 0 < removed < np.count_nonzero(q), name


def test_the_stereo_cases_change_and_keep():
    """the numbers of the issue: `noise` at (12, 16) removes and keeps, `d128` at (8, 16) removes 25 pixels and keeps
    the component of 10; `flat` has no valid pixel and `wide` is one component (all-or-nothing by what they are)"""
    got = {}
    for name, sp in K.STEREO_CASES.items():
        f = K.case_frame(name, sp)
        got[name] = _changes_and_keeps(f, P.case_planes(name, 0x0F)["disparity"]) + (K.census_of_sizes(f["sizes"]),)
    assert got["noise"][0] > 0 and got["noise"][1] > 0 and len(got["noise"][2]) == 605 and got["noise"][2][0] == 37
    assert got["d128"][0] == 25 and got["d128"][2][:4] == [7771, 10, 4, 3] and len(got["d128"][2]) == 17
    assert 10 in K.case_frame("d128", K.STEREO_CASES["d128"])["sizes"][K.case_frame("d128", K.STEREO_CASES["d128"])["disparity"] != 0]
    assert got["default-127x193-83"][0] > 0 and got["default-127x193-83"][2][:4] == [17882, 3516, 4, 1]
    assert got["flat"] == (0, 0, []) and got["wide"][0] == 0 and len(got["wide"][2]) == 1


def test_the_alternating_settings_differ_on_their_images():
    """K.ALTERNATING on K.ALTERNATING_IMAGES: every frame under a filter loses a pixel; the two settings differ on `noise`
    (a stale graph of the other setting would show), where (100, 32) takes every pixel -- the one frame of the sequence
    that keeps none -- and every other frame keeps some"""
    a, b = K.ALTERNATING_IMAGES
    assert P.inputs(a)[:3] == P.inputs(b)[:3]
    for name in (a, b):
        before = P.case_planes(name, 0x0F)["disparity"]
        for sp in (s for s in K.ALTERNATING if s is not None):
            gone, kept = _changes_and_keeps(K.case_frame(name, sp), before)
            assert gone > 0 and (kept > 0) == ((name, sp) != ("noise", (100, 32)))
    assert not np.array_equal(K.case_frame("noise", (12, 16))["disparity"], K.case_frame("noise", (100, 32))["disparity"])


def test_outside_changes_the_components_under_rig_b():
    """the components are those of the plane AFTER OUTSIDE: some pixel beside a pixel that only OUTSIDE took has
    another SIZE than the plane before OUTSIDE gives it"""
    w, h, st, rig, raw_l, raw_r, Q = RG.case("B")
    f = K.frame(Q, K.RIG_SPECKLE)
    assert _changes_and_keeps(f, Q["disparity"])[0] > 0 and f["disparity"].any()
    before = np.where(Q["flags_before"] == 0, Q["q"], 0).astype(np.uint16)
    only_outside = (before != 0) & (Q["disparity"] == 0)
    beside = np.zeros_like(only_outside)
    beside[:, 1:] |= only_outside[:, :-1]
    beside[:, :-1] |= only_outside[:, 1:]
    beside[1:, :] |= only_outside[:-1, :]
    beside[:-1, :] |= only_outside[1:, :]
    beside &= Q["disparity"] != 0
    assert only_outside.any() and (K.components(before, K.RIG_SPECKLE[1])[beside] != f["sizes"][beside]).any()


def test_the_gate_and_the_eight_path_cases_change_and_keep():
    for name, sp, mask in (K.GATE_CASE, K.PATHS8_CASE):
        gone, kept = _changes_and_keeps(K.case_frame(name, sp, mask), P.case_planes(name, mask)["disparity"])
        assert gone > 0 and kept > 0
    name, sp, mask = K.PATHS8_CASE
    assert not np.array_equal(K.case_frame(name, sp, mask)["sizes"], K.case_frame(name, sp, 0x0F)["sizes"])


# ---- 4. what is accepted -----------------------------------------------------------------------------

def _in_range(sp):
    return 1 <= sp[0] <= K.MAX_SIZE and 0 <= sp[1] <= K.MAX_DIFF


def test_check_speckle(pkg):
    """host only: the one statement of what is accepted, the struct's layout, the enum values and the binding"""
    F = pkg.frontend
    assert all(_in_range(sp) for sp in K.good_speckles()) and not any(_in_range(sp) for sp in K.bad_speckles())
    assert K.good_speckles() == [(1, 0), (2 ** 26, 65535)]
    assert {(0, 16), (-1, 16), (2 ** 26 + 1, 16), (12, -1), (12, 65536)} <= set(K.bad_speckles())
    assert C.sizeof(F.Speckle) == 8 and bytes(F.Speckle(5, 7)) == np.array([5, 7], np.int32).tobytes()
    for sp in K.good_speckles():
        assert F.check_speckle(K.to_struct(F, sp)), sp
    for sp in K.bad_speckles():
        assert not F.check_speckle(K.to_struct(F, sp)), sp
    assert not F.check_speckle(None)
    L = F.lib()
    out, isset = F.Speckle(3, 4), C.c_int(7)
    assert L.cvo_fe_set_stereo_speckle(None, C.byref(out)) != 0
    assert L.cvo_fe_get_stereo_speckle(None, C.byref(out), C.byref(isset)) != 0 and (out.max_size, isset.value) == (3, 7)
    assert (F.STEREO_SPECKLE, F.STAGE_SPECKLE_SIZE) == (K.SPECKLE, 23) == (32, 23)
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    assert re.search(r"CVO_FE_STEREO_SPECKLE = 32\b", text) and re.search(r"CVO_FE_STAGE_SPECKLE_SIZE = 23\b", text)
    for name in ("cvo_fe_check_speckle", "cvo_fe_set_stereo_speckle", "cvo_fe_get_stereo_speckle", "cvo_fe_filter_speckles"):
        assert name in F.SYMBOLS
    # host-only refusals of the context-free entry: they come before any device is touched
    plane, removed = np.ones((4, 4), np.uint16), C.c_int(-5)
    u16p = C.POINTER(C.c_uint16)
    for w, h, stride, sp in ((0, 4, 8, (1, 0)), (4, 8193, 8, (1, 0)), (4, 4, 7, (1, 0)), (4, 4, 8, (0, 0))):
        assert L.cvo_fe_filter_speckles(0, plane.ctypes.data_as(u16p), stride, w, h, C.byref(F.Speckle(*sp)), None,
                                        C.byref(removed)) != 0
    assert L.cvo_fe_filter_speckles(0, plane.ctypes.data_as(u16p), 8, 4, 4, None, None, C.byref(removed)) != 0
    assert L.cvo_fe_filter_speckles(0, None, 8, 4, 4, C.byref(F.Speckle(1, 0)), None, C.byref(removed)) != 0
    assert removed.value == -5 and plane.all()
