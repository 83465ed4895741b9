"""CPU: the stereo contract of include/cvo_frontend.h (at cvo_fe_stereo).  The numpy restatement
(tests/fe_stereo_ref.py) against answers written by hand and against a second, plain-loops form of the path
recurrence; the library's host-only cvo_fe_check_stereo and cvo_fe_stereo_depth_table; the structure against its
ctypes mirror; and the conditions the shared cases and the edge cases are there for, which the restatement alone must
meet, so that the GPU tests cannot pass on nothing, with mutants of the restatement (tests/fe_stereo_mutants.py) that
the edge cases must tell from it.  The contract is the library's own definition: PARITY UNPINNED against OpenCV's
or libSGM's matchers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_stereo_mutants as M
import fe_stereo_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against answers written by hand ---------------------------------------

def test_grey_is_the_formula_of_stage_gray():
    img = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 77]]], np.uint8)
    want = [255, 0, (255 * 4899 + 8192) >> 14, (255 * 9617 + 8192) >> 14, (255 * 1868 + 8192) >> 14,
            (10 * 4899 + 200 * 9617 + 77 * 1868 + 8192) >> 14]
    assert S.grey(img).tolist() == [want] and want[2:5] == [76, 150, 29]


def test_census_bit_order_and_clamped_neighbours():
    """one darker pixel: it is neighbour (dy, dx) = (0, -1) of the pixel to its right, the 31st of 62 comparisons
    (three rows of nine, then dx = -4 .. -1), and the first comparison ends as bit 61"""
    g = np.full((9, 11), 100, np.uint8)
    g[4, 4] = 50
    c = S.census(g)
    assert int(c[4, 5]) == 1 << (61 - 30)
    assert int(c[4, 4]) == 0                               # nothing is darker than the dark pixel: strict <
    assert int(c[1, 8]) == 1 << (61 - (6 * 9 - 1))         # (dy, dx) = (3, -4): six rows of nine less the skipped centre
    assert int(c[7, 0]) == 1 << (61 - (0 * 9 + 8))         # (dy, dx) = (-3, 4)
    assert int(c.max()) < 1 << 62
    # a dark corner pixel is, by the clamp, every neighbour up and to the left of the pixels beside it
    g = np.full((9, 11), 100, np.uint8)
    g[0, 0] = 50
    c = S.census(g)
    bits = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if (dy, dx) != (0, 0):
                bits = (bits << 1) | (1 if (min(max(1 + dy, 0), 8), min(max(1 + dx, 0), 10)) == (0, 0) else 0)
    assert int(c[1, 1]) == bits and bin(bits).count("1") == 3 * 4   # dy = -3 .. -1, dx = -4 .. -1


def test_cost_is_a_popcount_and_64_outside():
    cl = np.array([[0, 0b1011, (1 << 62) - 1]], np.uint64)
    cr = np.array([[0b1, 0b1000, 0]], np.uint64)
    Cv = S.cost(cl, cr, 4)
    assert Cv[0, 0].tolist() == [1, 64, 64, 64]
    assert Cv[0, 1].tolist() == [2, 2, 64, 64]            # 1011 ^ 1000, 1011 ^ 0001
    assert Cv[0, 2].tolist() == [62, 61, 61, 64]
    assert S.popcount(np.array([0xFFFFFFFFFFFFFFFF, 0x8000000000000001], np.uint64)).tolist() == [64, 2]


def test_the_recurrence_by_hand():
    """one line of three steps, D = 3, p1 = 2, p2 = 5"""
    Cs = np.array([[[4, 1, 9]], [[3, 3, 0]], [[7, 7, 7]]], np.int64)
    L = S._scan(Cs, 2, 5)
    # step 1: m = 1; d0: min(4, 1 + 2, 6) = 3 -> 3 + 3 - 1 = 5; d1: min(1, 4 + 2, 9 + 2, 6) = 1 -> 3; d2: min(9, 1 + 2, 6) = 3 -> 2
    assert L[1, 0].tolist() == [5, 3, 2]
    # step 2: m = 2; d0: min(5, 3 + 2, 7) = 5 -> 10; d1: min(3, 5 + 2, 2 + 2, 7) = 3 -> 8; d2: min(2, 3 + 2, 7) = 2 -> 7
    assert L[2, 0].tolist() == [10, 8, 7]
    assert L[0, 0].tolist() == [4, 1, 9]


def test_the_vector_form_equals_the_plain_loops():
    st, left, right, _ = S.case_inputs("default-64x64-81")
    left, right = left[20:32, 30:46], right[20:32, 30:46]      # 16 x 12
    for D, p1, p2 in ((8, 8, 32), (16, 1, 255)):
        Cv = S.cost(S.census(S.grey(left)), S.census(S.grey(right)), D)
        a, b = S.path_sums(Cv, p1, p2), S.path_sums_loops(Cv, p1, p2)
        assert a.dtype == b.dtype == np.uint16 and a.shape == (12, 16, D) and np.array_equal(a, b)
        assert len(np.unique(a)) > 20


def test_winner_uniqueness_subpixel_and_left_right_by_hand():
    Sv = np.zeros((1, 3, 8), np.uint16)
    Sv[0, 0] = [9, 9, 5, 9, 9, 5, 9, 9]        # a tie: the smallest d wins; the other minimum is far: not unique
    Sv[0, 1] = [20, 10, 4, 6, 20, 20, 20, 20]   # Sm = 10, Sp = 6: den = 8, off = floor((64 + 8) / 16) = 4
    Sv[0, 2] = [20, 6, 4, 10, 20, 20, 20, 7]    # Sm = 6, Sp = 10: off = floor((-64 + 8) / 16) = floor(-3.5) = -4
    ds, S1 = S.winners(Sv)
    assert ds.tolist() == [[2, 2, 2]] and S1.tolist() == [[5, 4, 4]]
    assert S.subpixel(Sv, ds, S1).tolist() == [[32, 36, 28]]
    # S2 = 5, 20, 7: 5 * 90 < 5 * 100; 20 * 90 < 400 is false; 7 * 90 = 630 < 400 is false, and at 50 per cent 350 < 400
    assert S.not_unique(Sv, ds, S1, 10).tolist() == [[True, False, False]]
    assert S.not_unique(Sv, ds, S1, 50).tolist() == [[True, False, True]]
    assert not S.not_unique(Sv, ds, S1, 0).any()
    # the ends of the range and a flat minimum have no offset
    E = np.array([[[1, 5, 5, 5, 5, 5, 5, 5], [5, 5, 5, 5, 5, 5, 5, 1], [5, 3, 3, 3, 5, 5, 5, 5]]], np.uint16)
    de, e1 = S.winners(E)
    assert de.tolist() == [[0, 7, 1]] and S.subpixel(E, de, e1).tolist() == [[0, 112, 16 + 8]]   # den = 2: (2*16 + 2) // 4 = 8
    # the right map: dR(x) = argmin over d of S(x + d, d), only x + d < w
    R = np.full((1, 3, 8), 50, np.uint16)
    R[0, 2, 2] = 1                              # left pixel 2 matches right pixel 0 at d = 2
    R[0, 1, 0] = 3
    dR = S.right_map(R)
    assert dR.tolist() == [[2, 0, 0]]
    dl = np.array([[0, 1, 2]])
    # pixel 0: x - d = 0, |dR(0) - 0| = 2; pixel 1: x - d = 0, |2 - 1| = 1; pixel 2: x - d = 0, |2 - 2| = 0
    assert S.lr_fails(dl, dR, 0).tolist() == [[True, True, False]]
    assert S.lr_fails(dl, dR, 1).tolist() == [[True, False, False]]
    assert not S.lr_fails(dl, dR, -1).any()
    assert S.lr_fails(np.array([[1, 2, 3]]), dR, 8).tolist() == [[True, True, True]]     # x - d < 0


def test_depth_table_by_hand():
    """fx 2, baseline 0.5, scale 10: (2 * 0.5 * 10) * 16 = 160; ties go to the even neighbour"""
    st = S.make_stereo(baseline=0.5, max_disp=8, min_disp=2)
    U = S.depth_table(st, 2.0, 10.0)
    assert len(U) == 128 and not U[:32].any()                 # below 16 * min_disp
    assert [int(U[q]) for q in (32, 64, 100, 107, 127)] == [5, 2, 2, 1, 1]   # 160 / 64 = 2.5 -> 2; 160 / 107 = 1.495 -> 1
    assert int(S.depth_table(S.make_stereo(baseline=0.5, max_disp=32), 2.0, 10.0)[320]) == 0    # 0.5 -> 0: outside [1, 65535]
    big = S.depth_table(S.make_stereo(baseline=0.5, max_disp=8), 2.0, 16384.0)   # 262144 / q
    assert int(big[16]) == 16384 and int(big[4 - 0]) == 0 and int(big[127]) == 2064


# ---- the library's host-only entries and the structure -------------------------------------

def test_check_stereo_table(pkg):
    F = pkg.frontend
    L = F.lib()
    assert L.cvo_fe_check_stereo(None) != 0
    for st in S.good_stereos():
        assert F.check_stereo(F.Stereo(**st)), st
    bad = S.bad_stereos()
    assert {k for st in bad for k in st if st[k] != dict(S.make_stereo(), pad_=0).get(k)} == {
        "baseline", "max_disp", "min_disp", "p1", "p2", "uniqueness", "lr_max", "pad_"}
    for st in bad:
        assert not F.check_stereo(F.Stereo(**st)), st
    # set / get / submit without a context
    good = F.Stereo()
    assert L.cvo_fe_set_stereo(None, C.byref(good)) != 0 and L.cvo_fe_set_stereo(None, None) != 0
    assert L.cvo_fe_get_stereo(None, C.byref(good), None) != 0
    assert L.cvo_fe_submit_stereo(None, None, 0, None, 0, 4, 1) != 0
    assert L.cvo_fe_create_pointcloud_stereo(None, None, 0, None, 0, 4, 1, None, None, 0, None) != 0


def test_stereo_structure(pkg):
    """32 bytes, and the header's members in the header's order against the ctypes mirror"""
    F = pkg.frontend
    assert C.sizeof(F.Stereo) == 32
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()
    body = re.search(r"typedef struct cvo_fe_stereo \{(.*?)\} cvo_fe_stereo;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for ctype, names in re.findall(r"\b(float|int32_t)\s+([^;]+);", body):
        members += [(n.strip(), ctype) for n in names.split(",")]
    mirror = [(n, "float" if t is C.c_float else "int32_t") for n, t in F.Stereo._fields_]
    assert members == mirror and len(mirror) == 8
    assert [getattr(F.Stereo, n).offset for n, _ in F.Stereo._fields_] == list(range(0, 32, 4))
    st = F.Stereo(0.54, 128, 2, 7, 90, 15, 0)
    assert eval(repr(st), {"Stereo": F.Stereo}) == st and st != F.Stereo(0.54, 128, 2, 7, 90, 15, 1)
    assert st.astuple()[1:] == (128, 2, 7, 90, 15, 0)
    assert (F.STAGE_RIGHT_GRAY, F.STAGE_CENSUS_L, F.STAGE_CENSUS_R, F.STAGE_SGM_SUM, F.STAGE_DISPARITY,
            F.STAGE_STEREO) == (15, 16, 17, 18, 19, 20)
    for name, value in (("RIGHT_GRAY", 15), ("CENSUS_L", 16), ("CENSUS_R", 17), ("SGM_SUM", 18), ("DISPARITY", 19),
                        ("STEREO", 20)):
        assert re.search(r"CVO_FE_STAGE_%s = %d\b" % (name, value), text), name
    assert (F.STEREO_UNIQUE, F.STEREO_LR, F.STEREO_MIN, F.STEREO_DEPTH) == (S.UNIQUE, S.LR, S.MIN, S.DEPTH) == (1, 2, 4, 8)
    assert re.search(r"CVO_FE_STEREO_UNIQUE = 1, CVO_FE_STEREO_LR = 2, CVO_FE_STEREO_MIN = 4, CVO_FE_STEREO_DEPTH = 8", text)
    for name in ("cvo_fe_check_stereo", "cvo_fe_set_stereo", "cvo_fe_get_stereo", "cvo_fe_submit_stereo",
                 "cvo_fe_create_pointcloud_stereo", "cvo_fe_stereo_depth_table"):
        assert name in F.SYMBOLS
    declared = set(re.findall(r"\b(cvo_fe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(F.SYMBOLS)


def test_depth_table_by_bytes(pkg):
    """rows 4 and 5 of the camera table with the baselines of their rigs, and a caller's camera"""
    F = pkg.frontend
    cams = []
    for seq, baseline in ((4, 0.54), (5, 0.537)):
        cam = F.camera(seq)
        assert cam["scaling_factor"] == 2000.0
        cams.append((cam["fx"], cam["scaling_factor"], baseline))
    cams.append((517.3, 5000.0, 0.075))                       # a caller's camera: TUM's pinhole on a 7.5 cm rig
    cams.append((S.FX, S.SCALE, 0.25))                        # ... and the shared cases'
    seen = set()
    for fx, scale, baseline in cams:
        for D, min_disp in ((8, 1), (32, 1), (48, 3), (128, 1), (128, 8), (64, 200)):
            st = S.make_stereo(baseline=baseline, max_disp=D, min_disp=min_disp)
            got = F.stereo_depth_table(F.Stereo(**st), fx, scale)
            want = S.depth_table(st, fx, scale)
            assert got.dtype == np.uint16 and got.shape == (16 * D,) and got.tobytes() == want.tobytes(), (fx, D, min_disp)
            assert not got[:16 * min_disp].any()
            seen |= {"zero" if not got.any() else "some", "overflow" if (got[16 * min_disp:] == 0).any() else "all"}
    assert seen == {"zero", "some", "overflow", "all"}
    # KITTI: 0.54 m * 718.856 px = 388 m px: 2000 units per metre overflow uint16 beyond 32.8 m, i.e. below 11.85 px
    U = F.stereo_depth_table(F.Stereo(0.54, 128), cams[0][0], 2000.0)
    assert U[189] == 0 and U[190] == 65378 and U[2047] == 6068
    L = F.lib()
    u16p = C.POINTER(C.c_uint16)
    out = np.zeros(16 * 128, np.uint16)
    good = F.Stereo(0.54, 128)
    assert L.cvo_fe_stereo_depth_table(None, 700.0, 2000.0, out.ctypes.data_as(u16p)) != 0
    assert L.cvo_fe_stereo_depth_table(C.byref(good), 700.0, 2000.0, None) != 0
    assert L.cvo_fe_stereo_depth_table(C.byref(F.Stereo(0.54, 100)), 700.0, 2000.0, out.ctypes.data_as(u16p)) != 0
    for fx, scale in ((0.0, 2000.0), (700.0, 0.0), (-1.0, 2000.0), (float("nan"), 2000.0), (700.0, float("inf"))):
        assert L.cvo_fe_stereo_depth_table(C.byref(good), fx, scale, out.ctypes.data_as(u16p)) != 0
    assert not out.any()


# ---- the cases reach what they are for -----------------------------------------------------

def _shares(name):
    w, h = S.CASES[name][:2]
    st, left, right, disp = S.case_inputs(name)
    P = S.case_planes(name)
    kept = P["flags"] == 0
    out = dict(kept=kept.mean(), flags={k: int(np.count_nonzero(P["flags"] & k)) for k in (1, 2, 4, 8)})
    if disp is not None:
        box, back, ramp = S.regions(w, h)
        err = np.abs(P["q"] - 16.0 * disp)
        out.update(box=(int((box & kept).sum()), bool((err[box & kept] <= 16).all())),
                   back=(int((back & kept).sum()), bool((err[back & kept] <= 16).all())),
                   ramp=(int((ramp & kept).sum()), float((err[ramp & kept] <= 8).mean())))
    return P, kept, out


@pytest.mark.parametrize("name", S.DEFAULTS)
def test_default_cases_fire_every_flag_keep_half_and_find_the_disparities(name):
    """Measured on the restatement, three seeds each (kept; box interior, lower background within one pixel; ramp
    within half a pixel): 64 x 64: 80 %, 100 %, 100 %, 97.3-98.2 %; 96 x 64: 85 %, 100 %, 100 %, 96.9-97.5 %;
    127 x 193 at D 48: 87 %, 100 %, 100 %, 98.3-98.6 %.  Every one of the four flags fires in every case: DEPTH because
    the cases' baseline of 0.25 m puts disparities below 5.5 pixels -- the left part of the ramp -- beyond what
    uint16 holds at 2000 units per metre."""
    P, kept, sh = _shares(name)
    print(name, sh)
    for k in (S.UNIQUE, S.LR, S.MIN, S.DEPTH):
        assert sh["flags"][k] >= 1, k
    assert sh["kept"] >= 0.5
    assert sh["box"][0] >= 100 and sh["box"][1]
    assert sh["back"][0] >= 500 and sh["back"][1]
    assert sh["ramp"][0] >= 100 and sh["ramp"][1] >= 0.95
    assert np.array_equal(P["depth"] != 0, kept) and np.array_equal(P["disparity"] != 0, kept)
    assert P["sum"].max() <= 4 * (64 + 255) and P["q"].max() < 16 * S.CASES[name][3]["max_disp"]
    assert len(np.unique(P["q"][kept] & 15)) >= 12            # sub-pixel offsets of many kinds


def test_the_other_cases():
    """Measured on the restatement (share of pixels kept): d128 76 %, with d* >= 64 in 1148 pixels, 8 of them kept (the
    box at 70 shows texture that the background at 6 shows too, so the left-right test takes most of it) and dR >= 64
    in 316; uniqueness0 85 % and no pixel UNIQUE; lr-off 90 % and no pixel LR; min8 (background at 10) 76 % with MIN
    on 1260 pixels against 220 under min_disp 1.  The floor for each is a quarter kept."""
    for name in ("d128", "uniqueness0", "lr-off", "min8"):
        P, kept, sh = _shares(name)
        print(name, sh)
        assert sh["kept"] >= 0.25, name
    P, kept, _ = _shares("d128")
    assert np.count_nonzero(P["dL"] >= 64) >= 100 and np.count_nonzero(kept & (P["dL"] >= 64)) >= 1
    assert np.count_nonzero(P["dR"] >= 64) >= 100
    base = S.case_planes("default-96x64-82")["flags"]
    off = S.case_planes("uniqueness0")["flags"]
    assert not (off & S.UNIQUE).any() and (base & S.UNIQUE).any()
    assert np.count_nonzero((off == 0) & (base == S.UNIQUE)) >= 1            # pixels the test alone had dropped
    off = S.case_planes("lr-off")["flags"]
    assert not (off & S.LR).any() and np.count_nonzero((off == 0) & (base == S.LR)) >= 100
    P8 = S.case_planes("min8")
    assert np.count_nonzero(P8["flags"] == S.MIN) >= 500                     # the rule decides alone
    assert P8["q"][P8["flags"] == S.MIN].max() >= 16 * 7 and not (P8["flags"] & S.DEPTH).any()


def test_a_texture_free_pair_gives_the_smallest_d():
    """Every census word is 0, so every cost with x - d >= 0 is 0 and three of the four paths tie over those d.  The
    path from the left does not: at x = 0 only d = 0 has a match (cost 64 for the others), and the recurrence carries
    that along the row as min(p1 * d, p2), for ever.  S is that ramp, and d* = 0, the smallest d, everywhere."""
    P, kept, sh = _shares("flat")
    st = S.CASES["flat"][3]
    assert not P["census_l"].any() and not P["census_r"].any()
    Sv = P["sum"].astype(np.int64)
    ramp = np.minimum(st["p1"] * np.arange(st["max_disp"]), st["p2"])
    assert (Sv[:, 40:, :] == ramp[None, None, :]).all()
    assert (Sv[:, :, 0] == 0).all() and (Sv[:, :, 1:] > 0).all()
    assert not P["dL"].any() and not P["dR"].any() and not P["q"].any()
    assert (P["flags"] == S.MIN).all() and not P["depth"].any() and not P["disparity"].any()


def test_ties_occur_in_the_textured_cases():
    """... so "the smallest d on ties" of both maps is put to the test by the textured cases: measured, the minimum of
    S(p, .) is attained more than once at 13-30 pixels of a case and that of the right map's diagonal at 73-999"""
    for name in ("default-64x64-81", "default-127x193-83", "d128"):
        Sv = S.case_planes(name)["sum"].astype(np.int64)
        h, w, D = Sv.shape
        assert np.count_nonzero((Sv == Sv.min(axis=2, keepdims=True)).sum(axis=2) > 1) >= 5
        SR = np.full((h, w, D), S.BIG, np.int64)
        for d in range(min(D, w)):
            SR[:, :w - d, d] = Sv[:, d:, d]
        assert np.count_nonzero((SR == SR.min(axis=2, keepdims=True)).sum(axis=2) > 1) >= 20


# ---- the edge cases reach what they are for ------------------------------------------------

def _edge(name):
    """(planes, kept, d*, sub-pixel offset) of an edge case"""
    P = S.edge_planes(name)
    return P, P["flags"] == 0, P["dL"], P["q"] - 16 * P["dL"]


def _kept_at(name, d):
    """(kept pixels with d* = d, those of them with a non-zero offset)"""
    P, kept, ds, off = _edge(name)
    here = kept & (ds == d)
    return int(here.sum()), int((here & (off != 0)).sum())


def test_the_vector_form_equals_the_plain_loops_across_the_seam():
    """the restatement itself across d = 63 | 64: a crop of 80 x 8 of seam-72's pair at D 72, so that d = 60 .. 71 have
    pixels inside the image, and at penalties under which the neighbour terms decide"""
    st, left, right, _ = S.edge_inputs("seam-72")
    left, right = left[24:32, 60:140], right[24:32, 60:140]
    for p1, p2 in ((8, 32), (1, 255)):
        Cv = S.cost(S.census(S.grey(left)), S.census(S.grey(right)), 72)
        assert (Cv[:, 72:, 60:] < 64).all()
        a, b = S.path_sums(Cv, p1, p2), S.path_sums_loops(Cv, p1, p2)
        assert a.dtype == b.dtype == np.uint16 and a.shape == (8, 80, 72) and np.array_equal(a, b)
        assert len(np.unique(a[:, :, 62:66])) > 20


def test_the_seam_cases_show_q_on_both_sides_of_the_seam():
    """uniqueness 0 and lr_max -1: the disparity plane shows q wherever there is a depth.  Measured on the restatement
    (kept pixels at that d*, those of them with a non-zero offset; the floor is 200 with an offset, 1000 kept for
    seam-back): seam-128 d* 63: 979, 955; d* 64: 1046, 1020.  seam-72 d* 64: 1000, 974; d* 65: 1033, 1010, with all
    2033 kept winners in the 8 live lanes of the upper register.  seam-back d* 62: 4949; d* 64: 2039."""
    for name, d in (("seam-128", 63), ("seam-128", 64), ("seam-72", 64), ("seam-72", 65)):
        n, with_offset = _kept_at(name, d)
        print(name, d, n, with_offset)
        assert with_offset >= 200, (name, d)
    for d in (62, 64):
        n, _ = _kept_at("seam-back", d)
        print("seam-back", d, n)
        assert n >= 1000, d
    for name in ("seam-128", "seam-72", "seam-back"):
        P, kept, ds, off = _edge(name)
        assert not (P["flags"] & (S.UNIQUE | S.LR)).any()
        assert np.array_equal(P["disparity"][kept], P["q"][kept]) and (P["disparity"][kept] != 0).all()
    assert S.EDGE_CASES["seam-72"][2]["max_disp"] == 72


def test_the_ends_of_D():
    """d* = D - 1 has no upper neighbour and no offset; d* = D - 2 has both.  Measured (kept, with an offset; the floor
    is 200, for d8 100): full-64 d* 62: 987, 957; d* 63: 1029, 0.  top-128 d* 126: 1471, 1424; d* 127: 1307, 0.  d8
    d* 6: 470, 446; d* 7: 564, 0.  d120 (box 100.5 over a background at 70): d* 100: 1548, 1505; d* 101: 1380, 1342,
    and 11722 kept winners from d = 64 up."""
    for name, D, floor in (("full-64", 64, 200), ("top-128", 128, 200), ("d8", 8, 100)):
        assert S.EDGE_CASES[name][2]["max_disp"] == D
        n, with_offset = _kept_at(name, D - 2)
        top, top_with_offset = _kept_at(name, D - 1)
        print(name, n, with_offset, top, top_with_offset)
        assert n >= floor and with_offset >= floor and top >= floor and top_with_offset == 0, name
    for d in (100, 101):
        assert _kept_at("d120", d)[1] >= 200
    P, kept, ds, off = _edge("d120")
    assert P["sum"].shape[2] == 120 and np.count_nonzero(kept & (ds >= 64)) >= 1000


def test_narrow_and_wide():
    """narrow: 64 pixels wide at D 128: x - d < 0 at 75 % of all (pixel, d), at half of the d for every pixel, and the
    right map still finds disparities up to 35.  wide: 1241 steps along a row, no multiple of 8, the box at 70: 13236
    pixels kept, every one with d* >= 64; beyond x = 1024 the background at 6 is found at 11714 of 13888 pixels."""
    P, kept, ds, off = _edge("narrow")
    Cv = S.cost(P["census_l"], P["census_r"], 128)
    assert P["sum"].shape == (64, 64, 128) and (Cv[:, :, 64:] == 64).all() and (Cv == 64).mean() >= 0.7
    assert kept.sum() >= 500 and ds.max() < 64 and P["dR"].max() < 64
    P, kept, ds, off = _edge("wide")
    assert P["sum"].shape == (64, 1241, 128) and 1241 % 8 != 0
    assert np.count_nonzero(kept & (ds >= 64)) >= 5000
    assert np.count_nonzero(ds[:, 1024:] == 6) >= 5000        # the background beyond step 1024 (no depth there: DEPTH)


def test_the_left_right_test_turns_on_dR_at_the_seam():
    """The seam scenes under uniqueness 10 and lr_max 0: a pixel is kept only where dR equals d* exactly.  Measured:
    seam-128-lr0: dR = 62, 63, 64, 65 at 42, 226, 91, 12 pixels, 164 kept with d* in 63..65; seam-72-lr0: 24, 48, 197,
    92 and 133.  The floors: 10 pixels for each value, 50 kept.  seam-back-lr0 has dR = 62, 63, 64 at 4886, 73, 2032
    pixels (none at 65: nothing lies there) and 2032 kept with d* in 63..65."""
    for name in ("seam-128-lr0", "seam-72-lr0"):
        P, kept, ds, off = _edge(name)
        assert S.EDGE_CASES[name][2]["lr_max"] == 0 and S.EDGE_CASES[name][2]["uniqueness"] == 10
        counts = [int(np.count_nonzero(P["dR"] == v)) for v in (62, 63, 64, 65)]
        n = int(np.count_nonzero(kept & (ds >= 63) & (ds <= 65)))
        print(name, counts, n)
        assert min(counts) >= 10 and n >= 50, name
        assert np.count_nonzero(P["flags"] & S.LR) >= 1000 and np.count_nonzero(P["flags"] & S.UNIQUE) >= 10
    P, kept, ds, off = _edge("seam-back-lr0")
    assert min(np.count_nonzero(P["dR"] == v) for v in (62, 63, 64)) >= 10
    assert np.count_nonzero(kept & (ds == 62)) >= 1000 and np.count_nonzero(kept & (ds == 64)) >= 1000


def test_the_settings_cases():
    """On the pair of default-96x64-82, measured (share kept; UNIQUE, LR, MIN, DEPTH): p255 84.6 %; 155, 677, 304, 73.
    p1 83.1 %; 141, 740, 233, 248.  u99-lr8 56.4 %; 2623, 289, 220, 19.  lr0 84.1 %; 47, 769, 220, 192.  min200 0 %;
    47, 604, 6144, 0.  baseline1e-6 0.1 %; 47, 604, 220, 5505: at the cases' camera 1e-6 m are 23 / q units, so the table
    is 1 up to q = 46 and six pixels keep a depth of 1, the smallest there is.  baseline1e-6-min3 0 %; 47, 604, 294,
    5505: the table begins at q = 48 and is all zero.  p255-noise 11.1 %; 2447, 2523, 2008, 793.
    The bound under every uint16 sum, ST_INF and the winner's keys, S <= 4 (64 + p2), is reached at p2 = 255 on the
    texture and on the noise: 1276.  At p1 = p2 = 1 it is 260 and reached too."""
    base = S.case_planes("default-96x64-82")
    for name in ("p255", "p255-noise"):
        assert int(S.edge_planes(name)["sum"].max()) == 4 * (64 + 255) == 1276, name
    assert int(S.edge_planes("p1")["sum"].max()) == 4 * (64 + 1)
    for name in ("p255", "p1", "u99-lr8", "lr0"):
        P, kept, ds, off = _edge(name)
        assert np.array_equal(P["census_l"], base["census_l"]) and kept.mean() >= 0.5, name
        assert not np.array_equal(P["flags"], base["flags"]), name
    assert np.array_equal(S.edge_planes("u99-lr8")["sum"], base["sum"])
    # uniqueness 99: S2 < 100 S1 flags all but a lone minimum of 0; lr_max 8 forgives what lr_max 1 does not
    u = S.edge_planes("u99-lr8")["flags"]
    assert np.count_nonzero(u & S.UNIQUE) >= 10 * np.count_nonzero(base["flags"] & S.UNIQUE) >= 10
    assert 1 <= np.count_nonzero(u & S.LR) < np.count_nonzero(base["flags"] & S.LR)
    assert np.count_nonzero(S.edge_planes("lr0")["flags"] & S.LR) > np.count_nonzero(base["flags"] & S.LR)
    P, kept, ds, off = _edge("min200")
    assert (P["flags"] & S.MIN).all() and not kept.any() and not P["depth"].any() and not P["table"].any()
    P, kept, ds, off = _edge("baseline1e-6-min3")
    assert not P["table"].any() and not kept.any()
    clean = P["flags"]
    assert np.count_nonzero(clean == S.DEPTH) >= 5000 and not (clean & S.DEPTH)[(clean & 7) != 0].any()
    P, kept, ds, off = _edge("baseline1e-6")
    assert int(P["table"].max()) == 1 and 1 <= kept.sum() <= 20 and (P["depth"][kept] == 1).all()
    assert np.count_nonzero(P["flags"] == S.DEPTH) >= 5000


def _tie_share(V):
    """the share of pixels at which the minimum over d is attained more than once"""
    return float(((V == V.min(axis=2, keepdims=True)).sum(axis=2) > 1).mean())


def test_the_hostile_images():
    """Measured on the restatement (share kept; UNIQUE, LR, MIN, DEPTH), 96 x 64 under the default settings:
    noise      17.2 %; 2843, 3682, 538, 409.  d* and dR take every one of the 32 values.
    stripes     0 %; 0, 0, 6144, 0.  The cost C(p, .) is 0 at every multiple of 8 inside the row; its minimum is
                attained more than once at 89.6 % of the pixels.  The minimum of S(p, .) is attained more than once at
                NO pixel (share 0): at x = 0 only d = 0 lies inside the image, and the path from the left carries that
                along the row as min(p1 d, p2) for ever, as it does on a texture-free pair.  What ties is the second
                minimum of the uniqueness test, over d outside d* - 1 .. d* + 1: it is attained more than once at
                83.3 % of the pixels, and from x = 26 on it is S(8) = S(16) = S(24) (46 in the middle of the image).
    checker     0 %; 0, 0, 6144, 0.  C ties at 93.8 % of the pixels (every even d), S at none, for the same reason.
    saturated   0 %; 0, 0, 6144, 0.  No pixel has a darker neighbour in either image: both census planes are zero.
    same        0 %; 0, 0, 6144, 0.  d* = dR = 0 at every pixel although the texture is there (C ties at 1 %).
    tail        0 %; 28, 70, 6076, 4.  See test_the_mutants_are_told_apart.
    What each is there for is asserted below; that all pixels are flagged where d* = 0 is the rule q < 16 min_disp."""
    out = {}
    for name in ("noise", "stripes", "checker", "saturated", "same", "tail"):
        P, kept, ds, off = _edge(name)
        Cv = S.cost(P["census_l"], P["census_r"], 32)
        out[name] = (P, kept, _tie_share(Cv), _tie_share(P["sum"].astype(np.int64)))
        print(name, kept.mean(), [int(np.count_nonzero(P["flags"] & k)) for k in (1, 2, 4, 8)], out[name][2:])
    P, kept, c_ties, s_ties = out["noise"]
    assert len(np.unique(P["dL"])) == 32 and len(np.unique(P["dR"])) == 32 and kept.sum() >= 500
    assert all(np.count_nonzero(P["flags"] & k) >= 100 for k in (1, 2, 4, 8))
    P, kept, c_ties, s_ties = out["stripes"]
    Cv = S.cost(P["census_l"], P["census_r"], 32)
    assert (Cv[:, 36:92, ::8] == 0).all() and c_ties >= 0.8 and s_ties == 0.0
    Sv = P["sum"].astype(np.int64)
    assert not Sv[:, :, 0].any() and Sv[:, :, 1:].min() >= 32                  # p2, from the path from the left
    assert (Sv[:, 26:, 8] == Sv[:, 26:, 16]).all() and (Sv[:, 26:, 8] == Sv[:, 26:, 24]).all()
    assert (Sv[:, 26:88, 8:9] == Sv[:, 26:88, 2:].min(axis=2, keepdims=True)).all() and _tie_share(Sv[:, :, 2:]) >= 0.8
    assert (P["flags"] == S.MIN).all() and not P["dL"].any()
    P, kept, c_ties, s_ties = out["checker"]
    assert P["census_l"].any() and c_ties >= 0.9 and (P["flags"] == S.MIN).all() and not P["dL"].any()
    P, kept, c_ties, s_ties = out["saturated"]
    assert (P["gray_l"] == 255).all() and not P["gray_r"].any() and not P["census_l"].any() and not P["census_r"].any()
    assert (P["flags"] == S.MIN).all() and not P["dL"].any()
    P, kept, c_ties, s_ties = out["same"]
    assert len(np.unique(P["census_l"])) > 5000 and np.array_equal(P["census_l"], P["census_r"])
    assert not P["dL"].any() and not P["dR"].any() and (P["flags"] == S.MIN).all() and c_ties < 0.05
    for name in ("stripes", "checker", "saturated", "same", "tail", "min200", "baseline1e-6-min3"):
        P = S.edge_planes(name)
        assert not P["depth"].any() and not P["disparity"].any(), name       # the GPU test expects an empty cloud


# ---- ... and would catch the errors they are there for -------------------------------------

def _differ(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def test_the_mutants_are_told_apart():
    """Each mutant of tests/fe_stereo_mutants.py against the restatement, on the cases named for it (measured: the
    number of elements that differ; the floor is one):
    seam cut in the path        sum: seam-128 33502, seam-72 7619, seam-back 33265, top-128 11179
    wrong register, sub-pixel   kept disparity: seam-128 2023, seam-72 806, seam-back 2062
    wrap at the top             sum: full-64 694, top-128 4003, d8 476
    right map without x + d < w flags: tail 7
    band cut at the seam        flags: seam-128-lr0 354, seam-back-lr0 14
    narrow keys                 p255-noise: d* 2414, flags 2098, disparity 117
    The right map's bound is all but redundant under this contract: what the diagonal reads beyond the row are pixels
    at the left end of the next row with x - d < 0, whose cost is 64 on every path, so their sum is above 256 and above
    every sum inside the row that won at its own pixel with less.  On the textured, noise and seam cases with lr_max >= 0
    the mutant changes dR at no more than 5 right pixels and no flag.  `tail` is made for it: under p2 = 255 the last two
    columns of the left image (noise against an otherwise identical pair) win at d = 0 with sums above 256 (23 pixels
    of the last column), the next row begins with d = 1 one step outside the image at 64 + p1 per path, and lr_max = 0
    turns on dR = 0 against dR = 1: 7 flags."""
    st = lambda name: S.EDGE_CASES[name][2]
    for name in ("seam-128", "seam-72", "seam-back", "top-128"):
        P = S.edge_planes(name)
        n = _differ(M.sums(P, st(name), seam_cut=True), P["sum"])
        print("seam cut", name, n)
        assert n >= 1, name
    for name in ("seam-128", "seam-72", "seam-back"):
        P = S.edge_planes(name)
        Q = M.planes(P, st(name), subpixel=M.subpixel_own_half)
        kept = P["flags"] == 0
        n = _differ(Q["disparity"][kept], P["disparity"][kept])
        print("wrong register", name, n)
        assert n >= 1, name
    for name in ("full-64", "top-128", "d8"):
        P = S.edge_planes(name)
        n = _differ(M.sums(P, st(name), wrap=True), P["sum"])
        print("wrap", name, n)
        assert n >= 1, name
    P = S.edge_planes("tail")
    assert st("tail")["lr_max"] >= 0
    n = _differ(M.planes(P, st("tail"), right_map=M.right_map_unbounded)["flags"], P["flags"])
    print("right map", n)
    assert n >= 1
    for name in ("seam-128-lr0", "seam-back-lr0"):
        P = S.edge_planes(name)
        n = _differ(M.planes(P, st(name), not_unique=M.not_unique_own_half)["flags"], P["flags"])
        print("band", name, n)
        assert n >= 1, name
    P = S.edge_planes("p255-noise")
    Q = M.planes(P, st("p255-noise"), winners=M.winners_narrow_keys, subpixel=M.subpixel_unchecked)
    print("narrow keys", [_differ(Q[k], P[k]) for k in ("dL", "flags", "disparity", "depth")])
    assert _differ(Q["flags"], P["flags"]) >= 1 and _differ(Q["disparity"], P["disparity"]) >= 1
    # the mutants are the restatement where their error cannot show: below the seam, and with every key in 10 bits
    P = S.case_planes("default-64x64-81")
    st0 = S.CASES["default-64x64-81"][3]
    assert np.array_equal(M.sums(P, st0, seam_cut=True), P["sum"]) and np.array_equal(M.sums(P, st0), P["sum"])
    for stage in (dict(subpixel=M.subpixel_own_half), dict(not_unique=M.not_unique_own_half),
                  dict(winners=M.winners_narrow_keys, subpixel=M.subpixel_unchecked), dict(subpixel=M.subpixel_unchecked)):
        Q = M.planes(P, st0, **stage)
        assert all(np.array_equal(Q[k], P[k]) for k in Q), list(stage)
