"""CPU: the stereo contract of include/cvo_frontend.h (at cvo_fe_stereo).  The numpy restatement
(tests/fe_stereo_ref.py) against answers written by hand and against a second, plain-loops form of the path
recurrence; the library's host-only cvo_fe_check_stereo and cvo_fe_stereo_depth_table; the structure against its
ctypes mirror; and the conditions the shared cases are there for, which the restatement alone must meet, so that the
GPU tests cannot pass on nothing.  The contract is the library's own definition: PARITY UNPINNED against OpenCV's
or libSGM's matchers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

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
