"""CPU: the rig contract of include/cvo_frontend.h (at cvo_fe_stereo_rig).  The library's host-only helper, maps and
check against the numpy restatement (tests/fe_stereo_rig_ref.py); properties of a rectification that do not depend on
the restatement; cases whose answer is known exactly; the conditions rigs A and B are there for, which the
restatement alone must meet, so that the GPU tests cannot pass on nothing; mutants of the restatement that rig B must
tell from it; the refusals.  The contract is the library's own definition: PARITY UNPINNED against cv::stereoRectify."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fe_rectify_ref as R
import fe_stereo_rig_ref as G
import fe_stereo_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _library_rig(F, name):
    w, h, _, calib = G.CALIBS[name]
    return F.stereo_rectify(G.calib_struct(F, calib), w, h, G.DEPTH_SCALE)


def _floats(struct):
    return np.frombuffer(bytes(struct), np.float32)


# ---- 1. the maps by bytes ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "I"])
def test_maps_equal_the_restatements_by_bytes(pkg, name):
    """from the float32 rig, both cameras; (for A and B the rig is the restatement's, so that the helper's last
    place -- test 2 -- stays out of this one)"""
    F = pkg.frontend
    if name == "I":
        w, h, rig = 64, 64, G.RIG_I
    else:
        w, h, _, rig = G.case(name)[:4]
    struct = G.to_struct(F, rig)
    assert F.check_stereo_rig(struct)
    assert np.array_equal(_floats(struct), G.rig_floats(rig))
    for which in (0, 1):
        qu, qv = F.stereo_rig_map(struct, which, w, h)
        want = G.rig_map(rig, which, w, h)
        assert qu.dtype == np.int32 and qu.shape == (h, w)
        assert qu.tobytes() == want[0].tobytes() and qv.tobytes() == want[1].tobytes(), (name, which)


# ---- 2. the helper -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_helper_against_the_restatement(pkg, name):
    """every member within 2 float32 ulps: the two differ through libm's sin, cos and atan2 only, i.e. by a few
    float64 ulps, which shows in a float32 member only at a rounding boundary"""
    F = pkg.frontend
    w, h, _, calib = G.CALIBS[name]
    got = _floats(_library_rig(F, name))
    want = G.rig_floats(G.rectify(calib, w, h, G.DEPTH_SCALE))
    assert got.shape == want.shape == (42,)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    # (members near zero: an ulp there is tiny and signs may differ; held to 2 ulps of the member's scale, 1 for R and pixels)
    small = np.abs(want) < 1e-3
    assert np.all(ulps[~small] <= 2), (got[~small][ulps[~small] > 2], want[~small][ulps[~small] > 2])
    assert np.all(np.abs(got[small].astype(np.float64) - want[small]) <= 2 * np.spacing(np.float32(1.0)))
    assert np.array_equal(got[:18], want[:18])                # the cameras are copied through


# ---- 3. properties that do not depend on the restatement ---------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_a_rectification_has_the_properties_of_one(pkg, name):
    """200 points 1 to 5 m in front of the rig, carried into both cameras by the calibration, turned by the float32
    R_k and projected with the rectified pinhole in float64: the same row, a disparity of f b / Z, both within 1e-4 px
    (float32 rotation entries bound the error near 2e-5 px at f = 100); the two optical axes land, on average, in the
    middle of the image"""
    F = pkg.frontend
    w, h, _, calib = G.CALIBS[name]
    rig = _library_rig(F, name)
    Rl = np.array(rig.R_left, np.float64).reshape(3, 3)
    Rr = np.array(rig.R_right, np.float64).reshape(3, 3)
    Rc = np.asarray(calib["R"], np.float64).reshape(3, 3)
    T = np.asarray(calib["T"], np.float64)
    rng = np.random.Generator(np.random.PCG64(G.SEED))
    pl = np.stack([rng.uniform(-1.0, 1.0, 200), rng.uniform(-1.0, 1.0, 200), rng.uniform(1.0, 5.0, 200)], axis=1)
    pr = pl @ Rc.T + T
    ql, qr = pl @ Rl.T, pr @ Rr.T
    f, b = float(rig.fx), float(rig.baseline)
    assert rig.fx == rig.fy
    ul, vl = f * ql[:, 0] / ql[:, 2] + rig.cx, f * ql[:, 1] / ql[:, 2] + rig.cy
    ur, vr = f * qr[:, 0] / qr[:, 2] + rig.cx, f * qr[:, 1] / qr[:, 2] + rig.cy
    print("rows differ by at most %.3g px, disparities from f b / Z by at most %.3g px"
          % (np.abs(vl - vr).max(), np.abs((ul - ur) - f * b / ql[:, 2]).max()))
    assert np.abs(vl - vr).max() <= 1e-4
    assert np.abs(ql[:, 2] - qr[:, 2]).max() <= 1e-5          # one depth along the common axis
    assert np.abs((ul - ur) - f * b / ql[:, 2]).max() <= 1e-4
    assert np.all(ul - ur > 0)
    land = [(f * Rk[0, 2] / Rk[2, 2] + rig.cx, f * Rk[1, 2] / Rk[2, 2] + rig.cy) for Rk in (Rl, Rr)]
    mean = np.mean(land, axis=0)
    assert abs(mean[0] - (w - 1) / 2.0) <= 1e-4 and abs(mean[1] - (h - 1) / 2.0) <= 1e-4


# ---- 4. exact cases ----------------------------------------------------------------------------

def test_exact_cases(pkg):
    F = pkg.frontend
    w = h = 64
    rng = np.random.Generator(np.random.PCG64(G.SEED))
    left, right = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    v, u = np.mgrid[0:h, 0:w]
    # rig I: the identity map, every pixel valid
    for which in (0, 1):
        qu, qv = F.stereo_rig_map(G.to_struct(F, G.RIG_I), which, w, h)
        assert np.array_equal(qu, 32 * u) and np.array_equal(qv, 32 * v)
        assert G.valid(qu, qv).all()
        assert np.array_equal(R.remap_colour(left, qu, qv), left)
    # a rectified cx of the raw cx + 3: the image shifted by three columns, the border replicated, V = 0 in columns 0..2
    shifted = dict(G.RIG_I, cx=34.5)
    qu, qv = F.stereo_rig_map(G.to_struct(F, shifted), 0, w, h)
    assert np.array_equal(qu, 32 * np.maximum(u - 3, -1)) and np.array_equal(qv, 32 * v)   # (the clamp to -1)
    got = R.remap_colour(left, qu, qv)
    assert np.array_equal(got[:, 3:], left[:, :-3]) and np.array_equal(got[:, :3], np.repeat(left[:, :1], 3, axis=1))
    V = G.valid(qu, qv)
    assert not V[:, :3].any() and V[:, 3:].all()
    # a right camera mounted upside down: exactly right[::-1, ::-1] -- which way the rotation is applied
    flipped = dict(G.RIG_I, R_right=np.diag([-1.0, -1.0, 1.0]).reshape(9))
    assert flipped["cx"] == (w - 1) / 2.0 and flipped["cy"] == (h - 1) / 2.0
    qu, qv = F.stereo_rig_map(G.to_struct(F, flipped), 1, w, h)
    assert np.array_equal(R.remap_colour(right, qu, qv), right[::-1, ::-1]) and G.valid(qu, qv).all()
    # a quarter turn about the axis (no symmetric matrix): p_rect = R p, so the map reads R^T, and the rectified image
    # is the raw one turned the way R turns
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    turned = dict(G.RIG_I, R_right=turn.reshape(9))
    qu, qv = F.stereo_rig_map(G.to_struct(F, turned), 1, w, h)
    assert np.array_equal(R.remap_colour(right, qu, qv), np.rot90(right, -1)) and G.valid(qu, qv).all()
    for rig in (shifted, flipped, turned):
        for which in (0, 1):
            a = F.stereo_rig_map(G.to_struct(F, rig), which, w, h)
            b = G.rig_map(rig, which, w, h)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the conditions the rigs are there for, on the restatement alone ---------------------------------

def test_the_rigs_reach_what_they_are_there_for():
    """rig A: a barrel pair whose maps stay inside the raw images (no OUTSIDE at all); rig B: a quarter of either map
    leaves its image and a tenth of the pixels have OUTSIDE as their only flag; both: nearly every tap is fractional,
    most pixels match, and the box and the background come out at their disparities"""
    for name, outside_min, only_min in (("A", None, None), ("B", 0.15, 0.05)):
        w, h, st, rig, raw_l, raw_r, P = G.case(name)
        for which in (0, 1):
            qu, qv = G.rig_map(rig, which, w, h)
            outside = 1.0 - G.valid(qu, qv).mean()
            frac = (((qu & 31) != 0) | ((qv & 31) != 0)).mean()
            print(name, which, "outside %.3f fractional %.3f" % (outside, frac))
            assert frac > 0.95
            assert outside == 0.0 if outside_min is None else outside >= outside_min
        before, only = (P["flags_before"] == 0).mean(), (P["flags"] == G.OUTSIDE).mean()
        print(name, "unflagged before OUTSIDE %.3f, OUTSIDE alone %.3f" % (before, only))
        assert before >= 0.70
        assert only == 0.0 if only_min is None else only >= only_min
        assert not (P["flags"] & G.OUTSIDE).any() if only_min is None else True
        box, back, _ = S.regions(w, h)
        keep = P["flags"] == 0
        assert np.median(P["q"][box & keep]) == 240 and np.median(P["q"][back & keep]) == 96
        assert not P["disparity"][~keep].any() and not P["depth"][~keep].any()
        assert np.array_equal(P["depth"][keep], P["table"][P["q"][keep]]) and P["depth"][keep].all()


# ---- 5. the cases decide -----------------------------------------------------------------------

def test_mutants_change_a_plane_on_rig_b():
    w, h, st, rig, raw_l, raw_r, P = G.case("B")
    own = (G.rig_map(rig, 0, w, h), G.rig_map(rig, 1, w, h))
    mutants = {
        "R_k transposed": dict(maps=tuple(G.rig_map(rig, k, w, h, transposed=True) for k in (0, 1))),
        "the two maps swapped": dict(maps=own[::-1]),
        "OUTSIDE without its right-image half": dict(outside_right=False),
        "(u - cx) with the raw cx": dict(maps=tuple(G.rig_map(rig, k, w, h, raw_cx=True) for k in (0, 1))),
    }
    planes = ("rect_l", "rect_r", "valid", "flags", "disparity", "depth")
    for what, kw in mutants.items():
        Q = G.frame(rig, raw_l, raw_r, st, **kw)
        changed = [p for p in planes if not np.array_equal(Q[p], P[p])]
        print(what, "changes", changed)
        assert changed, what


# ---- 6. what is refused ------------------------------------------------------------------------

def test_check_and_helper_refusals(pkg):
    F = pkg.frontend
    w, h, _, calib = G.CALIBS["A"]
    rig = G.case("A")[3]
    good = G.to_struct(F, rig)
    assert F.check_stereo_rig(good) and F.check_stereo_rig(G.to_struct(F, G.RIG_I))
    assert F.lib().cvo_fe_check_stereo_rig(None) != 0
    nan, inf = float("nan"), float("inf")
    off = np.asarray(rig["R_left"], np.float64).copy()
    off[0] += 2e-3
    almost = np.asarray(rig["R_left"], np.float64).copy()
    almost[0] += 2e-4
    bad = [dict(rig, cx=nan), dict(rig, baseline=inf), dict(rig, left=rig["left"][:4] + ((0.0, nan, 0.0, 0.0, 0.0),)),
           dict(rig, R_right=np.full(9, nan)), dict(rig, fx=0.0), dict(rig, fy=-1.0), dict(rig, depth_scale=0.0),
           dict(rig, left=(0.0,) + rig["left"][1:]), dict(rig, right=rig["right"][:1] + (-3.0,) + rig["right"][2:]),
           dict(rig, baseline=0.0), dict(rig, baseline=-0.1), dict(rig, R_left=off),
           dict(rig, R_right=np.diag([1.0, 1.0, -1.0]).reshape(9)), dict(rig, R_left=np.zeros(9))]
    for r in bad:
        assert not F.check_stereo_rig(G.to_struct(F, r)), r
    assert F.check_stereo_rig(G.to_struct(F, dict(rig, R_left=almost)))
    q = np.zeros((h, w), np.int32)
    i32p = C.POINTER(C.c_int32)
    L = F.lib()
    for r in bad:
        assert L.cvo_fe_stereo_rig_map(C.byref(G.to_struct(F, r)), 0, w, h, q.ctypes.data_as(i32p), q.ctypes.data_as(i32p)) != 0
    for which, ww, hh in ((2, w, h), (-1, w, h), (0, 0, h), (0, w, 0)):
        assert L.cvo_fe_stereo_rig_map(C.byref(good), which, ww, hh, q.ctypes.data_as(i32p), q.ctypes.data_as(i32p)) != 0
    assert L.cvo_fe_stereo_rig_map(C.byref(good), 0, w, h, None, q.ctypes.data_as(i32p)) != 0
    # the helper
    assert F.stereo_rectify(G.calib_struct(F, calib), w, h, G.DEPTH_SCALE) is not None
    refused = {
        "an angle of 0.6 rad": dict(calib, R=G.f32(G.exp_so3((0.0, 0.6, 0.0))).reshape(9)),
        "T pointing the wrong way": dict(calib, T=G.f32((0.11, 0.0, 0.0))),
        "a vertical rig": dict(calib, T=G.f32((-0.01, -0.11, 0.0))),
        "a rig along the axis": dict(calib, T=G.f32((-0.01, 0.0, -0.11))),
        "no baseline": dict(calib, T=G.f32((0.0, 0.0, 0.0))),
        "a member that is not a number": dict(calib, T=G.f32((nan, 0.0, 0.0))),
        "no focal length": dict(calib, left=(70.0, 0.0) + calib["left"][2:]),
        "R a reflection": dict(calib, R=np.diag([1.0, 1.0, -1.0]).reshape(9)),
    }
    for what, c in refused.items():
        assert G.rectify(c, w, h, G.DEPTH_SCALE) is None or what in ("a member that is not a number", "no focal length",
                                                                    "R a reflection"), what
        with pytest.raises(pkg.capi.CvoHipError):
            F.stereo_rectify(G.calib_struct(F, c), w, h, G.DEPTH_SCALE)
    for args in ((0, h, G.DEPTH_SCALE), (w, 0, G.DEPTH_SCALE), (w, h, 0.0), (w, h, nan)):
        with pytest.raises(pkg.capi.CvoHipError):
            F.stereo_rectify(G.calib_struct(F, calib), *args)
    # an angle just inside the limit is welcome
    assert F.check_stereo_rig(F.stereo_rectify(G.calib_struct(F, dict(calib, R=G.f32(G.exp_so3((0.0, 0.49, 0.0))).reshape(9))),
                                               w, h, G.DEPTH_SCALE))


# ---- the structures against their ctypes mirrors -----------------------------------------------------

def test_structs_mirror_the_header(pkg):
    F = pkg.frontend
    text = open(os.path.join(ROOT, "include", "cvo_frontend.h")).read()

    def members(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for ctype, names in re.findall(r"\b(float|cvo_fe_lens)\s+([^;]+);", body):
            for n in names.split(","):
                m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
                out.append((m.group(1), ctype, int(m.group(2) or 1)))
        return out

    def mirror(cls):
        out = []
        for n, t in cls._fields_:
            if t is F.Lens:
                out.append((n, "cvo_fe_lens", 1))
            elif t is C.c_float:
                out.append((n, "float", 1))
            else:
                assert t._type_ is C.c_float
                out.append((n, "float", t._length_))
        return out

    for struct, cls, size in (("cvo_fe_lens", F.Lens, 36), ("cvo_fe_stereo_calib", F.StereoCalib, 120),
                              ("cvo_fe_stereo_rig", F.StereoRig, 168)):
        assert members(struct) == mirror(cls), struct
        assert C.sizeof(cls) == size
    rig = G.to_struct(F, G.case("A")[3])
    assert eval(repr(rig), {"StereoRig": F.StereoRig}) == rig and rig != G.to_struct(F, G.RIG_I)
    assert (F.STAGE_RIGHT_BGR, F.STAGE_STEREO_VALID, F.STEREO_OUTSIDE) == (21, 22, G.OUTSIDE)
    for pat in (r"CVO_FE_STAGE_RIGHT_BGR = 21\b", r"CVO_FE_STAGE_STEREO_VALID = 22\b", r"CVO_FE_STEREO_OUTSIDE = 16\b"):
        assert re.search(pat, text), pat
    for name in ("cvo_fe_set_stereo_rig", "cvo_fe_get_stereo_rig", "cvo_fe_check_stereo_rig", "cvo_fe_stereo_rectify",
                 "cvo_fe_stereo_rig_map"):
        assert name in F.SYMBOLS
