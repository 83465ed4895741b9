"""ctypes binding of oracle/liboracle_fe.so -- the CPU restatement of the RGB-D
front end (oracle/frontend_oracle.c).

TEST INFRASTRUCTURE ONLY: importable from tests/ and __graft_entry__.smoke() --
never from the product package.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE, "liboracle_fe.so"])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "liboracle_fe.so")
        if not os.path.exists(path):
            build()
        _LIB = C.CDLL(path)
        _LIB.fe_create_pointcloud.restype = C.c_int
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def random_pattern(n):
    """srand(3141592); rand() & 0xFF -- the C library's own generator."""
    out = np.empty(n, np.uint8)
    lib().fe_random_pattern(C.c_int(n), _p(out, C.c_uint8))
    return out


def gray(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.empty((h, w), np.uint8)
    lib().fe_gray(_p(img, C.c_uint8), C.c_int(w), C.c_int(h), _p(out, C.c_uint8))
    return out


def hsv(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.empty((h, w, 3), np.uint8)
    lib().fe_hsv(_p(img, C.c_uint8), C.c_int(w), C.c_int(h), _p(out, C.c_uint8))
    return out


def pyramid(gray_img):
    """-> (I[3], dx0, dy0, ag[3])"""
    g = np.ascontiguousarray(gray_img, np.uint8)
    h, w = g.shape
    I = [np.zeros((h >> l, w >> l), np.float32) for l in range(3)]
    ag = [np.zeros((h >> l, w >> l), np.float32) for l in range(3)]
    dx0 = np.zeros((h, w), np.float32)
    dy0 = np.zeros((h, w), np.float32)
    FP = C.POINTER(C.c_float)
    Iarr = (FP * 3)(*[_p(a, C.c_float) for a in I])
    Aarr = (FP * 3)(*[_p(a, C.c_float) for a in ag])
    lib().fe_pyramid(_p(g, C.c_uint8), C.c_int(w), C.c_int(h), Iarr, _p(dx0, C.c_float), _p(dy0, C.c_float), Aarr)
    return I, dx0, dy0, ag


def thresholds(ag0):
    a = np.ascontiguousarray(ag0, np.float32)
    h, w = a.shape
    out = np.zeros((h // 32, w // 32), np.float32)
    lib().fe_thresholds(_p(a, C.c_float), C.c_int(w), C.c_int(h), _p(out, C.c_float))
    return out


def cell_thresholds(ag0):
    """-> (ths, thsSmoothed): the cells' median + 7 and their squared 3x3 mean"""
    a = np.ascontiguousarray(ag0, np.float32)
    h, w = a.shape
    raw = np.zeros((h // 32, w // 32), np.float32)
    out = np.zeros((h // 32, w // 32), np.float32)
    lib().fe_cell_thresholds(_p(a, C.c_float), C.c_int(w), C.c_int(h), _p(raw, C.c_float), _p(out, C.c_float))
    return raw, out


def _planes(ag0, ag1, ag2):
    a0, a1, a2 = (np.ascontiguousarray(a, np.float32) for a in (ag0, ag1, ag2))
    h, w = a0.shape
    if a1.shape != (h // 2, w // 2) or a2.shape != (h // 4, w // 4):
        raise ValueError("the planes of a %dx%d frame are %dx%d, %dx%d and %dx%d" % (w, h, w, h, w // 2, h // 2, w // 4, h // 4))
    return a0, a1, a2, w, h


def make_maps(ag0, ag1, ag2, num_want):
    """fe_thresholds + fe_make_maps on caller-given squared-gradient planes (what the reference's selector
    is given by ref_make_maps) -> dict(map, count, pot_used, reselected, ths, ths_smoothed)"""
    a0, a1, a2, w, h = _planes(ag0, ag1, ag2)
    raw, ths = cell_thresholds(a0)
    pattern = random_pattern(w * h)
    mp = np.zeros((h, w), np.float32)
    pot, nh = C.c_int(0), C.c_int(0)
    lib().fe_make_maps.restype = C.c_int
    n = lib().fe_make_maps(_p(a0, C.c_float), _p(a1, C.c_float), _p(a2, C.c_float), _p(ths, C.c_float),
                           _p(pattern, C.c_uint8), C.c_int(w), C.c_int(h), C.c_float(float(num_want)), _p(mp, C.c_float),
                           C.byref(pot), C.byref(nh))
    # a re-selection always moves the potential away from the 3 every frame starts at
    return {"map": mp, "count": n, "pot_used": pot.value, "reselected": int(pot.value != 3), "ths": raw,
            "ths_smoothed": ths, "num_have": nh.value}


_REF_SEL = False


def ref_selector_lib():
    """oracle/_ref/libselector_ref.so (the reference's own PixelSelector2.cpp, `make -C oracle ref`), or None when it
    is not built."""
    global _REF_SEL
    if _REF_SEL is False:
        path = os.path.join(_HERE, "_ref", "libselector_ref.so")
        _REF_SEL = C.CDLL(path) if os.path.exists(path) else None
        if _REF_SEL is not None:
            _REF_SEL.ref_selector_make_maps.restype = C.c_int
    return _REF_SEL


def ref_make_maps(ag0, ag1, ag2, num_want, define_unwritten):
    """The reference's makeMaps on a fresh selector (potential 3) -> dict(map, count, pot_used, reselected, ths,
    ths_smoothed, pot_after).  `define_unwritten`: the threshold cells the reference reads behind the last one it wrote
    take the last cell's value first (ref_selector_harness.cpp); without it that read is indeterminate wherever
    w % 32 > 5 or h % 32 > 3."""
    L = ref_selector_lib()
    if L is None:
        raise RuntimeError("oracle/_ref/libselector_ref.so is not built (make -C oracle ref)")
    a0, a1, a2, w, h = _planes(ag0, ag1, ag2)
    mp = np.zeros((h, w), np.float32)
    raw = np.zeros((h // 32, w // 32), np.float32)
    ths = np.zeros((h // 32, w // 32), np.float32)
    pots = np.zeros(2, np.int32)
    npass, after = C.c_int(0), C.c_int(0)
    n = L.ref_selector_make_maps(C.c_int(w), C.c_int(h), _p(a0, C.c_float), _p(a1, C.c_float), _p(a2, C.c_float),
                                 C.c_float(float(num_want)), C.c_int(1 if define_unwritten else 0), _p(mp, C.c_float),
                                 _p(raw, C.c_float), _p(ths, C.c_float), _p(pots, C.c_int32), C.byref(npass),
                                 C.byref(after))
    assert npass.value in (1, 2) and pots[0] == 3
    res = {"map": mp, "count": n, "pot_used": int(pots[npass.value - 1]), "reselected": npass.value - 1, "ths": raw,
           "ths_smoothed": ths, "pot_after": after.value}
    # what the final pass kept before the sub-sampling: that pass again, by the reference's own select()
    res["num_have"] = sum(ref_select(a0, a1, a2, res["pot_used"], define_unwritten)[1])
    return res


def ref_select(ag0, ag1, ag2, pot, define_unwritten):
    """One pass of the reference's select() at potential `pot`, nothing sub-sampled -> (map, [n2, n3, n4])"""
    L = ref_selector_lib()
    if L is None:
        raise RuntimeError("oracle/_ref/libselector_ref.so is not built (make -C oracle ref)")
    a0, a1, a2, w, h = _planes(ag0, ag1, ag2)
    mp = np.zeros((h, w), np.float32)
    n = np.zeros(3, np.int32)
    L.ref_selector_select(C.c_int(w), C.c_int(h), _p(a0, C.c_float), _p(a1, C.c_float), _p(a2, C.c_float),
                          C.c_int(int(pot)), C.c_int(1 if define_unwritten else 0), _p(mp, C.c_float), _p(n, C.c_int32))
    return mp, n.tolist()


def blur3(g):
    g = np.ascontiguousarray(g, np.uint8)
    h, w = g.shape
    out = np.empty((h, w), np.uint8)
    lib().fe_blur3(_p(g, C.c_uint8), C.c_int(w), C.c_int(h), _p(out, C.c_uint8))
    return out


def canny(g, low=0, high=25):
    g = np.ascontiguousarray(g, np.uint8)
    h, w = g.shape
    out = np.empty((h, w), np.uint8)
    lib().fe_canny(_p(g, C.c_uint8), C.c_int(w), C.c_int(h), C.c_int(low), C.c_int(high), _p(out, C.c_uint8))
    return out


def camera(dataset_seq):
    cam = np.zeros(5, np.float32)
    lib().fe_camera(C.c_int(dataset_seq), _p(cam, C.c_float))
    return cam


def create_pointcloud(img, depth, dataset_seq=1, feature_type=1, num_want=3000):
    """-> dict(positions, features, map, num_selected)"""
    img = np.ascontiguousarray(img, np.uint8)
    depth = np.ascontiguousarray(depth, np.uint16)
    h, w = depth.shape
    cap = w * h
    pos = np.zeros((cap, 3), np.float32)
    feat = np.zeros((cap, 5), np.float32)
    mp = np.zeros((h, w), np.float32)
    nsel = C.c_int(0)
    n = lib().fe_create_pointcloud(_p(img, C.c_uint8), _p(depth, C.c_uint16), C.c_int(w), C.c_int(h),
                                   C.c_int(dataset_seq), C.c_int(feature_type), C.c_int(num_want),
                                   _p(pos, C.c_float), _p(feat, C.c_float), C.c_int(cap), _p(mp, C.c_float),
                                   C.byref(nsel))
    return {"positions": pos[:n].copy(), "features": feat[:n].copy(), "map": mp, "num_selected": nsel.value}
