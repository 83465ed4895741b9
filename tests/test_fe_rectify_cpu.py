"""CPU: the rectification contract of include/cvo_frontend.h.  The library's host-only
cvo_fe_rectify_map against the numpy restatement (tests/fe_rectify_ref.py) by bytes, and the
restatement itself against answers written by hand.  The contract is the library's own
definition (cv::undistort's convention, a fixed-point tap in cv::remap's style): PARITY
UNPINNED against OpenCV, which is not available here."""
import ctypes as C

import numpy as np
import pytest

import fe_rectify_ref as R

MODELS = [(name,) + R.SMALL[name] for name in ("A", "B", "C")] + [("fr1", 640, 480, R.FR1), ("fr2", 640, 480, R.FR2)]


@pytest.mark.parametrize("name,w,h,model", MODELS, ids=[m[0] for m in MODELS])
def test_library_map_equals_the_restatement_by_bytes(pkg, name, w, h, model):
    F = pkg.frontend
    qu, qv = F.rectify_map(F.CameraModel(*model), w, h)
    ru, rv = R.rectify_map(model, w, h)
    assert qu.dtype == np.int32 and qu.shape == (h, w)
    assert qu.tobytes() == ru.tobytes() and qv.tobytes() == rv.tobytes()


def test_the_published_tum_rows(pkg):
    F = pkg.frontend
    assert F.TUM_CAMERAS["fr1"] == F.CameraModel(*R.FR1) and F.TUM_CAMERAS["fr2"] == F.CameraModel(*R.FR2)
    fr3 = F.TUM_CAMERAS["fr3"]
    assert fr3.astuple() == F.CameraModel(5000.0, 535.4, 539.2, 320.1, 247.6).astuple() and not any(fr3.dist)
    for k, name in ((1, "fr1"), (2, "fr2"), (3, "fr3")):   # the table's rows are these without the lens
        row = F.camera(k)
        assert list(row.values()) == list(F.TUM_CAMERAS[name].astuple()[:5])


def test_small_models_reach_the_border_branches():
    """A and B leave the image (outside depth samples, clamped colour taps); C never does;
    nearly every entry of each has a fraction, so the bilinear weights are exercised."""
    for name in ("A", "B", "C"):
        w, h, model = R.SMALL[name]
        outside, clamped, frac, shift = R.map_statistics(model, w, h)
        print(name, outside, clamped, frac, shift)
        if name == "C":
            assert outside == 0.0 and clamped == 0.0
        else:
            assert outside >= 0.01 and clamped >= 0.01
        assert frac >= 0.90
    # the figures the map was introduced with: fr1 moves a VGA pixel by 5.0 px on average, 24.7 px at most
    qu, qv = R.rectify_map(R.FR1, 640, 480)
    v, u = np.mgrid[0:480, 0:640]
    d = np.hypot(qu / 32.0 - u, qv / 32.0 - v)
    assert abs(d.mean() - 5.0) < 0.1 and abs(d.max() - 24.7) < 0.1


def test_zero_distortion_is_the_identity_map():
    for model in ((1000.0, 400.25, 399.5, 300.75, 250.125, (0, 0, 0, 0, 0)), R.FR1[:5] + ((0, 0, 0, 0, 0),)):
        qu, qv = R.rectify_map(model, 333, 251)
        v, u = np.mgrid[0:251, 0:333]
        assert np.array_equal(qu, 32 * u) and np.array_equal(qv, 32 * v)


def test_radial_only_keeps_the_row_of_the_centre():
    """p1 = p2 = 0 and an integer cy: on row v = cy, y = 0, so yd = 0 and vs = cy exactly."""
    model = (5000.0, 77.6, 77.5, 47.8, 38.0, (0.35, 0.1, 0.0, 0.0, -0.05))
    qu, qv = R.rectify_map(model, 96, 64)
    assert (qv[38] == 32 * 38).all()
    assert (qu[38] != 32 * np.arange(96)).any()      # ... while the row does move along itself


def test_centred_radial_map_is_point_symmetric():
    """cx, cy at the image centre and p1 = p2 = 0: pixel (u, v) and its mirror (w-1-u, h-1-v) have
    opposite (x, y), the same r2, so us - cx and vs - cy change sign exactly (rint is odd; the
    centre is a multiple of 1/2, so 32 * c is an integer and adds exactly)."""
    w, h = 97, 65
    model = (5000.0, 80.0, 79.0, (w - 1) / 2.0, (h - 1) / 2.0, (-0.25, 0.07, 0.0, 0.0, 0.01))
    qu, qv = R.rectify_map(model, w, h)
    assert np.array_equal(qu + qu[::-1, ::-1], np.full((h, w), 32 * (w - 1)))
    assert np.array_equal(qv + qv[::-1, ::-1], np.full((h, w), 32 * (h - 1)))
    assert qu[h // 2, w // 2] == 32 * (w // 2) and qv[h // 2, w // 2] == 32 * (h // 2)


def test_half_pixel_shift_of_one_bright_pixel():
    """A map that looks half a pixel right and down of every pixel: ax = ay = 16, four weights of
    256.  One pixel of 200 on black: (200 * 256 + 512) >> 10 = 50 at the four outputs that tap it."""
    h, w = 8, 9
    img = np.zeros((h, w, 3), np.uint8)
    img[4, 5] = (200, 100, 7)
    v, u = np.mgrid[0:h, 0:w]
    qu, qv = (32 * u + 16).astype(np.int32), (32 * v + 16).astype(np.int32)
    out = R.remap_colour(img, qu, qv)
    want = np.zeros_like(img)
    for (y, x) in ((3, 4), (3, 5), (4, 4), (4, 5)):
        want[y, x] = ((200 * 256 + 512) >> 10, (100 * 256 + 512) >> 10, (7 * 256 + 512) >> 10)
    assert want[3, 4].tolist() == [50, 25, 2]
    assert np.array_equal(out, want)
    # unequal weights: a quarter of a pixel to the right only: 24/32 and 8/32 of the row
    out = R.remap_colour(img, (32 * u + 8).astype(np.int32), (32 * v).astype(np.int32))
    assert out[4, 5, 0] == (200 * 24 * 32 + 512) >> 10 == 150 and out[4, 4, 0] == (200 * 8 * 32 + 512) >> 10 == 50
    # depth: the nearest sample; a fraction of exactly one half goes to the next pixel ((q + 16) >> 5)
    dep = np.arange(h * w, dtype=np.uint16).reshape(h, w) + 1
    d = R.remap_depth(dep, qu, qv)
    assert np.array_equal(d[:-1, :-1], dep[1:, 1:]) and not d[-1].any() and not d[:, -1].any()
    d = R.remap_depth(dep, (32 * u + 15).astype(np.int32), (32 * v - 16).astype(np.int32))
    assert np.array_equal(d, dep)
    dep[2, 3] = 0                                       # a zero stays a zero
    assert R.remap_depth(dep, (32 * u).astype(np.int32), (32 * v).astype(np.int32))[2, 3] == 0


def test_replicated_border_and_depth_outside():
    """Taps beyond the image repeat the border pixel (no black frame); depth outside is 0."""
    h, w = 6, 7
    rng = np.random.default_rng(3)
    img = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    dep = rng.integers(1, 60000, (h, w)).astype(np.uint16)
    v, u = np.mgrid[0:h, 0:w]
    qu, qv = (32 * u - 32).astype(np.int32), (32 * v + 32).astype(np.int32)    # one pixel left, one down
    out = R.remap_colour(img, qu, qv)
    assert np.array_equal(out[:-1, 1:], img[1:, :-1])
    assert np.array_equal(out[:-1, 0], img[1:, 0]) and np.array_equal(out[-1, 1:], img[-1, :-1])
    d = R.remap_depth(dep, qu, qv)
    assert np.array_equal(d[:-1, 1:], dep[1:, :-1]) and not d[:, 0].any() and not d[-1].any()


def test_coordinates_beyond_the_clamp_saturate():
    """A violent lens throws the corners far out: the map saturates at -32 and 32 w (32 h)."""
    w, h = 96, 64
    model = (5000.0, 30.0, 30.0, 47.5, 31.5, (4.0, 0.0, 0.0, 0.0, 0.0))
    qu, qv = R.rectify_map(model, w, h)
    assert qu.min() == -32 and qu.max() == 32 * w and qv.min() == -32 and qv.max() == 32 * h
    assert qu[0, 0] == -32 and qv[0, 0] == -32 and qu[-1, -1] == 32 * w and qv[-1, -1] == 32 * h
    us, vs = R.source_coordinates(model, w, h)
    assert us.min() < -500 and us.max() > 500           # (x = -47.5/30, r2 = 3.6: about -700 at the corner)
    # ... and such entries give the border colour and no depth
    img = np.full((h, w, 3), 9, np.uint8); img[0, 0] = 77
    dep = np.full((h, w), 5, np.uint16)
    assert R.remap_colour(img, qu, qv)[0, 0, 0] == 77 and R.remap_depth(dep, qu, qv)[0, 0] == 0


def test_argument_checks_of_the_host_entry(pkg):
    F = pkg.frontend
    L = F.lib()
    i32p = C.POINTER(C.c_int32)
    qu = np.zeros((4, 4), np.int32); qv = np.zeros((4, 4), np.int32)
    pu, pv = qu.ctypes.data_as(i32p), qv.ctypes.data_as(i32p)
    good = F.CameraModel(*R.FR1)
    assert L.cvo_fe_rectify_map(C.byref(good), 4, 4, pu, pv) == 0
    assert L.cvo_fe_rectify_map(None, 4, 4, pu, pv) == -1
    assert L.cvo_fe_rectify_map(C.byref(good), 4, 4, None, pv) == -1
    assert L.cvo_fe_rectify_map(C.byref(good), 4, 4, pu, None) == -1
    assert L.cvo_fe_rectify_map(C.byref(good), 0, 4, pu, pv) == -1
    assert L.cvo_fe_rectify_map(C.byref(good), 4, -3, pu, pv) == -1
    for field, value in (("fx", 0.0), ("fy", -1.0), ("depth_scale", 0.0), ("cx", float("nan")), ("fx", float("inf"))):
        bad = F.CameraModel(*R.FR1)
        setattr(bad, field, value)
        assert L.cvo_fe_rectify_map(C.byref(bad), 4, 4, pu, pv) == -1, field
    bad = F.CameraModel(*R.FR1)
    bad.dist[4] = float("nan")
    assert L.cvo_fe_rectify_map(C.byref(bad), 4, 4, pu, pv) == -1
    with pytest.raises(pkg.capi.CvoHipError):
        F.rectify_map(bad, 4, 4)
