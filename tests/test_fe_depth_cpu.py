"""CPU: the registration contract of include/cvo_frontend.h (at cvo_fe_depth_camera).  The
library's host-only cvo_fe_depth_rays against the numpy restatement (tests/fe_depth_ref.py)
by bytes, the refusals that need no context, the restatement itself against answers written
by hand, and the conditions the shared rigs are there for.  The contract is the library's
own definition (the footprint idea of the common SDKs' depth-to-colour alignment): PARITY
UNPINNED against any of them."""
import ctypes as C

import numpy as np
import pytest

import fe_depth_ref as D
import fe_rectify_ref as R

FR1_RIG = D.make_rig(640, 480, R.FR1[:5], R.FR1[5])
RAY_RIGS = [("K", D.RIGS["K"][3]), ("U", D.RIGS["U"][3]), ("W", D.RIGS["W"][3]), ("fr1", FR1_RIG),
            ("D", D.RIGS["D"][3])]


@pytest.mark.parametrize("name,rig", RAY_RIGS, ids=[r[0] for r in RAY_RIGS])
def test_library_rays_equal_the_restatement_by_bytes(pkg, name, rig):
    F = pkg.frontend
    xn, yn = F.depth_rays(D.to_struct(F, rig))
    rx, ry = D.rays(rig)
    assert xn.dtype == np.float32 and xn.shape == (rig["height"] + 1, rig["width"] + 1)
    assert xn.tobytes() == rx.tobytes() and yn.tobytes() == ry.tobytes()   # (NaNs included)
    if name == "W":
        assert np.isnan(rx).any()
    elif name != "D":
        assert not np.isnan(rx).any() and not np.array_equal(rx, D.rays(dict(rig, dist=D.ZERO))[0])


def test_the_fixed_point_converges_for_the_lenses_in_use():
    """twenty iterations: the forward distortion of the ray lands below 3e-5 px from its corner"""
    for rig in (FR1_RIG, D.RIGS["K"][3], D.RIGS["U"][3], D.VGA_RIG):
        xn, yn = D.rays(rig)
        f = [np.float64(np.float32(rig[k])) for k in ("fx", "fy", "cx", "cy")]
        us, vs = D._forward(xn.astype(np.float64), yn.astype(np.float64), *f,
                            np.array(rig["dist"], np.float32).astype(np.float64))
        j, i = np.mgrid[0:rig["height"] + 1, 0:rig["width"] + 1]
        # (the table is rounded to float32: 6e-8 relative, of up to 640 px)
        assert np.abs(us - (i - 0.5)).max() < 3e-5 + 640 * 2e-7 and np.abs(vs - (j - 0.5)).max() < 3e-5 + 640 * 2e-7


def test_host_entry_refuses_what_set_depth_camera_refuses(pkg):
    F = pkg.frontend
    L = F.lib()
    good = D.to_struct(F, D.RIGS["K"][3])
    n = 65 * 97
    xn, yn = np.zeros(n, np.float32), np.zeros(n, np.float32)
    fp = C.POINTER(C.c_float)
    px, py = xn.ctypes.data_as(fp), yn.ctypes.data_as(fp)
    assert L.cvo_fe_depth_rays(C.byref(good), px, py) == 0
    for args in ((None, px, py), (C.byref(good), None, py), (C.byref(good), px, None)):
        assert L.cvo_fe_depth_rays(*args) != 0
    for rig in D.bad_rigs():
        before = xn.copy()
        with pytest.raises(pkg.capi.CvoHipError):
            F.depth_rays(D.to_struct(F, rig))
        assert L.cvo_fe_depth_rays(C.byref(D.to_struct(F, rig)), px, py) != 0
        assert not F.check_depth_camera(D.to_struct(F, rig))
        assert np.array_equal(xn, before)
    # at the edge of what is accepted: 8 x 8, 8192 wide, R within 1e-3, max_range just above min_range
    for rig in (dict(good_rig(), width=8, height=8), dict(good_rig(), width=8192, height=8),
                dict(good_rig(), R=(1.0004,) + D.EYE[1:]), dict(good_rig(), min_range=0.5, max_range=0.5001),
                dict(good_rig(), min_range=3.0, max_range=0.0), dict(good_rig(), min_range=-1.0, max_range=-2.0)):
        assert F.check_depth_camera(D.to_struct(F, rig))
        F.depth_rays(D.to_struct(F, rig))
    assert L.cvo_fe_check_depth_camera(None) != 0 and F.check_depth_camera(good)
    # set / get without a context
    assert L.cvo_fe_set_depth_camera(None, C.byref(good)) != 0 and L.cvo_fe_set_depth_camera(None, None) != 0
    assert L.cvo_fe_get_depth_camera(None, C.byref(good), None) != 0


def good_rig():
    return dict(D.RIGS["K"][3])


def test_depth_camera_structure(pkg):
    F = pkg.frontend
    rig = D.to_struct(F, D.RIGS["U"][3])
    assert C.sizeof(F.DepthCamera) == 8 + 24 * 4
    assert (rig.width, rig.height) == (72, 112) and rig == D.to_struct(F, D.RIGS["U"][3])
    assert rig != D.to_struct(F, D.RIGS["K"][3])
    assert np.allclose(np.array(rig.R).reshape(3, 3) @ np.array(rig.R).reshape(3, 3).T, np.eye(3), atol=1e-6)
    assert F.STAGE_RAW_DEPTH == 12
    assert eval(repr(rig), {"DepthCamera": F.DepthCamera}) == rig


# ---- the restatement against answers written by hand ---------------------------------------

CAM = (1000.0, 128.0, 128.0, 50.0, 40.0)   # (powers of two: the hand-written answers are exact)


@pytest.mark.parametrize("name", ["I96x64", "I127x193", "vga"])
def test_identity_rig_returns_its_input(pkg, name):
    if name == "vga":
        w, h, cam = 640, 480, D.VGA_COLOUR
        rig = D.identity_rig(w, h, cam)
    else:
        w, h, cam, rig = D.RIGS[name]
    dep = D.scene(pkg.data, rig)
    assert (dep == 0).any() and (dep == 3000).any()
    assert np.array_equal(D.register(rig, cam, w, h, dep), dep)
    assert (D.footprint_sizes(rig, cam, w, h, dep) == 1).all()


def test_one_pixel_footprint_by_hand():
    """A depth camera of half the focal length: depth pixel (u, v) covers the colour pixels whose centres
    lie in [2(u - .5 - 10) + 50, 2(u + .5 - 10) + 50) = [2u + 29, 2u + 31): two per axis.
    Pixel (12, 9): x 53, 54 and y in [2(9 - .5 - 7.5) + 40, +2) = 42, 43."""
    rig = D.make_rig(32, 24, (1000.0, 64.0, 64.0, 10.0, 7.5))
    dep = np.zeros((24, 32), np.uint16)
    dep[9, 12] = 1500
    out = D.register(rig, CAM, 96, 64, dep)
    want = np.zeros((64, 96), np.uint16)
    want[42:44, 53:55] = 1500
    assert np.array_equal(out, want)
    # ... and from 10 cm to the side, 1.5 m away: 128 * 0.1 / 1.5 = 8.53 px to the left: [44.47, 46.47)
    out = D.register(dict(rig, T=(-0.1, 0.0, 0.0)), CAM, 96, 64, dep)
    want = np.zeros((64, 96), np.uint16)
    want[42:44, 45:47] = 1500
    assert np.array_equal(out, want)
    # a colour camera counting 5000 units per metre sees 1.5 m as 7500
    out = D.register(rig, (5000.0,) + CAM[1:], 96, 64, dep)
    assert out[42, 53] == 7500 and np.count_nonzero(out) == 4


def test_the_nearer_of_two_surfaces_wins():
    """T = (-0.125, 0, 0): a point at 1 m moves 16 px to the left, one at 2 m 8 px: depth pixels 36 (1 m)
    and 28 (2 m) of a row both land on colour pixel 20"""
    rig = D.make_rig(96, 64, CAM, T=(-0.125, 0.0, 0.0))
    dep = np.zeros((64, 96), np.uint16)
    dep[20, 36] = 1000
    dep[20, 28] = 2000
    out = D.register(rig, CAM, 96, 64, dep)
    assert out[20, 20] == 1000 and np.count_nonzero(out) == 1
    assert D.register(rig, CAM, 96, 64, dep, farthest=True)[20, 20] == 2000
    dep[20, 36] = 0
    assert D.register(rig, CAM, 96, 64, dep)[20, 20] == 2000


def test_a_rig_looking_backwards_writes_nothing(pkg):
    w, h, cam, rig = D.RIGS["I"]
    dep = D.scene(pkg.data, rig)
    back = dict(rig, R=tuple(D.rot_y(np.pi).reshape(-1)))
    assert not D.register(back, cam, w, h, dep).any()


def test_ranges_drop_exactly_the_pixels_outside(pkg):
    w, h, cam, rig = D.RIGS["I"]
    dep = D.scene(pkg.data, rig)            # 5000 per metre: the box at 0.6 m, the wall from 1.2 m
    f = np.float32
    z = dep.astype(f) / f(5000.0)
    for lo, hi in ((0.7, 0.0), (0.0, 1.5), (0.7, 1.5), (0.6, 0.0), (0.0, 0.6), (-1.0, -1.0)):
        keep = dep != 0
        if lo > 0:
            keep &= ~(z < f(lo))
        if hi > 0:
            keep &= ~(z > f(hi))
        out = D.register(dict(rig, min_range=lo, max_range=hi), cam, w, h, dep)
        assert np.array_equal(out, np.where(keep, dep, 0))
    assert (z[dep != 0] < 0.7).any() and (z > 1.5).any()
    # the limits themselves are inside: z < min_range drops, z == min_range stays
    assert (D.register(dict(rig, min_range=0.6), cam, w, h, dep) == 3000).any()
    assert set(np.unique(D.register(dict(rig, max_range=0.6), cam, w, h, dep))) == {0, 3000}


def test_a_depth_beyond_uint16_writes_nothing():
    """20 m in a depth image of 1000 units per metre is 100000 units of 1/5000 m"""
    rig = D.make_rig(96, 64, CAM)
    dep = np.zeros((64, 96), np.uint16)
    dep[10, 10] = 20000
    dep[10, 12] = 13107          # 13.107 m: 65535 units, the last that fits
    dep[10, 14] = 13108
    out = D.register(rig, (5000.0,) + CAM[1:], 96, 64, dep)
    assert out[10, 12] == 65535 and np.count_nonzero(out) == 1


# ---- the rigs reach the branches they are for ------------------------------------------------

def _registered(pkg, name, **kw):
    w, h, cam, rig = D.RIGS[name]
    dep = D.scene(pkg.data, rig)
    return D.register(rig, cam, w, h, dep, **kw)


@pytest.mark.parametrize("name", ["K", "U", "D"])
def test_the_z_test_decides(pkg, name):
    near = _registered(pkg, name).astype(np.int64)
    far = _registered(pkg, name, farthest=True).astype(np.int64)
    n = np.count_nonzero(far - near > 500)
    print(name, "pixels where nearest and farthest differ by more than 500 units:", n)
    assert n >= 20 and (far >= near).all()


def test_the_cap_decides_for_c(pkg):
    n = np.count_nonzero(_registered(pkg, "C") != _registered(pkg, "C", cap=None))
    print("C: pixels the 8 x 8 cap changes:", n)
    assert n >= 1000


def test_more_than_half_of_w_is_invalid():
    xn, yn = D.rays(D.RIGS["W"][3])
    print("W: invalid rays", np.isnan(xn).mean())
    assert np.isnan(xn).mean() > 0.5 and np.array_equal(np.isnan(xn), np.isnan(yn))
    assert not np.isnan(xn).all()


def test_u_has_footprints_of_one_two_and_four(pkg):
    w, h, cam, rig = D.RIGS["U"]
    sizes = set(np.unique(D.footprint_sizes(rig, cam, w, h, D.scene(pkg.data, rig))))
    print("U: footprint sizes", sorted(sizes))
    assert {1, 2, 4} <= sizes


def test_k_has_empty_footprints(pkg):
    w, h, cam, rig = D.RIGS["K"]
    dep = D.scene(pkg.data, rig)
    live, _, x0, x1, y0, y1 = D.footprints(rig, cam, w, h, dep)
    empty = ~live | (x1 <= x0) | (y1 <= y0)
    print("K: depth pixels with an empty footprint", empty.mean())
    assert empty.mean() >= 0.15
