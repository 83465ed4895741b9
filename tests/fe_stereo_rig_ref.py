"""A numpy restatement of the front end's rig contract (include/cvo_frontend.h, at cvo_fe_stereo_rig): the helper
that makes a rig from a calibration, the two maps, validity and the OUTSIDE flag, and a frame under a rig, plane by
plane.  float64 on float32 members widened exactly (numpy never contracts into an FMA); the order of operations
below is the contract.  The colour taps are fe_rectify_ref.remap_colour and the matcher is fe_stereo_ref.match.

A lens here is (fx, fy, cx, cy, (k1, k2, p1, p2, k3)); a calibration and a rig are dicts with the members of
cvo_fe_stereo_calib and cvo_fe_stereo_rig.  Also here: the rigs the tests share, and a renderer that warps a
rectified synthetic pair into the raw images a rig's cameras would deliver."""
import numpy as np

import fe_rectify_ref as R
import fe_stereo_ref as S

OUTSIDE = 16
SEED = 81
DEPTH_SCALE = 2000.0
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def f32(v):
    """the float32 the library's structs hold, widened exactly"""
    return np.asarray(v, np.float32).astype(np.float64)


def _lens32(lens):
    fx, fy, cx, cy, dist = lens
    v = f32([fx, fy, cx, cy] + list(dist))
    return (float(v[0]), float(v[1]), float(v[2]), float(v[3]), tuple(float(d) for d in v[4:]))


def exp_so3(om):
    """Rodrigues' formula, float64: the rotation of the axis-angle vector `om`"""
    om = np.asarray(om, np.float64)
    a = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    if a == 0.0:
        return np.eye(3)
    return _rodrigues(om / a, a)


def _rodrigues(k, a):
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    KK = np.array([[(K[i, 0] * K[0, j] + K[i, 1] * K[1, j]) + K[i, 2] * K[2, j] for j in range(3)] for i in range(3)])
    return (np.eye(3) + np.sin(a) * K) + (1.0 - np.cos(a)) * KK


def _mat(A, B):
    return np.array([[(A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)])


def make_calib(left, right, om, T):
    """a calibration as the struct holds it: every member a float32"""
    return dict(left=_lens32(left), right=_lens32(right), R=f32(exp_so3(om)).reshape(9), T=f32(T))


# ---- the helper --------------------------------------------------------------------------------

def rectify(calib, w, h, depth_scale):
    """cvo_fe_stereo_rectify: the rig of a calibration, or None where the helper refuses"""
    Rm = np.asarray(calib["R"], np.float64).reshape(3, 3)
    T = np.asarray(calib["T"], np.float64)
    c = (((Rm[0, 0] + Rm[1, 1]) + Rm[2, 2]) - 1.0) / 2.0                        # 1
    v = np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    angle = np.arctan2(n / 2.0, c)
    if not angle <= 0.5:
        return None
    k = v / n if n > 0.0 else np.zeros(3)
    Rl0, Rr0 = _rodrigues(k, angle / 2.0), _rodrigues(-k, angle / 2.0)          # 2 (sin is odd, K K even: the same terms)
    t = np.array([(Rr0[i, 0] * T[0] + Rr0[i, 1] * T[1]) + Rr0[i, 2] * T[2] for i in range(3)])   # 3
    b = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    if not b > 0.0:
        return None
    e1 = -t / b
    if not (e1[0] > 0.0 and e1[0] >= abs(e1[1]) and e1[0] >= abs(e1[2])):
        return None
    n2 = np.sqrt(e1[1] * e1[1] + e1[0] * e1[0])                                 # 4
    e2 = np.array([-e1[1] / n2, e1[0] / n2, 0.0])
    e3 = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    W = np.array([e1, e2, e3])
    Rk = [_mat(W, Rl0), _mat(W, Rr0)]
    f = (calib["left"][1] + calib["right"][1]) / 2.0                            # 5
    mx = (f * Rk[0][0, 2] / Rk[0][2, 2] + f * Rk[1][0, 2] / Rk[1][2, 2]) / 2.0  # 6
    my = (f * Rk[0][1, 2] / Rk[0][2, 2] + f * Rk[1][1, 2] / Rk[1][2, 2]) / 2.0
    cx = (float(w) - 1.0) / 2.0 - mx
    cy = (float(h) - 1.0) / 2.0 - my
    return dict(left=calib["left"], right=calib["right"], R_left=f32(Rk[0]).reshape(9), R_right=f32(Rk[1]).reshape(9),   # 7
                fx=float(f32(f)), fy=float(f32(f)), cx=float(f32(cx)), cy=float(f32(cy)), baseline=float(f32(b)),
                depth_scale=float(f32(depth_scale)))


def rig_floats(rig):
    """the 42 floats of the struct, in its order"""
    out = []
    for lens in (rig["left"], rig["right"]):
        out += list(lens[:4]) + list(lens[4])
    out += list(rig["R_left"]) + list(rig["R_right"])
    out += [rig[k] for k in ("fx", "fy", "cx", "cy", "baseline", "depth_scale")]
    return np.array(out, np.float32)


def to_struct(F, rig):
    """The rig as the package's StereoRig."""
    if rig is None:
        return None
    return F.StereoRig(F.Lens(*rig["left"]), F.Lens(*rig["right"]), rig["R_left"], rig["R_right"], rig["fx"], rig["fy"],
                       rig["cx"], rig["cy"], rig["baseline"], rig["depth_scale"])


def calib_struct(F, calib):
    return F.StereoCalib(F.Lens(*calib["left"]), F.Lens(*calib["right"]), calib["R"], calib["T"])


# ---- the maps, validity, a frame -----------------------------------------------------------------

def _distort(lens, x, y):
    """the forward formulae of the rectification contract at the ideal point (x, y): the pixel (us, vs)"""
    fx, fy, cx, cy, (k1, k2, p1, p2, k3) = lens
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + ((2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x))
    yd = y * rad + (p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y)
    return fx * xd + cx, fy * yd + cy


def rig_map(rig, which, w, h, transposed=False, raw_cx=False):
    """(qu, qv) of camera `which`: int32 h x w.  (The keywords are the mutants of the CPU test: R_k applied the wrong
    way round, and (u - cx) taken with the camera's own cx.)"""
    lens = rig["right"] if which else rig["left"]
    Rk = np.asarray(rig["R_right"] if which else rig["R_left"], np.float64).reshape(3, 3)
    if transposed:
        Rk = Rk.T
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    xr = (u - (lens[2] if raw_cx else rig["cx"])) / rig["fx"]
    yr = (v - rig["cy"]) / rig["fy"]
    X = (Rk[0, 0] * xr + Rk[1, 0] * yr) + Rk[2, 0]
    Y = (Rk[0, 1] * xr + Rk[1, 1] * yr) + Rk[2, 1]
    Z = (Rk[0, 2] * xr + Rk[1, 2] * yr) + Rk[2, 2]
    front = Z > 0.0
    with np.errstate(all="ignore"):
        Zs = np.where(front, Z, 1.0)
        us, vs = _distort(lens, X / Zs, Y / Zs)
        us = np.where(front, us, -1.0)
        vs = np.where(front, vs, -1.0)
        us = np.where(us >= -1.0, us, -1.0)   # (also what is not a number)
        us = np.where(us > float(w), float(w), us)
        vs = np.where(vs >= -1.0, vs, -1.0)
        vs = np.where(vs > float(h), float(h), vs)
    return np.rint(32.0 * us).astype(np.int32), np.rint(32.0 * vs).astype(np.int32)


def valid(qu, qv):
    """V: the nearest sample lies inside the raw image"""
    h, w = qu.shape
    xn = (qu.astype(np.int64) + 16) >> 5
    yn = (qv.astype(np.int64) + 16) >> 5
    return (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)


def frame(rig, raw_l, raw_r, st, maps=None, outside_right=True):
    """Every plane of a frame under a rig, by name: fe_stereo_ref.match()'s of the rectified pair with the rig's
    camera and baseline, `flags`, `disparity` and `depth` after OUTSIDE, and rect_l, rect_r, valid (bit 0 V_L, bit 1
    V_R), flags_before.  (The keywords are mutants: other maps, OUTSIDE without its right-image half.)"""
    h, w = raw_l.shape[:2]
    (qul, qvl), (qur, qvr) = maps or (rig_map(rig, 0, w, h), rig_map(rig, 1, w, h))
    rect_l, rect_r = R.remap_colour(raw_l, qul, qvl), R.remap_colour(raw_r, qur, qvr)
    VL, VR = valid(qul, qvl), valid(qur, qvr)
    P = S.match(rect_l, rect_r, dict(st, baseline=rig["baseline"]), rig["fx"], rig["depth_scale"])
    xr = np.arange(w)[None, :] - P["dL"]
    out = ~VL
    if outside_right:
        out = out | ((xr >= 0) & ~VR[np.arange(h)[:, None], np.clip(xr, 0, w - 1)])
    flags = (P["flags"] | np.where(out, OUTSIDE, 0)).astype(np.uint8)
    keep = flags == 0
    return dict(P, flags_before=P["flags"], flags=flags, disparity=np.where(keep, P["disparity"], 0).astype(np.uint16),
                depth=np.where(keep, P["depth"], 0).astype(np.uint16), rect_l=rect_l, rect_r=rect_r,
                valid=(VL.astype(np.uint8) | (VR.astype(np.uint8) << 1)))


# ---- the renderer: raw images for a rig ------------------------------------------------------------

def _undistort(lens, u, v):
    """the ideal point of raw pixel (u, v): 20 fixed-point iterations"""
    fx, fy, cx, cy, (k1, k2, p1, p2, k3) = lens
    xd = (u - cx) / fx
    yd = (v - cy) / fy
    x, y = xd, yd
    for _ in range(20):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = (2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x)
        dy = p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y
        x = (xd - dx) / rad
        y = (yd - dy) / rad
    return x, y


def unwarp(rig, which, rect):
    """The raw image camera `which` would deliver for the rectified image `rect`: every raw pixel is undistorted,
    turned by R_k, projected with the rectified pinhole and sampled bilinearly (float64, the border replicated)."""
    h, w = rect.shape[:2]
    lens = rig["right"] if which else rig["left"]
    Rk = np.asarray(rig["R_right"] if which else rig["R_left"], np.float64).reshape(3, 3)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = _undistort(lens, u, v)
    X = Rk[0, 0] * x + Rk[0, 1] * y + Rk[0, 2]
    Y = Rk[1, 0] * x + Rk[1, 1] * y + Rk[1, 2]
    Z = Rk[2, 0] * x + Rk[2, 1] * y + Rk[2, 2]
    ur = np.clip(rig["fx"] * X / Z + rig["cx"], 0.0, w - 1.0)
    vr = np.clip(rig["fy"] * Y / Z + rig["cy"], 0.0, h - 1.0)
    x0 = np.minimum(np.floor(ur).astype(np.int64), w - 2)
    y0 = np.minimum(np.floor(vr).astype(np.int64), h - 2)
    ax = (ur - x0)[:, :, None]
    ay = (vr - y0)[:, :, None]
    p = rect.astype(np.float64)
    out = (1.0 - ay) * ((1.0 - ax) * p[y0, x0] + ax * p[y0, x0 + 1]) + ay * ((1.0 - ax) * p[y0 + 1, x0] + ax * p[y0 + 1, x0 + 1])
    return np.ascontiguousarray(np.clip(np.rint(out), 0, 255).astype(np.uint8))


def render(rig, w, h, seed=SEED, **scene):
    """(raw_left, raw_right) of a rig for fe_stereo_ref.pair(w, h, seed)"""
    left, right, _ = S.pair(w, h, seed, **scene)
    return unwarp(rig, 0, left), unwarp(rig, 1, right)


# ---- the rigs of the tests -------------------------------------------------------------------------

CALIBS = {
    "A": (96, 64, 32, make_calib((70.0, 70.3, 47.2, 31.5, (-0.28, 0.07, 0.0002, 0.00002, 0.0)),
                                 (69.5, 69.9, 48.9, 32.6, (-0.283, 0.074, -0.0001, -0.00004, 0.0)),
                                 (0.010, -0.020, 0.005), (-0.11, 0.0004, -0.0008))),
    "B": (127, 193, 48, make_calib((100.0, 100.0, 63.0, 96.0, (0.20, 0.05, 0.002, -0.001, 0.0)),
                                   (101.0, 100.5, 61.0, 97.5, (0.18, 0.06, -0.001, 0.002, 0.0)),
                                   (-0.02, 0.08, -0.03), (-0.25, 0.004, 0.01))),
}
_PIN = (60.0, 60.0, 31.5, 31.5, ZERO)
_EYE = np.eye(3).reshape(9)
RIG_I = dict(left=_PIN, right=_PIN, R_left=_EYE, R_right=_EYE, fx=60.0, fy=60.0, cx=31.5, cy=31.5, baseline=float(f32(0.2)),
             depth_scale=DEPTH_SCALE)

_DONE = {}


def case(name):
    """(w, h, settings, rig, raw_left, raw_right, planes) of rig "A" or "B" at DEPTH_SCALE: computed once, left unchanged"""
    if name not in _DONE:
        w, h, D, calib = CALIBS[name]
        rig = rectify(calib, w, h, DEPTH_SCALE)
        st = S.make_stereo(max_disp=D)
        raw_l, raw_r = render(rig, w, h)
        P = frame(rig, raw_l, raw_r, st)
        for a in (raw_l, raw_r) + tuple(P.values()):
            a.setflags(write=False)
        _DONE[name] = (w, h, st, rig, raw_l, raw_r, P)
    return _DONE[name]
