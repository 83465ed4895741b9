"""A numpy restatement of the front end's registration contract (include/cvo_frontend.h, at
cvo_fe_depth_camera): the ray table in float64 and the forward warp with its z-buffer in
float32 (numpy never contracts into an FMA; its float32 division and np.rint are IEEE's).  The
order of operations below is the contract; csrc/cvo_fe_calib.cpp repeats it line by line in
cvo_fe_depth_rays and csrc/cvo_frontend.hip in k_fe_depth_warp.

A rig here is a dict with the members of cvo_fe_depth_camera (R as nine numbers, row-major);
a colour camera is (depth_scale, fx, fy, cx, cy).  Their numbers count as float32, as the
library's structs hold them.  Also here: the rigs and the scene the tests share."""
import numpy as np

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
EYE = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
FOOT = 8            # the cap of a footprint per axis
EMPTY = 0xFFFFFFFF  # a z-buffer entry nothing was written to


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def make_rig(width, height, cam, dist=ZERO, R=EYE, T=(0.0, 0.0, 0.0), min_range=0.0, max_range=0.0):
    scale, fx, fy, cx, cy = cam
    return dict(width=int(width), height=int(height), depth_scale=scale, fx=fx, fy=fy, cx=cx, cy=cy,
                dist=tuple(dist), R=tuple(float(v) for v in np.asarray(R, np.float64).reshape(-1)), T=tuple(T),
                min_range=min_range, max_range=max_range)


def identity_rig(width, height, cam):
    return make_rig(width, height, cam)


# the colour cameras of the small frames
COLOUR = {(96, 64): (5000.0, 77.6, 77.5, 47.8, 38.3), (127, 193): (5000.0, 100.0, 100.0, 63.0, 96.0)}
K_R = rot_z(0.003) @ rot_y(-0.007) @ rot_x(0.004)
K_T = (0.025, -0.001, 0.002)

# name: (colour width, colour height, colour camera, rig)
#   K: a Kinect-like pair          U: upsampling, footprints up to 2 x 2, odd sizes
#   D: downsampling, most depth pixels have an empty footprint
#   C: the 8 x 8 cap decides       W: a lens the fixed point cannot invert: invalid rays
RIGS = {
    "K": (96, 64, COLOUR[(96, 64)],
          make_rig(96, 64, (1000.0, 87.0, 87.2, 46.1, 30.9), (-0.12, 0.03, 0.001, -0.002, 0.0), K_R, K_T)),
    "U": (127, 193, COLOUR[(127, 193)],
          make_rig(72, 112, (1000.0, 58.0, 58.5, 35.5, 55.0), (0.05, -0.02, 0.0, 0.0, 0.0),
                   rot_z(-0.02) @ rot_y(0.012) @ rot_x(-0.01), (-0.05, 0.01, 0.0))),
    "D": (96, 64, COLOUR[(96, 64)],
          make_rig(200, 132, (5000.0, 160.0, 160.0, 100.0, 66.0), ZERO, rot_y(0.02), (0.03, 0.0, -0.01))),
    "C": (96, 64, (5000.0, 100.0, 100.0, 47.5, 31.5),
          make_rig(24, 16, (5000.0, 10.0, 10.0, 11.5, 7.5), ZERO, EYE, (0.01, 0.0, 0.0))),
    "W": (96, 64, COLOUR[(96, 64)],
          make_rig(96, 64, (5000.0, 30.0, 30.0, 47.5, 31.5), (4.0, 0.0, 0.0, 0.0, 0.0))),
}
for _size, _cam in COLOUR.items():
    RIGS["I%dx%d" % _size] = (_size[0], _size[1], _cam, identity_rig(_size[0], _size[1], _cam))
RIGS["I"] = RIGS["I96x64"]

# the VGA Kinect-like depth camera of the cloud tests, beside the table's row 1
VGA_COLOUR = (5000.0, 517.3, 516.5, 318.6, 255.3)
VGA_RIG = make_rig(640, 480, (1000.0, 580.0, 580.0, 314.0, 252.0), (-0.1, 0.3, 0.001, -0.001, -0.2), K_R, K_T)


def bad_rigs():
    """Rigs cvo_fe_set_depth_camera and cvo_fe_depth_rays refuse, one reason each."""
    good = RIGS["K"][3]
    nan, inf = float("nan"), float("inf")
    out = [dict(good, **{k: v}) for k, v in (
        ("width", 7), ("width", 8193), ("height", 7), ("height", 8193), ("width", -1), ("fx", nan), ("cy", inf),
        ("depth_scale", -inf), ("min_range", nan), ("max_range", inf), ("fx", 0.0), ("fy", 0.0), ("fy", -1.0),
        ("depth_scale", 0.0), ("depth_scale", -1000.0))]
    out.append(dict(good, min_range=0.5, max_range=0.5))
    out.append(dict(good, min_range=2.0, max_range=1.0))
    out.append(dict(good, dist=(nan, 0.0, 0.0, 0.0, 0.0)))
    out.append(dict(good, T=(0.0, inf, 0.0)))
    out.append(dict(good, R=(nan,) + EYE[1:]))
    out.append(dict(good, R=(1.002,) + EYE[1:]))                           # R R^T - I = 4e-3
    out.append(dict(good, R=(1.0, 0.002, 0.0) + EYE[3:]))                  # off-diagonal 2e-3
    out.append(dict(good, R=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0)))  # a reflection: det = -1
    out.append(dict(good, R=(0.0,) * 9))
    return out


def to_struct(F, rig):
    """The rig as the package's DepthCamera."""
    return F.DepthCamera(**rig)


def scene(data, rig, seed=72, **kw):
    """The depth image the rig sees: a box at 0.6 m (3000 units of 1/5000 m) in front of the wall of
    data.synthetic_rgbd_frame; for a rig counting 1000 units per metre the image is divided by 5."""
    w, h = rig["width"], rig["height"]
    _, dep = data.synthetic_rgbd_frame(width=w, height=h, seed=seed, texture=1.0, **kw)
    dep = dep.copy()
    box = dep[h // 4:3 * h // 5, w // 3:3 * w // 5]
    box[box != 0] = 3000
    if rig["depth_scale"] == 1000.0:
        dep //= 5
    return np.ascontiguousarray(dep, np.uint16)


def _f32(rig):
    f = np.float32
    return (f(rig["depth_scale"]), f(rig["fx"]), f(rig["fy"]), f(rig["cx"]), f(rig["cy"]),
            np.array(rig["dist"], f), np.array(rig["R"], f).reshape(3, 3), np.array(rig["T"], f),
            f(rig["min_range"]), f(rig["max_range"]))


def _forward(x, y, fx, fy, cx, cy, dist):
    """The rectification contract's distortion of (x, y) to image coordinates."""
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + ((2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x))
    yd = y * rad + (p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y)
    return fx * xd + cx, fy * yd + cy


def rays(rig):
    """(xn, yn): float32 (height+1) x (width+1), the rays through the corners (i - 0.5, j - 0.5)."""
    _, fx, fy, cx, cy, dist, _, _, _, _ = _f32(rig)
    fx, fy, cx, cy = (np.float64(v) for v in (fx, fy, cx, cy))
    dist = dist.astype(np.float64)
    k1, k2, p1, p2, k3 = dist
    j, i = np.mgrid[0:rig["height"] + 1, 0:rig["width"] + 1].astype(np.float64)
    px, py = i - 0.5, j - 0.5
    xd = (px - cx) / fx
    yd = (py - cy) / fy
    x, y = xd, yd
    if np.any(dist != 0.0):
        with np.errstate(all="ignore"):
            for _ in range(20):
                r2 = x * x + y * y
                rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
                dx = (2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x)
                dy = p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y
                x = (xd - dx) / rad
                y = (yd - dy) / rad
            us, vs = _forward(x, y, fx, fy, cx, cy, dist)
            ok = (np.abs(us - px) <= 1.0 / 32.0) & (np.abs(vs - py) <= 1.0 / 32.0)   # (NaN fails)
        x = np.where(ok, x, np.nan)
        y = np.where(ok, y, np.nan)
    with np.errstate(all="ignore"):
        return x.astype(np.float32), y.astype(np.float32)


def footprints(rig, colour_cam, w, h, depth, cap=FOOT):
    """Per depth pixel (flattened, row-major): `live`, its depth q in the colour camera's units and the
    half-open ranges [x0, x1) x [y0, y1) of colour pixels, already cut to the image."""
    f = np.float32
    scale, _, _, _, _, _, R, T, rmin, rmax = _f32(rig)
    sc, fxc, fyc, cxc, cyc = (f(v) for v in colour_cam)
    dw, dh = rig["width"], rig["height"]
    depth = np.asarray(depth)
    assert depth.shape == (dh, dw) and depth.dtype == np.uint16
    xn, yn = rays(rig)
    with np.errstate(all="ignore"):
        z = depth.astype(f) / scale
        live = depth != 0
        if rmin > 0:
            live &= ~(z < rmin)
        if rmax > 0:
            live &= ~(z > rmax)

        def corner(xr, yr):
            X = xr * z
            Y = yr * z
            return [((R[k, 0] * X + R[k, 1] * Y) + R[k, 2] * z) + T[k] for k in range(3)]

        Qa = corner(xn[:-1, :-1], yn[:-1, :-1])
        Qb = corner(xn[1:, 1:], yn[1:, 1:])
        live &= (Qa[2] > 0) & (Qb[2] > 0)
        ua = fxc * (Qa[0] / Qa[2]) + cxc
        va = fyc * (Qa[1] / Qa[2]) + cyc
        ub = fxc * (Qb[0] / Qb[2]) + cxc
        vb = fyc * (Qb[1] / Qb[2]) + cyc
        live &= np.isfinite(ua) & np.isfinite(va) & np.isfinite(ub) & np.isfinite(vb)
        q = np.rint((f(0.5) * (Qa[2] + Qb[2])) * sc)
        live &= (q >= 1) & (q <= 65535)
        assert z.dtype == f and ua.dtype == f and q.dtype == f

        def span(pa, pb, n):
            lo = np.where(live, np.minimum(pa, pb), f(0))
            hi = np.where(live, np.maximum(pa, pb), f(0))
            p0 = np.ceil(np.clip(lo, f(-1), f(n + 1))).astype(np.int64)
            p1 = np.ceil(np.clip(hi, f(-1), f(n + 1))).astype(np.int64)
            if cap is not None:
                p1 = np.minimum(p1, p0 + cap)
            return np.maximum(p0, 0), np.minimum(p1, n)

        x0, x1 = span(ua, ub, w)
        y0, y1 = span(va, vb, h)
    q = np.where(live, q, 0).astype(np.int64)
    return live.ravel(), q.ravel(), x0.ravel(), x1.ravel(), y0.ravel(), y1.ravel()


def register(rig, colour_cam, w, h, depth, cap=FOOT, farthest=False):
    """The registered depth image: uint16 h x w.  `cap` None and `farthest` are for the tests' questions
    about the rigs (what the cap and the z-test decide), not part of the contract."""
    live, q, x0, x1, y0, y1 = footprints(rig, colour_cam, w, h, depth, cap)
    Z = np.full((h, w), -1 if farthest else EMPTY, np.int64)
    nx, ny = np.where(live, x1 - x0, 0), np.where(live, y1 - y0, 0)
    for dy in range(int(ny.max(initial=0))):
        for dx in range(int(nx.max(initial=0))):
            m = (dx < nx) & (dy < ny)
            if farthest:
                np.maximum.at(Z, (y0[m] + dy, x0[m] + dx), q[m])
            else:
                np.minimum.at(Z, (y0[m] + dy, x0[m] + dx), q[m])
    return np.where((Z == EMPTY) | (Z < 0), 0, Z).astype(np.uint16)


def footprint_sizes(rig, colour_cam, w, h, depth):
    """The number of colour pixels each live depth pixel writes (0: an empty footprint)."""
    live, _, x0, x1, y0, y1 = footprints(rig, colour_cam, w, h, depth)
    n = np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)
    return n[live]
