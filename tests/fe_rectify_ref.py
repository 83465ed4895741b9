"""A numpy restatement of the front end's rectification contract (include/cvo_frontend.h,
at cvo_fe_camera_model): the map, the colour taps and the depth tap.  float64 for the map
(numpy never contracts into an FMA), integers after it.  The order of operations below is
the contract; csrc/cvo_fe_calib.cpp repeats it line by line in cvo_fe_rectify_map.

A model here is (depth_scale, fx, fy, cx, cy, (k1, k2, p1, p2, k3)); its numbers count as
float32, as the library's struct holds them."""
import numpy as np

# published TUM RGB-D calibrations (fx fy cx cy, d0..d4), depth 5000 units per metre
FR1 = (5000.0, 517.3, 516.5, 318.6, 255.3, (0.2624, -0.9531, -0.0054, 0.0026, 1.1633))
FR2 = (5000.0, 520.9, 521.0, 325.1, 249.7, (0.2312, -0.7849, -0.0033, -0.0001, 0.9172))

# the small models of the tests: (width, height, model)
#   A: fr1's intrinsics x 0.15 with fr1's distortion: a few per cent of the map leave the image
#   B: a strong pincushion-like lens: about a fifth leaves the image
#   C: a barrel lens on an odd size: nothing leaves the image, shifts of up to 30 px
SMALL = {
    "A": (96, 64, (5000.0, 517.3 * 0.15, 516.5 * 0.15, 318.6 * 0.15, 255.3 * 0.15, FR1[5])),
    "B": (96, 64, (5000.0, 77.6, 77.5, 47.8, 38.3, (0.35, 0.1, 0.004, -0.003, 0.0))),
    "C": (127, 193, (5000.0, 100.0, 100.0, 63.0, 96.0, (-0.30, 0.08, 0.002, 0.001, 0.0))),
}


def as_floats(model):
    """The model's ten numbers as the float32 the library holds, widened exactly to float64."""
    scale, fx, fy, cx, cy, dist = model
    v = np.array([scale, fx, fy, cx, cy] + list(dist), np.float32).astype(np.float64)
    return v[0], v[1], v[2], v[3], v[4], v[5:]


def source_coordinates(model, w, h):
    """(us, vs) before clamping and quantising: where output pixel (u, v) looks in the input."""
    _, fx, fy, cx, cy, (k1, k2, p1, p2, k3) = as_floats(model)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x = (u - cx) / fx
    y = (v - cy) / fy
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + ((2.0 * p1) * x * y + p2 * (r2 + (2.0 * x) * x))
    yd = y * rad + (p1 * (r2 + (2.0 * y) * y) + (2.0 * p2) * x * y)
    us = fx * xd + cx
    vs = fy * yd + cy
    return us, vs


def rectify_map(model, w, h):
    """(qu, qv): int32 h x w, source coordinates in 1/32 pixel, clamped to [-1, w] x [-1, h]."""
    us, vs = source_coordinates(model, w, h)
    with np.errstate(invalid="ignore"):
        us = np.where(us >= -1.0, us, -1.0)   # (also what is not a number)
        us = np.where(us > float(w), float(w), us)
        vs = np.where(vs >= -1.0, vs, -1.0)
        vs = np.where(vs > float(h), float(h), vs)
    return np.rint(32.0 * us).astype(np.int32), np.rint(32.0 * vs).astype(np.int32)


def remap_colour(img, qu, qv):
    """Bilinear at 1/32 pixel in integers, replicated border: h x w x 3 uint8."""
    h, w = img.shape[:2]
    qu = qu.astype(np.int64); qv = qv.astype(np.int64)
    x0 = qu >> 5; y0 = qv >> 5          # floor
    ax = qu - 32 * x0; ay = qv - 32 * y0
    xa = np.clip(x0, 0, w - 1); xb = np.clip(x0 + 1, 0, w - 1)
    ya = np.clip(y0, 0, h - 1); yb = np.clip(y0 + 1, 0, h - 1)
    p = img.astype(np.int64)
    acc = (((32 - ax) * (32 - ay))[..., None] * p[ya, xa] + (ax * (32 - ay))[..., None] * p[ya, xb] +
           ((32 - ax) * ay)[..., None] * p[yb, xa] + (ax * ay)[..., None] * p[yb, xb])
    return ((acc + 512) >> 10).astype(np.uint8)


def remap_depth(depth, qu, qv):
    """The nearest sample, 0 outside the image: h x w uint16."""
    h, w = depth.shape
    xn = (qu.astype(np.int64) + 16) >> 5
    yn = (qv.astype(np.int64) + 16) >> 5
    inside = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
    out = depth[np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)]
    return np.where(inside, out, 0).astype(np.uint16)


def rectify(model, bgr, depth):
    h, w = depth.shape
    qu, qv = rectify_map(model, w, h)
    return remap_colour(bgr, qu, qv), remap_depth(depth, qu, qv)


def map_statistics(model, w, h):
    """Fractions of the map whose nearest sample lies outside the image / that have a clamped
    colour tap / that have a non-zero fraction, and the largest shift in pixels (of the clamped map)."""
    qu, qv = rectify_map(model, w, h)
    xn = (qu.astype(np.int64) + 16) >> 5; yn = (qv.astype(np.int64) + 16) >> 5
    outside = (xn < 0) | (xn >= w) | (yn < 0) | (yn >= h)
    x0 = qu >> 5; y0 = qv >> 5
    clamped = (x0 < 0) | (x0 + 1 > w - 1) | (y0 < 0) | (y0 + 1 > h - 1)
    frac = ((qu & 31) != 0) | ((qv & 31) != 0)
    v, u = np.mgrid[0:h, 0:w]
    return outside.mean(), clamped.mean(), frac.mean(), float(np.hypot(qu / 32.0 - u, qv / 32.0 - v).max())
