"""Mutants of the restatement of the LiDAR contract (tests/fe_lidar_ref.py): each one restates the stage with one
plausible device error in it -- the errors a projection with a z-buffer and a tiled window minimum can make: a tie
rounded the other way, a conversion that truncates, the wrong end of the z-buffer, a splat that runs over the end of a
row, the range or the depth value taken from the wrong quantity, an empty pixel or the largest depth mistaken in the
minimum, a result read back as a neighbour's input, the comparison off by its equality, the window turned, neighbours
lost where two tiles meet, and the number of points of the frame before.
tests/test_fe_lidar_cpu.py holds that the scans made on purpose tell every one of them from the restatement at every
setting at which the error can show: a kernel with that error would fail the byte comparison of
tests/test_gpu_fe_lidar.py.  Python only; nothing here ever runs against the GPU."""
import numpy as np

import fe_lidar_ref as K

f32 = np.float32
BIG = K.BIG


def _project(points, s, cam, w, h, nearest=np.rint, farthest=False, wrap=False, range_on_norm=False, raw_z=False):
    """K.project with its switches: `nearest` in place of rint in step 8 (and what it gives is clamped afterwards),
    the z-buffer's maximum, pixels bounded by the plane's length only, |p| in step 4, z of the point in step 7"""
    p = np.asarray(points, f32)
    p = p.reshape(len(p), -1) if len(p) else np.zeros((0, 3), f32)
    cam = np.asarray(cam, f32)
    R, T = np.asarray(s.R, f32).reshape(3, 3), np.asarray(s.T, f32)
    lo, hi = f32(s.min_range), f32(s.max_range)
    Z = np.full(w * h, -1 if farthest else BIG, np.int64)
    if len(p) == 0:
        return np.zeros((h, w), np.uint16)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        alive = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        Q = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + T[k] for k in range(3)]
        alive &= Q[2] > 0
        d = np.sqrt((Q[0] * Q[0] + Q[1] * Q[1]) + Q[2] * Q[2]) if range_on_norm else Q[2]
        alive &= ~(((lo > 0) & (d < lo)) | ((hi > 0) & (d > hi)))
        u = cam[1] * (Q[0] / Q[2]) + cam[3]
        v = cam[2] * (Q[1] / Q[2]) + cam[4]
        alive &= np.isfinite(u) & np.isfinite(v)
        q = np.rint((z if raw_z else Q[2]) * cam[0])
        alive &= (q >= 1) & (q <= 65535)
        u, v, q = u[alive], v[alive], q[alive].astype(np.int64)
        xi = nearest(np.minimum(np.maximum(u, f32(-8)), f32(w + 8))).astype(np.int64)
        yi = nearest(np.minimum(np.maximum(v, f32(-8)), f32(h + 8))).astype(np.int64)
    for dy in range(-s.splat, s.splat + 1):
        for dx in range(-s.splat, s.splat + 1):
            px, py = xi + dx, yi + dy
            i = py * w + px
            inside = ((i >= 0) & (i < w * h)) if wrap else ((px >= 0) & (px < w) & (py >= 0) & (py < h))
            (np.maximum if farthest else np.minimum).at(Z, i[inside], q[inside])
    return np.where((Z == BIG) | (Z == -1), 0, Z).astype(np.uint16).reshape(h, w)


def _finish(P0, P, occluded):
    hit = P0 != 0
    flags = (hit * K.HIT + (occluded & hit) * K.OCCLUDED).astype(np.uint8)
    return P.astype(np.uint16), P0, flags


def _with_cull(P0, s):
    return _finish(P0, *_cull(P0, s))


def _cull(P0, s, zeros=False, max_none=False, at_equality=False, swapped=False, tile=None):
    """K.cull with its switches; gives (P, occluded)"""
    rx, ry = (s.ry, s.rx) if swapped else (s.rx, s.ry)
    h, w = P0.shape
    V = P0.astype(np.int64)
    member = np.ones(P0.shape, bool) if zeros else (V != 0)
    if max_none:
        member &= V != 65535
    keys = np.where(member, V, BIG)
    pad = np.pad(keys, ((ry, ry), (rx, rx)), constant_values=BIG)
    ty, tx = (np.arange(h) // (tile[1] if tile else h))[:, None], (np.arange(w) // (tile[0] if tile else w))[None, :]
    m = np.full(P0.shape, BIG, np.int64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            cand = pad[ry + dy:ry + dy + h, rx + dx:rx + dx + w]
            if tile:
                yy, xx = np.arange(h)[:, None] + dy, np.arange(w)[None, :] + dx
                cand = np.where((yy // tile[1] == ty) & (xx // tile[0] == tx), cand, BIG)
            m = np.minimum(m, cand)
    own = np.where(V == 65535, 0, V) if max_none else V
    hit = own != 0
    m = np.where(hit & (m != BIG), m, np.where(hit, own, 1))
    diff, bound = (own - m).astype(f32), f32(s.occl_rel) * m.astype(f32)
    occluded = hit & bool(f32(s.occl_rel) > 0) & ((diff >= bound) if at_equality else (diff > bound))
    return np.where(occluded, 0, own), occluded


def _mutant(project_kw=None, cull_kw=None):
    def run(points, s, cam, w, h):
        P0 = _project(points, s, cam, w, h, **(project_kw or {}))
        P, occluded = _cull(P0, s, **(cull_kw or {}))
        if (cull_kw or {}).get("max_none"):
            P0 = np.where(P0 == 65535, 0, P0).astype(np.uint16)
        return _finish(P0, P, occluded)
    return run


def _half_up(a):
    return np.floor(a + f32(0.5))


half_up = _mutant(dict(nearest=_half_up))                 # ties rounded half-up instead of to even
truncated = _mutant(dict(nearest=np.trunc))               # (int)u: truncation instead of rint
farthest_wins = _mutant(dict(farthest=True))              # atomicMax for atomicMin
splat_wraps = _mutant(dict(wrap=True))                    # the splat bounded by the plane, not by the row
range_on_norm = _mutant(dict(range_on_norm=True))         # the range tested on |Q|
raw_depth = _mutant(dict(raw_z=True))                     # q from the point's own z, before R and T
zeros_counted = _mutant(None, dict(zeros=True))           # a pixel without depth is a member of the window with value 0
max_is_none = _mutant(None, dict(max_none=True))          # 65535 taken for "none"
at_equality = _mutant(None, dict(at_equality=True))       # >= for >
window_swapped = _mutant(None, dict(swapped=True))        # rx for ry


def in_place(points, s, cam, w, h):
    """culled in place in scan order: a pixel's window holds the results of the pixels before it"""
    P0 = _project(points, s, cam, w, h)
    B = P0.astype(np.int64).copy()
    rel = f32(s.occl_rel)
    occluded = np.zeros(P0.shape, bool)
    if rel > 0:
        for y, x in zip(*np.nonzero(P0)):
            win = B[max(y - s.ry, 0):y + s.ry + 1, max(x - s.rx, 0):x + s.rx + 1]
            m = int(win[win != 0].min())
            if f32(int(B[y, x]) - m) > rel * f32(m):
                B[y, x] = 0
                occluded[y, x] = True
    return _finish(P0, B, occluded)


def tile_cut(tw, th):
    """neighbours outside the pixel's own tile of tw x th pixels dropped: no halo"""
    return _mutant(None, dict(tile=(tw, th)))


TILES = [(32, 8), (64, 4), (16, 16), K.TILE]

# name -> (the mutant, at which points of the grid (splat, rx, ry, rel) its error can show at all)
ALWAYS = lambda g: True
CULLS = lambda g: g[3] > 0 and (g[1] > 0 or g[2] > 0)       # the window holds another pixel and the test runs
PLAIN = {
    "half_up": (half_up, ALWAYS),
    "truncated": (truncated, ALWAYS),
    "farthest_wins": (farthest_wins, ALWAYS),
    "splat_wraps": (splat_wraps, ALWAYS),                   # (at splat 0 too: a nearest pixel left or right of the image)
    "range_on_norm": (range_on_norm, ALWAYS),
    "raw_depth": (raw_depth, ALWAYS),
    "zeros_counted": (zeros_counted, CULLS),
    "max_is_none": (max_is_none, ALWAYS),                   # (the pixel itself loses its depth)
    "at_equality": (at_equality, CULLS),                    # (in a window of one pixel 0 >= rel * m never holds: m >= 1)
    "window_swapped": (window_swapped, lambda g: g[3] > 0 and g[1] != g[2]),
    "in_place": (in_place, CULLS),
}
for _t in TILES:
    PLAIN["tile_cut_%dx%d" % _t] = (tile_cut(*_t), CULLS)


def stale_counts(scans, s, cam, w, h, capacity):
    """the frames of one context whose kernel takes the number of points of the frame BEFORE (the first frame: 0) from a
    staging buffer that keeps what earlier frames left behind their own points: one (P, P0, flags) per scan"""
    staging = np.zeros((capacity, 3), np.float32)
    out, before = [], 0
    for pts in scans:
        staging[:len(pts)] = np.asarray(pts, np.float32)[:, :3]
        out.append(_with_cull(_project(staging[:before], s, cam, w, h), s))
        before = len(pts)
    return out
