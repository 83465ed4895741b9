"""The LiDAR contract of include/cvo_frontend.h (at cvo_fe_lidar) restated in numpy: the projection of a scan into the
colour camera in float32, operation by operation in the contract's order, with np.minimum.at as the z-buffer; the
occlusion cull as a plain loop over the pixels and in a vectorised form; and the scans and settings made on purpose that
tests/test_fe_lidar_cpu.py (what they reach, which mutants they tell) and tests/test_gpu_fe_lidar.py (the device against
this file, by bytes) share.  numpy's float32 operations are single IEEE operations, rounded once: nothing is fused."""
from collections import namedtuple

import numpy as np

f32 = np.float32
HIT, OCCLUDED = 1, 2
BIG = 1 << 20
TILE = (64, 16)          # of k_fe_lidar_cull
MAX_POINTS = 1 << 21

# one scan source: cvo_fe_lidar without max_points
Setting = namedtuple("Setting", "splat R T min_range max_range occl_rel rx ry")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

# why a point wrote nothing: the step of the contract that skipped it; 0: it wrote a pixel; OUTSIDE: it passed every
# step and no pixel of its splat lies inside the image
WROTE, NOT_FINITE, BEHIND, RANGE, UV, DEPTH, OUTSIDE = 0, 1, 3, 4, 6, 7, 9


def to_struct(F, s, max_points=4200):
    return None if s is None else F.Lidar(max_points, s.splat, s.R, s.T, s.min_range, s.max_range, s.occl_rel, s.rx, s.ry)


def project(points, s, cam, w, h):
    """Steps 1 to 9: (P0 as h x w uint16, why as one code per point).  `points`: n x k, x y z first; `cam`: depth scale,
    fx, fy, cx, cy."""
    p = np.asarray(points, f32)
    p = p.reshape(len(p), -1) if len(p) else np.zeros((0, 3), f32)
    n = len(p)
    cam = np.asarray(cam, f32)
    R, T = np.asarray(s.R, f32).reshape(3, 3), np.asarray(s.T, f32)
    lo, hi = f32(s.min_range), f32(s.max_range)
    why = np.zeros(n, np.int32)
    Z = np.full((h, w), BIG, np.int64)
    if n == 0:
        return np.zeros((h, w), np.uint16), why
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        alive = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)                                  # 1
        why[~alive] = NOT_FINITE
        Q = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + T[k] for k in range(3)]                # 2
        step = alive & ~(Q[2] > 0)                                                                # 3
        why[step] = BEHIND
        alive &= ~step
        step = alive & (((lo > 0) & (Q[2] < lo)) | ((hi > 0) & (Q[2] > hi)))                      # 4
        why[step] = RANGE
        alive &= ~step
        u = cam[1] * (Q[0] / Q[2]) + cam[3]                                                       # 5
        v = cam[2] * (Q[1] / Q[2]) + cam[4]
        step = alive & ~(np.isfinite(u) & np.isfinite(v))                                         # 6
        why[step] = UV
        alive &= ~step
        q = np.rint(Q[2] * cam[0])                                                                # 7
        step = alive & ~((q >= 1) & (q <= 65535))
        why[step] = DEPTH
        alive &= ~step
        assert u.dtype == v.dtype == q.dtype == np.float32
        u, v, q = u[alive], v[alive], q[alive].astype(np.int64)
        xi = np.rint(np.minimum(np.maximum(u, f32(-8)), f32(w + 8))).astype(np.int64)             # 8: ties to even
        yi = np.rint(np.minimum(np.maximum(v, f32(-8)), f32(h + 8))).astype(np.int64)
    wrote = np.zeros(len(q), bool)
    for dy in range(-s.splat, s.splat + 1):                                                       # 9
        for dx in range(-s.splat, s.splat + 1):
            px, py = xi + dx, yi + dy
            inside = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            np.minimum.at(Z, (py[inside], px[inside]), q[inside])
            wrote |= inside
    idx = np.nonzero(alive)[0]
    why[idx[~wrote]] = OUTSIDE
    return np.where(Z == BIG, 0, Z).astype(np.uint16), why


def cull_loop(P0, s):
    """The occlusion test, pixel by pixel as the contract states it: (P, flags)."""
    P0 = np.asarray(P0)
    h, w = P0.shape
    P, flags = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint8)
    rel = f32(s.occl_rel)
    for y in range(h):
        for x in range(w):
            own = int(P0[y, x])
            if own == 0:
                continue
            win = P0[max(y - s.ry, 0):y + s.ry + 1, max(x - s.rx, 0):x + s.rx + 1]
            m = int(win[win != 0].min())
            occluded = bool(rel > 0) and bool(f32(own - m) > rel * f32(m))
            P[y, x] = 0 if occluded else own
            flags[y, x] = HIT | (OCCLUDED if occluded else 0)
    return P, flags


def window_min(P0, rx, ry):
    """m of the contract for every pixel (BIG where the window holds no depth): rows first, then columns"""
    h, w = P0.shape
    K = np.where(P0 == 0, BIG, P0.astype(np.int64))
    pad = np.pad(K, ((0, 0), (rx, rx)), constant_values=BIG)
    rows = np.min([pad[:, j:j + w] for j in range(2 * rx + 1)], axis=0)
    pad = np.pad(rows, ((ry, ry), (0, 0)), constant_values=BIG)
    return np.min([pad[j:j + h, :] for j in range(2 * ry + 1)], axis=0)


def cull(P0, s):
    """cull_loop, vectorised"""
    P0 = np.asarray(P0)
    m = window_min(P0, s.rx, s.ry)
    hit = P0 != 0
    m = np.where(hit, m, 1)
    occluded = hit & bool(f32(s.occl_rel) > 0) & ((P0.astype(np.int64) - m).astype(f32) > f32(s.occl_rel) * m.astype(f32))
    flags = (hit * HIT + occluded * OCCLUDED).astype(np.uint8)
    return np.where(occluded, 0, P0).astype(np.uint16), flags


def lidar(points, s, cam, w, h):
    """The whole stage: (P, P0, flags, hits, occluded) as cvo_fe_project_points returns them."""
    P0, _ = project(points, s, cam, w, h)
    P, flags = cull(P0, s)
    return P, P0, flags, int(np.count_nonzero(flags & HIT)), int(np.count_nonzero(flags & OCCLUDED))


# ---- the settings -------------------------------------------------------------------------------------

SPLATS = (0, 1, 2, 3)
WINDOWS = ((0, 0), (7, 0), (0, 7), (3, 1), (7, 7))
RELS = (0.0, 0.25)
GRID = [(sp, rx, ry, rel) for sp in SPLATS for (rx, ry) in WINDOWS for rel in RELS]       # 40


def rotation(ax, ay, az):
    """a rotation about x, then y, then z (radians), float64, row-major"""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


# a scanner above and beside the camera, tilted: what R and T are for
MOUNT_R = tuple(float(v) for v in rotation(0.05, -0.08, 0.03).astype(np.float32).reshape(-1))
MOUNT_T = (0.12, -0.3, 0.21)


def setting(grid, R=IDENTITY, T=(0.0, 0.0, 0.0), min_range=0.0, max_range=0.0):
    sp, rx, ry, rel = grid
    return Setting(sp, tuple(R), tuple(T), min_range, max_range, rel, rx, ry)


# ---- the cameras --------------------------------------------------------------------------------------

SIZES = ((96, 64), (127, 193))


def exact_cam(w, h):
    """powers of two: a point made for a pixel position lands on it exactly, in float32"""
    return (1024.0, 64.0, 64.0, float(w // 2), float(h // 2))


def plain_cam(w, h):
    """KITTI's shape at the size of the image"""
    return (2000.0, 0.58 * w, 0.58 * w, 0.49 * w - 0.3, 0.47 * h + 0.2)


def lift(u, v, q, cam):
    """the point of an exact camera (R = I, T = 0) that lands on (u, v) with depth value q: exact where u, v are
    multiples of 1/64 and q / 1024 is a float32"""
    u, v, q = np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(q, np.float64)
    z = q / cam[0]
    return np.stack([(u - cam[3]) / cam[1] * z, (v - cam[4]) / cam[2] * z, z], axis=1).astype(np.float32)


def back(u, v, z, cam, s):
    """the LiDAR points that the colour camera sees at (u, v) with depth z metres under the mount of `s`; float64, then
    rounded: they land near (u, v), not on it"""
    pc = np.stack([(u - cam[3]) / cam[1] * z, (v - cam[4]) / cam[2] * z, z], axis=1)
    R, T = np.asarray(s.R, np.float64).reshape(3, 3), np.asarray(s.T, np.float64)
    return ((pc - T) @ R).astype(np.float32)          # R^T (pc - T), row by row


# ---- the scans made on purpose ------------------------------------------------------------------------

def scan_halves(w, h):
    """points landing on k + 0.5 in u and in v, k even and odd, beside points landing on pixel centres, depths all
    different: ties go to even, so (2.5, 3.5) is pixel (2, 4)"""
    cam = exact_cam(w, h)
    us, vs, qs = [], [], []
    k = 0
    for y in range(2, h - 2, 5):
        for x in range(2, w - 2, 5):
            kind = k % 4
            us.append(x + (0.5 if kind in (0, 1) else 0.0))
            vs.append(y + (0.5 if kind in (0, 2) else 0.0))
            qs.append(1024 + 8 * k)
            k += 1
    return lift(us, vs, qs, cam)


def scan_borders(w, h):
    """points whose nearest pixel lies 1, 2, 3 and 4 outside each of the four borders and each corner, on the border
    pixels themselves, and far outside (clamped to 8 outside: beyond any splat)"""
    cam = exact_cam(w, h)
    us, vs, qs = [], [], []
    k = 0
    for d in (0, 1, 2, 3, 4):
        for (u, v) in ((-d, 7 + 3 * d), (w - 1 + d, 9 + 3 * d), (11 + 3 * d, -d), (13 + 3 * d, h - 1 + d),
                       (-d, -d), (w - 1 + d, -d), (-d, h - 1 + d), (w - 1 + d, h - 1 + d)):
            us.append(u); vs.append(v); qs.append(2048 + 16 * k)
            k += 1
    for (u, v) in ((-4000.0, 20.0), (4000.0 + w, 21.0), (22.0, -4000.0), (23.0, 4000.0 + h), (-4000.0, -4000.0)):
        us.append(u); vs.append(v); qs.append(1024 + k)
        k += 1
    return lift(us, vs, qs, cam)


def scan_skips(w, h):
    """one point, at the least, for every step that skips, beside points that are kept: NaN and +-inf in each
    coordinate; z <= 0; u not finite; q at 0, 1, 65535 and 65536"""
    cam = exact_cam(w, h)
    keep = lift([10, 20, 30], [10, 12, 14], [3000, 3100, 3200], cam)
    bad = []
    for c in range(3):
        for val in (np.nan, np.inf, -np.inf):
            p = keep[0].copy()
            p[c] = val
            bad.append(p)
    behind = np.array([[0.1, 0.1, 0.0], [0.1, 0.1, -2.0], [0.0, 0.0, -0.0]], np.float32)
    uv = np.array([[3e38, 0.0, 1.0 / 1024], [0.0, -3e38, 1.0 / 1024]], np.float32)         # x / z overflows: u is inf
    # q = rint(z * 1024): 0.4 -> 0 (skip), 0.5 -> 0 (ties to even: skip), 0.6 -> 1, 1, 65535, 65535.4 -> 65535,
    # 65535.5 -> 65536 (skip), 65536 (skip)
    zs = np.array([0.4, 0.5, 0.6, 1.0, 65535.0, 65535.4, 65535.5, 65536.0]) / 1024.0
    depth = np.stack([np.zeros(8), np.zeros(8), zs], axis=1).astype(np.float32)
    depth[:, 0] = (np.arange(8) * 2 + 40 - cam[3]) / cam[1] * depth[:, 2]               # (side by side in row h/2)
    return np.concatenate([keep, np.array(bad, np.float32), behind, uv, depth])


SKIP_COUNTS = {NOT_FINITE: 9, BEHIND: 3, UV: 2, DEPTH: 4, WROTE: 7, RANGE: 0, OUTSIDE: 0}

RANGE_LIMITS = (1.5, 3.0)


def scan_ranges(w, h):
    """under min_range 1.5 and max_range 3.0, along the axis: the limits themselves (kept), the float32 next below and
    above (skipped), and points far off the axis whose distance |p| is beyond a limit while their Q.z is inside"""
    cam = exact_cam(w, h)
    lo, hi = f32(RANGE_LIMITS[0]), f32(RANGE_LIMITS[1])
    zs = [lo, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(9)), hi, np.nextafter(hi, f32(9)), np.nextafter(hi, f32(0)),
          f32(1.0), f32(3.5), f32(2.0)]
    pts = [[(8 + 6 * k - cam[3]) / cam[1] * float(z), 0.0, float(z)] for k, z in enumerate(zs)]
    # off the axis: Q.z 2.9 and |p| > 3 (kept); Q.z 1.45 and |p| > 1.5 (skipped)
    pts.append([(2 - cam[3]) / cam[1] * 2.9, (3 - cam[4]) / cam[2] * 2.9, 2.9])
    pts.append([(w - 3 - cam[3]) / cam[1] * 1.45, (h - 3 - cam[4]) / cam[2] * 1.45, 1.45])
    return np.array(pts, np.float32)


RANGE_COUNTS = {WROTE: 6, RANGE: 5}


def scan_pile(w, h):
    """many points on one pixel and on its neighbours, depths in no order: the nearest wins, whatever the order"""
    cam = exact_cam(w, h)
    rng = np.random.RandomState(5)
    us = np.concatenate([np.full(60, 31.0), np.full(40, 33.0), rng.randint(28, 37, 60).astype(float)])
    vs = np.concatenate([np.full(60, 17.0), np.full(40, 18.0), rng.randint(14, 22, 60).astype(float)])
    qs = rng.permutation(np.arange(160) * 37 + 1500)
    return lift(us, vs, qs, cam)


def shuffled(points, seed=9):
    return np.asarray(points)[np.random.RandomState(seed).permutation(len(points))]


THRESHOLD_PAIRS = ((7, 0), (0, 7), (3, 1), (1, 3), (7, 7), (4, 0), (8, 8))


def scan_threshold(w, h):
    """occl_rel 0.25 beside a 4000: a 5000 is kept (1000 > 1000.0 is false), a 5001 dropped -- at the offsets of
    THRESHOLD_PAIRS, so that each window of the grid reaches some and not others, and (8, 8) is out of every window's
    reach.  Each pair has a cell of 24 x 16 pixels of its own: at splat 0 no pair is in reach of another.  In the last
    cell a 65535 beside a 60000: a depth like any other."""
    cam = exact_cam(w, h)
    us, vs, qs = [], [], []
    cell = 0
    for (dx, dy) in THRESHOLD_PAIRS:
        for far in (5000, 5001):
            x0, y0 = 1 + 24 * (cell % 4), 1 + 16 * (cell // 4)
            us += [x0, x0 + dx]; vs += [y0, y0 + dy]; qs += [4000, far]
            cell += 1
    x0, y0 = 1 + 24 * (cell % 4), 1 + 16 * (cell // 4)
    us += [x0, x0 + 2]; vs += [y0, y0]; qs += [60000, 65535]
    return lift(us, vs, qs, cam)


def scan_chains(w, h):
    """A = 4000, B = 5001, C = 6253 in a line, 7 apart in a row, 7 apart in a column and 3 apart in a row: B is dropped
    for A, and C for B, which a window around C reaches while it does not reach A.  A cull that has dropped B already
    when it comes to C keeps C."""
    cam = exact_cam(w, h)
    us, vs, qs = [], [], []
    for (x0, y0, dx, dy) in ((5, 5, 7, 0), (40, 5, 0, 7), (60, 40, 3, 0)):
        for k, q in enumerate((4000, 5001, 6253)):
            us.append(x0 + k * dx); vs.append(y0 + k * dy); qs.append(q)
    return lift(us, vs, qs, cam)


def blobs(w, h, seed):
    """which pixels a near object covers: a few rectangles"""
    rng = np.random.RandomState(seed)
    near = np.zeros((h + 16, w + 16), bool)
    for _ in range(6):
        x0, y0 = rng.randint(0, w), rng.randint(0, h)
        near[y0:y0 + rng.randint(5, max(6, h // 2)), x0:x0 + rng.randint(5, max(6, w // 3))] = True
    return near


def scan_clutter(w, h, n, seed, s, cam=None):
    """`n` points of a scene of two layers under the mount of `s`: a background at 2.5 to 6 m and near objects at 1 to
    1.2 m through which half of the points see the background, as a scanner beside the camera does; positions up to 6
    pixels outside the image.  Every step of the arithmetic carries a rounding here."""
    cam = plain_cam(w, h) if cam is None else cam
    rng = np.random.RandomState(seed)
    u, v = rng.uniform(-6, w + 6, n), rng.uniform(-6, h + 6, n)
    near = blobs(w, h, seed)[np.clip(v.astype(int) + 8, 0, h + 15), np.clip(u.astype(int) + 8, 0, w + 15)]
    z = np.where(near & (rng.rand(n) < 0.5), rng.uniform(1.0, 1.2, n), rng.uniform(2.5, 6.0, n))
    return back(u, v, z, cam, s)


COUNTS = (0, 1, 255, 256, 257, 4097)
MOUNT = dict(R=MOUNT_R, T=MOUNT_T)

# name -> (the scan at w x h, the camera at w x h, what of a Setting the case fixes)
MADE = {
    "halves": (scan_halves, exact_cam, {}),
    "borders": (scan_borders, exact_cam, {}),
    "skips": (scan_skips, exact_cam, {}),
    "ranges": (scan_ranges, exact_cam, dict(min_range=RANGE_LIMITS[0], max_range=RANGE_LIMITS[1])),
    "pile": (scan_pile, exact_cam, {}),
    "threshold": (scan_threshold, exact_cam, {}),
    "chains": (scan_chains, exact_cam, {}),
}
MADE_NAMES = list(MADE) + ["clutter-%d" % n for n in COUNTS]
_CACHE = {}


def case(name, size, grid):
    """(points, setting, cam, w, h) of a made case at an image size and a point of the grid"""
    w, h = size
    if name.startswith("clutter-"):
        s = setting(grid, **MOUNT)
        key = (name, size)
        if key not in _CACHE:
            _CACHE[key] = scan_clutter(w, h, int(name[8:]), 11 + w, s)
            _CACHE[key].setflags(write=False)
        return _CACHE[key], s, plain_cam(w, h), w, h
    make, cam, fixed = MADE[name]
    key = (name, size)
    if key not in _CACHE:
        _CACHE[key] = make(w, h)
        _CACHE[key].setflags(write=False)
    return _CACHE[key], setting(grid, **fixed), cam(w, h), w, h


def made(name, size, grid):
    """case() and its reference result, computed once: (points, setting, cam, w, h, (P, P0, flags, hits, occluded))"""
    key = (name, size, grid)
    if key not in _CACHE:
        c = case(name, size, grid)
        out = lidar(*c)
        for a in out[:3]:
            a.setflags(write=False)
        _CACHE[key] = c + (out,)
    return _CACHE[key]


def with_stride(points, floats, fill=np.nan):
    """the scan as records of `floats` float32 (stride 4 * floats bytes): x y z first, the rest what must not be read"""
    points = np.asarray(points, np.float32)
    out = np.full((len(points), floats), fill, np.float32)
    out[:, :3] = points[:, :3]
    return out


# ---- frames on a context ------------------------------------------------------------------------------

ALTERNATING = (300, 0, 4097, 1)


def frame_scans(w, h, s, cam, counts=ALTERNATING, seed=40):
    """one scan per count, each of another scene"""
    return [scan_clutter(w, h, n, seed + k, s, cam) for k, n in enumerate(counts)]


def good_lidars():
    """(max_points, splat, R, T, min_range, max_range, occl_rel, rx, ry, pad_) that cvo_fe_check_lidar accepts"""
    I, Z = IDENTITY, (0.0, 0.0, 0.0)
    return [(1, 0, I, Z, 0.0, 0.0, 0.0, 0, 0, 0), (MAX_POINTS, 3, MOUNT_R, MOUNT_T, 0.5, 80.0, 0.25, 7, 7, 0),
            (130000, 1, MOUNT_R, MOUNT_T, -1.0, -2.0, 0.0, 7, 1, 0), (5, 2, I, Z, 3.0, 0.0, 1e-6, 0, 7, 0),
            (5, 2, I, (1e6, -1e6, 0.0), 0.0, 1e-3, 5.0, 3, 1, 0)]


def bad_lidars():
    """one reason each: {reason: settings}"""
    I, Z = IDENTITY, (0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    shear = (1.0, 0.01, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    mirror = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0)
    return {
        "max_points 0": (0, 0, I, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "max_points above 2^21": (MAX_POINTS + 1, 0, I, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "splat -1": (5, -1, I, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "splat 4": (5, 4, I, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "R not finite": (5, 0, (nan,) + I[1:], Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "T not finite": (5, 0, I, (0.0, inf, 0.0), 0.0, 0.0, 0.0, 0, 0, 0),
        "min_range not finite": (5, 0, I, Z, nan, 0.0, 0.0, 0, 0, 0),
        "max_range not finite": (5, 0, I, Z, 0.0, inf, 0.0, 0, 0, 0),
        "occl_rel not finite": (5, 0, I, Z, 0.0, 0.0, inf, 0, 0, 0),
        "occl_rel negative": (5, 0, I, Z, 0.0, 0.0, -0.25, 0, 0, 0),
        "occl_rx -1": (5, 0, I, Z, 0.0, 0.0, 0.25, -1, 0, 0),
        "occl_rx 8": (5, 0, I, Z, 0.0, 0.0, 0.25, 8, 0, 0),
        "occl_ry -1": (5, 0, I, Z, 0.0, 0.0, 0.25, 0, -1, 0),
        "occl_ry 8": (5, 0, I, Z, 0.0, 0.0, 0.25, 0, 8, 0),
        "max_range equal to min_range": (5, 0, I, Z, 2.0, 2.0, 0.0, 0, 0, 0),
        "max_range below min_range": (5, 0, I, Z, 2.0, 1.0, 0.0, 0, 0, 0),
        "R sheared": (5, 0, shear, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "R a reflection": (5, 0, mirror, Z, 0.0, 0.0, 0.0, 0, 0, 0),
        "pad_ not 0": (5, 0, I, Z, 0.0, 0.0, 0.0, 0, 0, 1),
    }
