"""The sweep contract of include/cvo_frontend.h (at cvo_fe_lidar_sweep) restated in numpy float32, operation by operation
in the contract's order and with its parentheses: the phase of a point, the move, and then tests/fe_lidar_ref.py's stage on
p'.  numpy's float32 operations are single IEEE operations, rounded once: nothing is fused.  Beside it the float64
side: the closed-form Exp and Log of SE(3), the helper cvo_fe_lidar_twist in numpy, and a simulator -- a scanner with a
constant twist in a static scene of planes, each ray measured at its own phase from the pose of that phase -- that also
gives the same surface points as seen from the pose at s_ref.  And the scans, sweeps and twists made on purpose that
tests/test_fe_lidar_sweep_cpu.py (what they reach, which mutants they tell) and tests/test_gpu_fe_lidar_sweep.py (the
device against this file, by bits and bytes) share."""
from collections import namedtuple

import numpy as np

import fe_lidar_ref as K

f32 = np.float32
TIME_F32, TIME_U32, AZIMUTH = 1, 2, 3
MAX_ROTATION, MAX_TRANSLATION = 1.0, 64.0

# cvo_fe_lidar_sweep without pad_
Sweep = namedtuple("Sweep", "mode time_offset time_origin time_scale phase0 direction s_ref")


def to_struct(F, sw):
    return None if sw is None else F.LidarSweep(*sw)


def _fact(k):
    return f32(np.prod(np.arange(1, k + 1, dtype=np.float64)))


# CVO_FE_SWEEP_ATAN_C0 .. C5, and the series' coefficients: float32 divisions of float32 numbers, as the header's
ATAN = tuple(f32(v) for v in (1.591517329e-01, -5.294376612e-02, 3.082358837e-02, -1.856560260e-02, 8.407119662e-03,
                              -1.873333240e-03))
SER_A = tuple(f32((-1) ** k) / _fact(2 * k + 1) for k in range(6))
SER_B = tuple(f32((-1) ** k) / _fact(2 * k + 2) for k in range(6))
SER_C = tuple(f32((-1) ** k) / _fact(2 * k + 3) for k in range(5))


def horner(coef, t):
    """(((c[n]*t + c[n-1])*t + ...)*t + c[0]"""
    acc = coef[-1] * t + coef[-2]
    for c in coef[-3::-1]:
        acc = acc * t + c
    return acc


def time_words(records, sw):
    """the raw time word of every record, as uint32"""
    rec = np.asarray(records, f32)
    return np.ascontiguousarray(rec[:, sw.time_offset // 4]).view(np.uint32)


def turn_fraction(x, y):
    """q of the azimuth mode: atan2(y, x) / 2 pi in (-0.5, 0.5], by the contract's polynomial and fix-ups"""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    ax, ay = np.abs(x), np.abs(y)
    lo, hi = np.minimum(ax, ay), np.maximum(ax, ay)
    with np.errstate(all="ignore"):
        r = np.where(hi > 0, lo / hi, f32(0)).astype(f32)
    r2 = r * r
    q = horner(ATAN, r2)
    q = q * r
    q = np.where(ay > ax, f32(0.25) - q, q)
    q = np.where(x < 0, f32(0.5) - q, q)
    q = np.where(y < 0, -q, q)
    assert q.dtype == np.float32
    return q


def phase(records, sw):
    """(s as float32, alive): the phase of every record, and which records have one (step 1 passed, the time finite)"""
    rec = np.asarray(records, f32)
    rec = rec if rec.ndim == 2 else np.zeros((0, 4), f32)
    x, y, z = rec[:, 0], rec[:, 1], rec[:, 2]
    alive = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        if sw.mode == TIME_F32:
            t = time_words(rec, sw).view(f32)
            alive &= np.isfinite(t)
            s = (t - f32(sw.time_origin)) * f32(sw.time_scale)
            s = np.minimum(np.maximum(s, f32(0)), f32(1))
        elif sw.mode == TIME_U32:
            s = time_words(rec, sw).astype(f32) * f32(sw.time_scale)
            s = np.minimum(np.maximum(s, f32(0)), f32(1))
        else:
            s = f32(sw.direction) * turn_fraction(x, y) + f32(sw.phase0)
            s = s - np.floor(s)
    assert s.dtype == np.float32
    return s, alive


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def move(p, s, s_ref, twist):
    """p' of the contract for points p (n x 3 float32) at phases s under the twist (w then v): n x 3 float32"""
    p = np.asarray(p, f32)
    tw = np.asarray(twist, f32)
    with np.errstate(all="ignore"):
        a = s - f32(s_ref)
        w = [a * tw[k] for k in range(3)]
        tau = [a * tw[3 + k] for k in range(3)]
        t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        A, B, C = horner(SER_A, t2), horner(SER_B, t2), horner(SER_C, t2)
        pk = [p[:, 0], p[:, 1], p[:, 2]]
        c1 = cross(w, pk)
        c2 = cross(w, c1)
        d1 = cross(w, tau)
        d2 = cross(w, d1)
        out = [((pk[k] + A * c1[k]) + B * c2[k]) + ((tau[k] + B * d1[k]) + C * d2[k]) for k in range(3)]
    out = np.stack(out, axis=1)
    assert out.dtype == np.float32
    return out


def sweep(records, sw, twist):
    """(s, p') as cvo_fe_project_points_sweep returns them: NaN for a record without a phase"""
    rec = np.asarray(records, f32)
    rec = rec if rec.ndim == 2 else np.zeros((0, 4), f32)
    s, alive = phase(rec, sw)
    moved = move(rec[:, :3], s, sw.s_ref, twist)
    s = np.where(alive, s, f32(np.nan))
    moved = np.where(alive[:, None], moved, f32(np.nan))
    return s, moved


def lidar_sweep(records, setting, cam, w, h, sw, twist):
    """The whole stage under a sweep: (P, P0, flags, hits, occluded, s, p')"""
    s, moved = sweep(records, sw, twist)
    return K.lidar(moved, setting, cam, w, h) + (s, moved)


# ---- float64 ------------------------------------------------------------------------------------------

def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(xi):
    """Exp of a twist (w then v) as a 4 x 4 matrix, closed form"""
    xi = np.asarray(xi, np.float64)
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = skew(w)
    if th < 1e-9:
        A, B, Cc = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * W + B * W @ W
    T[:3, 3] = (np.eye(3) + B * W + Cc * W @ W) @ v
    return T


def log_se3(T):
    """the twist (w then v) of a 4 x 4 rigid motion whose angle is below pi"""
    R, t = T[:3, :3], T[:3, 3]
    ax = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn, cs = np.linalg.norm(ax), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(sn, cs)
    w = ax * (1.0 + th * th / 6 if th < 1e-6 else th / sn)
    W = skew(w)
    # (1 - (th/2) cot(th/2)) / th^2, from the angle itself: 1 - cos from the matrix loses what the matrix's rounding leaves
    k = 1.0 / 12 + th * th / 720 + th ** 4 / 30240 if th < 1e-2 else (1 - 0.5 * th / np.tan(0.5 * th)) / th ** 2
    return np.concatenate([w, (np.eye(3) - 0.5 * W + k * W @ W) @ t])


def move64(p, s, s_ref, twist):
    """Exp((s - s_ref) * twist) p by the closed form in float64, on the float32 inputs"""
    p, s = np.asarray(p, f32).astype(np.float64), np.asarray(s, f32).astype(np.float64)
    tw = np.asarray(twist, f32).astype(np.float64)
    out = np.empty_like(p)
    for i in range(len(p)):
        T = exp_se3((s[i] - float(f32(s_ref))) * tw)
        out[i] = T[:3, :3] @ p[i] + T[:3, 3]
    return out


def mount(setting):
    """X = [R | T] of a Setting: the scanner's pose in the camera's frame"""
    X = np.eye(4)
    X[:3, :3] = np.asarray(setting.R, f32).astype(np.float64).reshape(3, 3)
    X[:3, 3] = np.asarray(setting.T, f32).astype(np.float64)
    return X


def lidar_twist64(transform, setting, sweep_fraction):
    """cvo_fe_lidar_twist in numpy: `transform` takes coordinates in the earlier camera's frame to the later one's, so
    the camera moved by its inverse; conjugated with the mount, the logarithm, times sweep_fraction"""
    M = np.linalg.inv(np.asarray(transform, np.float64))
    X = mount(setting)
    return log_se3(np.linalg.inv(X) @ M @ X) * float(f32(sweep_fraction))


def transform_of(twist, setting, sweep_fraction):
    """the `transform` a registration returns for a scanner that moves by `twist` per sweep, constantly: the inverse of
    the camera's motion X Exp(twist / sweep_fraction) X^-1 over a frame interval"""
    X = mount(setting)
    return np.linalg.inv(X @ exp_se3(np.asarray(twist, np.float64) / sweep_fraction) @ np.linalg.inv(X))


# a static scene: planes n . X = c in the world (a floor, a wall in front, two at the sides, one behind), metres
PLANES = ((np.array([0.0, 0.0, 1.0]), -1.7), (np.array([1.0, 0.0, 0.0]), 30.0), (np.array([0.0, 1.0, 0.0]), 12.0),
          (np.array([0.0, 1.0, 0.0]), -9.0), (np.array([1.0, 0.0, 0.0]), -25.0), (np.array([0.0, 0.0, 1.0]), 40.0))


def simulate(n, twist, sw, seed=3, T0=None, seam=1e-3):
    """A spinning scanner (x forward, z up) whose pose at phase s is T0 Exp(s twist), in the scene of PLANES: `n` rays,
    azimuths all around, elevations of +-15 degrees, the ray of azimuth a fired at the phase the sweep `sw` gives that
    azimuth in its azimuth mode (no ray within `seam` turns of the seam).  Returns (p: the points as measured, in the
    scanner's frame of their own phase, float64; s: their phases, float64; p_ref: the same surface points in the
    scanner's frame at s_ref)."""
    rng = np.random.RandomState(seed)
    T0 = np.eye(4) if T0 is None else T0
    turn = rng.uniform(-0.5 + seam, 0.5 - seam, n)               # the azimuth in turns, atan2(y, x) / 2 pi
    s = sw.direction * turn + sw.phase0
    s = s - np.floor(s)
    keep = (s > seam) & (s < 1 - seam)
    turn, s = turn[keep], s[keep]
    el = rng.uniform(-0.26, 0.26, len(turn))
    d = np.stack([np.cos(el) * np.cos(2 * np.pi * turn), np.cos(el) * np.sin(2 * np.pi * turn), np.sin(el)], axis=1)
    p, p_ref = np.empty_like(d), np.empty_like(d)
    to_ref = np.linalg.inv(T0 @ exp_se3(float(sw.s_ref) * np.asarray(twist, np.float64)))
    for i in range(len(d)):
        T = T0 @ exp_se3(s[i] * np.asarray(twist, np.float64))
        o, dw = T[:3, 3], T[:3, :3] @ d[i]
        best = np.inf
        for nrm, c in PLANES:
            den = nrm @ dw
            if abs(den) > 1e-9:
                r = (c - nrm @ o) / den
                if 0.5 < r < best:
                    best = r
        p[i] = best * d[i]
        p_ref[i] = to_ref[:3, :3] @ (o + best * dw) + to_ref[:3, 3]
    ok = np.isfinite(p).all(axis=1)
    return p[ok], s[ok], p_ref[ok]


# ---- scans, sweeps and twists made on purpose ---------------------------------------------------------

COUNTS = K.COUNTS
SIZES = K.SIZES
# (floats per record, the time word's index): strides 16 and 32, the time word at offset 12 and at stride - 4
LAYOUTS = ((4, 3), (8, 3), (8, 7))
TWISTS = {
    "turn": (0.10, -0.20, 0.15, 0.5, -0.3, 1.0),
    "unit": (0.0, 1.0, 0.0, 0.2, 0.1, -0.4),                     # |w| = 1 exactly
    "zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "shift": (0.0, 0.0, 0.0, -0.6, 0.25, 0.8),
}
S_REF = 0.5


def sweep_of(mode, layout=(4, 3), s_ref=S_REF, direction=1, phase0=0.25):
    if mode == TIME_F32:
        return Sweep(mode, 4 * layout[1], 1000.0, 8.0, 0.0, 0, s_ref)           # seconds, a sweep of 1/8 s from t = 1000
    if mode == TIME_U32:
        return Sweep(mode, 4 * layout[1], 0.0, 1e-8, 0.0, 0, s_ref)             # nanoseconds, a sweep of 0.1 s
    return Sweep(mode, 0, 0.0, 0.0, phase0, direction, s_ref)


def records_of(points, sw, layout=(4, 3), seed=1):
    """`points` as records of layout[0] float32 with a time word at index layout[1] (NaN elsewhere: not to be read):
    phases all over [-0.1, 1.1], so that both ends clamp; and in front of them the hostile records of the mode"""
    points = np.asarray(points, f32)[:, :3]
    n = len(points)
    rng = np.random.RandomState(seed + n)
    rec = K.with_stride(points, layout[0])
    ph = rng.uniform(-0.1, 1.1, n)
    words = rec[:, layout[1]].view(np.uint32)
    if sw.mode == TIME_F32:
        rec[:, layout[1]] = (sw.time_origin + ph / sw.time_scale).astype(f32)
        hostile = [np.nan, np.inf, -np.inf, sw.time_origin + sw.s_ref / sw.time_scale, 0.0, 3e38, -3e38]
        for k, t in enumerate(hostile[:n]):
            rec[k, layout[1]] = f32(t)
    elif sw.mode == TIME_U32:
        words[:] = np.clip(ph, 0, None) / sw.time_scale
        hostile = [0xFFFFFFFF, 0, int(round(sw.s_ref / sw.time_scale)), 0x7FC00000, 0x7F800000, 1, 0x80000000]
        for k, t in enumerate(hostile[:n]):
            words[k] = t
    else:
        # x = y = 0, each axis in both directions, both diagonals' ties, and -0
        front = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1), (-0.0, 1), (1, -0.0)]
        for k, (x, y) in enumerate(front[:n]):
            rec[k, 0], rec[k, 1] = f32(x) * abs(rec[k, 2]) * f32(0.01), f32(y) * abs(rec[k, 2]) * f32(0.01)
    return rec


def case(mode, n, size, layout=(4, 3), twist="turn", grid=(1, 7, 1, 0.25), s_ref=S_REF, direction=1):
    """(records, setting, cam, w, h, sweep, twist) of a made case"""
    w, h = size
    s = K.setting(grid, **K.MOUNT)
    cam = K.plain_cam(w, h)
    sw = sweep_of(mode, layout, s_ref, direction)
    pts = K.scan_clutter(w, h, n, 17 + w + mode, s, cam)
    rec = records_of(pts, sw, layout) if mode != AZIMUTH else records_of(pts, sw, (layout[0], layout[1]))
    return rec, s, cam, w, h, sw, np.asarray(TWISTS[twist], f32)


_CACHE = {}


def made(mode, n, size, layout=(4, 3), twist="turn", grid=(1, 7, 1, 0.25), s_ref=S_REF, direction=1):
    """case() and its reference result, computed once"""
    key = (mode, n, size, layout, twist, grid, s_ref, direction)
    if key not in _CACHE:
        c = case(*key)
        out = lidar_sweep(*c)
        for a in (c[0],) + out[:3] + out[5:]:
            a.setflags(write=False)
        _CACHE[key] = c + (out,)
    return _CACHE[key]


def good_sweeps():
    return [Sweep(TIME_F32, 12, 1000.0, 10.0, 0.0, 0, 0.5), Sweep(TIME_F32, 28, -3.5, -1e-3, 0.0, 0, 0.0),
            Sweep(TIME_U32, 12, 0.0, 1e-8, 0.0, 0, 1.0), Sweep(TIME_U32, 4096, 0.0, 1.0, 0.5, 0, 0.25),
            Sweep(AZIMUTH, 0, 0.0, 0.0, 0.0, 1, 0.5), Sweep(AZIMUTH, 7, 0.0, 5.0, 0.999, -1, 0.0)]


def bad_sweeps():
    """one reason each: {reason: (mode, time_offset, time_origin, time_scale, phase0, direction, s_ref, pad_)}"""
    nan, inf = float("nan"), float("inf")
    return {
        "mode 0": (0, 12, 0.0, 10.0, 0.0, 0, 0.5, 0),
        "mode 4": (4, 12, 0.0, 10.0, 0.0, 0, 0.5, 0),
        "time_offset 8": (TIME_F32, 8, 0.0, 10.0, 0.0, 0, 0.5, 0),
        "time_offset 14": (TIME_U32, 14, 0.0, 10.0, 0.0, 0, 0.5, 0),
        "time_offset negative": (TIME_U32, -4, 0.0, 10.0, 0.0, 0, 0.5, 0),
        "time_scale 0": (TIME_F32, 12, 0.0, 0.0, 0.0, 0, 0.5, 0),
        "time_scale not finite": (TIME_U32, 12, 0.0, inf, 0.0, 0, 0.5, 0),
        "time_origin not finite": (TIME_F32, 12, nan, 10.0, 0.0, 0, 0.5, 0),
        "time_origin under uint32": (TIME_U32, 12, 1.0, 10.0, 0.0, 0, 0.5, 0),
        "time_origin under azimuth": (AZIMUTH, 0, 1.0, 0.0, 0.0, 1, 0.5, 0),
        "direction under a field mode": (TIME_F32, 12, 0.0, 10.0, 0.0, 1, 0.5, 0),
        "direction 0 under azimuth": (AZIMUTH, 0, 0.0, 0.0, 0.0, 0, 0.5, 0),
        "direction 2": (AZIMUTH, 0, 0.0, 0.0, 0.0, 2, 0.5, 0),
        "phase0 1": (AZIMUTH, 0, 0.0, 0.0, 1.0, 1, 0.5, 0),
        "phase0 negative": (AZIMUTH, 0, 0.0, 0.0, -0.1, 1, 0.5, 0),
        "phase0 not finite": (AZIMUTH, 0, 0.0, 0.0, nan, 1, 0.5, 0),
        "s_ref above 1": (AZIMUTH, 0, 0.0, 0.0, 0.0, 1, 1.5, 0),
        "s_ref negative": (TIME_F32, 12, 0.0, 10.0, 0.0, 0, -0.01, 0),
        "s_ref not finite": (TIME_F32, 12, 0.0, 10.0, 0.0, 0, nan, 0),
        "pad_ not 0": (AZIMUTH, 0, 0.0, 0.0, 0.0, 1, 0.5, 1),
    }


def bad_twists():
    nan, inf = float("nan"), float("inf")
    return {
        "w not finite": (nan, 0, 0, 0, 0, 0), "v not finite": (0, 0, 0, 0, inf, 0),
        "|w| above 1": (0.8, 0.7, 0, 0, 0, 0), "|v| above 64": (0, 0, 0, 40.0, 40.0, 40.0),
        "w just above 1": (float(np.nextafter(f32(1), f32(2))), 0, 0, 0, 0, 0),
    }


# frames on a context: the count and the twist both change from frame to frame
FRAME_COUNTS = (300, 0, 4097, 1)
FRAME_TWISTS = ("turn", "shift", "zero", "unit")
