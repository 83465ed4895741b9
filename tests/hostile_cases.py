"""Hostile geometry for the bounds the library skips work by: the float32 slack of the MFMA pre-filter, the bounding-sphere
cull of the 64-point Morton runs, the travel bounds that keep a tile list or a candidate record alive.  Named cloud pairs
on top of data.synthetic_pair(1500, 1300, seed=21), every shift done in float64 and rounded to float32 once, and poses
that rotate ABOUT THE FIXED CLOUD'S BOX CENTRE (a rotation about the origin moves a cloud 1.5 km away by metres and empties
A).  Shared by tests/test_hostile_cpu.py, tests/test_gpu_hostile.py and tools/gpu_soak.py.  A plain module; no test lives here.

    far150 / far600 / far1500   both clouds + (80, -120, 60) / (300, -500, 200) / (800, -1200, 600): coordinates whose ulp
                                (8e-6 .. 1.2e-4 m) is what apply_tf's rounding costs the cull's spheres and the filter
    far3700                     both clouds + (2000, -3000, 1500): ulp 2.4e-4 m.  Not in NAMES (which multiplies every hostile test):
                                reached through FAR_REUSE by the registrations that re-use lists far out (tests/test_reuse_cpu.py,
                                tests/test_gpu_reuse_far.py), 40 iterations each with the break tests off (long_params)
    blob                        both x 0.08 + (0, 0, 1.2): everything within reach of everything -- dense tiles, 700 000 members;
                                with the lists started small (test switch "list_init") they overflow and grow
    dup                         the first third of fixed and the first half of moving once more: ties in `best`, equal keys
    plane                       z = 1.5: no extent on one axis (the Morton key's inv = 0 path)
    point                       300 copies of one point against 200 copies of it + 0.01: no extent on any axis
    unequal                     1500 against the first 32
    tiny_1x1 / _1x700 / _64x1   a handful of points: fewer rows than a wave, than a tile
    edge_NxM                    N, M around 64 (a run), 256 (a tile / a block): the densest patch of either cloud
    jump                        moving + (0.05, -0.04, 0.06): lists die young, re-use ends in a rebuild
"""
import numpy as np

BASE = (1500, 1300, 21)
FAR = {"far150": (80.0, -120.0, 60.0), "far600": (300.0, -500.0, 200.0), "far1500": (800.0, -1200.0, 600.0)}
FAR_REUSE = {"far3700": (2000.0, -3000.0, 1500.0)}
REUSE_NAMES = tuple(FAR) + tuple(FAR_REUSE)   # the registrations kept running while they re-use lists
REUSE_ITERATIONS = 40
EDGE_SIZES = (63, 64, 65, 255, 256, 257)
# every size once as n and once as m, a boundary of one kind against a boundary of the other, and four pairs at one boundary
# on both sides -- 10 of the 36 pairs of the product: every pair costs six primitive tests, two scans and two registrations
# with four option settings each on the GPU, and the suite runs again for every later change
EDGE_PAIRS = tuple(zip(EDGE_SIZES, EDGE_SIZES[::-1])) + ((64, 64), (256, 256), (65, 63), (257, 255))
ELLS = (0.15, 0.06, 0.03)
THETAS = (0.0, 1e-4, 1e-3, 0.02)
SHIFTS = ((0.0, 0.0, 0.0), (0.002, -0.001, 0.003))
AXIS = (0.3, -0.5, 0.8)

NAMES = tuple(FAR) + ("blob", "dup", "plane", "point", "unequal", "tiny_1x1", "tiny_1x700", "tiny_64x1") + \
    tuple("edge_%dx%d" % nm for nm in EDGE_PAIRS) + ("jump",)


def _shift(x, off, scale=1.0):
    return (x.astype(np.float64) * scale + np.asarray(off, np.float64)).astype(np.float32)


def _patch(x, f, k):
    """The k points nearest to the cloud's median point: a patch at the cloud's full density."""
    d = np.linalg.norm(x.astype(np.float64) - np.median(x.astype(np.float64), axis=0), axis=1)
    keep = np.sort(np.argsort(d, kind="stable")[:k])
    return x[keep], f[keep]


def clouds(data, name, acvo=False):
    """(xf, ff, xm, fm) of a named case, float32, C-contiguous."""
    return shape(name, *data.synthetic_pair(*BASE[:2], seed=BASE[2], acvo=acvo))


def shape(name, xf, ff, xm, fm):
    """The named case made of any pair of clouds (tools/gpu_soak.py applies the kinds to random pairs)."""
    if name in FAR or name in FAR_REUSE:
        off = FAR[name] if name in FAR else FAR_REUSE[name]
        xf, xm = _shift(xf, off), _shift(xm, off)
    elif name == "blob":
        xf, xm = _shift(xf, (0.0, 0.0, 1.2), 0.08), _shift(xm, (0.0, 0.0, 1.2), 0.08)
    elif name == "dup":
        xf, ff = np.concatenate([xf, xf[:len(xf) // 3]]), np.concatenate([ff, ff[:len(ff) // 3]])
        xm, fm = np.concatenate([xm, xm[:len(xm) // 2]]), np.concatenate([fm, fm[:len(fm) // 2]])
    elif name == "plane":
        xf, xm = xf.copy(), xm.copy()
        xf[:, 2] = 1.5
        xm[:, 2] = 1.5
    elif name == "point":
        xf, ff = np.repeat(xf[:1], 300, axis=0), np.repeat(ff[:1], 300, axis=0)
        xm, fm = np.repeat(_shift(xf[:1], (0.01, 0.01, 0.01)), 200, axis=0), np.repeat(ff[:1], 200, axis=0)
    elif name == "unequal":
        xm, fm = xm[:32], fm[:32]
    elif name.startswith("tiny_") or name.startswith("edge_"):
        n, m = (int(v) for v in name.split("_")[1].split("x"))
        xf, ff = _patch(xf, ff, n)
        xm, fm = _patch(xm, fm, m)
    elif name == "jump":
        xm = _shift(xm, (0.05, -0.04, 0.06))
    else:
        raise KeyError(name)
    return tuple(np.ascontiguousarray(a, np.float32) for a in (xf, ff, xm, fm))


def rot(axis, th):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def box_centre(x):
    x = np.asarray(x, np.float64)
    return 0.5 * (x.min(axis=0) + x.max(axis=0))


def about(c, R, t=(0.0, 0.0, 0.0)):
    """The pose (R, T) that rotates by R about the point c and then shifts by t: T = (I - R) c + t, float64, rounded once."""
    R = np.asarray(R, np.float64)
    T = (np.eye(3) - R) @ np.asarray(c, np.float64) + np.asarray(t, np.float64)
    return R.astype(np.float32), T.astype(np.float32)


def poses(xf):
    """[(label, R, T)]: the rotations THETAS about the fixed cloud's box centre, without and with the small shift."""
    c = box_centre(xf)
    out = []
    for th in THETAS:
        for t in SHIFTS:
            R, T = about(c, rot(AXIS, th), t)
            out.append(("th%g%s" % (th, "+t" if any(t) else ""), R, T))
    return out


def scan_poses(xf, accuracy_poses):
    """pose_scan_ref.accuracy_poses re-centred: each of its poses (R, t) becomes the rotation R about the fixed cloud's box
    centre followed by t."""
    c = box_centre(xf)
    Rs, Ts = accuracy_poses(rot(AXIS, 0.02), np.asarray(SHIFTS[1]))
    out = [about(c, R, t) for R, t in zip(Rs.astype(np.float64), Ts.astype(np.float64))]
    return np.asarray([o[0] for o in out], np.float32), np.asarray([o[1] for o in out], np.float32)


# ---- the extremal stream of the cull (tests/test_gpu_hostile.py; tests/cpp/cull_host.cpp draws the same kind of trial)
CULL_CLASSES = (((0.0, 0.0, 1.5), -3e-3, 1e-4),
                ((80.0, -120.0, 60.0), -1e-4, 3e-5),
                ((300.0, -500.0, 200.0), -4e-4, 1e-4),
                ((800.0, -1200.0, 600.0), -1e-3, 3e-4),
                ((2000.0, -3000.0, 1500.0), -3e-3, 1e-3))
CULL_THETA_MAX = (3e-4, 1e-3, 3e-3)


def cull_trial(rng, offset, gl, gh, theta_max, tau):
    """One trial: two collinear runs of 64 points, the nearest end points sqrt(tau) (1 + U(gl, gh)) apart at the pose.
    Returns (xf, xm, R, T), float32; xm = fl32(R Y + T) with Y the wanted positions, so the pose (R, T) brings it back."""
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    O = np.asarray(offset, np.float64) + rng.uniform(-1.0, 1.0, 3)
    s = np.linspace(-0.1, 0.1, 64)
    g = np.sqrt(tau) * (1.0 + rng.uniform(gl, gh))
    X = O + s[:, None] * d
    Y = O + (0.1 + g + 0.1 + s)[:, None] * d
    R = rot(rng.normal(size=3), theta_max * 10.0 ** rng.uniform(-1.0, 0.0))
    T = rng.normal(0.0, 0.02, 3)
    return X.astype(np.float32), (Y @ R.T + T).astype(np.float32), R.astype(np.float32), T.astype(np.float32)


# ---- registrations that keep running (tests/test_reuse_cpu.py, tests/test_gpu_reuse_far.py)
def long_params(p):
    """The parameters (the library's or the oracle's) with both break tests off and REUSE_ITERATIONS iterations: from the identity
    the far* cases otherwise stop after 1 - 7 iterations, before any list is re-used.  cvo then walks its whole length-scale
    schedule, 0.15 -> 0.03; acvo runs from 0.10 down to ell_min."""
    p.eps = np.float32(0.0)
    p.eps_2 = np.float32(0.0)
    p.max_iter = REUSE_ITERATIONS
    return p


_LONG_ALIGN = {}


def oracle_long_align(po, data, name, acvo, search=None):
    """(iterations, trace, state bytes) of the oracle's registration of a REUSE_NAMES case under long_params; computed once per
    (case, mode, search) and shared."""
    search = po.SEARCH_GRID if search is None else search
    key = (name, acvo, search)
    if key not in _LONG_ALIGN:
        p = long_params(po.default_params(po.MODE_ACVO if acvo else po.MODE_CVO))
        st = po.init_state(p)
        n_or, tr = po.align(p, st, *clouds(data, name, acvo), search=search, trace_cap=REUSE_ITERATIONS)
        _LONG_ALIGN[key] = (n_or, tr, bytes(st))
    return _LONG_ALIGN[key]
