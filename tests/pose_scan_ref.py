"""Float64 restatement of the pose scan (include/cvo_hip.h cvo_hip_pose_scan): for each candidate pose the score of
tests/pose_score_ref.py on the oracle's member sets, reduced to the entry's fields, plus ``best`` by the header's rule.
Also the inputs the CPU and the GPU tests of the scan share: the scenario that motivates it (a pair displaced beyond
the kernel's reach and a coarse grid of candidate poses) and the list of poses of the accuracy tests.
Shared by tests/test_pose_scan_cpu.py and tests/test_gpu_pose_scan.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_score_ref as ref  # noqa: E402

U = 2.0 ** -53


def gamma(n):
    """The bound of a float64 sum of n terms in any order: n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def best_of(inner, nnz):
    """Index of the largest inner among the poses with members, the smallest such index if several share it; -1 if none."""
    best, top = -1, 0.0
    for k in range(len(inner)):
        if nnz[k] > 0 and (best < 0 or inner[k] > top):
            best, top = k, inner[k]
    return best


def scan(po, pmode, ell, xf, ff, xm, fm, Rs, Ts, search=None):
    """The scan's fields (a dict: arrays over the poses, the summary's scalars) of the fixed cloud xf against the moving
    cloud xm at the poses (Rs[k], Ts[k]).  Each entry is pose_score_ref.score's of the same name (the norms of the two
    clouds, which do not depend on the pose, are computed once)."""
    if search is None:
        search = po.SEARCH_DENSE if pmode == po.MODE_MATLAB else po.SEARCH_GRID
    p = po.default_params(pmode)
    sf, nf = ref.self_norm(po, p, ell, xf, ff, search)
    sm, nm = ref.self_norm(po, p, ell, xm, fm, search)
    n = len(Rs)
    inner, mean_d2, nnz = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    for k in range(n):
        y = po.transform(Rs[k], Ts[k], xm)
        rows, cols, a = ref.members(po, p, ell, xf, ff, y, fm, search)
        a = a.astype(np.float64)
        nnz[k] = len(rows)
        if len(rows):
            inner[k] = float(np.sum(a))
            mean_d2[k] = float(np.sum(a * ref.sq_dist(xf, y, rows, cols))) / inner[k]
    cos = inner / np.sqrt(sf * sm) if sf > 0 and sm > 0 else np.zeros(n)
    return dict(inner=inner, cos_angle=cos, mean_d2=mean_d2, nnz=nnz, self_fixed=sf, self_moving=sm, nnz_fixed=nf,
                nnz_moving=nm, count=n, best=best_of(inner, nnz))


def rot(axis, th):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rot_y(deg):
    return rot([0.0, 1.0, 0.0], np.deg2rad(deg))


# The scenario that motivates the scan: (seed of data.synthetic_pair(3000, 3000), yaw in degrees about y, shift g) and what
# the oracle gives for it at ell = 0.15 with the cvo defaults -- poses of the 343-pose grid with an empty member set,
# index of the winner IN THE GRID, its cosine and the runner-up's, iterations of align() from the winner, the cosine of
# the final pose.  From the identity the oracle's align() runs one iteration on an empty member set.
SCENARIOS = [
    dict(seed=7, yaw=18.0, g=(0.35, 0.0, -0.25), empty=275, winner=60, cos=0.6450, second=0.5971, iters=57, final=0.9652),
    dict(seed=13, yaw=-23.0, g=(-0.3, 0.05, 0.4), empty=271, winner=316, cos=0.6928, second=0.5166, iters=123, final=0.9675),
]
SCENARIO_ELL = 0.15


def scenario_clouds(pkg, sc):
    """The displaced pair: the moving cloud of the synthetic pair taken through xm = (xm0 - g) G, float64 in between."""
    xf, ff, xm0, fm = pkg.data.synthetic_pair(3000, 3000, seed=sc["seed"])
    G = rot_y(sc["yaw"])
    xm = ((xm0.astype(np.float64) - np.asarray(sc["g"], np.float64)) @ G).astype(np.float32)
    return xf, ff, xm, fm


def scenario_grid():
    """343 candidate poses: yaw about y -30 .. 30 step 10 degrees (outer) x tx -0.6 .. 0.6 step 0.2 x tz likewise (inner)."""
    steps = [-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6]
    Rs, Ts = [], []
    for a in (-30.0, -20.0, -10.0, 0.0, 10.0, 20.0, 30.0):
        for tx in steps:
            for tz in steps:
                Rs.append(rot_y(a))
                Ts.append((tx, 0.0, tz))
    return np.asarray(Rs, np.float32), np.asarray(Ts, np.float32)


def accuracy_poses(R0, T0):
    """The 25 poses of the accuracy tests: (R0, T0), the identity, 20 perturbations of (R0, T0) (rotation 2 .. 10 degrees
    about random axes, translation 3 .. 15 cm; PCG64 seed 20260), two poses far away (every member set empty) and one
    rotation by 170 degrees."""
    rng = np.random.Generator(np.random.PCG64(20260))
    R0 = np.asarray(R0, np.float64)
    T0 = np.asarray(T0, np.float64)
    Rs, Ts = [R0, np.eye(3)], [T0, np.zeros(3)]
    for _ in range(20):
        dR = rot(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 10.0)))
        d = rng.normal(size=3)
        Rs.append(R0 @ dR)
        Ts.append(T0 + d / np.linalg.norm(d) * rng.uniform(0.03, 0.15))
    Rs += [np.eye(3), rot([0.0, 0.0, 1.0], 0.3)]
    Ts += [np.array([50.0, -20.0, 10.0]), np.array([-7.0, 300.0, 2.0])]
    Rs.append(rot([0.2, 1.0, 0.1], np.deg2rad(170.0)))
    Ts.append(np.array([0.05, 0.0, -0.02]))
    return np.asarray(Rs, np.float32), np.asarray(Ts, np.float32)
