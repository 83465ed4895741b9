"""Float64 restatement of the pose score (include/cvo_hip.h cvo_hip_pose_score) on the oracle's member sets:
    inner = sum_A a,  self_fixed = sum_{A_X} a,  self_moving = sum_{A_Y} a,  cos_angle = inner / sqrt(self_fixed self_moving),
    mean_d2 = sum_A a d2 / sum_A a,  fixed_matched / moving_matched = rows of either cloud with a member in A.
A, A_X and A_Y are what the oracle's se_kernel keeps for (x, T.y), (x, x) and (y, y) -- cvo_hip_flow's member rule.
Shared by tests/test_pose_score_cpu.py and tests/test_gpu_pose_score.py."""
import numpy as np


def members(po, p, ell, xa, fa, xb, fb, search):
    """(rows, cols, weights) of the oracle's member set of xa against xb."""
    rp, col, val = po.se_kernel(p, ell, xa, fa, xb, fb, search=search)
    return np.repeat(np.arange(len(xa)), np.diff(rp)), col, val


def sq_dist(xa, xb, rows, cols):
    """Squared distances of the members from the float32 coordinates (the float32 differences, squared and added in
    float64: within an ulp of float32 of the kernels' fma form)."""
    out = np.empty(len(rows))
    for k in range(0, len(rows), 1 << 20):
        e = (np.asarray(xa, np.float32)[rows[k:k + (1 << 20)]] - np.asarray(xb, np.float32)[cols[k:k + (1 << 20)]]).astype(np.float64)
        out[k:k + (1 << 20)] = np.einsum("nk,nk->n", e, e)
    return out


def self_norm(po, p, ell, x, f, search):
    """(sum a, members) of a cloud against itself, untransformed."""
    rows, cols, a = members(po, p, ell, x, f, x, f, search)
    return float(np.sum(a.astype(np.float64))), len(rows)


def score(po, pmode, ell, xf, ff, xm, fm, R, T, search=None):
    """The score's fields (a dict) of the fixed cloud xf against the moving cloud xm at the pose (R, T)."""
    if search is None:
        search = po.SEARCH_DENSE if pmode == po.MODE_MATLAB else po.SEARCH_GRID
    p = po.default_params(pmode)
    y = po.transform(R, T, xm)
    rows, cols, a = members(po, p, ell, xf, ff, y, fm, search)
    a = a.astype(np.float64)
    inner = float(np.sum(a))
    sf, nf = self_norm(po, p, ell, xf, ff, search)
    sm, nm = self_norm(po, p, ell, xm, fm, search)
    d2 = sq_dist(xf, y, rows, cols)
    return dict(inner=inner, self_fixed=sf, self_moving=sm, nnz=len(rows), nnz_fixed=nf, nnz_moving=nm,
                cos_angle=inner / np.sqrt(sf * sm) if sf > 0 and sm > 0 else 0.0,
                mean_d2=float(np.sum(a * d2)) / inner if len(rows) else 0.0,
                fixed_matched=len(np.unique(rows)), moving_matched=len(np.unique(cols)))
