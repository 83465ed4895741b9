"""Float64 restatement of the pose Hessian of the CVO objective (include/cvo_hip.h cvo_hip_pose_hessian), written in the
definition's own terms: per member r = y - x, J = [[y]x, -I], u = J^T r,
    grad a = -(a / l^2) u,    hess a = (a / l^4) u u^T - (a / l^2) (J^T J + S).
Shared by tests/test_pose_hessian_cpu.py (which pins it against finite differences) and tests/test_gpu_pose_hessian.py."""
import numpy as np


def skew(v):
    """[v]x for an (n, 3) array: (n, 3, 3)."""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1),
                     np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], 1)


def member_terms(x, y, a, ell):
    """Per-member gradient (n, 6) and Hessian (n, 6, 6) terms, float64."""
    x, y, a = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(a, np.float64)
    n, l2 = len(a), float(ell) ** 2
    eye = np.broadcast_to(np.eye(3), (n, 3, 3))
    r = y - x
    J = np.concatenate([skew(y), -eye], 2)                      # (n, 3, 6)
    u = np.einsum("nki,nk->ni", J, r)
    JtJ = np.einsum("nki,nkj->nij", J, J)
    S = np.zeros((n, 6, 6))
    ry = np.einsum("nk,nk->n", r, y)
    S[:, :3, :3] = 0.5 * (r[:, :, None] * y[:, None, :] + y[:, :, None] * r[:, None, :]) - ry[:, None, None] * eye
    S[:, :3, 3:] = -0.5 * skew(r)
    S[:, 3:, :3] = 0.5 * skew(r)
    g = -(a / l2)[:, None] * u
    H = (a / l2 ** 2)[:, None, None] * u[:, :, None] * u[:, None, :] - (a / l2)[:, None, None] * (JtJ + S)
    return g, H


def abs_scale(x, y, a, ell):
    """The sums of the absolute values of every product a member's terms are made of (the magnitude float32 rounding of
    the per-member terms is relative to): for g (6,) and for H (6, 6)."""
    x, y, a = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(a, np.float64)
    l2 = float(ell) ** 2
    r = np.abs(y - x)
    ax = np.abs(x)
    ut = np.stack([r[:, 1] * ax[:, 2] + r[:, 2] * ax[:, 1], r[:, 2] * ax[:, 0] + r[:, 0] * ax[:, 2],
                   r[:, 0] * ax[:, 1] + r[:, 1] * ax[:, 0], r[:, 0], r[:, 1], r[:, 2]], 1)
    xy = np.abs(x[:, :, None] * y[:, None, :])                  # |x_k y_l|
    M = np.zeros((len(a), 6, 6))
    for k in range(3):
        M[:, k, k] = sum(xy[:, b, b] for b in range(3) if b != k)
        for l in range(3):
            if l != k:
                M[:, k, l] = 0.5 * (xy[:, k, l] + xy[:, l, k])
    m = 0.5 * np.abs(x + y)
    for k in range(3):
        for l in range(3):
            if l != k:
                M[:, k, 3 + l] = M[:, 3 + l, k] = m[:, 3 - k - l]
        M[:, 3 + k, 3 + k] = 1.0
    sg = ((a / l2)[:, None] * ut).sum(0)
    sH = ((a / l2 ** 2)[:, None, None] * ut[:, :, None] * ut[:, None, :] + (a / l2)[:, None, None] * M).sum(0)
    return sg, sH


def restate(x, y, rows, cols, a, ell):
    """f, g, H, nnz and the absolute scales of g and H over the members (rows[k], cols[k]) with weights a[k]."""
    x, y, a = np.asarray(x), np.asarray(y), np.asarray(a)
    g, H, sg, sH = np.zeros(6), np.zeros((6, 6)), np.zeros(6), np.zeros((6, 6))
    for k in range(0, len(rows), 1 << 18):   # (in chunks: a few million members would need gigabytes at once)
        X, Y, w = x[rows[k:k + (1 << 18)]], y[cols[k:k + (1 << 18)]], a[k:k + (1 << 18)]
        mg, mH = member_terms(X, Y, w, ell)
        cg, cH = abs_scale(X, Y, w, ell)
        g += mg.sum(0)
        H += mH.sum(0)
        sg += cg
        sH += cH
    return dict(f=float(np.sum(a.astype(np.float64))), g=g, H=H, nnz=len(rows), sg=sg, sH=sH)


def frozen_objective_delta(x, y, a, ell, xi):
    """F(xi) - F(0) of the frozen-set objective, y(xi) = exp(-xi^) y (scipy.linalg.expm of the 4 x 4 twist)."""
    from scipy.linalg import expm
    w, v = xi[:3], xi[3:]
    X = np.zeros((4, 4))
    X[:3, :3] = skew(np.asarray(w, np.float64)[None])[0]
    X[:3, 3] = v
    E = expm(-X)
    yx = y @ E[:3, :3].T + E[:3, 3]
    d = np.einsum("nk,nk->n", yx - y, yx + y - 2.0 * x)         # |x - y(xi)|^2 - |x - y|^2 without cancellation
    return float(np.sum(a * np.expm1(-d / (2.0 * ell * ell))))
