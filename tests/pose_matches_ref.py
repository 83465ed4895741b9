"""Numpy restatement of cvo_hip_pose_matches (include/cvo_hip.h) on the oracle's member set (pose_score_ref.members):
per row (fixed point) and per column (moving point) of A
    support = the float64 sum of the float32 weights of the point's members,
    count   = the number of its members,
    best    = the other index of the member with the largest weight, the smallest such index among equals; -1 if none,
    best_w  = that weight (float32); 0 if none.
Shared by tests/test_pose_matches_cpu.py and tests/test_gpu_pose_matches.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_score_ref  # noqa: E402


def one_side(own, other, val, n):
    """(support, count, best, best_w) over the n points of one cloud: `own` the members' indices in that cloud,
    `other` their indices in the other cloud, `val` their float32 weights."""
    own, other = np.asarray(own, np.int64), np.asarray(other, np.int64)
    val = np.asarray(val, np.float32)
    support = np.zeros(n, np.float64)
    np.add.at(support, own, val.astype(np.float64))
    count = np.bincount(own, minlength=n).astype(np.int32)
    best = np.full(n, -1, np.int32)
    best_w = np.zeros(n, np.float32)
    order = np.lexsort((other, -val.astype(np.float64), own))   # by point, then (-weight, other index)
    first = np.ones(len(order), bool)
    first[1:] = own[order][1:] != own[order][:-1]
    head = order[first]
    best[own[head]] = other[head]
    best_w[own[head]] = val[head]
    return support, count, best, best_w


def from_members(rows, cols, val, n_fixed, n_moving):
    """{"fixed": (support, count, best, best_w), "moving": ...} of a member set in COO form."""
    return {"fixed": one_side(rows, cols, val, n_fixed), "moving": one_side(cols, rows, val, n_moving)}


def matches(po, pmode, ell, xf, ff, xm, fm, R, T, search=None):
    """The restatement for the fixed cloud xf against the moving cloud xm at the pose (R, T), with the member set's
    (rows, cols, val) under "members"."""
    if search is None:
        search = po.SEARCH_DENSE if pmode == po.MODE_MATLAB else po.SEARCH_GRID
    p = po.default_params(pmode)
    y = po.transform(R, T, xm)
    rows, cols, val = pose_score_ref.members(po, p, ell, xf, ff, y, fm, search)
    out = from_members(rows, cols, val, len(xf), len(xm))
    out["members"] = (rows, cols, val)
    return out
