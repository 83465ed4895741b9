"""Mutants of the diagonal scan of tests/fe_stereo_paths_ref.py: each one restates a diagonal direction with one
plausible device error in it -- the errors of a wave that walks a WRAPPED line (one column index, one row per step, the
column moving by rx and wrapping round the image) or one true diagonal.  tests/test_fe_stereo_paths_cpu.py holds that
the cases tell every one of them from the restatement: a kernel with that error would fail the byte comparison of
tests/test_gpu_fe_stereo_paths.py.  Python only; nothing here ever runs against the GPU."""
import numpy as np

import fe_stereo_paths_ref as P


def _wrapped(C, p1, p2, rx, ry, restart_at=None, next_cost=False):
    """A diagonal direction as w wrapped lines, every line's predecessor the previous row rolled by rx.  `restart_at`:
    the column in which a line begins anew (None: in none, the line runs on across the border); `next_cost`: where it
    begins anew it takes the cost of the line's next step (the row after, the column one further)."""
    C = np.asarray(C, np.int64)
    h, w, D = C.shape
    assert rx != 0 and ry != 0
    L = np.empty_like(C)
    rows = list(range(h) if ry > 0 else range(h - 1, -1, -1))
    x = np.arange(w)
    fresh = np.zeros(w, bool) if restart_at is None else x == restart_at
    for k, y in enumerate(rows):
        if k == 0:
            L[y] = C[y]
            continue
        prev = L[rows[k - 1]][(x - rx) % w]
        begin = C[y]
        if next_cost and k + 1 < h:
            begin = C[rows[k + 1]][(x + rx) % w]
        L[y] = np.where(fresh[:, None], begin, P._step(prev, C[y], p1, p2))
    return L


def _diagonal_only(mutant):
    """a form of one direction that mutates the diagonals and leaves rows and columns to the restatement"""
    def one(C, p1, p2, rx, ry):
        if rx == 0 or ry == 0:
            return P.direction(C, p1, p2, rx, ry)
        return mutant(C, p1, p2, rx, ry)
    return one


def _border(C, rx):
    """the column whose p - r lies outside the image"""
    return 0 if rx > 0 else C.shape[1] - 1


# 1. no restart where the line leaves the image: it runs on across the border
no_restart = _diagonal_only(lambda C, p1, p2, rx, ry: _wrapped(C, p1, p2, rx, ry, restart_at=None))
# 2. ry negated
ry_negated = _diagonal_only(lambda C, p1, p2, rx, ry: P.direction(C, p1, p2, rx, -ry))
# 3. the restart on the wrong vertical border: x = w - 1 for rx = +1, x = 0 for rx = -1
wrong_border = _diagonal_only(
    lambda C, p1, p2, rx, ry: _wrapped(C, p1, p2, rx, ry, restart_at=C.shape[1] - 1 - _border(C, rx)))
# 4. the prefetch's off-by-one: after a wrap the cost of step t + 1 at step t
next_cost = _diagonal_only(
    lambda C, p1, p2, rx, ry: _wrapped(C, p1, p2, rx, ry, restart_at=_border(C, rx), next_cost=True))

MUTANTS = {"no-restart": no_restart, "ry-negated": ry_negated, "wrong-border": wrong_border, "next-cost": next_cost}


def restated(C, p1, p2, rx, ry):
    """_wrapped() without an error: the restatement's diagonal again (held in the CPU test, so that a mutant differs by
    its error and not by its form)"""
    return _diagonal_only(lambda C, p1, p2, rx, ry: _wrapped(C, p1, p2, rx, ry, restart_at=_border(C, rx)))(C, p1, p2, rx, ry)


def sums(C, st, mask, name):
    """the cost sums of the volume C under a mask through a mutant"""
    Sv = np.zeros(C.shape, np.int64)
    for b in P.bits(mask):
        Sv += MUTANTS[name](C, st["p1"], st["p2"], *P.DIRS[b])
    return Sv.astype(np.uint16)
