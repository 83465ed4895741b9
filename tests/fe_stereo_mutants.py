"""Mutants of the numpy restatement of the stereo contract (tests/fe_stereo_ref.py): each one restates one stage with
one plausible device error in it -- the errors a wave with two disparities per lane (d = lane and d = lane + 64) can
make where d = 63 and d = 64 meet, at d = D - 1, at the end of a row and in a packed key.  tests/test_fe_stereo_cpu.py
holds that the edge cases tell every one of them from the restatement: a kernel with that error would fail the byte
comparison of tests/test_gpu_fe_stereo.py.  Python only; nothing here ever runs against the GPU."""
import numpy as np

import fe_stereo_ref as S

HALF = 64       # the lanes of a wave: disparities below and from HALF lie in two registers


def _scan(Cs, p1, p2, seam_cut=False, wrap=False):
    """S._scan with the d - 1 / d + 1 neighbours cut between d = 63 and d = 64, or with d = 0 as the upper neighbour
    of d = D - 1"""
    D = Cs.shape[2]
    out = np.empty_like(Cs)
    L = Cs[0].copy()
    out[0] = L
    for t in range(1, Cs.shape[0]):
        m = L.min(axis=1, keepdims=True)
        below = np.full_like(L, S.BIG)
        below[:, 1:] = L[:, :-1] + p1
        above = np.full_like(L, S.BIG)
        above[:, :-1] = L[:, 1:] + p1
        if seam_cut and D > HALF:
            below[:, HALF] = S.BIG
            above[:, HALF - 1] = S.BIG
        if wrap:
            above[:, D - 1] = L[:, 0] + p1
        L = Cs[t] + np.minimum(np.minimum(L, m + p2), np.minimum(below, above)) - m
        out[t] = L
    return out


def path_sums(C, p1, p2, **error):
    """S.path_sums over the mutated recurrence"""
    Ct = C.transpose(1, 0, 2)
    Sv = _scan(Ct, p1, p2, **error).transpose(1, 0, 2)
    Sv = Sv + _scan(Ct[::-1], p1, p2, **error)[::-1].transpose(1, 0, 2)
    Sv = Sv + _scan(C, p1, p2, **error)
    Sv = Sv + _scan(C[::-1], p1, p2, **error)[::-1]
    return Sv.astype(np.uint16)


def subpixel_unchecked(Sv, ds, S1, own_half=False):
    """S.subpixel without its assertion, for winners that are not the minimum"""
    Sv = Sv.astype(np.int64)
    D = Sv.shape[2]
    half = HALF * (ds // HALF)
    at = lambda d: np.take_along_axis(Sv, np.clip(d, 0, D - 1)[:, :, None], 2)[:, :, 0]
    Sm, Sp = (at(half + (ds - 1) % HALF), at(half + (ds + 1) % HALF)) if own_half else (at(ds - 1), at(ds + 1))
    den = Sm + Sp - 2 * S1
    ok = (ds > 0) & (ds < D - 1) & (den > 0)
    off = np.where(ok, ((Sm - Sp) * 16 + den) // np.where(ok, 2 * den, 1), 0)
    return 16 * ds + np.clip(off, -8, 8)        # (what a wrong neighbour gives is not bounded: kept inside q's digit)


def subpixel_own_half(Sv, ds, S1):
    """S.subpixel with S(d* - 1) and S(d* + 1) read at (d* -+ 1) mod 64 within d*'s own half"""
    return subpixel_unchecked(Sv, ds, S1, own_half=True)


def right_map_unbounded(Sv):
    """S.right_map without x + d < w: the diagonal S(x + d, y, d) runs on into the next row (and ends with the plane)"""
    Sv = Sv.astype(np.int64)
    h, w, D = Sv.shape
    flat = Sv.reshape(h * w, D)
    SR = np.full((h * w, D), S.BIG, np.int64)
    for d in range(min(D, h * w)):
        SR[:h * w - d, d] = flat[d:, d]
    return SR.argmin(axis=1).reshape(h, w)


def not_unique_own_half(Sv, ds, S1, uniqueness):
    """S.not_unique with d* - 1 and d* + 1 left out only where they lie in d*'s half"""
    Sv = Sv.astype(np.int64)
    d = np.arange(Sv.shape[2])[None, None, :]
    far = (np.abs(d - ds[:, :, None]) > 1) | (d // HALF != ds[:, :, None] // HALF)
    S2 = np.where(far, Sv, S.BIG).min(axis=2)
    return far.any(axis=2) & (S2 * (100 - uniqueness) < S1 * 100)


def winners_narrow_keys(Sv):
    """S.winners through keys that keep 10 bits of S"""
    key = ((Sv.astype(np.int64) & 1023) << 8) | np.arange(Sv.shape[2])[None, None, :]
    key = key.min(axis=2)
    return key & 255, key >> 8


def planes(P, st, **stage):
    """S.decide on the cost sums of the planes P with one stage replaced"""
    return S.decide(P["sum"], st, S.FX, S.SCALE, **stage)


def sums(P, st, **error):
    """the cost sums of the planes P through the mutated recurrence"""
    return path_sums(S.cost(P["census_l"], P["census_r"], st["max_disp"]), st["p1"], st["p2"], **error)
